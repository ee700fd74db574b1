#!/usr/bin/env python3
"""What diversifying recommendation lists costs (HipEngine.rerank_mmr, sml_rerank_mmr) at the Yelp shape: U = 60,000 users,
I = 123,000 items, every user's pool of C = 100 and 128 items taken by topk_items, re-ranked to k = 20 at lam = 0.7 with the
cosine of the item rows, at d = 32 and 64 on fp32 tables and d = 128 on fp16 tables.

Routes, in the same process on the same pools:

  kernel   rerank_mmr with a ready norm table (the norm table's own build, item_adjust_cosine, is timed beside it)
  torch    per chunk of 4,096 lists: a gather of the [n, C, d] candidate rows, scaled to unit length, then a Python loop of k
           dependent steps (value, masked argmax, scatter, gather of the picked rows, bmm, maximum); its peak extra memory is
           reported.  It rounds differently and breaks ties by torch's rule: it is timed and its lists are compared as a share
           of equal rows, not byte for byte
  pool     the topk_items call that made the pool: what the caller has already paid

Also reported per leg: the mean intra-list similarity (sim_sum / (k (k - 1) / 2) of the k picks) at lam = 1, 0.7 and 0.3, and
that lam = 1 returned the pool's first k columns.  HIP events around each call after warm-up, repetitions alternated between
the routes; medians, minima, interquartile spread.  One JSON line on stdout (and --out).
usage: python tools/rerank_probe.py [--d 32,64,128] [--reps 10] [--out profiles/r19_rerank_probe.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from candidates_probe import rounds                                   # noqa: E402
from half_retrieval_probe import I, K, U, stats, timed                # noqa: E402
from sml_amd.engine import HipEngine                                  # noqa: E402

POOLS = (100, 128)
LAM = 0.7
TORCH_CHUNK = 4096


def torch_route(wi, nrm, pool_i, pool_s, k, lam):
    out = []
    for c0 in range(0, pool_i.shape[0], TORCH_CHUNK):
        it, sc = pool_i[c0:c0 + TORCH_CHUNK], pool_s[c0:c0 + TORCH_CHUNK]
        m, c = it.shape
        rows = wi.index_select(0, it.reshape(-1)).view(m, c, -1).float() * nrm[it].unsqueeze(2)
        lo, hi = sc.min(1, keepdim=True).values, sc.max(1, keepdim=True).values
        r = (sc - lo) / (hi - lo).clamp_min(1e-30)
        pen = torch.full_like(sc, float("-inf"))
        taken = torch.zeros_like(sc, dtype=torch.bool)
        ar = torch.arange(m, device=it.device)
        picks = []
        for t in range(k):
            v = lam * r - (1.0 - lam) * pen if t else lam * r
            j = v.masked_fill(taken, float("-inf")).argmax(1)
            picks.append(j)
            taken[ar, j] = True
            pen = torch.maximum(pen, torch.bmm(rows, rows[ar, j].unsqueeze(2)).squeeze(2))
        out.append(torch.gather(it, 1, torch.stack(picks, 1)))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--users", type=int, default=U)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.users
    users = torch.arange(n, device=dev)
    pairs = K * (K - 1) / 2.0
    result = {"tool": "rerank_probe", "device": torch.cuda.get_device_name(dev), "U": n, "I": I, "k": K, "lam": LAM, "metric": "cosine",
              "reps": args.reps, "torch_chunk": TORCH_CHUNK, "by_d": {}}
    for d in [int(x) for x in args.d.split(",") if x]:
        gd = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=gd) * 0.3).half().to(dev)
        wi = (torch.randn(I, d, generator=gd) * 0.3).half().to(dev)
        if d != 128:
            wu, wi = wu.float(), wi.float()
        eng = HipEngine(dev, d, 256)
        adj = eng.item_adjust_cosine(wi)
        nrm = adj[0]
        res = {"dtype": "fp16" if d == 128 else "fp32", "row_bytes": d * wi.element_size(),
               "norm_table": stats([timed(lambda: eng.item_adjust_cosine(wi, adj), dev)[0] for _ in range(args.reps + 2)][2:])}
        for c in POOLS:
            pool_i, pool_s = eng.topk_items(wu, wi, users, c)
            fns = {"kernel": lambda: eng.rerank_mmr(wi, pool_i, pool_s, K, LAM, nrm=adj),
                   "torch": lambda: torch_route(wi, nrm, pool_i, pool_s, K, LAM),
                   "pool": lambda: eng.topk_items(wu, wi, users, c)}
            r = rounds(fns, args.reps, args.warmup, dev)
            ms = r["kernel"]["ms"]
            r["kernel"]["lists_per_s"] = round(n / (ms * 1e-3))
            for other in ("torch", "pool"):
                r[other]["over_kernel"] = round(r[other]["ms"] / ms, 2)
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            t_items = torch_route(wi, nrm, pool_i, pool_s, K, LAM)
            torch.cuda.synchronize(dev)
            r["torch"]["peak_extra_mb"] = round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)
            got = eng.rerank_mmr(wi, pool_i, pool_s, K, LAM, nrm=adj)
            r["torch"]["rows_equal_to_kernel"] = round(float((t_items == got[0]).all(1).float().mean()), 4)
            r["picks_per_list"] = float(got[3].float().mean())
            ils = {}
            for lam in (1.0, LAM, 0.3):
                o = eng.rerank_mmr(wi, pool_i, pool_s, K, lam, nrm=adj)
                ils[str(lam)] = round(float((o[4].double() / pairs).mean()), 5)
                if lam == 1.0:
                    r["lam1_is_the_pool_prefix"] = bool(torch.equal(o[0], pool_i[:, :K]))
            r["mean_intra_list_similarity"] = ils
            res["C%d" % c] = r
            del pool_i, pool_s, got, t_items
        result["by_d"][str(d)] = res
        del eng, wu, wi
    ok = all(v["lam1_is_the_pool_prefix"] for r in result["by_d"].values() for v in r.values() if isinstance(v, dict) and "kernel" in v)
    result["lam1_prefix_held_everywhere"] = ok
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
