#!/usr/bin/env python3
"""What the clustered item index costs and buys (sml_amd.retrieval.ItemIndex, HipEngine.ivf_search) at the Yelp shape: U = 60,000
users, I = 123,000 items, k = 20, d = 32 / 64 on fp32 tables and d = 128 on fp16 tables, a Seen of the Yelp history's size (five
periods of 200,000 Zipf interactions, as tools/item_filter_probe.py builds it).  One run records

  build       ItemIndex.build (10 iterations, cosine) at n_list = 128 / 512 / 2,048 and refresh(iters=2), wall time, three runs each
  search      at n_list = 512 and nprobe = 1 .. 64: ItemIndex.probe and HipEngine.ivf_search, timed apart, against
                walk        topk_items for the same users over the whole catalogue (the same commit)
                candidates  the same candidates written out as a ragged list on the device (torch) and given to topk_candidates,
                            with that route's peak extra memory (nprobe <= --ragged_max: the list grows with nprobe)
                torch       chunked matmul + Seen mask + topk over the whole catalogue
              nine rounds that run every route once, in turn, after warm-up; medians, minima, interquartile spread; the search's
              gathered row traffic (eligible entries x row bytes / time) beside the 5.8 TB/s measured for bare random rows; the
              indexed rows are compared byte for byte with the candidates route's
  recall      sml_amd.evaluation.index_recall at 20 against nprobe on two generated tables (d = 64, fp32, 4,096 users): uniform
              random rows, where clustering has nothing to find, and a 64-component Gaussian mixture
  scale       one reading at 1,000,000 items (d = 64, n_list = 1,000, nprobe = 8)

Not measured: trained (non-random) SML tables; recall across periods under refresh.  One JSON line on stdout (and --out).
usage: python tools/ivf_probe.py [--d 32,64,128] [--reps 9] [--out profiles/r21_ivf_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from candidates_probe import rounds                                   # noqa: E402
from half_retrieval_probe import CHUNK, I, K, U, same, stats, timed   # noqa: E402
from sml_amd import synth                                             # noqa: E402
from sml_amd.engine import HipEngine                                  # noqa: E402
from sml_amd.evaluation import index_recall                           # noqa: E402
from sml_amd.mf import MFbasemode                                     # noqa: E402
from sml_amd.retrieval import ItemIndex, SeenItems                    # noqa: E402

GATHER_TBPS = 5.8
NPROBES = (1, 2, 4, 8, 16, 32, 64)


def note(msg):
    sys.stderr.write("[ivf_probe] %s\n" % msg)
    sys.stderr.flush()


def wall(fn, dev, runs=3):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts), out


def ragged_from_probes(idx, probes):
    """(cand_off int64 [n + 1], cand int32): the members of each row's probed lists, in probe order, written out with torch."""
    n, P = probes.shape
    p = probes.long().clamp(min=0)
    start = idx.list_off[p]
    ln = torch.where(probes >= 0, idx.list_off[p + 1] - start, torch.zeros_like(start)).reshape(-1)
    end = torch.cumsum(ln, 0)
    total = int(end[-1])
    seg = torch.repeat_interleave(torch.arange(n * P, device=probes.device), ln, output_size=total)
    pos = torch.arange(total, device=probes.device) - (end - ln)[seg] + start.reshape(-1)[seg]
    off = torch.cat([end.new_zeros(1), end.view(n, P)[:, -1]])
    return off, idx.list_items[pos]


def torch_route(wu, wi, users, keys, n_item):
    out_i, out_s = [], []
    for c0 in range(0, users.shape[0], CHUNK):
        u = users[c0:c0 + CHUNK]
        s = (wu.index_select(0, u) @ wi.t()).float()
        if keys is not None:
            lo, hi = torch.searchsorted(keys, u * n_item), torch.searchsorted(keys, (u + 1) * n_item)
            r = torch.repeat_interleave(torch.arange(u.shape[0], device=u.device), hi - lo)
            at = torch.arange(r.shape[0], device=u.device) - torch.repeat_interleave(torch.cumsum(hi - lo, 0) - (hi - lo), hi - lo) + lo[r]
            s[r, keys[at] - u[r] * n_item] = float("-inf")
        v, j = torch.topk(s, K, dim=1)
        out_s.append(v)
        out_i.append(j)
    return torch.cat(out_i), torch.cat(out_s)


def peak_extra_mb(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)


def recall_table(name, wu, wi, dev, n_users=4096):
    model = MFbasemode(wu.shape[0], wi.shape[0], wu.shape[1]).to(dev)
    model.user_laten.weight.data.copy_(wu)
    model.item_laten.weight.data.copy_(wi)
    idx = ItemIndex.build(model.item_laten.weight.data, n_list=512, iters=10, seed=0)
    users = torch.arange(n_users, device=dev)
    sizes = idx.sizes().cpu().numpy()
    out = {"table": name, "n_list": 512, "users": n_users, "list_size_min_median_max": [int(sizes.min()), float(np.median(sizes)), int(sizes.max())],
           "recall_at_20": {}, "probed_share_of_catalogue": {}}
    for p in NPROBES:
        out["recall_at_20"][str(p)] = round(index_recall(model, idx, users, K, nprobe=p), 4)
        pr = idx.probe(model.user_laten.weight.data, users, p).long()
        out["probed_share_of_catalogue"][str(p)] = round(float(idx.sizes()[pr].sum(1).double().mean()) / wi.shape[0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64,128")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ragged_max", type=int, default=16)
    ap.add_argument("--scale_items", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    csr = seen.device(dev)
    keys = torch.from_numpy(seen._keys).to(dev)
    users = torch.randperm(U, generator=torch.Generator().manual_seed(17)).to(dev)
    result = {"tool": "ivf_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "k": K, "seen_pairs": int(len(seen)),
              "reps": args.reps, "register_gather_tb_per_s": GATHER_TBPS, "ragged_route_up_to_nprobe": args.ragged_max, "by_d": {},
              "not_measured": ["trained (non-random) SML tables", "recall across periods under refresh"]}
    equal = True
    for d in [int(x) for x in args.d.split(",") if x]:
        gd = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=gd) * 0.3).half().to(dev)
        wi = (torch.randn(I, d, generator=gd) * 0.3).half().to(dev)
        if d != 128:
            wu, wi = wu.float(), wi.float()
        eng = HipEngine(dev, d, 256)
        row_bytes = d * wi.element_size()
        res = {"dtype": "fp16" if d == 128 else "fp32", "row_bytes": row_bytes, "build": {}, "search": {}}
        idx512 = None
        for n_list in (128, 512, 2048):
            b, idx = wall(lambda: ItemIndex.build(wi, n_list=n_list, iters=10, seed=0, engine=eng), dev)
            r, _ = wall(lambda: idx.refresh(wi, iters=2), dev)
            sizes = idx.sizes().cpu().numpy()
            res["build"][str(n_list)] = {"build_10_iters": b, "refresh_2_iters": r, "empty_lists": int((sizes == 0).sum()),
                                         "list_size_median_max": [float(np.median(sizes)), int(sizes.max())]}
            if n_list == 512:
                idx512 = ItemIndex.build(wi, n_list=512, iters=10, seed=0, engine=eng)
        idx = idx512
        note("d = %d: built" % d)
        for nprobe in NPROBES:
            note("d = %d, nprobe = %d" % (d, nprobe))
            probes = idx.probe(wu, users, nprobe)
            fns = {"probe": lambda: idx.probe(wu, users, nprobe),
                   "ivf_search": lambda: eng.ivf_search(wu, wi, users, idx, probes, K, csr)}
            if nprobe <= args.ragged_max:
                fns["candidates"] = lambda: eng.topk_candidates(wu, wi, users, ragged_from_probes(idx, probes), K, csr)
            if nprobe == 8:
                fns["walk"] = lambda: eng.topk_items(wu, wi, users, K, csr)
                fns["torch"] = lambda: torch_route(wu, wi, users, keys, I)
            r = rounds(fns, args.reps, args.warmup, dev)
            got = eng.ivf_search(wu, wi, users, idx, probes, K, csr)
            elig = int(got[2].sum(dtype=torch.int64))
            ms = r["ivf_search"]["ms"]
            r["probe_plus_search_ms"] = round(r["probe"]["ms"] + ms, 4)
            r["ivf_search"].update(eligible_entries=elig, gathered_gb_per_s=round(elig * row_bytes / (ms * 1e-3) / 1e9, 1),
                                   share_of_register_gather=round(elig * row_bytes / (ms * 1e-3) / (GATHER_TBPS * 1e12), 3))
            if "candidates" in fns:
                r["candidates"]["peak_extra_mb"] = peak_extra_mb(fns["candidates"], dev)
                r["rows_equal_candidates_route"] = same(got, fns["candidates"]())
                equal = equal and r["rows_equal_candidates_route"]
            if "torch" in fns:
                r["torch"]["peak_extra_mb"] = peak_extra_mb(fns["torch"], dev)
            res["search"][str(nprobe)] = r
            del got
        result["by_d"][str(d)] = res
        del eng, wu, wi, idx, idx512
    note("recall tables")
    # recall against nprobe: a table with nothing to find, and one with 64 clusters
    g = torch.Generator().manual_seed(99)
    d = 64
    uni_u, uni_i = torch.randn(U, d, generator=g).to(dev), torch.randn(I, d, generator=g).to(dev)
    centres = torch.randn(64, d, generator=g)
    mix_i = (centres[torch.randint(0, 64, (I,), generator=g)] + 0.3 * torch.randn(I, d, generator=g)).to(dev)
    mix_u = (centres[torch.randint(0, 64, (U,), generator=g)] + 0.3 * torch.randn(U, d, generator=g)).to(dev)
    result["recall"] = [recall_table("uniform random rows", uni_u, uni_i, dev),
                        recall_table("64-component Gaussian mixture (sigma 0.3)", mix_u, mix_i, dev)]
    del uni_u, uni_i, mix_i, mix_u
    if args.scale_items:
        n_big = args.scale_items
        note("scale reading")
        eng = HipEngine(dev, d, 256)
        wu = (torch.randn(U, d, generator=g) * 0.3).to(dev)
        wi = (torch.randn(n_big, d, generator=g) * 0.3).to(dev)
        b, idx = wall(lambda: ItemIndex.build(wi, n_list=1000, iters=4, seed=0, engine=eng), dev, runs=1)
        probes = idx.probe(wu, users, 8)
        r = rounds({"probe": lambda: idx.probe(wu, users, 8), "ivf_search": lambda: eng.ivf_search(wu, wi, users, idx, probes, K),
                    "walk": lambda: eng.topk_items(wu, wi, users, K)}, args.reps, args.warmup, dev)
        r["probe_plus_search_ms"] = round(r["probe"]["ms"] + r["ivf_search"]["ms"], 4)
        result["scale"] = dict(r, items=n_big, d=d, n_list=1000, nprobe=8, build_4_iters=b)
    result["rows_equal_candidates_route_everywhere"] = equal
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
