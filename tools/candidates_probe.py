#!/usr/bin/env python3
"""What ranking per-user candidate lists costs (HipEngine.topk_candidates, sml_topk_candidates) at the Yelp shape: U = 60,000
users, I = 123,000 items, k = 20, at d = 32 and 64 on fp32 tables and d = 128 on fp16 tables, with and without a Seen of the
Yelp history's size (five periods of 200,000 Zipf interactions, as tools/item_filter_probe.py builds it).  Shapes:

  a  period   100,000 dense int64 rows [user, 1,000 candidates] read in place (stride 1,001, first 1): a test period
  b  ragged   60,000 users with 200 ragged int32 candidates each

Routes, in the same process on the same tables:

  kernel      topk_candidates
  torch       chunked index_select of the candidate rows, bmm against the user rows, Seen masked by a searchsorted over the
              sorted (user, item) keys, torch.topk, a gather of the ids; its peak extra memory is reported.  It orders ties by
              torch's rule and lists a repeated id twice: it is timed, not compared
  walk        (b only) topk_items for the same users over the whole catalogue: what a caller without this call would run and
              then post-filter
  eval_ranks  (a only, fp32 tables) the evaluation kernel on the same rows: it gathers the same item rows and keeps one integer
              per row -- the natural floor.  Timed as the engine runs it by default and as the plain kernel

For 64 sampled lists of each shape the kernel's rows are compared byte for byte with topk_items for that user alone under the
filter made of the list (the defining identity); the result records that it held.  HIP events around each call after warm-up,
repetitions alternated between the routes; medians, minima, interquartile spread.  Rates: candidates per second, and the
gathered item-row bytes per second (eligible entries x row bytes) as a share of the 5.5 to 5.8 TB/s at which random whole rows
have been read into registers on this GPU.  One JSON line on stdout (and --out).
usage: python tools/candidates_probe.py [--d 32,64,128] [--reps 10] [--out profiles/r17_candidates_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from half_retrieval_probe import I, K, U, same, stats, timed          # noqa: E402
from sml_amd import synth                                             # noqa: E402
from sml_amd.engine import HipEngine                                  # noqa: E402
from sml_amd.retrieval import CandidateRows, SeenItems                # noqa: E402

N_A, C_A, N_B, C_B = 100000, 1000, 60000, 200
GATHER_TBPS = (5.5, 5.8)
TORCH_CHUNK = 4096


def rounds(fns, reps, warmup, dev):
    """Every route `warmup` times, then `reps` rounds that run each route once, in turn."""
    for _ in range(warmup):
        for f in fns.values():
            timed(f, dev)
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, f in fns.items():
            ts[name].append(timed(f, dev)[0])
    return {name: stats(t) for name, t in ts.items()}


def torch_route(wu, wi, users, cand, keys):
    """cand: int64 [n, C] (ids inside the catalogue).  keys: the sorted u * I + i of Seen, or None."""
    out_i, out_s = [], []
    for c0 in range(0, users.shape[0], TORCH_CHUNK):
        u, c = users[c0:c0 + TORCH_CHUNK], cand[c0:c0 + TORCH_CHUNK]
        rows = wi.index_select(0, c.reshape(-1)).view(c.shape[0], c.shape[1], -1)
        s = torch.bmm(rows, wu.index_select(0, u).unsqueeze(2)).squeeze(2).float()
        if keys is not None:
            q = u.unsqueeze(1) * I + c
            at = torch.searchsorted(keys, q).clamp_(max=keys.shape[0] - 1)
            s = s.masked_fill(keys[at] == q, float("-inf"))
        v, j = torch.topk(s, K, dim=1)
        out_s.append(v)
        out_i.append(torch.gather(c, 1, j))
    return torch.cat(out_i), torch.cat(out_s)


def identity_holds(eng, wu, wi, users, lists, got, csr, rng, count=64):
    """The kernel's rows against topk_items for the user alone under the filter made of the list, for `count` sampled lists."""
    for x in rng.choice(users.shape[0], size=count, replace=False):
        allow = eng.item_filter_from_ids(lists(int(x)), I)
        it, sc = eng.topk_items(wu, wi, users[x:x + 1], K, csr, allow=allow)
        if not same((got[0][x], got[1][x]), (it[0], sc[0])):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    csr = seen.device(dev)
    keys = torch.from_numpy(seen._keys).to(dev)
    g = torch.Generator().manual_seed(17)
    rows_a = torch.cat([torch.randint(0, U, (N_A, 1), generator=g), torch.randint(0, I, (N_A, C_A), generator=g)], 1).to(dev)
    users_b = torch.randperm(U, generator=g)[:N_B].to(dev)
    cand_b = torch.randint(0, I, (N_B, C_B), generator=g, dtype=torch.int32).to(dev)
    off_b = torch.arange(N_B + 1, device=dev, dtype=torch.int64) * C_B
    cr_a = CandidateRows(rows_a, first_col=1)
    assert cr_a.geometry == (C_A + 1, 1, C_A) and cr_a.rows.data_ptr() == rows_a.data_ptr()
    users_a, dense_a, dense_b = rows_a[:, 0].contiguous(), rows_a[:, 1:], cand_b.long()
    result = {"tool": "candidates_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "k": K,
              "shapes": {"a": {"lists": N_A, "candidates": C_A, "form": "dense int64, stride %d, first 1" % (C_A + 1)},
                         "b": {"lists": N_B, "candidates": C_B, "form": "ragged int32"}},
              "seen_pairs": int(len(seen)), "reps": args.reps, "register_gather_tb_per_s": list(GATHER_TBPS), "by_d": {}}
    rng = np.random.RandomState(5)
    for d in [int(x) for x in args.d.split(",") if x]:
        gd = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=gd) * 0.3).half().to(dev)
        wi = (torch.randn(I, d, generator=gd) * 0.3).half().to(dev)
        if d != 128:
            wu, wi = wu.float(), wi.float()
        eng = HipEngine(dev, d, 256)
        row_bytes = d * wi.element_size()
        res = {"dtype": "fp16" if d == 128 else "fp32", "row_bytes": row_bytes}
        for sname, s in (("noseen", None), ("seen", csr)):
            k_ = keys if s is not None else None
            for shape, n, c, users, cand, dense in (("a", N_A, C_A, None, cr_a, dense_a), ("b", N_B, C_B, users_b, (off_b, cand_b.reshape(-1)), dense_b)):
                uu = users_a if users is None else users
                fns = {"kernel": lambda: eng.topk_candidates(wu, wi, users, cand, K, s),
                       "torch": lambda: torch_route(wu, wi, uu, dense, k_)}
                if shape == "b":
                    fns["walk"] = lambda: eng.topk_items(wu, wi, uu, K, s)
                elif d != 128 and s is None:
                    fns["eval_ranks"] = lambda: eng.eval_ranks(wu, wi, rows_a)
                    fns["eval_ranks_plain"] = lambda: eng.eval_ranks(wu, wi, rows_a, blocked=False, sliced=False)
                r = rounds(fns, args.reps, args.warmup, dev)
                got = eng.topk_candidates(wu, wi, users, cand, K, s)
                elig = int(got[2].sum(dtype=torch.int64))
                ms = r["kernel"]["ms"]
                r["kernel"].update(candidates_per_s=round(n * c / (ms * 1e-3)), eligible_entries=elig,
                                   gathered_gb_per_s=round(elig * row_bytes / (ms * 1e-3) / 1e9, 1),
                                   share_of_register_gather=[round(elig * row_bytes / (ms * 1e-3) / (t * 1e12), 3) for t in GATHER_TBPS])
                torch.cuda.synchronize(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                torch_route(wu, wi, uu, dense, k_)
                torch.cuda.synchronize(dev)
                r["torch"]["peak_extra_mb"] = round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)
                for other in fns:
                    if other != "kernel":
                        r[other]["over_kernel"] = round(r[other]["ms"] / ms, 2)
                lists = (lambda x: dense[x].to(torch.int32))
                r["identity_64_lists_byte_equal"] = identity_holds(eng, wu, wi, uu, lists, got, s, rng)
                res["%s_%s" % (shape, sname)] = r
                del got
        result["by_d"][str(d)] = res
        del eng, wu, wi
    ok = all(v["identity_64_lists_byte_equal"] for r in result["by_d"].values() for v in r.values() if isinstance(v, dict))
    result["identity_held_everywhere"] = ok
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
