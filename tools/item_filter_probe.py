#!/usr/bin/env python3
"""What an item filter buys at the Yelp shape (U = 60,000 users, I = 123,000 items, the Seen / test rows / held-out sets of
tools/half_retrieval_probe.py), in one process: topk_items K = 20 over all users, full_rank over 10,000 rows and user_ranks
over the period's held-out sets, each with allow= against the same build's unfiltered call on the same tables, at d = 32
and 64 on fp32 tables and d = 128 on fp16 tables.  Filters:

  range10     about 10 % allowed as ONE contiguous id range (a period's new items): whole tiles are skipped
  scatter10   about 10 % allowed, scattered uniformly: almost no 32-item tile is empty, nothing is skipped
  scatter50   about 50 % allowed, scattered

The Seen' route (the filter's complement added to every user's Seen range) is not timed: its CSR size is reported.
HIP events around each call after warm-up, repetitions alternated between the filtered and the unfiltered call; medians,
minima and the interquartile spread.  One JSON line on stdout (and --out).
usage: python tools/item_filter_probe.py [--d 32,64,128] [--reps 20] [--out f.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from half_retrieval_probe import I, K, KS, N_HELD, N_ROWS, U, alternate, stats      # noqa: E402
from sml_amd import synth                                                           # noqa: E402
from sml_amd.engine import HipEngine                                                # noqa: E402
from sml_amd.retrieval import ItemFilter, SeenItems, held_out, nonempty_users       # noqa: E402


def filters():
    rng = np.random.RandomState(77)
    lo = I - I // 10
    out = {"range10": ItemFilter(I).allow(np.arange(lo, I)),
           "scatter10": ItemFilter.from_mask(rng.rand(I) < 0.1),
           "scatter50": ItemFilter.from_mask(rng.rand(I) < 0.5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64,128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    _, test = synth.sample_period(np.random.RandomState(2010), N_ROWS, U, I, neg=1)
    _, held = synth.sample_period(np.random.RandomState(2005), N_HELD, U, I, neg=1)
    h_users, pos_off, pos_items = nonempty_users(held_out(held, U, I))
    csr = seen.device(dev)
    rows = torch.from_numpy(test[:, :2].copy()).to(dev)
    users = torch.arange(U, device=dev)
    flt = filters()
    result = {"tool": "item_filter_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "rows": N_ROWS, "k": K,
              "held_out_users": int(len(h_users)), "seen_pairs": int(len(seen)), "reps": args.reps, "filters": {}, "by_d": {}}
    for name, f in flt.items():
        words = f.host()
        empty = int((words == 0).sum())
        entries = len(seen) + U * (I - len(f))          # an upper bound that ignores the overlap with Seen (under 1 %)
        result["filters"][name] = {"allowed": len(f), "allowed_frac": round(len(f) / I, 4), "tiles": int(len(words)),
                                   "empty_tiles": empty, "seen_prime_csr_entries": int(entries),
                                   "seen_prime_csr_gb": round(entries * 4 / 1e9, 1)}
    for d in [int(x) for x in args.d.split(",") if x]:
        g = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=g) * 0.3).half().to(dev)
        wi = (torch.randn(I, d, generator=g) * 0.3).half().to(dev)
        if d != 128:
            wu, wi = wu.float(), wi.float()
        eng = HipEngine(dev, d, 256)
        calls = {"topk_items": lambda a: eng.topk_items(wu, wi, users, K, csr, allow=a),
                 "full_rank": lambda a: eng.full_rank(wu, wi, rows, csr, allow=a),
                 "user_ranks": lambda a: eng.user_ranks(wu, wi, h_users, pos_off, pos_items, csr, KS, allow=a)}
        res = {"dtype": "fp16" if d == 128 else "fp32"}
        for cname, fn in calls.items():
            res[cname] = {}
            for name, f in flt.items():
                a = f.device(dev)
                ta, tb, _, _ = alternate(lambda: fn(a), lambda: fn(None), args.reps, args.warmup, dev)
                sa, sb = stats(ta), stats(tb)
                res[cname][name] = {"filtered": sa, "unfiltered": sb, "filtered_over_unfiltered": round(sa["ms"] / sb["ms"], 3)}
        result["by_d"][str(d)] = res
        del eng, wu, wi
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
