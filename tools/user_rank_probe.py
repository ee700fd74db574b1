#!/usr/bin/env python3
"""Per-user ranking of held-out sets at the Yelp shape (U = 60,000 users, I = 123,000 items, d = 32 and 64; Seen = the
train pairs of 5 synthetic periods, held out = the 75,000 pairs of the next period, both from sml_amd.synth.sample_period):

  (a) HipEngine.user_ranks over the users with a held-out item (one catalogue pass per user, metrics at K = 20, 10, 5)
  (b) HipEngine.full_rank over the distinct (user, item) pairs of the period (one catalogue pass per pair)
  (c) HipEngine.full_rank over all rows of the period (one pass per row)

HIP events around each call after warm-up, repetitions alternated between the three routes; the median is reported.
`above` of (a) is checked against the ranks of (b).  FLOPs count the scored (user, item) pairs, 2 d each.  One JSON line
on stdout (and in --out).
usage: python tools/user_rank_probe.py [--d 32,64] [--reps 20] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd import synth                                   # noqa: E402
from sml_amd.engine import HipEngine                        # noqa: E402
from sml_amd.retrieval import SeenItems, held_out, nonempty_users    # noqa: E402

PEAK_TF = 157.3          # fp32 MFMA, MI355X
U, I, N_ROWS = 60000, 123000, 75000
KS = (20, 10, 5)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    _, test = synth.sample_period(np.random.RandomState(2005), N_ROWS, U, I, neg=1)
    sets = held_out(test, U, I)
    users, pos_off, pos_items = nonempty_users(sets)
    m = np.diff(pos_off)
    csr = seen.device(dev)
    rows = torch.from_numpy(test[:, :2].copy()).to(dev)
    pairs = torch.from_numpy(np.stack([np.repeat(users, m), pos_items.astype(np.int64)], 1)).to(dev)
    result = {"tool": "user_rank_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "rows": N_ROWS,
              "pairs": int(len(pos_items)), "users": int(len(users)), "max_m": int(m.max()), "p99_m": float(np.percentile(m, 99)),
              "seen_pairs": int(len(seen)), "ks": list(KS), "reps": args.reps, "peak_tf_fp32_mfma": PEAK_TF, "by_d": {}}
    for d in [int(x) for x in args.d.split(",")]:
        g = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=g) * 0.3).to(dev)
        wi = (torch.randn(I, d, generator=g) * 0.3).to(dev)
        eng = HipEngine(dev, d, 256)
        routes = (("user_ranks", lambda: eng.user_ranks(wu, wi, users, pos_off, pos_items, csr, KS), len(users)),
                  ("full_rank_pairs", lambda: eng.full_rank(wu, wi, pairs, csr), len(pos_items)),
                  ("full_rank_rows", lambda: eng.full_rank(wu, wi, rows, csr), N_ROWS))
        for _ in range(args.warmup):
            for _, fn, _ in routes:
                timed(fn, dev)
        times = {name: [] for name, _, _ in routes}
        outs = {}
        for _ in range(args.reps):
            for name, fn, _ in routes:
                t, outs[name] = timed(fn, dev)
                times[name].append(t)
        res = {}
        for name, _, passes in routes:
            ms = float(np.median(times[name]))
            flop = 2.0 * passes * I * d
            res[name] = {"ms": round(ms, 4), "min_ms": round(min(times[name]), 4), "catalogue_passes": int(passes),
                         "us_per_1000_passes": round(1000.0 * ms / passes * 1000.0, 2),
                         "tflops": round(flop / ms / 1e9, 1), "pct_mfma_peak": round(100.0 * flop / ms / 1e9 / PEAK_TF, 1)}
        res["above_equals_full_rank"] = bool(torch.equal(outs["user_ranks"]["above"], outs["full_rank_pairs"]))
        res["speedup_vs_pairs"] = round(res["full_rank_pairs"]["ms"] / res["user_ranks"]["ms"], 2)
        res["speedup_vs_rows"] = round(res["full_rank_rows"]["ms"] / res["user_ranks"]["ms"], 2)
        result["by_d"][str(d)] = res
        del eng
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
