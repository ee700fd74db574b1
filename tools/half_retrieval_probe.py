#!/usr/bin/env python3
"""Full-catalogue retrieval on fp16 tables at the Yelp shape (U = 60,000 users, I = 123,000 items; Seen = the train pairs
of 5 synthetic periods, test rows and held-out sets from the next period, all from sml_amd.synth.sample_period), in one
process:

  d = 32, 64   the _f16 entry points on fp16 tables against the fp32 entry points on `.float()` copies of the same tables
               (same MFMA work, half the table bytes, plus the widening): full_rank over 10,000 rows, topk_items K = 20
               over all users, user_ranks over the period's held-out sets.  Outputs are compared byte for byte.
  d = 128      the _f16 entry points (the only form of d = 128) against the unfused torch route of full_rank_probe.py on
               the same fp16 tables: chunked half matmul + Seen mask + strict compare / torch.topk; user_ranks against
               full_rank over the distinct held-out pairs, as user_rank_probe.py does.
  --scale_items N   one reading: topk_items K = --scale_k (20) of all users over N items at d = 128 fp16.  The engine
               chunks the users when the candidate scratch exceeds HipEngine.TOPK_SCRATCH_BYTES: at N = 1,000,000 that
               is not the case at K = 20 (77 MB) and is at K = 128 (two calls); "calls" in the output says which.

HIP events around each call after warm-up, repetitions alternated between the two routes; medians, minima and the
interquartile spread are reported.  FLOPs come from the shapes (2 d per scored pair).  One JSON line on stdout (and --out).
usage: python tools/half_retrieval_probe.py [--d 32,64,128] [--reps 20] [--scale_items 1000000 [--scale_k 128]] [--no_torch] [--out f.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd import synth                                            # noqa: E402
from sml_amd.engine import HipEngine                                 # noqa: E402
from sml_amd.retrieval import SeenItems, held_out, nonempty_users    # noqa: E402

PEAK_TF = 157.3          # fp32 MFMA, MI355X
U, I, N_ROWS, N_HELD, K = 60000, 123000, 10000, 75000, 20
KS = (20, 10, 5)
CHUNK = 2048             # torch route: rows / users per matmul (a [2048, 123000] fp16 score block = 0.5 GB)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def chunk_masks(off, items, users, dev):
    out = []
    for c0 in range(0, len(users), CHUNK):
        us = users[c0:c0 + CHUNK]
        lens = off[us + 1] - off[us]
        r = np.repeat(np.arange(len(us)), lens)
        i = np.concatenate([items[off[u]:off[u + 1]] for u in us]) if lens.sum() else np.zeros(0, np.int32)
        out.append((torch.from_numpy(r).to(dev), torch.from_numpy(i.astype(np.int64)).to(dev)))
    return out


def stats(ts):
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"ms": round(float(med), 4), "min_ms": round(float(min(ts)), 4), "iqr_ms": round(float(q3 - q1), 4)}


def alternate(fa, fb, reps, warmup, dev):
    for _ in range(warmup):
        timed(fa, dev)
        timed(fb, dev)
    ta, tb = [], []
    out_a = out_b = None
    for _ in range(reps):
        t, out_a = timed(fa, dev)
        ta.append(t)
        t, out_b = timed(fb, dev)
        tb.append(t)
    return ta, tb, out_a, out_b


def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return all(same(x, y) for x, y in zip(a, b))
    return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))


def rate(flop, ms):
    return {"tflops": round(flop / ms / 1e9, 1), "pct_fp32_mfma_peak": round(100.0 * flop / ms / 1e9 / PEAK_TF, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64,128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale_items", type=int, default=0)
    ap.add_argument("--scale_k", type=int, default=K, help="K of the --scale_items reading (128: the user chunking engages)")
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route at d = 128 (profiling runs)")
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
    off, items = seen.host()
    csr = seen.device(dev)
    rows = torch.from_numpy(test[:, :2].copy()).to(dev)
    users = torch.arange(U, device=dev)
    pairs = torch.from_numpy(np.stack([np.repeat(h_users, np.diff(pos_off)), pos_items.astype(np.int64)], 1)).to(dev)
    result = {"tool": "half_retrieval_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "rows": N_ROWS, "k": K,
              "held_out_users": int(len(h_users)), "held_out_pairs": int(len(pos_items)), "seen_pairs": int(len(seen)),
              "reps": args.reps, "peak_tf_fp32_mfma": PEAK_TF, "by_d": {}}
    neg_inf = None
    for d in [int(x) for x in args.d.split(",") if x]:
        g = torch.Generator().manual_seed(d)
        hu = (torch.randn(U, d, generator=g) * 0.3).half().to(dev)
        hi = (torch.randn(I, d, generator=g) * 0.3).half().to(dev)
        eng = HipEngine(dev, d, 256)
        calls = {"full_rank": (lambda wu, wi: eng.full_rank(wu, wi, rows, csr), N_ROWS),
                 "topk_items": (lambda wu, wi: eng.topk_items(wu, wi, users, K, csr), U),
                 "user_ranks": (lambda wu, wi: eng.user_ranks(wu, wi, h_users, pos_off, pos_items, csr, KS), len(h_users))}
        res = {}
        if d != 128:
            fu, fi = hu.float(), hi.float()
            for name, (fn, passes) in calls.items():
                ta, tb, oa, ob = alternate(lambda: fn(hu, hi), lambda: fn(fu, fi), args.reps, args.warmup, dev)
                flop = 2.0 * passes * I * d
                sa, sb = stats(ta), stats(tb)
                res[name] = {"fp16": dict(sa, **rate(flop, sa["ms"])), "fp32": dict(sb, **rate(flop, sb["ms"])),
                             "fp16_over_fp32": round(sa["ms"] / sb["ms"], 3), "same_bytes": same(oa, ob),
                             "catalogue_passes": int(passes)}
            del fu, fi
        else:
            if neg_inf is None:
                neg_inf = torch.tensor(-float("inf"), device=dev, dtype=torch.float16)
                row_masks = chunk_masks(off, items, test[:, 0], dev)
                user_masks = chunk_masks(off, items, np.arange(U), dev)

            def torch_rank():
                out = []
                for c, (mr, mi) in zip(range(0, N_ROWS, CHUNK), row_masks):
                    r = rows[c:c + CHUNK]
                    s = hu[r[:, 0]] @ hi.T
                    sp = s.gather(1, r[:, 1:2])
                    s.index_put_((mr, mi), neg_inf)
                    out.append((s > sp).sum(1))
                return torch.cat(out)

            def torch_topk():
                out_i, out_s = [], []
                for c, (mr, mi) in zip(range(0, U, CHUNK), user_masks):
                    s = hu[c:c + CHUNK] @ hi.T
                    s.index_put_((mr, mi), neg_inf)
                    v, ix = torch.topk(s, K, dim=1)
                    out_i.append(ix)
                    out_s.append(v)
                return torch.cat(out_i), torch.cat(out_s)

            others = {"full_rank": ("torch", torch_rank), "topk_items": ("torch", torch_topk),
                      "user_ranks": ("full_rank_pairs", lambda: eng.full_rank(hu, hi, pairs, csr))}
            for name, (fn, passes) in calls.items():
                other_name, other = others[name]
                if args.no_torch and other_name == "torch":
                    other = lambda: None                                # noqa: E731
                ta, tb, oa, ob = alternate(lambda: fn(hu, hi), other, args.reps, args.warmup, dev)
                flop = 2.0 * passes * I * d
                sa, sb = stats(ta), stats(tb)
                res[name] = {"fp16": dict(sa, **rate(flop, sa["ms"])), "catalogue_passes": int(passes),
                             "floor_ms_at_fp32_mfma_peak": round(flop / PEAK_TF / 1e9, 3)}
                if not (args.no_torch and other_name == "torch"):
                    res[name][other_name] = sb
                    res[name]["speedup"] = round(sb["ms"] / sa["ms"], 2)
                if name == "user_ranks":
                    res[name]["above_equals_full_rank"] = bool(torch.equal(oa["above"], ob))
                elif ob is not None and name == "full_rank":
                    # (the torch route scores in fp16 with the library's own accumulation: ranks agree only roughly)
                    res[name]["ranks_equal_frac_vs_torch_half"] = round(float((oa.long() == ob).float().mean()), 5)
        result["by_d"][str(d)] = res
        del eng, hu, hi
    if args.scale_items:
        d, n_item, k = 128, int(args.scale_items), int(args.scale_k)
        g = torch.Generator().manual_seed(7)
        hu = (torch.randn(U, d, generator=g) * 0.3).half().to(dev)
        hi = torch.empty(n_item, d, device=dev, dtype=torch.float16)
        for c0 in range(0, n_item, 1 << 18):
            hi[c0:c0 + (1 << 18)] = (torch.randn(min(1 << 18, n_item - c0), d, generator=g) * 0.3).half().to(dev)
        eng = HipEngine(dev, d, 256)
        timed(lambda: eng.topk_items(hu, hi, users[:4096], k), dev)               # warm-up on a slice of the users
        ms, _ = timed(lambda: eng.topk_items(hu, hi, users, k), dev)
        flop = 2.0 * U * n_item * d
        total, cap = int(eng.lib.sml_topk_scratch_bytes(eng._ctx, U, k, n_item)), HipEngine.TOPK_SCRATCH_BYTES
        result["scale"] = dict({"d": d, "dtype": "fp16", "users": U, "items": n_item, "k": k, "ms_single_reading": round(ms, 2),
                                "item_table_mb": round(n_item * d * 2 / 1e6, 1),
                                "calls": 1 if total <= cap else int(-(-U // max(1, U * cap // total)))},
                               **rate(flop, ms))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
