#!/usr/bin/env python3
"""The fp32 retrieval entry points of the in-tree libsml_hip.so against ANOTHER build of the library (e.g. the previous
commit's, built by hand into tools/_ab/), alternating in one process at the Yelp shape of tools/half_retrieval_probe.py:
full_rank over 10,000 rows, topk_items K = 20 over all 60,000 users, user_ranks over the held-out sets, d = 32 and 64
(--half_d 128: the _f16 entry points on fp16 tables at those widths as well).  --allow: every call with the contiguous
10 % filter of tools/item_filter_probe.py (the _filtered entry points); --adjust: with the terms of
tools/item_score_probe.py (the _adjusted ones); neither: allow=None, adjust=None.
Medians, minima and the interquartile spread of the alternated repetitions; outputs compared byte for byte.  The other
build may be older than the header: only the symbols it exports are bound.
usage: python tools/retrieval_ab.py <other.so> [--d 32,64] [--half_d 128] [--allow] [--adjust] [--reps 20] [--out file.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from half_retrieval_probe import I, K, KS, N_HELD, N_ROWS, U, alternate, same, stats    # noqa: E402
from sml_amd import _lib, synth                                                         # noqa: E402
from sml_amd.engine import HipEngine                                                    # noqa: E402
from sml_amd.retrieval import ItemFilter, SeenItems, held_out, nonempty_users           # noqa: E402


def load_other(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--d", default="32,64")
    ap.add_argument("--half_d", default="", help="widths measured on fp16 tables (the _f16 entry points)")
    ap.add_argument("--allow", action="store_true", help="filter every call to the last tenth of the item ids")
    ap.add_argument("--adjust", action="store_true", help="per-item terms on every call: scales in [0.25, 4], randn offsets")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    other = load_other(args.other)
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
    allow = ItemFilter(I).allow(np.arange(I - I // 10, I)).device(dev) if args.allow else None
    rng = np.random.RandomState(12)
    scale = torch.from_numpy(rng.uniform(0.25, 4.0, I).astype(np.float32)).to(dev)
    offset = torch.from_numpy(rng.randn(I).astype(np.float32)).to(dev)
    result = {"tool": "retrieval_ab", "device": torch.cuda.get_device_name(dev), "other": os.path.basename(args.other), "U": U, "I": I,
              "rows": N_ROWS, "k": K, "held_out_users": int(len(h_users)), "reps": args.reps, "dtype": "fp32", "allow": args.allow,
              "adjust": args.adjust, "by_d": {}}
    widths = [(int(x), False) for x in args.d.split(",") if x] + [(int(x), True) for x in args.half_d.split(",") if x]
    for d, half in widths:
        g = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=g) * 0.3).half().to(dev)               # the probe's tables (fp32: widened)
        wi = (torch.randn(I, d, generator=g) * 0.3).half().to(dev)
        if not half:
            wu, wi = wu.float(), wi.float()
        engs = {"tree": HipEngine(dev, d, 256), "other": HipEngine(dev, d, 256, lib=other)}
        adj = engs["tree"].item_adjust(I, scale, offset) if args.adjust else None
        calls = {"full_rank": lambda e: e.full_rank(wu, wi, rows, csr, allow=allow, adjust=adj),
                 "topk_items": lambda e: e.topk_items(wu, wi, users, K, csr, allow=allow, adjust=adj),
                 "user_ranks": lambda e: e.user_ranks(wu, wi, h_users, pos_off, pos_items, csr, KS, allow=allow, adjust=adj)}
        res = {}
        for name, fn in calls.items():
            ta, tb, oa, ob = alternate(lambda: fn(engs["tree"]), lambda: fn(engs["other"]), args.reps, args.warmup, dev)
            sa, sb = stats(ta), stats(tb)
            res[name] = {"tree": sa, "other": sb, "tree_over_other": round(sa["ms"] / sb["ms"], 3), "same_bytes": same(oa, ob)}
        result["by_d"][str(d) + ("_fp16" if half else "")] = res
        del engs
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
