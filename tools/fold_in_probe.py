#!/usr/bin/env python3
"""What the closed-form fold-in costs (HipEngine.gram / als_solve, sml_amd.als) at the Yelp shape: U = 60,000 users, I = 123,000
items, a Seen of the Yelp history's size (five periods of 200,000 Zipf interactions, as tools/ivf_probe.py builds it), d = 32 / 64
on fp32 and fp16 tables.  One run records, per (d, element type),

  gram        HipEngine.gram over the item table and over the user table
  solve       HipEngine.als_solve for all users against the item table, and for all items against the user table over the
              transposed set; the user call again on the light rows (1 .. 5 members) and on the others alone, to say which
              kind the time goes to; the fp64 fma the definition asks of a row (members * d (d + 1) / 2 + about d^3 / 6 + d^2) over
              the time, beside the fma the wavefront actually issues (every lane runs every step of its row-per-lane layout)
  sweep       one full sml_amd.als.fit sweep (two Gram matrices, two solves, the transposed set, two objectives)
  torch       the same user half-step in torch: a chunked gather of member rows, bmm into an [n, d, d] float64 batch,
              torch.linalg.solve -- its time, its peak extra memory, and the largest difference of its rows from the kernel's

nine rounds that run every route once, in turn, after two warm-up rounds; medians, minima, interquartile spread (the torch route
three rounds).  Not measured: trained (non-random) tables, recall of folded-in new users on real periods, shapes beyond this one;
serving two rows per wavefront at d = 32 was not built, so there is no reading of it.  One JSON line on stdout (and --out).
usage: python tools/fold_in_probe.py [--d 32,64] [--reps 9] [--out profiles/r22_fold_in_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from candidates_probe import rounds                              # noqa: E402
from half_retrieval_probe import I, U, stats, timed              # noqa: E402
from sml_amd import als, synth                                   # noqa: E402
from sml_amd.engine import HipEngine                             # noqa: E402
from sml_amd.mf import MFbasemode                                # noqa: E402
from sml_amd.retrieval import SeenItems                          # noqa: E402

PAIR_CHUNK = 16384       # torch route: member rows per outer-product block ([16384, 64, 64] float64 = 0.5 GB)
REG, ALPHA0 = 0.1, 0.1


def note(msg):
    sys.stderr.write("[fold_in_probe] %s\n" % msg)
    sys.stderr.flush()


def torch_route(out, other, gram, off, items, reg, alpha0):
    n, d = out.shape
    lens = off[1:] - off[:-1]
    owner = torch.repeat_interleave(torch.arange(n, device=out.device), lens)
    a = (alpha0 * gram + reg * torch.eye(d, device=out.device, dtype=torch.float64)).expand(n, d, d).contiguous()
    rhs = torch.zeros(n, d, device=out.device, dtype=torch.float64)
    for c0 in range(0, owner.shape[0], PAIR_CHUNK):
        y = other.index_select(0, items[c0:c0 + PAIR_CHUNK].long()).double()
        o = owner[c0:c0 + PAIR_CHUNK]
        a.index_add_(0, o, torch.bmm(y.unsqueeze(2), y.unsqueeze(1)))
        rhs.index_add_(0, o, y)
    return torch.linalg.solve(a, rhs).to(out.dtype)


def peak_extra_mb(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)


def fma_counts(lens, d):
    """(the fma the definition asks of these rows, the fma lanes the kernel issues for them): rows with members only."""
    lens = lens[lens > 0].double()
    asked = lens.sum() * d * (d + 1) / 2 + lens.shape[0] * (d * (d - 1) * (d - 2) / 6.0 + d * (d - 1) / 2.0 + d * (d - 1))
    issued = 64.0 * (lens.sum() * d + lens.shape[0] * (d * (d - 1) / 2.0 + d + d * (d - 1) / 2.0))
    return float(asked), float(issued)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch_reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    by_user = seen.device(dev)
    lens_u = by_user[0][1:] - by_user[0][:-1]
    result = {"tool": "fold_in_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "seen_pairs": int(len(seen)),
              "reg": REG, "alpha0": ALPHA0, "reps": args.reps, "torch_reps": args.torch_reps, "by_case": {},
              "users_by_members": {"0": int((lens_u == 0).sum()), "1..5": int(((lens_u > 0) & (lens_u <= 5)).sum()),
                                   "6..64": int(((lens_u > 5) & (lens_u <= 64)).sum()), ">64": int((lens_u > 64).sum()),
                                   "max": int(lens_u.max())},
              "d32_two_rows_per_wave": "not built, not measured: the upper half of the wave idles at d = 32",
              "not_measured": ["trained (non-random) tables", "recall of folded-in new users on real periods",
                               "shapes beyond the Yelp one"]}
    light = torch.nonzero((lens_u > 0) & (lens_u <= 5)).reshape(-1)
    heavy = torch.nonzero(lens_u > 5).reshape(-1)
    for d in [int(x) for x in args.d.split(",") if x]:
        eng = HipEngine(dev, d, 256)
        by_item = als.transpose_sets(by_user, U, I, eng)
        lens_i = by_item[0][1:] - by_item[0][:-1]
        for dtype in (torch.float32, torch.float16):
            name = "d%d_%s" % (d, "fp32" if dtype == torch.float32 else "fp16")
            note(name)
            gd = torch.Generator().manual_seed(d)
            wu = (torch.randn(U, d, generator=gd) * 0.3).to(dev).to(dtype)
            wi = (torch.randn(I, d, generator=gd) * 0.3).to(dev).to(dtype)
            gi, gu = eng.gram(wi), eng.gram(wu)
            out_u, out_i = wu.clone(), wi.clone()
            model = MFbasemode(U, I, d).to(dev).to(dtype)
            fns = {"gram_items": lambda: eng.gram(wi), "gram_users": lambda: eng.gram(wu),
                   "solve_users": lambda: eng.als_solve(wi, gi, by_user, out_u, reg=REG, alpha0=ALPHA0),
                   "solve_items": lambda: eng.als_solve(wu, gu, by_item, out_i, reg=REG, alpha0=ALPHA0),
                   "solve_users_light_rows": lambda: eng.als_solve(wi, gi, by_user, out_u, rows=light, reg=REG, alpha0=ALPHA0),
                   "solve_users_other_rows": lambda: eng.als_solve(wi, gi, by_user, out_u, rows=heavy, reg=REG, alpha0=ALPHA0),
                   "fit_one_sweep": lambda: als.fit(model, by_user, sweeps=1, reg=REG, alpha0=ALPHA0, engine=eng)}
            r = rounds(fns, args.reps, args.warmup, dev)
            status = eng.als_solve(wi, gi, by_user, out_u, reg=REG, alpha0=ALPHA0)
            r["solve_users"]["status_counts"] = torch.bincount(status.long(), minlength=3).tolist()
            for key, lens in (("solve_users", lens_u), ("solve_items", lens_i), ("solve_users_light_rows", lens_u[light]),
                              ("solve_users_other_rows", lens_u[heavy])):
                asked, issued = fma_counts(lens, d)
                ms = r[key]["ms"]
                r[key].update(rows=int(lens.shape[0]), pairs=int(lens.sum()), asked_fp64_gfma_per_s=round(asked / ms / 1e6, 1),
                              issued_fp64_gfma_lanes_per_s=round(issued / ms / 1e6, 1))
            tr = lambda: torch_route(out_u, wi, gi, by_user[0], by_user[1], REG, ALPHA0)
            for _ in range(1):
                timed(tr, dev)
            ts = []
            for _ in range(args.torch_reps):
                t, ref = timed(tr, dev)
                ts.append(t)
            has = lens_u > 0
            r["torch_users"] = dict(stats(ts), peak_extra_mb=peak_extra_mb(tr, dev),
                                    max_abs_diff_from_kernel=float((ref[has].double() - out_u[has].double()).abs().max()))
            del ref
            result["by_case"][name] = r
            del wu, wi, out_u, out_i, model
            torch.cuda.empty_cache()
        del eng
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
