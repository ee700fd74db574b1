#!/usr/bin/env python3
"""Deep lists (HipEngine.topk_deep, sml_topk_deep) at the Yelp shape of tools/half_retrieval_probe.py: U = 60,000 users,
I = 123,000 items, the same Seen, fp32 d = 32 / 64 and fp16 d = 128, in one process:

  depth   topk_deep at k = 20, 64, 100, 128, 256, 512, 1024 over all users; for k <= 128 alternated with topk_items of ANOTHER
          build of the library (the parent commit's, built by hand into tools/_ab/ and loaded the way tools/retrieval_ab.py loads
          it), outputs compared byte for byte.  `deep_from` is the smallest probed k from which the deep call's median is below
          the other build's topk_items minimum at every width (129: none) -- the rule behind sml_amd.retrieval.DEEP_FROM.
  pool    recommend(diversify=0.7, pool=128, topK=20) end to end, this build (with DEEP_FROM as committed and with the pool
          forced through the deep kernels) against the other build.
  torch   the chunked torch route (matmul + Seen mask + topk) at k = 500, with its peak extra memory.
  --passes K   nothing but --reps topk_deep calls at k = K per width: the target of a `rocprofv3 --kernel-trace --stats` run,
          whose per-kernel table times the count, pick, collect and sort launches separately
          (profiles/r20_deep_topk_kernel_stats.csv).
  --trace F    no GPU work: read that run's kernel trace (`*_kernel_trace.csv`) and print, per kernel, the median / min / max
          microseconds of every launch of a call in launch order -- the four counting passes (shift 24, 16, 8, 0) and the four
          picks apart, the collecting walk apart from the tie walk (profiles/r20_deep_topk_passes.json).

HIP events around each call after warm-up, repetitions alternated; medians, minima and the interquartile spread.  One JSON
line on stdout (and --out).
usage: python tools/deep_topk_probe.py <other.so> [--d 32,64] [--half_d 128] [--reps 5] [--passes K] [--trace F] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from half_retrieval_probe import CHUNK, I, U, alternate, chunk_masks, same, stats, timed       # noqa: E402
from retrieval_ab import load_other                                                            # noqa: E402
from sml_amd import retrieval, synth                                                           # noqa: E402
from sml_amd.engine import HipEngine                                                           # noqa: E402
from sml_amd.mf import MFbasemode                                                              # noqa: E402
from sml_amd.retrieval import SeenItems                                                        # noqa: E402

DEPTHS = (20, 64, 100, 128, 256, 512, 1024)


def repeat(fn, reps, warmup, dev):
    for _ in range(warmup):
        timed(fn, dev)
    ts, out = [], None
    for _ in range(reps):
        t, out = timed(fn, dev)
        ts.append(t)
    return ts, out


def torch_topk(wu, wi, masks, k):
    items, scores = [], []
    for q, c0 in enumerate(range(0, wu.shape[0], CHUNK)):
        s = wu[c0:c0 + CHUNK] @ wi.T
        r, i = masks[q]
        s[r, i] = float("-inf")
        v, ix = torch.topk(s, k, dim=1)
        items.append(ix)
        scores.append(v)
    return torch.cat(items), torch.cat(scores)


def summarize_trace(path):
    """{kernel: {"launch_<q>": {us, min_us, max_us, calls}}}: the q-th launch of each kernel inside one sml_topk_deep call."""
    import csv
    import re
    per_call = {"k_deep_count": 4, "k_deep_pick": 4, "k_deep_collect": 2, "k_deep_sort": 1}
    rows = list(csv.DictReader(open(path)))
    by_name = {}
    for r in rows:
        m = re.search(r"k_deep_[a-z]+", r["Kernel_Name"])
        if not m:
            continue
        width = re.search(r"k_deep_[a-z]+(?:<|ILi)(\d+)(?:, |E)(float|half|f|DF16_)", r["Kernel_Name"])
        name = m.group(0) + ("<%s, %s>" % (width.group(1), {"f": "float", "DF16_": "half"}.get(width.group(2), width.group(2))) if width else "")
        by_name.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for name, spans in sorted(by_name.items()):
        spans.sort()
        n = per_call[name.split("<")[0]]
        out[name] = {}
        for q in range(n):
            us = [(e - s) / 1000.0 for s, e in spans[q::n]]
            if not us:
                continue
            out[name]["launch_%d" % q] = {"us": round(float(np.median(us)), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
                                          "calls": len(us)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", nargs="?", default=None)
    ap.add_argument("--d", default="32,64")
    ap.add_argument("--half_d", default="128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        line = json.dumps({"tool": "deep_topk_probe --trace", "launches_per_call": "count and pick: shift 24, 16, 8, 0; collect: the "
                           "collecting walk, then the tie walk", "kernels": summarize_trace(args.trace)})
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    dev = torch.device("cuda:0")
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(2000 + p), 200000, U, I, neg=1)
        seen.add(train)
    csr = seen.device(dev)
    users = torch.arange(U, device=dev)
    result = {"tool": "deep_topk_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "reps": args.reps,
              "other": os.path.basename(args.other) if args.other else None, "deep_from_committed": retrieval.DEEP_FROM, "by_d": {}}
    other = load_other(args.other) if args.other else None
    widths = [(int(x), False) for x in args.d.split(",") if x] + [(int(x), True) for x in args.half_d.split(",") if x]
    wins = {k: True for k in DEPTHS if k <= 128}
    for d, half in widths:
        g = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=g) * 0.3).half().to(dev)               # half_retrieval_probe's tables (fp32: widened)
        wi = (torch.randn(I, d, generator=g) * 0.3).half().to(dev)
        if not half:
            wu, wi = wu.float(), wi.float()
        tree = HipEngine(dev, d, 256)
        if args.passes:
            ts, _ = repeat(lambda: tree.topk_deep(wu, wi, users, args.passes, csr), args.reps, args.warmup, dev)
            result["by_d"][str(d) + ("_fp16" if half else "")] = {"passes_k": args.passes, "topk_deep": stats(ts)}
            continue
        res = {"depth": {}}
        old = HipEngine(dev, d, 256, lib=other) if other is not None else None
        for k in DEPTHS:
            if k <= 128 and old is not None:
                reps = args.reps if k <= 64 else max(2, args.reps // 2)          # (the other build's deep lists take a second each)
                ta, tb, oa, ob = alternate(lambda: tree.topk_deep(wu, wi, users, k, csr), lambda: old.topk_items(wu, wi, users, k, csr),
                                           reps, args.warmup, dev)
                sa, sb = stats(ta), stats(tb)
                res["depth"][str(k)] = {"topk_deep": sa, "other_topk_items": sb, "same_bytes": same(oa[:2], ob)}
                wins[k] = wins[k] and sa["ms"] < sb["min_ms"]
            else:
                ts, _ = repeat(lambda: tree.topk_deep(wu, wi, users, k, csr), args.reps, args.warmup, dev)
                res["depth"][str(k)] = {"topk_deep": stats(ts)}
        if old is not None:
            model = MFbasemode(U, I, d).to(dev)
            if half:
                model.half()
            with torch.no_grad():
                model.user_laten.weight.copy_(wu)
                model.item_laten.weight.copy_(wi)
            model._sml_engine = tree
            pool = lambda: model.recommend(users, 20, exclude=csr, diversify=0.7, pool=128)      # noqa: E731

            def with_engine(eng, deep_from):
                def run():
                    keep = retrieval.DEEP_FROM
                    model._sml_engine, retrieval.DEEP_FROM = eng, deep_from
                    try:
                        return pool()
                    finally:
                        model._sml_engine, retrieval.DEEP_FROM = tree, keep
                return run
            reps = max(2, args.reps // 2)
            ta, tb, oa, ob = alternate(with_engine(tree, retrieval.DEEP_FROM), with_engine(old, 129), reps, args.warmup, dev)
            tc, oc = repeat(with_engine(tree, 128), reps, args.warmup, dev)
            res["pool_mmr"] = {"tree": stats(ta), "other": stats(tb), "tree_pool_through_deep": stats(tc), "same_bytes": same(oa, ob) and same(oa, oc)}
        if not half or d == 128:
            off, items = seen.host()
            masks = chunk_masks(off, items, np.arange(U), dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            tt, ot = repeat(lambda: torch_topk(wu, wi, masks, 500), max(2, args.reps // 2), args.warmup, dev)
            peak = torch.cuda.max_memory_allocated(dev) - base
            td, od = repeat(lambda: tree.topk_deep(wu, wi, users, 500, csr), max(2, args.reps // 2), args.warmup, dev)
            res["torch_k500"] = {"torch": stats(tt), "topk_deep": stats(td), "torch_peak_extra_MB": round(peak / 2 ** 20, 1),
                                 "rows_with_equal_items": round(float((ot[0] == od[0]).all(1).float().mean()), 4)}
            del masks
        result["by_d"][str(d) + ("_fp16" if half else "")] = res
        del tree, old
    if other is not None and not args.passes:
        ok = [k for k in sorted(wins) if all(wins[j] for j in wins if j >= k)]
        result["deep_from"] = ok[0] if ok else 129
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
