#!/usr/bin/env python3
"""What the adjusted score A(u, i) = fmaf(S(u, i), scale[i], offset[i]) costs at the Yelp shape (U = 60,000 users, I =
123,000 items, the Seen / test rows / held-out sets of tools/half_retrieval_probe.py), in one process, at d = 32 and 64 on
fp32 tables and d = 128 on fp16 tables.  Per call -- topk_items K = 20 over all users, full_rank over 10,000 rows,
user_ranks over the period's held-out sets:

  adjusted     the call with adjust= (random scales in [0.25, 4] and randn offsets)
  unadjusted   the same build's call without terms, alternated with it: the overhead of the terms
  torch        what a user would write instead (topk_items and full_rank): chunked matmul, mul_ / add_ with the per-item
               vectors, Seen masked with index_put_, then topk or a compare, as tools/full_rank_probe.py does for the bare
               score; alternated with the adjusted call.  (user_ranks has no torch route here: tools/user_rank_probe.py
               measured the bare one.)

Plus similar_items (cosine, top-20, self excluded) for the whole catalogue, in chunks of 60,000 queries.
HIP events around each call after warm-up; medians, minima and the interquartile spread.  One JSON line (and --out).
usage: python tools/item_score_probe.py [--d 32,64,128] [--reps 10] [--out f.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from half_retrieval_probe import CHUNK, I, K, KS, N_HELD, N_ROWS, U, alternate, chunk_masks, stats, timed   # noqa: E402
from sml_amd import synth                                                                                  # noqa: E402
from sml_amd.engine import HipEngine                                                                       # noqa: E402
from sml_amd.mf import MFbasemode                                                                          # noqa: E402
from sml_amd.retrieval import SeenItems, held_out, nonempty_users                                          # noqa: E402


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
    _, test = synth.sample_period(np.random.RandomState(2010), N_ROWS, U, I, neg=1)
    _, held = synth.sample_period(np.random.RandomState(2005), N_HELD, U, I, neg=1)
    h_users, pos_off, pos_items = nonempty_users(held_out(held, U, I))
    off, items = seen.host()
    csr = seen.device(dev)
    rows = torch.from_numpy(test[:, :2].copy()).to(dev)
    users = torch.arange(U, device=dev)
    row_masks = chunk_masks(off, items, test[:, 0], dev)
    user_masks = chunk_masks(off, items, np.arange(U), dev)
    rng = np.random.RandomState(12)
    scale = torch.from_numpy(rng.uniform(0.25, 4.0, I).astype(np.float32)).to(dev)
    offset = torch.from_numpy(rng.randn(I).astype(np.float32)).to(dev)
    ninf = torch.tensor(-float("inf"), device=dev)
    result = {"tool": "item_score_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "rows": N_ROWS, "k": K,
              "held_out_users": int(len(h_users)), "seen_pairs": int(len(seen)), "reps": args.reps, "by_d": {}}
    for d in [int(x) for x in args.d.split(",") if x]:
        g = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=g) * 0.3).half().to(dev)
        wi = (torch.randn(I, d, generator=g) * 0.3).half().to(dev)
        if d != 128:
            wu, wi = wu.float(), wi.float()
        eng = HipEngine(dev, d, 256)
        adj = eng.item_adjust(I, scale, offset)
        sc, of = (scale, offset) if d != 128 else (scale.half(), offset.half())

        def torch_topk():
            out_i, out_s = [], []
            for c, (mr, mi) in zip(range(0, U, CHUNK), user_masks):
                s = wu[c:c + CHUNK] @ wi.T
                s.mul_(sc).add_(of)
                s.index_put_((mr, mi), ninf.to(s.dtype))
                v, ix = torch.topk(s, K, dim=1)
                out_i.append(ix)
                out_s.append(v)
            return torch.cat(out_i), torch.cat(out_s)

        def torch_rank():
            out = []
            for c, (mr, mi) in zip(range(0, N_ROWS, CHUNK), row_masks):
                r = rows[c:c + CHUNK]
                s = wu[r[:, 0]] @ wi.T
                s.mul_(sc).add_(of)
                sp = s.gather(1, r[:, 1:2])
                s.index_put_((mr, mi), ninf.to(s.dtype))
                out.append((s > sp).sum(1))
            return torch.cat(out)

        calls = {"topk_items": (lambda a: eng.topk_items(wu, wi, users, K, csr, adjust=a), torch_topk),
                 "full_rank": (lambda a: eng.full_rank(wu, wi, rows, csr, adjust=a), torch_rank),
                 "user_ranks": (lambda a: eng.user_ranks(wu, wi, h_users, pos_off, pos_items, csr, KS, adjust=a), None)}
        res = {"dtype": "fp16" if d == 128 else "fp32"}
        for name, (fn, torch_fn) in calls.items():
            ta, tb, _, _ = alternate(lambda: fn(adj), lambda: fn(None), args.reps, args.warmup, dev)
            sa, sb = stats(ta), stats(tb)
            entry = {"adjusted": sa, "unadjusted": sb, "adjusted_over_unadjusted": round(sa["ms"] / sb["ms"], 3)}
            if torch_fn is not None:
                ta, tt, out_a, out_t = alternate(lambda: fn(adj), torch_fn, args.reps, args.warmup, dev)
                sa2, st = stats(ta), stats(tt)
                entry.update(adjusted_beside_torch=sa2, torch=st, torch_over_adjusted=round(st["ms"] / sa2["ms"], 2))
                if name == "full_rank":          # (fp32: matmul sums in another order; fp16: the torch route rounds scores to half)
                    entry["ranks_equal_frac"] = round(float((out_a.long() == out_t).float().mean()), 5)
                else:
                    entry["lists_equal_frac"] = round(float((out_a[0] == out_t[0]).all(1).float().mean()), 5)
            res[name] = entry
        # similar items for the whole catalogue: the item table on both sides, cosine, self excluded
        mf = MFbasemode(1, 1, d)
        mf.user_num, mf.item_num = U, I
        mf.item_laten = torch.nn.Embedding.from_pretrained(wi, freeze=True)
        mf.user_laten = torch.nn.Embedding.from_pretrained(wu, freeze=True)
        mf._sml_engine = eng
        every = torch.arange(I, device=dev)

        def similar():
            return [mf.similar_items(every[c:c + U], topK=K) for c in range(0, I, U)]
        ts = []
        for r in range(args.warmup + args.reps):
            t, _ = timed(similar, dev)
            if r >= args.warmup:
                ts.append(t)
        res["similar_items_whole_catalogue"] = dict(stats(ts), queries=I)
        result["by_d"][str(d)] = res
        del eng, wu, wi, mf
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
