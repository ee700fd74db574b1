#!/usr/bin/env python3
"""Full-catalogue retrieval at the Yelp shape (U = 60,000 users, I = 123,000 items, d = 32 and 64, Seen = the train
pairs of 5 synthetic periods from sml_amd.synth.sample_period), fused HIP kernels against the unfused torch route on
the same tables in the same process:

  (a) ranks of 10,000 test rows:   HipEngine.full_rank   vs  chunked matmul + Seen mask + strict compare + row sum
  (b) top-20 of all 60,000 users:  HipEngine.topk_items  vs  chunked matmul + Seen mask + torch.topk

HIP events around each call after warm-up, repetitions alternated between the two routes; the median is reported.
FLOPs and bytes come from the shapes.  One JSON line on stdout (and in --out).
usage: python tools/full_rank_probe.py [--d 32,64] [--reps 20] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd import synth                    # noqa: E402
from sml_amd.engine import HipEngine         # noqa: E402
from sml_amd.retrieval import SeenItems      # noqa: E402

PEAK_TF = 157.3          # fp32 MFMA, MI355X
U, I, N_ROWS, K = 60000, 123000, 10000, 20
CHUNK = 2048             # torch route: rows / users per matmul (a [2048, 123000] fp32 score block = 1.0 GB)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def chunk_masks(off, items, users, dev):
    """Per chunk of `users`: (row-in-chunk, item) index tensors of Seen, for the torch route's index_put_."""
    out = []
    for c0 in range(0, len(users), CHUNK):
        us = users[c0:c0 + CHUNK]
        lens = off[us + 1] - off[us]
        r = np.repeat(np.arange(len(us)), lens)
        i = np.concatenate([items[off[u]:off[u + 1]] for u in us]) if lens.sum() else np.zeros(0, np.int32)
        out.append((torch.from_numpy(r).to(dev), torch.from_numpy(i.astype(np.int64)).to(dev)))
    return out


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
    _, test = synth.sample_period(np.random.RandomState(2010), N_ROWS, U, I, neg=1)
    off, items = seen.host()
    csr = seen.device(dev)
    rows = torch.from_numpy(test[:, :2].copy()).to(dev)
    users = torch.arange(U, device=dev)
    row_masks = chunk_masks(off, items, test[:, 0], dev)
    user_masks = chunk_masks(off, items, np.arange(U), dev)
    result = {"tool": "full_rank_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "rows": N_ROWS, "k": K,
              "seen_pairs": int(len(seen)), "reps": args.reps, "peak_tf_fp32_mfma": PEAK_TF, "by_d": {}}
    for d in [int(x) for x in args.d.split(",")]:
        g = torch.Generator().manual_seed(d)
        wu = (torch.randn(U, d, generator=g) * 0.3).to(dev)
        wi = (torch.randn(I, d, generator=g) * 0.3).to(dev)
        eng = HipEngine(dev, d, 256)

        def fused_rank():
            return eng.full_rank(wu, wi, rows, csr)

        def torch_rank():
            out = []
            for c, (mr, mi) in zip(range(0, N_ROWS, CHUNK), row_masks):
                r = rows[c:c + CHUNK]
                s = wu[r[:, 0]] @ wi.T
                sp = s.gather(1, r[:, 1:2])
                s.index_put_((mr, mi), torch.tensor(-float("inf"), device=dev))
                out.append((s > sp).sum(1))
            return torch.cat(out)

        def fused_topk():
            return eng.topk_items(wu, wi, users, K, csr)

        def torch_topk():
            out_i, out_s = [], []
            for c, (mr, mi) in zip(range(0, U, CHUNK), user_masks):
                s = wu[c:c + CHUNK] @ wi.T
                s.index_put_((mr, mi), torch.tensor(-float("inf"), device=dev))
                v, ix = torch.topk(s, K, dim=1)
                out_i.append(ix)
                out_s.append(v)
            return torch.cat(out_i), torch.cat(out_s)

        res = {}
        for name, fa, fb, n_users in (("full_rank", fused_rank, torch_rank, N_ROWS), ("topk_items", fused_topk, torch_topk, U)):
            for _ in range(args.warmup):
                timed(fa, dev)
                timed(fb, dev)
            ta, tb = [], []
            for _ in range(args.reps):
                t, out_a = timed(fa, dev)
                ta.append(t)
                t, out_b = timed(fb, dev)
                tb.append(t)
            flop = 2.0 * n_users * I * d
            ma, mb = float(np.median(ta)), float(np.median(tb))
            entry = {"fused_ms": round(ma, 4), "torch_ms": round(mb, 4), "fused_min_ms": round(min(ta), 4),
                     "torch_min_ms": round(min(tb), 4), "speedup": round(mb / ma, 2), "gflop": round(flop / 1e9, 1),
                     "fused_tflops": round(flop / ma / 1e9, 1), "fused_pct_mfma_peak": round(100.0 * flop / ma / 1e9 / PEAK_TF, 1),
                     "floor_ms_at_peak": round(flop / PEAK_TF / 1e9, 3),
                     "torch_score_bytes_gb": round(n_users * I * 4 / 1e9, 2),
                     "fused_table_bytes_mb": round((U + I) * d * 4 / 1e6, 1)}
            if name == "full_rank":
                a, b = out_a.long().cpu(), out_b.cpu()
                entry["ranks_equal_frac"] = round(float((a == b).float().mean()), 5)
                entry["ranks_max_abs_diff"] = int((a - b).abs().max())
            else:
                a, b = out_a[0].cpu(), out_b[0].cpu()
                entry["lists_equal_frac"] = round(float((a == b).all(1).float().mean()), 5)
            res[name] = entry
        result["by_d"][str(d)] = res
        del eng
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
