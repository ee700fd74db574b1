#!/usr/bin/env python3
"""What preparing a period's test set on the device costs, at the Yelp shape of bench.py: 60,000 users x 123,000 items, 40
periods of 100,000 Zipf rows (synth.sample_period, Zipf 1.1 / 1.0), neg_num = 999, leave_for_init_train = 0.7 (periods 28..39
get negatives).

  timeline     Timeline(periods, ...) from rows already on the device: a host clock around work that ends in a synchronise,
               one warm-up, then --repeats builds
  neg_sets     HipEngine.neg_sets (sml_neg_sets) per period: one warm-up call, then --repeats calls, each between two device
               events; per period the median / min / max, and the output bytes (n x 1001 x 8) over the median
  host         sml_host_neg_sets, the library's single-threaded walk of the same definition, on the last period (host clock);
               it is a different function from the kernel and is its comparison
  equal        the device and host outputs of that period, byte for byte, and the failure counters

One JSON line on stdout and in --out.
usage: python tools/neg_sets_probe.py [--out profiles/r16_neg_sets_probe.json] [--repeats 5] [--periods 40]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd import _lib, synth                              # noqa: E402
from sml_amd.engine import HipEngine                         # noqa: E402
from sml_amd.prepare import Timeline                         # noqa: E402

U, I, PER, NEG, LEAVE, SEED = 60000, 123000, 100000, 999, 0.7, 2000


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3), "max_ms": round(float(ms.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--periods", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = HipEngine(dev, 32, 256)
    perm = np.random.RandomState(SEED - 1)
    user_perm, item_perm = perm.permutation(U), perm.permutation(I)
    periods = [synth.sample_period(np.random.RandomState(SEED + p), PER, U, I, neg=1, user_perm=user_perm, item_perm=item_perm)[0]
               for p in range(args.periods)]
    on_dev = [torch.from_numpy(p).to(dev) for p in periods]
    start = round(args.periods * LEAVE)

    build_ms = []
    for k in range(args.repeats + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tl = Timeline(on_dev, U, I, eng)
        torch.cuda.synchronize(dev)
        if k:
            build_ms.append((time.perf_counter() - t0) * 1e3)

    per_period, last = {}, None
    out_bytes = PER * (2 + NEG) * 8
    for p in range(start, args.periods):
        ms = []
        for k in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, failed = eng.neg_sets(tl.rows[p], tl.g0[p], tl, NEG, SEED)
            e1.record()
            e1.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        s = stats(ms)
        s["failed_rows"] = int(failed)
        s["n_cat_last_row"] = int(tl.n_cat[p][-1])
        s["out_gb_per_s"] = round(out_bytes / (s["median_ms"] * 1e-3) / 1e9, 1)
        per_period[str(p)] = s
        last = (p, out.cpu().numpy(), int(failed))
        del out
    med = [v["median_ms"] for v in per_period.values()]

    # the host entry on the last period
    p, dev_out, dev_failed = last
    lib = _lib.load()
    h = tl.host()
    rows = np.ascontiguousarray(periods[p])
    n_cat = np.ascontiguousarray(h.n_cat[tl.g0[p]:tl.g0[p + 1]])
    host_out, host_failed = np.empty((PER, 2 + NEG), np.int64), np.zeros(1, np.int32)
    t0 = time.perf_counter()
    _lib.check(lib.sml_host_neg_sets(rows.ctypes.data, PER, 2, tl.g0[p], n_cat.ctypes.data, h.order.ctypes.data, h.h_off.ctypes.data, U,
                                     h.h_items.ctypes.data, h.h_since.ctypes.data, NEG, SEED, host_out.ctypes.data,
                                     host_failed.ctypes.data), "sml_host_neg_sets")
    host_ms = (time.perf_counter() - t0) * 1e3
    equal = dev_out.tobytes() == host_out.tobytes() and dev_failed == int(host_failed[0])
    dev_ms = per_period[str(p)]["median_ms"]
    result = {"tool": "neg_sets_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "periods": args.periods,
              "rows_per_period": PER, "neg_num": NEG, "first_period_with_negatives": start, "repeats": args.repeats,
              "stream_rows": tl.total, "distinct_pairs": int(tl.h_items.shape[0]), "items_seen": int(tl.order.shape[0]),
              "longest_history": int((tl.h_off[1:] - tl.h_off[:-1]).max()),
              "timeline_build_from_device_rows": stats(build_ms),
              "neg_sets_per_period": per_period,
              "neg_sets_median_of_period_medians_ms": round(float(np.median(med)), 3),
              "neg_sets_rows_per_s": round(PER / (float(np.median(med)) * 1e-3)),
              "output_bytes_per_period": out_bytes,
              "host_entry": {"period": p, "ms": round(host_ms, 1), "rows_per_s": round(PER / (host_ms * 1e-3)),
                             "device_median_ms_same_period": dev_ms, "host_over_device": round(host_ms / dev_ms, 1)},
              "device_and_host_byte_equal": bool(equal)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
