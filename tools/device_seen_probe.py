#!/usr/bin/env python3
"""What keeping the Seen set on the device buys in a period loop, at the Yelp shape (60,000 users x 123,000 items,
synth.sample_period, Zipf 1.1 / 1.0): 30 periods of 100,000 pairs are added one by one, and every period is timed on three
routes that alternate inside one process (the order rotates from period to period):

  a  SeenItems.add + .device()            the host route: union1d over the whole history, CSR rebuild, full upload
  b  DeviceSeen.add from a host array     the pairs are uploaded, the set is built and united on the device
  c  DeviceSeen.add from device rows      the pairs are on the device already

Each timing is a host clock around work that ends in a synchronise; every route is warmed up on a set of its own first.
Reported: every period's time, and the median / min / max / interquartile spread of periods 21-30.  The final sets of the
three routes must be byte-equal, and b and c must be below a in this same run (exit code 1 otherwise).

Then one reading at table scale for route c alone: 10 M users x 1 M items, 50 M pairs in adds of 5 M (the pairs are drawn
on the device from the same Zipf laws, outside the timed region; --no-table skips it).

One JSON line on stdout and in --out.
usage: python tools/device_seen_probe.py [--out profiles/r15_device_seen_probe.json] [--no-table]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd import synth                                    # noqa: E402
from sml_amd.engine import HipEngine                         # noqa: E402
from sml_amd.retrieval import DeviceSeen, SeenItems          # noqa: E402

U, I, PERIODS, PER = 60000, 123000, 30, 100000
TU, TI, T_ADDS, T_PER = 10_000_000, 1_000_000, 10, 5_000_000


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    q1, q3 = np.percentile(ms, [25, 75])
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3), "max_ms": round(float(ms.max()), 3),
            "iqr_ms": round(float(q3 - q1), 3)}


def zipf_rows(n, n_user, n_item, seed, dev):
    """int64 [n, 2] device rows with Zipf(1.1) users and Zipf(1.0) items (inverse CDF in float64)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    cols = []
    for size, a in ((n_user, 1.1), (n_item, 1.0)):
        cdf = torch.cumsum(torch.arange(1, size + 1, device=dev, dtype=torch.float64) ** -a, 0)
        u = torch.rand(n, device=dev, dtype=torch.float64, generator=g) * cdf[-1]
        cols.append(torch.searchsorted(cdf, u).clamp_(max=size - 1))
    return torch.stack(cols, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-table", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = HipEngine(dev, 32, 256)
    periods = [synth.sample_period(np.random.RandomState(2000 + p), PER, U, I, neg=1)[0] for p in range(PERIODS)]
    on_dev = [torch.from_numpy(p).to(dev) for p in periods]
    routes = {"a_host_seen_items": (SeenItems(U, I), lambda s, p: s.add(periods[p]).device(dev)),
              "b_device_seen_host_pairs": (DeviceSeen(U, I, eng), lambda s, p: s.add(periods[p])),
              "c_device_seen_device_rows": (DeviceSeen(U, I, eng), lambda s, p: s.add(on_dev[p]))}
    for name, (s, fn) in routes.items():                      # warm-up on sets of their own
        w = SeenItems(U, I) if name.startswith("a") else DeviceSeen(U, I, eng)
        for p in range(3):
            timed(lambda: fn(w, p), dev)
    names = list(routes)
    ms = {n: [] for n in names}
    sizes = []
    for p in range(PERIODS):
        for k in range(3):
            n = names[(p + k) % 3]
            s, fn = routes[n]
            ms[n].append(round(timed(lambda: fn(s, p), dev), 3))
        sizes.append(len(routes[names[0]][0]))
    finals = [routes[n][0].host() for n in names]
    equal = all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                for f in finals[1:] for x, y in zip(finals[0], f))
    tail = {n: stats(ms[n][20:30]) for n in names}
    a, b, c = (tail[n]["median_ms"] for n in names)
    result = {"tool": "device_seen_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "periods": PERIODS,
              "pairs_per_period": PER, "keys_after_period": sizes, "per_period_ms": ms, "periods_21_30": tail,
              "a_over_b": round(a / b, 2), "a_over_c": round(a / c, 2), "final_sets_byte_equal": bool(equal),
              "speed_condition_b_and_c_below_a": bool(b < a and c < a),
              "csr_upload_mb_route_a_last_period": round((8 * (U + 1) + 4 * sizes[-1]) / 1e6, 1)}
    del routes, on_dev, finals
    if not args.no_table:
        seen = DeviceSeen(TU, TI, eng)
        DeviceSeen(TU, TI, eng).add(zipf_rows(T_PER, TU, TI, 1, dev))          # warm-up
        t_ms, t_sizes = [], []
        for k in range(T_ADDS):
            rows = zipf_rows(T_PER, TU, TI, 100 + k, dev)
            t_ms.append(round(timed(lambda: seen.add(rows), dev), 3))
            t_sizes.append(len(seen))
            del rows
        result["table_scale_route_c"] = {"U": TU, "I": TI, "adds": T_ADDS, "pairs_per_add": T_PER, "per_add_ms": t_ms,
                                         "keys_after_add": t_sizes, "last_add_ms": t_ms[-1],
                                         "peak_device_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal and result["speed_condition_b_and_c_below_a"] else 1


if __name__ == "__main__":
    sys.exit(main())
