#!/usr/bin/env python3
"""What a training negative costs on the device, at the Yelp shape of bench.py: 60,000 users x 123,000 items, a Seen CSR of
about 0.58 M pairs (as many Zipf periods of synth.sample_period as it takes), users drawn as the rows' user column.

  configurations  n = 100,000 (a period) and 3,000,000 (30 periods of history); d = 32 and 64; pool 1 / 4 / 16 / 64; alpha 0
                  and 0.75 (the cdf of the 3 M rows' item column).  Each figure: sml_sample_negatives_ex called --calls times
                  (per n) between two device events, one warm-up window, then --repeats windows; the median / min / max of
                  the per-call time.  Outputs are allocated once; the entry is asynchronous, nothing is read back inside a
                  window.  Bytes: the item rows (M * d * 4) and the user row (d * 4) an element needs, over the median,
                  beside the 5.8 TB/s this project measured for bare random-row traffic (tools/micro_gather.hip); the
                  bisection's and item_all's bytes are stated per element and not counted in the rate.
  old_vs_new      pool = 1, cdf = None: sml_sample_negatives and sml_sample_negatives_ex alternated in ONE process, nine
                  alternations, both medians and the old entry's min .. max; accepted when the new median lies inside that
                  spread.  The outputs are compared byte for byte.  The new one-lane kernel k_neg_one missed that acceptance
                  when it was measured, so the entry launches the old kernel for this case; k_neg_one is still timed in the
                  same alternation (reached with max_workgroups = the grid the call would choose) and its figures are kept.
  torch           for pool > 1: randint [n, M] -> index_select -> bmm -> argmax, WITHOUT any Seen rejection -- it does less, so
                  its time is a lower bound for a torch route -- with the peak extra memory it allocates; configurations
                  whose gather alone exceeds --torch_gb are left "not measured".
  training        "not measured" per configuration unless --train: `fine` (SPMF._epoch on the device route) on one synthetic
                  Yelp-shaped period, --epochs epochs from fresh tables, pool 1 / 4 / 16: recall@20 of SPMF.test on the
                  next period's test rows (99 negatives).  No claim beyond what that run shows.

One JSON line on stdout and in --out.
usage: python tools/neg_sampler_probe.py [--out profiles/r18_neg_sampler_probe.json] [--repeats 9] [--train] [--tiny] [--dry]"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sml_amd import synth                                    # noqa: E402
from sml_amd.sampling import popularity_cdf                  # noqa: E402

SEED = 2000
BARE_ROW_TBPS = 5.8


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4)}


def make_data(U, I, PER, n_hist, seen_target):
    perm = np.random.RandomState(SEED - 1)
    user_perm, item_perm = perm.permutation(U), perm.permutation(I)
    periods = [synth.sample_period(np.random.RandomState(SEED + p), PER, U, I, neg=1, user_perm=user_perm, item_perm=item_perm)[0][:, :2]
               for p in range(n_hist)]
    hist = np.concatenate(periods).astype(np.int64)
    codes, used = np.zeros(0, np.int64), 0
    while used < n_hist and codes.shape[0] < seen_target:      # Seen: as many periods as reach the target
        codes = np.unique(np.concatenate([codes, periods[used][:, 0].astype(np.int64) * I + periods[used][:, 1]]))
        used += 1
    ptr = np.searchsorted(codes // I, np.arange(U + 1)).astype(np.int64)
    items = (codes % I).astype(np.int64)
    item_all = np.unique(hist[:, 1])
    return dict(hist=hist, user_ptr=ptr, user_items=items, item_all=item_all, seen_pairs=int(codes.shape[0]), seen_periods=used,
                cdf=popularity_cdf(item_all, hist[:, 1], 0.75), user_perm=user_perm, item_perm=item_perm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--torch_gb", type=float, default=16.0)
    ap.add_argument("--tiny", action="store_true", help="a rehearsal shape")
    ap.add_argument("--dry", action="store_true", help="stop before the device is touched")
    args = ap.parse_args()
    U, I, PER, n_hist, target = (600, 1230, 1000, 30, 5800) if args.tiny else (60000, 123000, 100000, 30, 580000)
    data = make_data(U, I, PER, n_hist, target)
    sizes = {PER: 200, PER * n_hist: 5}                       # n -> calls per window
    if args.dry:
        print(json.dumps({"dry": True, "seen_pairs": data["seen_pairs"], "seen_periods": data["seen_periods"], "pop": int(data["item_all"].shape[0]),
                          "cdf_last": float(data["cdf"][-1])}))
        return 0

    import torch
    from sml_amd import _lib
    from sml_amd.engine import HipEngine, _ptr
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    item_all, ptr, items, cdf = t(data["item_all"]), t(data["user_ptr"]), t(data["user_items"]), t(data["cdf"])
    pop = int(item_all.shape[0])
    users = {n: t(data["hist"][:n, 0]) for n in sizes}
    seed = ctypes.c_uint64(SEED)

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    configs, engines = [], {}
    rng = np.random.RandomState(1)
    for d in (32, 64):
        eng = engines[d] = HipEngine(dev, d, 4096)
        wu, wi = t((rng.randn(U, d) * 0.1).astype(np.float32)), t((rng.randn(I, d) * 0.1).astype(np.float32))
        for n, calls in sizes.items():
            negs = torch.empty(n, device=dev, dtype=torch.int64)
            score = torch.empty(n, device=dev, dtype=torch.float32)
            failed = torch.zeros(1, device=dev, dtype=torch.int32)
            for pool in (1, 4, 16, 64):
                for alpha in (0.0, 0.75):
                    if pool == 1 and d == 64:
                        continue                              # no table is read: the d = 32 figure is the figure
                    st = eng._stream()

                    def call():
                        _lib.check(eng.lib.sml_sample_negatives_ex(eng._ctx, _ptr(users[n]), n, _ptr(item_all), pop, _ptr(ptr), U, _ptr(items),
                                                                   _ptr(cdf) if alpha else None, pool, _ptr(wu) if pool > 1 else None,
                                                                   _ptr(wi) if pool > 1 else None, d, seed, 0, _ptr(negs), _ptr(score),
                                                                   _ptr(failed), st), "sml_sample_negatives_ex")
                    window(call, calls)
                    s = stats([window(call, calls) for _ in range(args.repeats)])
                    row_bytes = pool * d * 4 if pool > 1 else 0
                    user_bytes = d * 4 if pool > 1 else 0
                    avg_range = data["seen_pairs"] / float(U)
                    s.update({"d": d, "n": n, "pool": pool, "alpha": alpha, "calls_per_window": calls, "failed": int(failed),
                              "elements_per_s": round(n / (s["median_ms"] * 1e-3)),
                              "bytes_per_element": {"item_rows": row_bytes, "user_row": user_bytes, "item_all_draws": 8 * pool,
                                                    "bisection_estimate": int(8 * pool * (np.log2(max(avg_range, 1.0)) + 1))},
                              "kernel": "k_neg_pool<%d>" % d if pool > 1 else "k_neg_one" if alpha else "k_sample_negatives (the fallback)",
                              "training_effect": "not measured"})
                    if pool > 1:
                        s["row_traffic_TB_per_s"] = round((row_bytes + user_bytes) * n / (s["median_ms"] * 1e-3) / 1e12, 3)
                        gather_gb = n * pool * d * 4 / 1e9
                        if gather_gb <= args.torch_gb:
                            def torch_route():
                                idx = torch.randint(0, pop, (n, pool), device=dev)
                                rows = wi.index_select(0, item_all[idx.reshape(-1)]).reshape(n, pool, d)
                                sc = torch.bmm(rows, wu[users[n]].unsqueeze(2)).squeeze(2)
                                return item_all[idx.gather(1, sc.argmax(1, keepdim=True)).squeeze(1)]
                            torch_route()
                            torch.cuda.synchronize(dev)
                            base = torch.cuda.memory_allocated(dev)
                            torch.cuda.reset_peak_memory_stats(dev)
                            tc = max(1, calls // 20)
                            ts = stats([window(torch_route, tc) for _ in range(args.repeats)])
                            s["torch_no_seen_rejection_lower_bound"] = dict(ts, extra_memory_bytes=int(torch.cuda.max_memory_allocated(dev) - base),
                                                                            calls_per_window=tc)
                        else:
                            s["torch_no_seen_rejection_lower_bound"] = "not measured (the gather alone is %.1f GB)" % gather_gb
                    configs.append(s)
                    print("d=%d n=%d pool=%d alpha=%g: %.4f ms" % (d, n, pool, alpha, s["median_ms"]), file=sys.stderr, flush=True)

    # old against new, alternated in this one process
    eng = engines[32]
    old_new = {}
    for n, calls in sizes.items():
        a_negs, b_negs = torch.empty(n, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.int64)
        a_failed, b_failed = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
        st = eng._stream()

        def old():
            _lib.check(eng.lib.sml_sample_negatives(eng._ctx, _ptr(users[n]), n, _ptr(item_all), pop, _ptr(ptr), U, _ptr(items), seed, _ptr(a_negs),
                                                    _ptr(a_failed), st), "sml_sample_negatives")

        def new(max_workgroups=0):
            _lib.check(eng.lib.sml_sample_negatives_ex(eng._ctx, _ptr(users[n]), n, _ptr(item_all), pop, _ptr(ptr), U, _ptr(items), None, 1, None,
                                                       None, 32, seed, max_workgroups, _ptr(b_negs), None, _ptr(b_failed), st),
                       "sml_sample_negatives_ex")
        # max_workgroups = the grid the call would choose itself: the new one-lane kernel k_neg_one, which the entry does not
        # launch on its own for this case (it launches the old kernel: k_neg_one missed the acceptance below when measured)
        one_lane = lambda: new((n + 255) // 256)
        window(old, calls), window(new, calls), window(one_lane, calls)
        o, w, k = [], [], []
        for _ in range(9):
            o.append(window(old, calls))
            w.append(window(new, calls))
            k.append(window(one_lane, calls))
        one_lane()
        so, sn, sk = stats(o), stats(w), stats(k)
        inside = lambda s: bool(so["min_ms"] <= s["median_ms"] <= so["max_ms"])
        old_new[str(n)] = {"old_sml_sample_negatives": so, "new_sml_sample_negatives_ex": sn, "new_one_lane_kernel_k_neg_one": sk,
                           "alternations": 9, "calls_per_window": calls, "new_median_inside_old_spread": inside(sn),
                           "k_neg_one_median_inside_old_spread": inside(sk),
                           "bytes_equal": bool(torch.equal(a_negs, b_negs) and int(a_failed) == int(b_failed))}

    training = "not measured"
    if args.train:
        from sml_amd.baseline import SPMF
        from sml_amd.datasets import offlineDataset_withsample
        mk = lambda p, neg: synth.sample_period(np.random.RandomState(SEED + 100 + p), PER, U, I, neg=neg, user_perm=data["user_perm"],
                                                item_perm=data["item_perm"])
        train_rows, test_rows = mk(0, 1)[0][:, :2].astype(np.int64), mk(1, 99)[1].astype(np.int64)
        training = {"method": "fine", "epochs": args.epochs, "rows": PER, "d": 64, "batch_size": 1024, "lr": 0.01, "alpha": 0.0,
                    "test_rows": int(test_rows.shape[0]), "test_negatives": int(test_rows.shape[1] - 2), "recall_at_20": {}}
        for pool in (1, 4, 16):
            a = types.SimpleNamespace(lr=0.01, pool_size=0, neg_num=1, batch_size=1024, l2_u=1e-5, l2_i=1e-5, epochs=args.epochs, pool_init_type=0,
                                      device_batches=1, neg_pool=pool, neg_pop_alpha=0.0)
            stream = types.SimpleNamespace(test_new_user=np.zeros(0, np.int64), test_new_item=np.zeros(0, np.int64))
            torch.manual_seed(2000)
            with contextlib.redirect_stdout(io.StringIO()):
                sp = SPMF(a, stream, U, I, 64, device=dev, engine=HipEngine(dev, 64, 4096))
                ds = offlineDataset_withsample(train_rows)
            losses = [sp._epoch(ds, 1, e) for e in range(args.epochs)]
            rec = sp.test(test_rows)[0]
            training["recall_at_20"]["pool_%d" % pool] = {"recall_at_20": round(float(rec[-1]), 4), "first_loss": round(losses[0], 4),
                                                          "last_loss": round(losses[-1], 4)}

    result = {"tool": "neg_sampler_probe", "device": torch.cuda.get_device_name(dev), "U": U, "I": I, "pop": pop,
              "seen_pairs": data["seen_pairs"], "seen_periods": data["seen_periods"], "repeats": args.repeats,
              "bare_random_row_traffic_TB_per_s_measured_by_this_project": BARE_ROW_TBPS,
              "configurations": configs, "old_vs_new_pool1_no_cdf": old_new,
              "pool1_no_cdf_falls_back_to_the_old_kernel": True,
              "fallback_reason": "k_neg_one's median lay outside the old kernel's run-to-run spread when first measured (0.0240 against 0.0236 .. "
                                 "0.0238 ms at n = 100,000; 0.2050 against 0.1955 .. 0.2004 ms at n = 3,000,000), so sml_sample_negatives_ex "
                                 "launches the old kernel for pool = 1, cdf = None, max_workgroups = 0",
              "training_effect": training}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
