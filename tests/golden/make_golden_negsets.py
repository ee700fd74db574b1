#!/usr/bin/env python3
"""Generate tests/golden/g17_select_neg.npz by IMPORTING the reference's data/dataset2.py and running its own
select_neg_forinteraction on the CPU.  Runs only where the reference checkout is available; nothing from it is copied.

The toy set: 6 periods x 150 rows, 40 users, items uniform over a catalogue that grows from 40 (period 0) to 90 (period 5),
neg_num = 30, leave_for_init_train = 0.5 (so periods 3, 4, 5 get negatives), np.random.seed(5) before the call.

Recorded, all int32: hyper = [n_periods, rows, n_user, n_item, neg_num, start], train.<p> [150, 2] for every period and
test.<p> [150, 32] for p >= start exactly as the reference saved them.  Data only.

usage: python tests/golden/make_golden_negsets.py --ref <reference checkout>
"""
import argparse
import importlib.util
import os
import shutil
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_PERIODS, ROWS, N_USER, ITEMS0, ITEMS1, NEG, LEAVE = 6, 150, 40, 40, 90, 30, 0.5


def toy_stream(seed=17):
    rng = np.random.RandomState(seed)
    out = []
    for p in range(N_PERIODS):
        n_cat = ITEMS0 + (ITEMS1 - ITEMS0) * p // (N_PERIODS - 1)
        out.append(np.stack([rng.randint(0, N_USER, ROWS), rng.randint(0, n_cat, ROWS)], 1).astype(np.int64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_dataset2", os.path.join(a.ref, "data", "dataset2.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    stream = toy_stream()
    tmp = tempfile.mkdtemp()
    try:
        base = os.path.join(tmp, "toy")
        os.makedirs(os.path.join(base, "test"))
        np.save(os.path.join(base, "information.npy"), np.array([N_PERIODS * ROWS, N_USER, ITEMS1], dtype=np.int64))
        names = [str(p) for p in range(N_PERIODS)]
        for name, rows in zip(names, stream):
            np.save(os.path.join(base, name + ".npy"), rows)
        np.random.seed(5)
        ref.select_neg_forinteraction(path=tmp + os.sep, datasetname="toy", file_path_list=names, leave_for_init_train=LEAVE, neg_num=NEG)
        start = round(N_PERIODS * LEAVE)
        out = {"hyper": np.array([N_PERIODS, ROWS, N_USER, ITEMS1, NEG, start], dtype=np.int32)}
        for p, rows in enumerate(stream):
            out["train.%d" % p] = rows.astype(np.int32)
        written = sorted(os.listdir(os.path.join(base, "test")))
        assert written == ["%d.npy" % p for p in range(start, N_PERIODS)], written
        for p in range(start, N_PERIODS):
            t = np.load(os.path.join(base, "test", "%d.npy" % p))
            assert t.shape == (ROWS, 2 + NEG), t.shape
            out["test.%d" % p] = t.astype(np.int32)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dst = os.path.join(HERE, "g17_select_neg.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
