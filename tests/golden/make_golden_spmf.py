#!/usr/bin/env python3
"""Generate tests/golden/g16_spmf.npz by IMPORTING the reference's model/baseline.py (SPMF) and running it on CPU.

Runs only where the reference checkout is available; nothing from it is copied.  Shims: those of make_golden.py
(install_shims), plus one for a reference defect -- SPMF.run_one_stage unpacks two values from its first `test` call,
which returns four, so that first call per stage is made to return the first two.

Recorded (prefix r<k>. for the reservoir sequences, t<type>. for the SPMF runs with pool_init_type = type):
  reservoir: the ops of a sequence (kind, rows) and pool / t / pool_have after each, then one np.random.rand() draw
             (the generator's state after the sequence); the sequences cover a partial fill whose pool_have overshoots
             (zero rows behind it), a fill that ends exactly at len, len = 0 and init_pool;
  SPMF:      the initial tables, p per stage (distinct rows asserted to score distinctly; the
             reservoir's arithmetic can hold copies of a row, which the reference's argsort orders either way), every batch sample_batch returned, the pool
             after every stage, every test result, the epoch losses and the captured log.

usage: python tests/golden/make_golden_spmf.py [--ref <reference checkout>]
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims  # noqa: E402

U, I, D, B, EPOCHS, N_PERIODS, POOL = 60, 50, 32, 64, 3, 4, 200
NEG = 20


def stream(seed=16):
    """Periods 0..3: ~300 distinct (user, item) rows each, test rows (user, pos, 20 negatives)."""
    rng = np.random.RandomState(seed)
    codes = rng.permutation(U * I)          # every (user, item) pair at most once in the whole stream: tie-free scores
    train, test = [], []
    o = 0
    for p in range(N_PERIODS):
        n = 280 + 20 * p
        c = codes[o:o + n]
        o += n
        train.append(np.stack([c // I, c % I], 1).astype(np.int64))
        t = np.zeros((60, 2 + NEG), dtype=np.int64)
        for r in range(60):
            t[r, 0], t[r, 1] = rng.randint(0, U), rng.randint(0, I)
            t[r, 2:] = rng.choice(np.setdiff1d(np.arange(I), [t[r, 1]]), size=NEG, replace=False)
        test.append(t)
    return train, test


def write_stream(root, train, test):
    os.makedirs(os.path.join(root, "train"))
    os.makedirs(os.path.join(root, "test"))
    for p in range(N_PERIODS):
        np.save(os.path.join(root, "train", "%d.npy" % p), train[p])
        np.save(os.path.join(root, "test", "%d.npy" % p), test[p])
    np.save(os.path.join(root, "information.npy"), np.array([sum(t.shape[0] for t in train), U, I], dtype=np.int64))
    np.save(os.path.join(root, "test_new_user.npy"), np.arange(0, U, 7, dtype=np.int64))
    np.save(os.path.join(root, "test_new_item.npy"), np.arange(0, I, 5, dtype=np.int64))


RES_SEQS = [  # (len, [(kind, n_rows)])
    (10, [("updata", 3), ("updata", 4), ("updata", 6), ("updata", 5)]),
    (6, [("updata", 6), ("updata", 4), ("updata", 9)]),
    (0, [("updata", 5), ("updata", 3)]),
    (5, [("init_pool", 12), ("updata", 7)]),
    (8, [("updata", 3), ("updata", 2), ("updata", 2), ("updata", 8)]),
]


def gen_reservoir(B_mod, out):
    rng = np.random.RandomState(5)
    np.random.seed(1616)
    for k, (length, ops) in enumerate(RES_SEQS):
        with contextlib.redirect_stdout(io.StringIO()):
            r = B_mod.Reservious(length)
        for j, (kind, n) in enumerate(ops):
            rows = np.stack([rng.randint(1, U, n), rng.randint(1, I, n)], 1).astype(np.int64)
            getattr(r, kind)(rows)
            out["r%d.op%d.rows" % (k, j)] = rows
            out["r%d.op%d.pool" % (k, j)] = r.pool.copy()
            out["r%d.op%d.t_have" % (k, j)] = np.array([r.t, r.pool_have], dtype=np.int64)
        out["r%d.after" % k] = np.array([np.random.rand()])
    out["r.kinds"] = np.array([";".join("%d:%s" % (length, ",".join("%s/%d" % o for o in ops)) for length, ops in RES_SEQS)])


def gen_spmf(B_mod, root, pool_init_type, out):
    pre = "t%d." % pool_init_type
    args = types.SimpleNamespace(lr=0.01, pool_size=POOL, neg_num=1, batch_size=B, l2_u=1e-5, l2_i=1e-5, epochs=EPOCHS,
                                 pool_init_type=pool_init_type)
    rec = dict(p=[], batches=[], tests=[], pools=[])
    S = B_mod.SPMF
    orig = dict(test=S.test, run_one_stage=S.run_one_stage, compute=S.compute_R_W_P, sample=S.sample_batch, upd=S.updata_reservious)

    def test(self, *a, **k):
        r = orig["test"](self, *a, **k)
        rec["tests"].append(np.concatenate([np.asarray(r[0], dtype=np.float64), np.asarray(r[1], dtype=np.float64)]))
        if getattr(self, "_first_test", False):
            self._first_test = False
            return r[:2]
        return r

    def run_one_stage(self, stage_id):
        self._first_test = True
        return orig["run_one_stage"](self, stage_id)

    def compute(self, data):
        with torch.no_grad():
            _, _, s = self.MFbase(torch.from_numpy(data[:, 0]), torch.from_numpy(data[:, 1]))
        s = s.reshape(-1).numpy()
        codes = data[:, 0] * I + data[:, 1]
        # tie-free up to the reservoir's duplicated rows (its arithmetic copies rows twice): distinct pairs, distinct scores
        assert np.unique(s).shape[0] == np.unique(codes).shape[0], "scores are not tie-free"
        p = orig["compute"](self, data)
        rec["p"].append(np.asarray(p, dtype=np.float32).copy())
        return p

    def sample(self, *a, **k):
        u, i, j = orig["sample"](self, *a, **k)
        rec["batches"].append(np.concatenate([u, i, j], 1).astype(np.int64))
        return u, i, j

    def upd(self, data):
        orig["upd"](self, data)
        rv = self.Reservious
        rec["pools"].append((rv.pool.copy(), np.array([rv.t, rv.pool_have], dtype=np.int64)))

    S.test, S.run_one_stage, S.compute_R_W_P, S.sample_batch, S.updata_reservious = test, run_one_stage, compute, sample, upd
    try:
        buf = io.StringIO()
        torch.manual_seed(2000)
        np.random.seed(2002)
        data = B_mod.StreamingData(root + "/")
        sp = S(args, data, U, I, D)
        with torch.no_grad():
            sp.MFbase.user_laten.weight.mul_(0.3)
            sp.MFbase.item_laten.weight.mul_(0.3)
        for k, v in sp.MFbase.state_dict().items():
            out[pre + "init." + k] = v.detach().numpy().copy()
        with contextlib.redirect_stdout(buf):
            sp.base_train_not_train(1)
            sp.run(2, method="spmf")
    finally:
        S.test, S.run_one_stage, S.compute_R_W_P, S.sample_batch, S.updata_reservious = (
            orig["test"], orig["run_one_stage"], orig["compute"], orig["sample"], orig["upd"])
    log = buf.getvalue()
    for s, p in enumerate(rec["p"]):
        out[pre + "p%d" % s] = p
    out[pre + "batches"] = np.stack(rec["batches"], 0)
    out[pre + "tests"] = np.stack(rec["tests"], 0)
    for s, (pool, th) in enumerate(rec["pools"]):
        out[pre + "pool%d" % s] = pool
        out[pre + "pool%d.t_have" % s] = th
    out[pre + "losses"] = np.array([float(l.split("loss:")[1]) for l in log.splitlines() if l.startswith("epoch:")])
    out[pre + "log"] = np.array(log)
    out[pre + "final"] = np.concatenate([sp.MFbase.user_laten.weight.detach().numpy().ravel(),
                                         sp.MFbase.item_laten.weight.detach().numpy().ravel()])
    print("G16 type %d: %d stages, %d batches, losses %s" % (pool_init_type, len(rec["p"]), len(rec["batches"]), out[pre + "losses"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    install_shims(a.ref)
    import model.baseline as B_mod
    assert os.path.realpath(B_mod.__file__).startswith(os.path.realpath(a.ref))
    out = {"hyper": np.array([U, I, D, B, EPOCHS, POOL, 0.01, 1e-5], dtype=np.float64)}
    gen_reservoir(B_mod, out)
    train, test = stream()
    tmp = tempfile.mkdtemp()
    try:
        root = os.path.join(tmp, "tiny")
        write_stream(root, train, test)
        for t in (0, 1):
            gen_spmf(B_mod, root, t, out)
    finally:
        shutil.rmtree(tmp)
    path = os.path.join(HERE, "g16_spmf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
