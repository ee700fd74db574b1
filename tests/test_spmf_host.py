"""SPMF host logic (sml_amd.baseline: Reservious, StreamingData, the stream-exact sampler, run_one_stage, run) against
fixture G16 (tests/golden/make_golden_spmf.py: the reference's model/baseline.py run on CPU).  No GPU involved."""
import contextlib
import io
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import sml_oracle as O

U, I, B, EPOCHS, POOL, NEG = 60, 50, 64, 3, 200, 20


def g16():
    return golden("g16_spmf.npz")


def g16_stream(seed=16):
    """The stream G16 was recorded on (make_golden_spmf.stream)."""
    rng = np.random.RandomState(seed)
    codes = rng.permutation(U * I)
    train, test = [], []
    o = 0
    for p in range(4):
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
    for p in range(len(train)):
        np.save(os.path.join(root, "train", "%d.npy" % p), train[p])
        np.save(os.path.join(root, "test", "%d.npy" % p), test[p])
    np.save(os.path.join(root, "information.npy"), np.array([sum(t.shape[0] for t in train), U, I], dtype=np.int64))
    np.save(os.path.join(root, "test_new_user.npy"), np.arange(0, U, 7, dtype=np.int64))
    np.save(os.path.join(root, "test_new_item.npy"), np.arange(0, I, 5, dtype=np.int64))


RES_SEQS = [(10, ["updata"] * 4), (6, ["updata"] * 3), (0, ["updata"] * 2), (5, ["init_pool", "updata"]), (8, ["updata"] * 4)]


def test_reservoir_replays_g16_byte_for_byte():
    """Every recorded sequence -- an overshooting pool_have with zero rows behind it, a fill ending exactly at len,
    len = 0, init_pool -- leaves pool, t and pool_have as the reference did, and the generator where it left it."""
    from sml_amd.baseline import Reservious
    g = g16()
    np.random.seed(1616)
    quirks = 0
    for k, (length, ops) in enumerate(RES_SEQS):
        with contextlib.redirect_stdout(io.StringIO()):
            r = Reservious(length)
        for j, kind in enumerate(ops):
            getattr(r, kind)(g["r%d.op%d.rows" % (k, j)])
            assert np.array_equal(r.pool, g["r%d.op%d.pool" % (k, j)]), (k, j)
            assert [r.t, r.pool_have] == g["r%d.op%d.t_have" % (k, j)].tolist(), (k, j)
            quirks += r.pool_have > r.len
        assert np.random.rand() == g["r%d.after" % k][0], k
    assert quirks > 0


def test_streaming_data_both_types_and_end(tmp_path):
    from sml_amd.baseline import StreamingData
    train, test = g16_stream()
    write_stream(str(tmp_path / "d"), train, test)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        sd = StreamingData(str(tmp_path / "d") + "/")
        assert (sd.user_num, sd.item_num, sd.itr_num) == (U, I, sum(t.shape[0] for t in train))
        tr, te = sd.get_next(3, types="not_only_new")
        assert np.array_equal(tr, np.concatenate(train[:3])) and np.array_equal(te, test[3])
        tr, te = sd.get_next(3, types="only_new")
        assert np.array_equal(tr, train[2]) and np.array_equal(te, test[3])
        assert sd.get_next(4, types="only_new") == (None, None)       # test/4.npy missing
        assert sd.get_next(5, types="only_new") == (None, None)       # train/4.npy missing
        assert sd.get_next(0, types="not_only_new") == (None, None)   # no period before 0
    log = out.getvalue()
    assert "NOTICED: will train: 2 , will test:3 " in log and "read test data roung" in log and "read train data roung" in log


def _spmf(engine, args_over=None, data=None):
    from sml_amd.baseline import SPMF
    args = types.SimpleNamespace(lr=0.01, pool_size=POOL, neg_num=1, batch_size=B, l2_u=1e-5, l2_i=1e-5, epochs=EPOCHS,
                                 pool_init_type=0)
    for k, v in (args_over or {}).items():
        setattr(args, k, v)
    if data is None:
        data = types.SimpleNamespace(test_new_user=np.zeros(0, np.int64), test_new_item=np.zeros(0, np.int64))
    with contextlib.redirect_stdout(io.StringIO()):
        return SPMF(args, data, U, I, 32, device="cpu", engine=engine)


def _cpu_engine():
    from _cpu_engine import CpuEngine
    eng = CpuEngine(d=32)
    eng.mf_forward = lambda wu, wi, u, i, norm=False: O.mf_forward(wu, wi, u, i, norm)
    return eng


def test_stream_exact_sampler_equals_numpy_choice_across_batches():
    """sample_batch draws exactly np.random.choice(arange(N), B, p=p) and then, per row, np.random.choice(all_item, 1)
    until the item is not the user's -- the rows' and negatives' draws interleaving batch by batch."""
    sp = _spmf(_cpu_engine())
    rng = np.random.RandomState(3)
    n = 500
    data = np.stack([rng.randint(0, U, n), rng.randint(0, I, n)], 1).astype(np.int64)
    sp.all_item = np.unique(rng.randint(0, I, 35))
    sp.user_hit_num_in_W_R(data)
    hit = {}
    for u, i in data.tolist():
        hit.setdefault(u, set()).add(i)
    p = rng.gamma(0.5, size=n).astype(np.float32)
    p /= p.sum()
    sp._begin_sampling(p)
    np.random.seed(77)
    got = [np.concatenate(sp.sample_batch(data, B, p, 1), 1) for _ in range(6)]
    after = np.random.rand()
    np.random.seed(77)
    want = []
    for _ in range(6):
        bat = data[np.random.choice(np.arange(n), B, p=p)]
        negs = []
        for u in bat[:, 0]:
            m = np.random.choice(sp.all_item, 1)
            while m[0] in hit[u]:
                m = np.random.choice(sp.all_item, 1)
            negs.append(m[0])
        want.append(np.concatenate([bat, np.array(negs)[:, None]], 1))
    assert np.random.rand() == after
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_neg_num_other_than_one_raises():
    with pytest.raises(ValueError):
        _spmf(_cpu_engine(), {"neg_num": 2})


def _p_formula(wu, wi, rows):
    s = O.mf_forward(torch.as_tensor(wu), torch.as_tensor(wi), torch.as_tensor(rows[:, 0]), torch.as_tensor(rows[:, 1]))[2]
    s = s.reshape(-1).numpy().astype(np.float32)
    n = s.shape[0]
    order = np.argsort(-s, kind="stable")
    rank = np.empty(n, np.float32)
    rank[order] = np.arange(1, n + 1, dtype=np.float32)
    w = np.exp(rank / np.float32(n)).astype(np.float32)
    return (w / np.float32(w.astype(np.float64).sum())).astype(np.float32)


def _ulp_diff(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("ptype", [0, 1])
def test_p_formula_within_2ulp_of_g16(ptype, tmp_path):
    """Stage 2's p (computed on the initial tables after base_train_not_train) from the float32 formula is within 4 ulp
    of the reference's, row by row for rows held once (the reference's argsort orders copies of a row either way).
    (4, not 2: the reference sums w in float32, the formula in float64; S differs by up to 3 ulp at this N.)"""
    g = g16()
    train, test = g16_stream()
    from sml_amd.baseline import Reservious
    np.random.seed(2002)
    with contextlib.redirect_stdout(io.StringIO()):
        r = Reservious(POOL)
    if ptype == 1:
        r.init_pool(train[0])
    else:
        r.updata(train[0])
    rows = np.concatenate([r.pool[:r.pool_have], train[1]])
    p = _p_formula(g["t%d.init.user_laten.weight" % ptype], g["t%d.init.item_laten.weight" % ptype], rows)
    ref = g["t%d.p0" % ptype]
    assert p.shape == ref.shape
    assert _ulp_diff(np.sort(p), np.sort(ref)).max() <= 4
    codes = rows[:, 0] * I + rows[:, 1]
    uniq, cnt = np.unique(codes, return_counts=True)
    once = np.isin(codes, uniq[cnt == 1])
    assert once.sum() > 0.5 * rows.shape[0]
    assert _ulp_diff(p[once], ref[once]).max() <= 4


class _G16Engine(object):
    """The CPU oracle with G16's p handed out as the engine's rank weights, one stage after another."""

    def __init__(self, ps):
        self.inner = _cpu_engine()
        self.ps = list(ps)
        self.seen = []
        self.device = torch.device("cpu")

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def rank_weights(self, wu, wi, rows):
        p = torch.from_numpy(self.ps.pop(0))
        assert p.shape[0] == rows.shape[0]
        return None, None, None, p

    def bare_adam_epoch(self, mf, triples, *a, **k):
        self.seen.append(np.asarray(triples).copy())
        return self.inner.bare_adam_epoch(mf, triples, *a, **k)


def run_g16(ptype, engine, tmp_path, device="cpu"):
    """base_train_not_train(1) + run(2, 'spmf') of the product under G16's seeds; returns (spmf, log)."""
    from sml_amd.baseline import SPMF, StreamingData
    g = g16()
    train, test = g16_stream()
    root = str(tmp_path / ("t%d" % ptype))
    write_stream(root, train, test)
    args = types.SimpleNamespace(lr=0.01, pool_size=POOL, neg_num=1, batch_size=B, l2_u=1e-5, l2_i=1e-5, epochs=EPOCHS,
                                 pool_init_type=ptype)
    torch.manual_seed(2000)
    np.random.seed(2002)
    data = StreamingData(root + "/")
    with contextlib.redirect_stdout(io.StringIO()):
        sp = SPMF(args, data, U, I, 32, device=device, engine=engine)
    with torch.no_grad():
        for name in ("user_laten", "item_laten", "user_bais", "item_bais"):
            getattr(sp.MFbase, name).weight.copy_(torch.from_numpy(g["t%d.init.%s.weight" % (ptype, name)]))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        sp.base_train_not_train(1)
        sp.run(2, method="spmf")
    return g, sp, buf.getvalue()


_NUM = re.compile(r"-?\d+\.\d*(?:e[-+]?\d+)?|-?\d+")


def compare_logs(log, ref, atol):
    """Line by line: the same text apart from times; numbers within atol."""
    a = [re.sub(r"time:\d+\.\d", "time:#", l) for l in log.splitlines()]
    b = [re.sub(r"time:\d+\.\d", "time:#", l) for l in ref.splitlines()]
    assert len(a) == len(b), (len(a), len(b))
    for la, lb in zip(a, b):
        assert _NUM.sub("#", la).replace(" ", "") == _NUM.sub("#", lb).replace(" ", ""), (la, lb)
        na, nb = [float(x) for x in _NUM.findall(la)], [float(x) for x in _NUM.findall(lb)]
        assert len(na) == len(nb) and np.allclose(na, nb, atol=atol, rtol=0), (la, lb)


def check_g16_run(g, sp, log, seen, ptype, exact_batches=True):
    pre = "t%d." % ptype
    n_ep = len(g[pre + "losses"])
    assert len(seen) == n_ep
    batches = g[pre + "batches"]
    per = batches.shape[0] // n_ep
    if exact_batches:
        for e in range(n_ep):
            assert np.array_equal(np.asarray(seen[e]), batches[e * per:(e + 1) * per].reshape(-1, 3)), e
    losses = [float(l.split("loss:")[1]) for l in log.splitlines() if l.startswith("epoch:")]
    np.testing.assert_allclose(losses, g[pre + "losses"], atol=1.01e-4)
    tests = g[pre + "tests"]
    np.testing.assert_allclose(np.array(sp.recall), tests[[5, 10], :3], atol=1e-9)
    np.testing.assert_allclose(np.array(sp.ndcg), tests[[5, 10], 3:], atol=1e-5)
    compare_logs(log, str(g[pre + "log"]), atol=1.01e-4)
    last = max(int(k[len(pre) + 4:]) for k in g.keys() if k.startswith(pre + "pool") and not k.endswith("t_have"))
    pool, th = g[pre + "pool%d" % last], g[pre + "pool%d.t_have" % last]
    assert np.array_equal(sp.Reservious.pool, pool) and [sp.Reservious.t, sp.Reservious.pool_have] == th.tolist()


@pytest.mark.parametrize("ptype", [0, 1])
def test_spmf_run_one_stage_replays_g16(ptype, tmp_path):
    """The product's SPMF with the oracle as the bare step and G16's p: the triples handed to bare_adam_epoch are the
    reference's batches bit for bit, the epoch losses, recall / ndcg, the reservoir and the log are the reference's."""
    g = g16()
    eng = _G16Engine([g["t%d.p0" % ptype], g["t%d.p1" % ptype]])
    g, sp, log = run_g16(ptype, eng, tmp_path)
    check_g16_run(g, sp, log, eng.seen, ptype)


def test_run_summary_arithmetic_and_method_dispatch():
    from sml_amd.baseline import SPMF
    sp = SPMF.__new__(SPMF)
    calls = []
    stages = {"n": 0}

    def one(stage_id):
        calls.append(("spmf", stage_id))
        return _next()

    def two(stage_id, read_data_type="only_new"):
        calls.append((read_data_type, stage_id))
        return _next()

    rng = np.random.RandomState(1)
    recall, ndcg, tn = rng.rand(5, 3), rng.rand(5, 3), rng.randint(10, 100, 5)

    def _next():
        k = stages["n"]
        if k == 5:
            return False
        sp.recall.append(recall[k]); sp.ndcg.append(ndcg[k]); sp.test_num.append(int(tn[k]))
        stages["n"] += 1
        return True

    sp.run_one_stage, sp.run_one_stage2 = one, two
    for method, kind in (("spmf", "spmf"), ("full", "not_only_new"), ("fine", "only_new")):
        sp.recall, sp.ndcg, sp.test_num, sp.hit_new_user, sp.hit_new_item = [], [], [], [], []
        stages["n"] = 0
        calls.clear()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            sp.run(7, method=method)
        assert calls == [(kind, 7 + k) for k in range(6)]
        out = {l.split(":")[0]: l for l in buf.getvalue().splitlines() if ":" in l}
        w = tn / tn.sum()
        n3 = round(5 / 3)
        h = tn[:n3] / tn[:n3].sum()
        t = tn[n3:] / tn[n3:].sum()
        expect = {"weight average recall@20": (recall * w[:, None]).sum(0), "weight average ndcg@20": (ndcg * w[:, None]).sum(0),
                  "pre 3 (val) reslut,recall,ndcg": np.concatenate([(recall[:n3] * h[:, None]).sum(0), (ndcg[:n3] * h[:, None]).sum(0)]),
                  "last 7 (test) results,recall ,ndcg": np.concatenate([(recall[n3:] * t[:, None]).sum(0), (ndcg[n3:] * t[:, None]).sum(0)])}
        for k, v in expect.items():
            got = [float(x) for x in _NUM.findall(out[k].split(":", 1)[1])]
            np.testing.assert_allclose(got, v, atol=1e-7)
        assert "hit new user: []" in buf.getvalue()
