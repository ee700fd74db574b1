"""The fold-in on the MI355X: sml_gram / sml_als_solve through HipEngine.gram / als_solve, sml_amd.als (fold_in, transpose_sets,
fit) and MFbasemode.fold_in_users / fold_in_items.

Every comparison of rows, Gram matrices and status is byte equality against the host walks of the same definitions, which
tests/test_als_host.py holds to a restatement of the header.  Shapes: U = 40 rows against I = 420 (tests/_als_cases.py), set sizes
0 .. 420, a Gram table of 2,500 rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _als_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(t, a, what):
    """A device tensor and a numpy array, byte for byte."""
    A.same_bytes(t.cpu().numpy(), a, what)


@functools.lru_cache(maxsize=None)
def dev_case(dtype, d):
    c = dict(A.case(dtype, d))
    c["t_other"], c["sets_dev"] = gpu(c["other"]), tuple(gpu(t) for t in c["csr"])
    c["gram"] = A.host_gram(c["other"], d)
    return c


@functools.lru_cache(maxsize=None)
def host_rows(dtype, d, reg, alpha0):
    c = dev_case(dtype, d)
    return A.host_solve(c["other"], d, c["gram"], reg, alpha0, c["csr"], None, c["out0"])


@pytest.mark.parametrize("dtype,d", A.PAIRS)
def test_gram_equals_the_host_walk(dtype, d):
    c = dev_case(dtype, d)
    tab = gpu(c["gram_tab"])
    for n_rows in A.GRAM_N:
        same(engine(d).gram(tab, n_rows), A.host_gram(c["gram_tab"], d, n_rows), (dtype, d, n_rows))
    same(engine(d).gram(tab), A.host_gram(c["gram_tab"], d), (dtype, d, "all rows"))
    same(engine(d).gram(c["t_other"]), c["gram"], (dtype, d, "the case's table"))


@pytest.mark.parametrize("reg,alpha0", A.PARAMS)
@pytest.mark.parametrize("dtype,d", A.PAIRS)
def test_solve_equals_the_host_walk(dtype, d, reg, alpha0):
    c = dev_case(dtype, d)
    eng = engine(d)
    want, want_st = host_rows(dtype, d, reg, alpha0)
    assert want_st[0] == 1 and (want_st[1:] == 0).all()
    g = eng.gram(c["t_other"])
    for mw in (0, 1):
        out = gpu(c["out0"])
        st = eng.als_solve(c["t_other"], g, c["sets_dev"], out, reg=reg, alpha0=alpha0, max_workgroups=mw)
        same(st, want_st, (dtype, d, reg, alpha0, mw, "status"))
        same(out, want, (dtype, d, reg, alpha0, mw))
    if alpha0 == 0.0:
        out = gpu(c["out0"])
        st = eng.als_solve(c["t_other"], None, c["sets_dev"], out, reg=reg, alpha0=alpha0)
        same(st, want_st, "no Gram: status")
        same(out, want, "no Gram")


@pytest.mark.parametrize("dtype,d", A.PAIRS)
def test_named_rows_in_place(dtype, d):
    """rows=None against an explicit permuted list with a repeat; only the named rows change."""
    c = dev_case(dtype, d)
    eng = engine(d)
    full, full_st = host_rows(dtype, d, 0.1, 0.1)
    g = eng.gram(c["t_other"])
    perm = np.random.RandomState(5).permutation(A.U)
    rows = np.concatenate([perm, perm[:1]]).astype(np.int64)
    out = gpu(c["out0"])
    st = eng.als_solve(c["t_other"], g, c["sets_dev"], out, rows=gpu(rows), reg=0.1, alpha0=0.1)
    same(st, full_st[rows], "status follows rows")
    same(out, full, "every row named: the table of rows=None")
    rows = np.array([17, 3, 0, 39, 3, 6, 17], np.int64)
    out = gpu(c["out0"])
    st = eng.als_solve(c["t_other"], g, c["sets_dev"], out, rows=rows, reg=0.1, alpha0=0.1, max_workgroups=1)
    want = c["out0"].copy()
    want[rows] = full[rows]
    same(st, full_st[rows], "status")
    same(out, want, "rows not named keep their bytes")
    out = gpu(c["out0"])
    st = eng.als_solve(c["t_other"], g, c["sets_dev"], out, rows=np.zeros(0, np.int64))
    assert st.numel() == 0
    same(out, c["out0"], "n == 0")


def test_status_codes_on_the_device():
    c = dev_case("fp32", 32)
    eng = engine(32)
    other = c["other"].copy()
    other[10] = 0.0
    other[11, 5] = np.nan
    other[12, 5] = np.inf
    sets = [[], [10], [3, 11], [12], [3, 4]]
    junk = np.full((5, 32), 7.0, np.float32)
    nan_gram = c["gram"].copy()
    nan_gram[0, 0] = np.nan
    for reg, alpha0, g in ((0.0, 0.0, c["gram"]), (0.1, 0.1, c["gram"]), (0.1, 0.1, nan_gram)):
        want, want_st = A.host_solve(other, 32, g, reg, alpha0, A.csr(sets), None, junk)
        out = gpu(junk)
        st = eng.als_solve(gpu(other), gpu(g), tuple(gpu(t) for t in A.csr(sets)), out, reg=reg, alpha0=alpha0)
        same(st, want_st, (reg, alpha0, "status"))
        same(out, want, (reg, alpha0))
        assert want_st[0] == 1 and (want_st[1:4] == 2).sum() >= 2
    out = gpu(junk)
    st = eng.als_solve(gpu(other), gpu(c["gram"]), None, out)
    assert (st == 1).all() and (out.view(torch.int32) == 0).all()


@pytest.mark.parametrize("d", (32, 64))
def test_fp16_output_is_the_rounded_fp32_output(d):
    c = dev_case("fp16", d)
    eng = engine(d)
    wide = c["t_other"].float()
    g = eng.gram(c["t_other"])
    assert torch.equal(g.view(torch.int64), eng.gram(wide).view(torch.int64))
    for reg, alpha0 in A.PARAMS:
        h, f = gpu(c["out0"]), gpu(c["out0"]).float()
        st_h = eng.als_solve(c["t_other"], g, c["sets_dev"], h, reg=reg, alpha0=alpha0)
        st_f = eng.als_solve(wide, g, c["sets_dev"], f, reg=reg, alpha0=alpha0)
        assert torch.equal(st_h, st_f)
        assert torch.equal(h.view(torch.int16), f.half().view(torch.int16)), (d, reg, alpha0)


def test_refusals_of_the_device_call():
    from sml_amd._lib import SmlError
    c = dev_case("fp32", 32)
    eng = engine(32)
    g = eng.gram(c["t_other"])
    out = gpu(c["out0"])
    with pytest.raises(SmlError):
        eng.als_solve(c["t_other"], g, c["sets_dev"], out, max_workgroups=-1)
    with pytest.raises(SmlError):
        eng.als_solve(c["t_other"], g, c["sets_dev"], out, reg=-0.1)
    with pytest.raises(SmlError):
        eng.als_solve(c["t_other"], g, c["sets_dev"], out, alpha0=float("nan"))
    with pytest.raises(SmlError):
        eng.als_solve(c["t_other"], None, c["sets_dev"], out, alpha0=0.1)
    pad = torch.zeros(32 * 32 + 1, device=DEV, dtype=torch.float64)
    with pytest.raises(SmlError):
        eng.als_solve(c["t_other"], pad[1:].view(32, 32), c["sets_dev"], out)            # a gram 8 bytes off
    same(out, c["out0"], "a refused call writes nothing")
    lib, st = eng.lib, torch.zeros(A.U, device=DEV, dtype=torch.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    off, items = c["sets_dev"]
    assert lib.sml_als_solve(eng._ctx, ptr(c["t_other"]), 4, A.I, ptr(g), 0.1, 0.1, ptr(off), None, None, A.U, ptr(out), A.U, 0, ptr(st),
                             eng._stream()) != 0                                           # exactly one of set_off / set_items
    assert lib.sml_als_solve(eng._ctx, ptr(c["t_other"]), 4, A.I, ptr(g), 0.1, 0.1, ptr(off), ptr(items), None, A.U, ptr(c["t_other"]), A.I, 0,
                             ptr(st), eng._stream()) != 0                                  # w_out is w_other
    assert lib.sml_als_solve(eng._ctx, ptr(c["t_other"]), 8, A.I, ptr(g), 0.1, 0.1, ptr(off), ptr(items), None, A.U, ptr(out), A.U, 0,
                             ptr(st), eng._stream()) != 0
    assert lib.sml_gram_scratch_bytes(eng._ctx, 0) < 0 and lib.sml_gram_scratch_bytes(eng._ctx, 2500) == 3 * 32 * 32 * 8
    scratch = torch.zeros(3 * 32 * 32 + 1, device=DEV, dtype=torch.float64)
    gg = torch.zeros(32, 32, device=DEV, dtype=torch.float64)
    assert lib.sml_gram(eng._ctx, ptr(c["t_other"]), 4, A.I, ptr(scratch[1:]), ptr(gg), eng._stream()) != 0     # scratch 8 bytes off
    assert lib.sml_gram(eng._ctx, ptr(c["t_other"]), 4, A.I, None, ptr(gg), eng._stream()) != 0
    torch.cuda.synchronize()
    from sml_amd.mf import MFbasemode, MF2
    with pytest.raises(ValueError, match="128"):
        MFbasemode(4, 4, 128).to(DEV).fold_in_users(A.csr([[0], [1], [], [2]]))
    with pytest.raises(ValueError, match="MF2"):
        MF2(4, 4, 32).to(DEV).fold_in_items(A.csr([[0], [1], [], [2]]))


def test_transpose_sets():
    from sml_amd import als
    c = dev_case("fp32", 32)
    off, users = als.transpose_sets(c["sets_dev"], A.U, A.I, engine(32))
    want_off, want_users = A.csr(A.transpose(c["sets"], A.I))
    same(off, want_off, "off")
    same(users, want_users, "users")


def model_of(c, dtype, d):
    from sml_amd.mf import MFbasemode
    m = MFbasemode(A.U, A.I, d).to(DEV)
    if dtype == "fp16":
        m = m.half()
    m.user_laten.weight.data.copy_(gpu(c["out0"]))
    m.item_laten.weight.data.copy_(gpu(c["other"]))
    return m


@pytest.mark.parametrize("dtype,d", A.PAIRS)
def test_model_fold_in_and_recommend(dtype, d):
    from sml_amd.retrieval import SeenItems
    c = dev_case(dtype, d)
    pairs = np.array([(u, i) for u, s in enumerate(c["sets"]) for i in s], np.int64)
    history = SeenItems(A.U, A.I).add(pairs)
    # users: the default is every user with a non-empty history
    m = model_of(c, dtype, d)
    res = m.fold_in_users(history)
    want = host_rows(dtype, d, 0.1, 0.1)[0].copy()
    want[0] = c["out0"][0]                                   # user 0 has no history: not named, not touched
    assert (res.solved, res.empty, res.failed) == (A.U - 1, 0, 0)
    same(m.user_laten.weight.data, want, "fold_in_users")
    same(m.item_laten.weight.data, c["other"], "the item table is not touched")
    ref = model_of(c, dtype, d)
    ref.user_laten.weight.data.copy_(gpu(want))
    users = torch.arange(A.U, device=DEV)
    for a, b in zip(m.recommend(users, 20, exclude=history), ref.recommend(users, 20, exclude=history)):
        assert torch.equal(a, b)
    # items, from the transposed history, against the folded-in user table; the CSR pair form and explicit ids
    by_item = A.transpose(c["sets"], A.I)
    ids = np.array([i for i, s in enumerate(by_item) if len(s)][::3], np.int64)
    res = m.fold_in_items(c["csr"], items=ids, reg=1.0, alpha0=1.0)
    want_i, st = A.host_solve(want, d, A.host_gram(want, d), 1.0, 1.0, A.csr(by_item), ids, c["other"])
    assert (st == 0).all() and (res.solved, res.empty, res.failed) == (len(ids), 0, 0)
    same(m.item_laten.weight.data, want_i, "fold_in_items")
    same(m.user_laten.weight.data, want, "the user table is not touched")


def test_fit_objectives_and_tables():
    """fit's tables are the host walks' tables byte for byte, and each objective it returns is the objective of the tables at
    that half-step (recomputed on the host in float64; the two sums differ in order only: 1e-9 relative)."""
    from sml_amd import als
    c = dev_case("fp32", 32)
    m = model_of(c, "fp32", 32)
    got = als.fit(m, c["sets_dev"], sweeps=2, reg=0.1, alpha0=0.1)
    p, q = c["out0"].copy(), c["other"].copy()
    csr_i = A.csr(A.transpose(c["sets"], A.I))
    want = []
    for _ in range(2):
        p, _ = A.host_solve(q, 32, A.host_gram(q, 32), 0.1, 0.1, c["csr"], None, p)
        want.append(als.objective(torch.from_numpy(p), torch.from_numpy(q), c["csr"], 0.1, 0.1))
        q, _ = A.host_solve(p, 32, A.host_gram(p, 32), 0.1, 0.1, csr_i, None, q)
        want.append(als.objective(torch.from_numpy(p), torch.from_numpy(q), c["csr"], 0.1, 0.1))
    same(m.user_laten.weight.data, p, "user table")
    same(m.item_laten.weight.data, q, "item table")
    assert len(got) == 4 and all(abs(a - b) <= 1e-9 * abs(b) for a, b in zip(got, want)), (got, want)
    assert all(b < a for a, b in zip(got, got[1:]))
    last = als.objective(m.user_laten.weight.data, m.item_laten.weight.data, c["sets_dev"], 0.1, 0.1)
    assert abs(last - got[-1]) <= 1e-12 * abs(last)
