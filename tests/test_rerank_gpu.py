"""Greedy MMR re-ranking on the MI355X: sml_rerank_mmr called in place (pool_stride > pool_cols) and through
HipEngine.rerank_mmr, MFbasemode.recommend(diversify=) and sml_amd.evaluation.intra_list_similarity.

Every comparison is exact: ids, positions, counts and the bits of value and sim_sum against the plain-numpy restatement of
tests/_rerank_cases.py and against the host walk.  Shapes: I = 4,099, 40 lists of at most 128 entries, k in {1, 20, 128}."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _rerank_cases as R
from conftest import make_mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # (a copy: the cases' arrays are read-only)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


@functools.lru_cache(maxsize=None)
def on_device(d, half):
    c = R.case(d, half)
    return dict(table=gpu(c["table"]), pool_items=gpu(c["pool_items"]), pool_rel=gpu(c["pool_rel"]), nrm=gpu(c["nrm"]), n=c["n"])


def raw(eng, g, pool_cols, nrm, lam, normalize, k, max_workgroups=0, n=None, rc_only=False, **over):
    """sml_rerank_mmr on the case's own arrays, read in place (pool_stride = STRIDE); the outputs start as junk."""
    from sml_amd import _lib
    n = g["n"] if n is None else n
    a = dict(table=g["table"], pool_items=g["pool_items"], pool_rel=g["pool_rel"], stride=R.STRIDE,
             items=torch.full((n, k), 77, device=DEV, dtype=torch.int32), pos=torch.full((n, k), 77, device=DEV, dtype=torch.int32),
             value=torch.full((n, k), 7.0, device=DEV, dtype=torch.float32), n_sel=torch.full((n,), 77, device=DEV, dtype=torch.int32),
             sim_sum=torch.full((n,), 7.0, device=DEV, dtype=torch.float32))
    a.update(over)
    t = a["table"]
    as_ptr = lambda v: v if isinstance(v, ctypes.c_void_p) else ptr(v)        # noqa: E731
    rc = eng.lib.sml_rerank_mmr(eng._ctx, as_ptr(t), g["table"].element_size(), g["table"].shape[0], as_ptr(a["pool_items"]),
                                as_ptr(a["pool_rel"]), n, pool_cols, a["stride"], ptr(nrm), lam, normalize, k, max_workgroups, as_ptr(a["items"]),
                                as_ptr(a["pos"]), as_ptr(a["value"]), as_ptr(a["n_sel"]), as_ptr(a["sim_sum"]), eng._stream())
    if rc_only:
        return rc
    _lib.check(rc, "sml_rerank_mmr")
    return tuple(a[key].cpu().numpy() for key in ("items", "pos", "value", "n_sel", "sim_sum"))


def setting_args(g, s):
    lam, metric, normalize = R.SETTINGS[s]
    return (g["nrm"] if metric == "cosine" else None), lam, normalize


@pytest.mark.parametrize("width", R.WIDTHS, ids=R.WIDTH_IDS)
def test_device_equals_the_restatement_and_the_host_walk(width):
    from test_rerank_host import host_case
    d, half = width
    eng, g = engine(d), on_device(d, half)
    for s in range(len(R.SETTINGS)):
        for k in R.KS:
            got = raw(eng, g, R.C, *setting_args(g, s), k)
            assert R.same_bytes(got, R.expected(d, half, s, k)) is None, (R.SETTING_IDS[s], k)
    for cols in R.LENGTHS[:-1]:
        assert R.same_bytes(raw(eng, g, cols, *setting_args(g, 0), 20), R.expected(d, half, 0, 20, cols)) is None, cols
    assert R.same_bytes(raw(eng, g, R.C, *setting_args(g, 0), 20), host_case(R.case(d, half), 0, 20)) is None


@pytest.mark.parametrize("width", R.WIDTHS, ids=R.WIDTH_IDS)
def test_launch_geometry_does_not_change_the_bytes(width):
    """max_workgroups 1 and 3: a wave then walks several lists, a short one directly after a 128-entry one among them
    (lists 28 .. 31 and 32 .. 35 share their waves under max_workgroups = 1)."""
    d, half = width
    eng, g = engine(d), on_device(d, half)
    for s, k in ((0, 20), (1, 128), (3, 1)):
        want = R.expected(d, half, s, k)
        for mw in (1, 3):
            assert R.same_bytes(raw(eng, g, R.C, *setting_args(g, s), k, max_workgroups=mw), want) is None, (s, k, mw)


@pytest.mark.parametrize("d", [32, 64])
def test_fp16_tables_equal_their_fp32_copies(d):
    eng, g = engine(d), on_device(d, True)
    c = R.case(d, True)
    for s, k in ((0, 20), (1, 128)):
        lam, metric, normalize = R.SETTINGS[s]
        half = eng.rerank_mmr(g["table"], g["pool_items"][:, :R.C], g["pool_rel"][:, :R.C], k, lam, metric=metric, normalize=bool(normalize),
                              nrm=g["nrm"])
        full = eng.rerank_mmr(g["table"].float(), g["pool_items"][:, :R.C], g["pool_rel"][:, :R.C], k, lam, metric=metric,
                              normalize=bool(normalize), nrm=g["nrm"])
        for a, b in zip(half, full):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        want = R.expected(d, True, s, k)
        assert half[0].dtype == torch.int64 and np.array_equal(half[0].cpu().numpy(), want[0])
        assert R.same_bytes(tuple(t.cpu().numpy() for t in half[1:]), want[1:]) is None
    assert c["table"].dtype == np.float16


def test_engine_call_narrows_int64_pools_and_builds_the_norms():
    d = 32
    eng, g, c = engine(d), on_device(d, False), R.case(d, False)
    wide = g["pool_items"][:, :R.C].long().clone()
    wide[21, 0], wide[21, 5] = 2 ** 40 + 3, -(2 ** 40)                 # padding of the case, now beyond int32
    want = R.expected(d, False, 0, 20)
    got = eng.rerank_mmr(g["table"], wide, g["pool_rel"][:, :R.C], 20, 0.7, nrm=g["nrm"])
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and R.same_bytes(tuple(t.cpu().numpy() for t in got[1:]), want[1:]) is None
    # the norms built by the engine from the current weights: the restatement on that table's plane 0
    adj = eng.item_adjust_cosine(g["table"])
    nrm = adj[0, :R.I].cpu().numpy()
    built = eng.rerank_mmr(g["table"], wide, g["pool_rel"][:, :R.C], 20, 0.7)
    ready = eng.rerank_mmr(g["table"], wide, g["pool_rel"][:, :R.C], 20, 0.7, nrm=adj)
    ref = R.ref_rerank(c["table32"], c["pool_items"], c["pool_rel"], R.C, nrm, 0.7, 1, 20, S=R.pairwise(d, False))
    for out in (built, ready):
        assert np.array_equal(out[0].cpu().numpy(), ref[0]) and R.same_bytes(tuple(t.cpu().numpy() for t in out[1:]), ref[1:]) is None
    dot = eng.rerank_mmr(g["table"], wide, g["pool_rel"][:, :R.C], 128, 0.3, metric="dot", normalize=False)
    assert R.same_bytes(tuple(t.cpu().numpy() for t in dot[1:]), R.expected(d, False, 1, 128)[1:]) is None
    with pytest.raises(ValueError):
        eng.rerank_mmr(g["table"], wide, g["pool_rel"][:, :64], 20, 0.7)
    with pytest.raises(ValueError):
        eng.rerank_mmr(g["table"], g["pool_items"], g["pool_rel"], 20, 0.7)            # 131 columns
    with pytest.raises(ValueError):
        eng.rerank_mmr(g["table"], wide, g["pool_rel"][:, :R.C], 20, 0.7, nrm=g["nrm"][:100])


@functools.lru_cache(maxsize=None)
def model(d):
    c = R.case(d, False)
    return make_mf(64, R.I, d, np.array(c["users"]), np.array(c["table32"]), device=DEV)      # (copies: the arrays are read-only)


@pytest.mark.parametrize("d", [32, 64])
def test_recommend_diversify(d):
    mf = model(d)
    users = torch.arange(64, device=DEV)
    rng = np.random.RandomState(3)
    seen = {u: rng.choice(R.I, size=30, replace=False) for u in range(64)}
    from _fp32_chain import seen_csr
    off, its = seen_csr(64, R.I, seen)
    exclude = (gpu(off), gpu(its))
    for topK, P in ((20, 100), (1, 1), (20, 128), (50, 50)):
        plain_i, plain_s = mf.recommend(users, topK=P, exclude=exclude)
        # diversify = 1: the plain list's first topK columns (min-max scaling keeps the order), scores gathered through pos
        it, sc = mf.recommend(users, topK=topK, exclude=exclude, diversify=1.0, pool=P)
        assert it.dtype == torch.int64 and sc.dtype == torch.float32 and tuple(it.shape) == (64, topK)
        assert torch.equal(it, plain_i[:, :topK]) and torch.equal(sc.view(torch.int32), plain_s[:, :topK].view(torch.int32))
        # diversify = None: today's call, the same bytes
        again_i, again_s = mf.recommend(users, topK=P, exclude=exclude, diversify=None, pool=None)
        assert torch.equal(again_i, plain_i) and torch.equal(again_s.view(torch.int32), plain_s.view(torch.int32))
    # a real trade-off: the engine call on the same pool, the scores are the pool's at pos, and the lists are less alike
    from sml_amd.evaluation import intra_list_similarity
    pool_i, pool_s = mf.recommend(users, topK=100, exclude=exclude)
    it, sc = mf.recommend(users, topK=20, exclude=exclude, diversify=0.5)
    eng = engine(d)
    picked, at, _, n_sel, _ = eng.rerank_mmr(mf.item_laten.weight.data, pool_i, pool_s, 20, 0.5)
    assert (n_sel == 20).all() and torch.equal(it, picked) and torch.equal(sc.view(torch.int32), pool_s.gather(1, at.long()).view(torch.int32))
    assert torch.equal(pool_i.gather(1, at.long()), it)
    ils_plain = intra_list_similarity(mf, pool_i[:, :20]).mean().item()
    ils_div = intra_list_similarity(mf, it).mean().item()
    assert ils_div < ils_plain, (ils_div, ils_plain)
    # candidates= and score= go through the same call
    cand = torch.from_numpy(np.stack([rng.choice(R.I, size=60, replace=False) for _ in range(64)])).to(DEV)
    ci, cs = mf.recommend(users, topK=30, candidates=cand, score="cosine")
    di, ds = mf.recommend(users, topK=10, candidates=cand, score="cosine", diversify=1.0, pool=30)
    assert torch.equal(di, ci[:, :10]) and torch.equal(ds.view(torch.int32), cs[:, :10].view(torch.int32))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_intra_list_similarity(metric):
    from sml_amd.evaluation import intra_list_similarity
    d = 32
    mf, c, eng = model(d), R.case(d, False), engine(d)
    lists = np.ascontiguousarray(c["pool_items"][:, :R.C]).astype(np.int64)
    lists[(lists < 0) | (lists >= R.I)] = -1
    got = intra_list_similarity(mf, gpu(lists), metric=metric)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["n"],)
    nrm = eng.item_adjust_cosine(mf.item_laten.weight.data)[0, :R.I].cpu().numpy() if metric == "cosine" else None
    rel = -np.arange(R.C, dtype=np.float32)[None, :].repeat(c["n"], 0)
    _, pos, _, n_sel, total = R.ref_rerank(c["table32"], lists, rel, R.C, nrm, 1.0, 0, R.C, S=R.pairwise(d, False))
    m = n_sel.astype(np.float32)
    pairs = m * (m - np.float32(1)) / np.float32(2)
    with np.errstate(all="ignore"):
        want = np.where(pairs > 0, total / np.maximum(pairs, np.float32(1)), np.float32(0)).astype(np.float32)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert want[36] == 0 and want[33] == 0 and (n_sel[33], n_sel[36]) == (1, 0), "fewer than two items: 0"
    live = [x for x in range(c["n"]) if n_sel[x] > 1]
    assert all((np.diff(pos[x, :n_sel[x]]) > 0).all() for x in live), "the list order is kept"
    if metric == "cosine":
        assert np.abs(want[list(R.LONG)]).max() < 0.1, "random rows are nearly orthogonal"


def test_capi_refusals():
    d = 32
    eng, g = engine(d), on_device(d, False)
    nrm = g["nrm"]

    def refused(word, **kw):
        args = dict(pool_cols=R.C, nrm=nrm, lam=0.7, normalize=1, k=20)
        args.update({key: kw.pop(key) for key in list(kw) if key in ("pool_cols", "nrm", "lam", "normalize", "k", "max_workgroups", "n")})
        rc = raw(eng, g, args.pop("pool_cols"), args.pop("nrm"), args.pop("lam"), args.pop("normalize"), args.pop("k"), rc_only=True, **args, **kw)
        assert rc != 0, (word, kw)
        assert word in eng.lib.sml_last_error().decode(), (word, eng.lib.sml_last_error())
    assert raw(eng, g, R.C, nrm, 0.7, 1, 20, rc_only=True) == 0
    refused("max_workgroups", max_workgroups=-1)
    refused("pool_cols", pool_cols=0)
    refused("pool_cols", pool_cols=129)
    refused("pool_stride", stride=R.C - 1)
    refused("k <= 128", k=0)
    refused("k <= 128", k=129)
    refused("lam", lam=-0.5)
    refused("lam", lam=2.0)
    refused("lam", lam=float("nan"))
    refused("normalize", normalize=3)
    refused("16-byte aligned", table=ctypes.c_void_p(g["table"].data_ptr() + 8))
    refused("null", items=None)
    refused("null", pool_rel=None)
    out = torch.zeros(2 * g["n"] * 20, device=DEV, dtype=torch.int32)
    refused("outputs overlap", items=out, pos=out[20:])
    refused("overlaps an input", items=g["pool_items"])
    refused("overlaps an input", sim_sum=g["nrm"])
    # a (d, elem_bytes) pair without kernels: fp32 at d = 128
    e128 = engine(128)
    t128 = torch.zeros(R.I, 128, device=DEV)
    rc = e128.lib.sml_rerank_mmr(e128._ctx, ptr(t128), 4, R.I, ptr(g["pool_items"]), ptr(g["pool_rel"]), 1, R.C, R.STRIDE, None, 0.5, 1, 20, 0,
                                 ptr(out), ptr(out[100:]), ptr(out[200:]), ptr(out[300:]), ptr(out[400:]), e128._stream())
    assert rc != 0 and "d must be" in e128.lib.sml_last_error().decode()
    torch.cuda.synchronize()


def test_no_lists_is_a_valid_call():
    d = 32
    eng, g = engine(d), on_device(d, False)
    assert raw(eng, g, R.C, g["nrm"], 0.7, 1, 20, n=0, rc_only=True) == 0
    none = ctypes.c_void_p(0)
    assert raw(eng, g, R.C, None, 0.7, 1, 20, n=0, rc_only=True, table=none, pool_items=none, pool_rel=none, items=none, pos=none, value=none,
               n_sel=none, sim_sum=none) == 0
    out = eng.rerank_mmr(g["table"], g["pool_items"][:0, :R.C], g["pool_rel"][:0, :R.C], 20, 0.7, nrm=g["nrm"])
    assert [tuple(t.shape) for t in out] == [(0, 20), (0, 20), (0, 20), (0,), (0,)]
    torch.cuda.synchronize()
