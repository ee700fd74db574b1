"""Full-catalogue retrieval on the MI355X: sml_full_rank / sml_topk_items through HipEngine, MFbasemode and
sml_amd.evaluation, against numpy.

Dyadic tables (entries k/8, |k| <= 16) make every product and every sum over d <= 64 exact in fp32 in any order, so
ranks, lists and scores are compared exactly there; random normal tables are compared against float64 with a
tolerance tau = 1e-5 * ||u|| * max ||x||, except where both retrieval paths must agree with each other bit for bit.
"""
import numpy as np
import pytest
import torch

from conftest import make_mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def dyadic(rng, rows, d):
    return (rng.randint(-16, 17, size=(rows, d)) / 8.0).astype(np.float32)


def make_seen(rng, U, I, sizes):
    """CSR of sizes[u] distinct random items per user."""
    from sml_amd.retrieval import SeenItems
    seen = SeenItems(U, I)
    pairs = [np.stack([np.full(s, u), rng.choice(I, size=s, replace=False)], 1) for u, s in enumerate(sizes) if s > 0]
    if pairs:
        seen.add(np.concatenate(pairs))
    return seen


def seen_sets(seen):
    off, items = seen.host()
    return [set(items[off[u]:off[u + 1]].tolist()) for u in range(seen.n_user)]


def ref_rank(S, u, p, excl):
    """#{i != p, i not excluded, S[u, i] > S[u, p]} (S exact or float64)."""
    s = S[u]
    m = s > s[p]
    m[p] = False
    if excl:
        m[list(excl)] = False
    return int(m.sum())


def ref_topk(S, u, k, excl):
    s = S[u]
    ok = ~np.isnan(s)
    if excl:
        ok[list(excl)] = False
    ids = np.nonzero(ok)[0]
    order = ids[np.lexsort((ids, -s[ids]))][:k]
    items = np.full(k, -1, dtype=np.int64)
    scores = np.full(k, -np.inf, dtype=np.float64)
    items[:len(order)] = order
    scores[:len(order)] = s[order]
    return items, scores


def gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("d", [32, 64])
def test_exact_on_dyadic_data(d):
    rng = np.random.RandomState(100 + d)
    U, I, n = 300, 2053, 257
    wu, wi = dyadic(rng, U, d), dyadic(rng, I, d)
    users = rng.randint(0, U, size=n)
    users[:4] = [0, 1, 2, 3]
    pos = rng.randint(0, I, size=n)
    # plant exact ties with the positive: item rows equal to the positive's row
    for r in range(0, n, 7):
        for q in rng.choice(I, size=3, replace=False):
            wi[q] = wi[pos[r]]
    sizes = rng.randint(0, 40, size=U)
    sizes[0] = 0                 # empty Seen
    sizes[1] = 1500              # long Seen
    sizes[2] = I - 50            # fewer than K = 128 eligible items: padding
    seen = make_seen(rng, U, I, sizes)
    sets = seen_sets(seen)
    pos[3] = next(iter(sets[3])) if sets[3] else pos[3]     # a positive inside Seen(u): never excluded from its own row
    rows = np.concatenate([np.stack([users, pos], 1), rng.randint(0, I, size=(n, 5))], 1).astype(np.int64)
    S = wu.astype(np.float64) @ wi.astype(np.float64).T
    eng = engine(d)
    tu, ti = gpu(wu), gpu(wi)
    csr = seen.device(DEV)
    rank = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
    want = np.array([ref_rank(S, users[r], pos[r], sets[users[r]]) for r in range(n)])
    np.testing.assert_array_equal(rank, want)
    for k in (1, 20, 128):
        items, scores = eng.topk_items(tu, ti, gpu(users), k, csr)
        items, scores = items.cpu().numpy(), scores.cpu().numpy()
        assert items.dtype == np.int64 and scores.dtype == np.float32 and items.shape == (n, k)
        for r in range(n):
            wi_r, ws_r = ref_topk(S, users[r], k, sets[users[r]])
            np.testing.assert_array_equal(items[r], wi_r)
            np.testing.assert_array_equal(scores[r].astype(np.float64), ws_r)
        if k == 128:
            assert (items[2, 50:] == -1).all() and np.isneginf(scores[2, 50:]).all() and (items[2, :50] >= 0).all()
        # consistency of the two paths (include/sml_hip.h): the positive's position in the list
        for r in range(n):
            u, p = users[r], pos[r]
            if p in sets[u]:
                continue
            s = S[u]
            ties = sum(1 for i in np.nonzero(s == s[p])[0] if i < p and i != p and i not in sets[u])
            at = rank[r] + ties
            if at < k:
                assert items[r, at] == p, (d, k, r)


@pytest.mark.parametrize("d", [32, 64])
def test_anchored_to_sampled_rank_kernel(d):
    rng = np.random.RandomState(200 + d)
    U, I, n = 120, 1030, 96
    wu, wi = dyadic(rng, U, d), dyadic(rng, I, d)
    seen = make_seen(rng, U, I, [5] * U)
    sets = seen_sets(seen)
    users = rng.randint(0, U, size=n)
    pos = np.array([rng.choice([i for i in rng.choice(I, size=10, replace=False) if i not in sets[u]]) for u in users])
    rows = np.stack([np.concatenate([[u, p], [i for i in range(I) if i != p and i not in sets[u]]]) for u, p in zip(users, pos)])
    assert rows.shape == (n, 2 + I - 6)
    mf = make_mf(U, I, d, wu, wi, device=DEV)
    rows_t = gpu(rows)
    _, sampled, _, _ = mf.test2(rows_t, topK=10)
    full = engine(d).full_rank(mf.user_laten.weight.data, mf.item_laten.weight.data, rows_t[:, :2], seen.device(DEV))
    np.testing.assert_array_equal(full.cpu().numpy(), sampled.cpu().numpy())
    for k in (5, 10, 20):
        h0, n0, r0 = mf.test(rows_t, topK=k)
        h1, n1, r1 = mf.test_full(rows_t, topK=k, exclude=seen)
        assert h0 == h1 and float(n0) == float(n1)
        np.testing.assert_array_equal(r0.cpu().numpy(), r1.cpu().numpy())


def check_float64(eng, wu, wi, rows, users, k, seen, sets):
    """(3): ranks inside the tau bracket, returned scores within tau, the top-K set valid up to tau."""
    U64, I64 = wu.astype(np.float64), wi.astype(np.float64)
    tau_u = 1e-5 * np.linalg.norm(U64, axis=1) * np.linalg.norm(I64, axis=1).max()
    rank = eng.full_rank(gpu(wu), gpu(wi), gpu(rows), seen.device(DEV)).cpu().numpy()
    for r in range(rows.shape[0]):
        u, p = rows[r, 0], rows[r, 1]
        s = I64 @ U64[u]
        tau = tau_u[u]
        m = np.ones(len(s), dtype=bool)
        m[p] = False
        m[list(sets[u])] = False
        lo, hi = int((s[m] > s[p] + tau).sum()), int((s[m] > s[p] - tau).sum())
        assert lo <= rank[r] <= hi, (r, lo, rank[r], hi)
    items, scores = eng.topk_items(gpu(wu), gpu(wi), gpu(users), k, seen.device(DEV))
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    for x, u in enumerate(users):
        s = I64 @ U64[u]
        tau = tau_u[u]
        it, sc = items[x], scores[x]
        assert (it >= 0).all()
        assert len(set(it.tolist())) == k and not (set(it.tolist()) & sets[u])
        assert (np.diff(sc) <= 0).all()
        np.testing.assert_array_less(np.abs(sc - s[it]), tau + 1e-30)
        elig = np.ones(len(s), dtype=bool)
        elig[list(sets[u])] = False
        kth = np.sort(s[elig])[::-1][k - 1]
        assert (s[it] >= kth - 2 * tau).all()
        must = np.nonzero(elig & (s > kth + 2 * tau))[0]
        assert set(must.tolist()) <= set(it.tolist())


@pytest.mark.parametrize("d", [32, 64])
def test_random_floats_against_float64(d):
    rng = np.random.RandomState(300 + d)
    U, I, n = 400, 5000, 300
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(I, d).astype(np.float32)
    seen = make_seen(rng, U, I, rng.randint(0, 200, size=U))
    sets = seen_sets(seen)
    rows = np.stack([rng.randint(0, U, size=n), rng.randint(0, I, size=n)], 1).astype(np.int64)
    check_float64(engine(d), wu, wi, rows, rng.choice(U, size=128, replace=False), 20, seen, sets)


def test_both_paths_agree_on_random_floats():
    d, k, U, I = 32, 128, 1000, 50000
    rng = np.random.RandomState(400)
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(I, d).astype(np.float32)
    seen = make_seen(rng, U, I, rng.randint(0, 300, size=U))
    eng = engine(d)
    csr = seen.device(DEV)
    users = np.arange(U)
    items, scores = eng.topk_items(gpu(wu), gpu(wi), gpu(users), k, csr)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert (items >= 0).all()
    rows = np.stack([np.repeat(users, k), items.reshape(-1)], 1)
    rank = eng.full_rank(gpu(wu), gpu(wi), gpu(rows), csr).cpu().numpy().reshape(U, k)
    # the position of items[x, j] is its rank plus the equal-scoring eligible items of smaller id, all of which sit
    # before it in the list
    ties = np.array([[int((scores[x, :j] == scores[x, j]).sum()) for j in range(k)] for x in range(U)])
    np.testing.assert_array_equal(rank + ties, np.broadcast_to(np.arange(k), (U, k)))


def test_determinism_and_nan():
    d, k, U, I = 32, 20, 200, 3000
    rng = np.random.RandomState(500)
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(I, d).astype(np.float32)
    wu[7] = np.nan
    nan_items = [11, 900, 2999]
    wi[nan_items] = np.nan
    seen = make_seen(rng, U, I, rng.randint(0, 50, size=U))
    eng = engine(d)
    csr = seen.device(DEV)
    rows = np.stack([rng.randint(0, U, size=500), rng.randint(0, I, size=500)], 1).astype(np.int64)
    rows[:5, 0] = 7
    rows[5, 1] = 900           # a NaN positive
    tu, ti = gpu(wu), gpu(wi)
    r1 = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
    r2 = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
    assert r1.tobytes() == r2.tobytes()
    assert (r1[:6] == 0).all()
    users = np.arange(U)
    i1, s1 = eng.topk_items(tu, ti, gpu(users), k, csr)
    i2, s2 = eng.topk_items(tu, ti, gpu(users), k, csr)
    assert i1.cpu().numpy().tobytes() == i2.cpu().numpy().tobytes()
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    i1, s1 = i1.cpu().numpy(), s1.cpu().numpy()
    assert (i1[7] == -1).all() and np.isneginf(s1[7]).all()
    assert not np.isin(i1, nan_items).any()
    assert not np.isnan(s1).any()


def test_argument_checks():
    from sml_amd._lib import SmlError
    eng = engine(32)
    tu = torch.zeros(10, 32, device=DEV)
    ti = torch.zeros(20, 32, device=DEV)
    off = torch.zeros(11, dtype=torch.int64, device=DEV)
    items = torch.zeros(0, dtype=torch.int32, device=DEV)
    for k in (0, 129):
        with pytest.raises(SmlError):
            eng.topk_items(tu, ti, torch.arange(3), k)
    lib = eng.lib
    rank = torch.empty(1, dtype=torch.int32, device=DEV)
    rows = torch.zeros(1, 2, dtype=torch.int64, device=DEV)
    args = lambda n_item, n_cols, so, si: (eng._ctx, tu.data_ptr(), ti.data_ptr(), n_item, rows.data_ptr(), 1, n_cols,  # noqa: E731
                                           so, si, rank.data_ptr(), None)
    assert lib.sml_full_rank(*args(20, 2, off.data_ptr(), None)) != 0          # exactly one of the CSR arrays
    assert lib.sml_full_rank(*args(20, 2, None, items.data_ptr() or 16)) != 0
    assert lib.sml_full_rank(*args(20, 1, None, None)) != 0                    # n_cols < 2
    assert lib.sml_full_rank(*args(0, 2, None, None)) != 0                     # n_item <= 0
    assert lib.sml_full_rank(*args(1 << 31, 2, None, None)) != 0               # n_item >= 2^31
    assert lib.sml_topk_scratch_bytes(eng._ctx, 5, 129, 20) < 0
    e128 = engine(128)
    with pytest.raises(SmlError):
        e128.full_rank(torch.zeros(10, 128, device=DEV), torch.zeros(20, 128, device=DEV), rows)
    with pytest.raises(SmlError):
        e128.topk_items(torch.zeros(10, 128, device=DEV), torch.zeros(20, 128, device=DEV), torch.arange(3), 5)
    assert eng.full_rank(tu, ti, rows, (off, items)).cpu().tolist() == [0]


def test_yelp_scale():
    from sml_amd import synth
    from sml_amd.evaluation import test_model_full
    from sml_amd.retrieval import SeenItems
    d, U, I = 32, 60000, 123000
    rng = np.random.RandomState(600)
    seen = SeenItems(U, I)
    for p in range(5):
        train, _ = synth.sample_period(np.random.RandomState(610 + p), 100000, U, I, neg=1)
        seen.add(train)
    _, test = synth.sample_period(np.random.RandomState(620), 10000, U, I, neg=1)
    rows = test[:, :2]
    sets_needed = {}
    wu = (rng.randn(U, d) * 0.3).astype(np.float32)
    wi = (rng.randn(I, d) * 0.3).astype(np.float32)
    off, items = seen.host()
    pick_r = rng.choice(rows.shape[0], size=256, replace=False)
    pick_u = rng.choice(U, size=1024, replace=False)
    for u in np.concatenate([rows[pick_r, 0], pick_u]):
        sets_needed[u] = set(items[off[u]:off[u + 1]].tolist())

    class Sets(dict):
        def __missing__(self, u):
            return set(items[off[u]:off[u + 1]].tolist())

    sets = Sets(sets_needed)
    eng = engine(d)
    # the full 10,000-row pass once, the sampled rows checked against float64
    full = eng.full_rank(gpu(wu), gpu(wi), gpu(rows), seen.device(DEV)).cpu().numpy()
    assert full.shape == (10000,) and (full >= 0).all() and (full < I).all()
    check_float64(eng, wu, wi, rows[pick_r], pick_u, 20, seen, sets)
    full_sub = eng.full_rank(gpu(wu), gpu(wi), gpu(rows[pick_r]), seen.device(DEV)).cpu().numpy()
    np.testing.assert_array_equal(full_sub, full[pick_r])
    mf = make_mf(U, I, d, wu, wi, device=DEV)
    np_state = np.random.get_state()
    t_state = torch.get_rng_state()
    c_state = torch.cuda.get_rng_state(DEV)
    recall, ndcg = test_model_full(mf, rows, seen=seen, topK=10)
    assert np.random.get_state()[1].tobytes() == np_state[1].tobytes() and np.random.get_state()[2] == np_state[2]
    assert torch.equal(torch.get_rng_state(), t_state) and torch.equal(torch.cuda.get_rng_state(DEV), c_state)
    assert recall == pytest.approx(float((full < 10).sum()) / 10000)
    want_ndcg = float((1.0 / np.log2(full[full < 10] + 2.0)).sum()) / 10000
    assert float(ndcg) == pytest.approx(want_ndcg, rel=1e-5)
