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


# ---- exact comparisons against the fp32 chain of the kernels (tests/_fp32_chain.py) ---------------------------------
# Every score is the fmaf chain in the kernels' k order, emulated exactly; ranks, item lists and score BYTES must equal
# the reference.  test_retrieval_host.py::test_exact_tests_have_teeth shows the same data tells other orders apart.

def csr_dev(seen):
    return None if seen is None else (gpu(seen[0]), gpu(seen[1]))


def check_exact(eng, wu, wi, rows=None, users=None, ks=(), seen=None, ref_device="cpu", chunk=1 << 16):
    """ranks of `rows` and the top-k lists of `users` for every k in ks, exactly as the fp32-chain reference has them.
    wu / wi: numpy arrays or device tensors."""
    import _fp32_chain as F
    tu = wu if torch.is_tensor(wu) else gpu(wu)
    ti = wi if torch.is_tensor(wi) else gpu(wi)
    csr = csr_dev(seen)
    if rows is not None:
        got = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
        want = F.ref_full_rank(wu, wi, rows, seen, device=ref_device, chunk=chunk)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, ("rank", len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    if ks:
        want_i, want_s = F.ref_topk(wu, wi, users, max(ks), seen, device=ref_device, chunk=chunk)
        for k in ks:
            items, scores = eng.topk_items(tu, ti, gpu(users), k, csr)
            items, scores = items.cpu().numpy(), scores.cpu().numpy()
            wi_k, ws_k = want_i[:, :k], np.ascontiguousarray(want_s[:, :k])
            bad = np.nonzero((items != wi_k).any(1) | (scores.view(np.int32) != ws_k.view(np.int32)).any(1))[0]
            assert len(bad) == 0, ("topk", k, len(bad), bad[:4], items[bad[:1]], wi_k[bad[:1]])


@pytest.mark.parametrize("d", [32, 64])
def test_exact_on_random_floats(d):
    import _fp32_chain as F
    c = F.random_case(d, seed=800 + d)
    check_exact(engine(d), c["wu"], c["wi"], c["rows"], c["users"], (1, 20, 128), c["seen"])


@pytest.mark.parametrize("d", [32, 64])
def test_exact_on_planted_near_ties(d):
    """Exact copies, +-1 ulp copies and rounding-only copies of the positives; k-th entries copied across slices; users
    whose scores are all subnormal (a flushing path would tie them all)."""
    import _fp32_chain as F
    c = F.near_tie_case(d)
    check_exact(engine(d), c["wu"], c["wi"], c["rows"], c["users"], (1, 20, 128), c["seen"])


def _sweep_users(rng, U, n):
    """n user ids, unsorted, with duplicates."""
    users = rng.randint(0, U, size=n)
    if n > 2:
        users[n // 2] = users[0]
        users[-1] = users[1]
    return users


def test_geometry_every_topk_wave_count():
    """k in {1, 2, 63, 64, 65, 85, 86, 127, 128}: 4-, 3- and 2-wave blocks of k_topk_slice."""
    import _fp32_chain as F
    ks = (1, 2, 63, 64, 65, 85, 86, 127, 128)
    assert {F.topk_waves(k) for k in ks} == {4, 3, 2}
    c = F.random_case(32, seed=900, U=200, I=3001)
    users = _sweep_users(c["rng"], 200, 200)
    check_exact(engine(32), c["wu"], c["wi"], None, users, ks, c["seen"])


@pytest.mark.parametrize("n", [1, 31, 33, 95, 97, 127, 129])
def test_geometry_user_counts(n):
    """Partial waves and blocks: n around 32 (a wave), 96 (a 3-wave block) and 128 (a 4-wave block); duplicate and
    unsorted users and rows."""
    import _fp32_chain as F
    c = F.random_case(32, seed=1000 + n, U=150, I=1500, n=n)
    rng = c["rng"]
    users = _sweep_users(rng, 150, n)
    rows = c["rows"].copy()
    rows[:, 0] = _sweep_users(rng, 150, n)
    if n > 3:
        rows[2] = rows[0]
    check_exact(engine(32), c["wu"], c["wi"], rows, users, (20, 65, 128), c["seen"])


@pytest.mark.parametrize("n_item", [1, 5, 31, 32, 33])
@pytest.mark.parametrize("d", [32, 64])
def test_geometry_small_catalogue(d, n_item):
    """Catalogues of one tile or less (most slices empty), k above n_item, Seen covering all items / all but one."""
    import _fp32_chain as F
    rng = np.random.RandomState(1100 + n_item + d)
    U = 40
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(n_item, d).astype(np.float32)
    lists = {0: range(n_item), 1: [i for i in range(n_item) if i != n_item // 2], 2: {0, n_item - 1},
             3: {i for i in (31, 32) if i < n_item}}
    seen = F.seen_csr(U, n_item, lists)
    rows = np.stack([np.repeat(np.arange(U), 2)[:70], rng.randint(0, n_item, size=70)], 1).astype(np.int64)
    check_exact(engine(d), wu, wi, rows, _sweep_users(rng, U, 40), (1, 2, 33, 128), seen)
    items, _ = engine(d).topk_items(gpu(wu), gpu(wi), gpu(np.arange(4)), 128, csr_dev(seen))
    items = items.cpu().numpy()
    assert (items[0] == -1).all() and items[1, 0] == n_item // 2 and (items[1, 1:] == -1).all()


def _slice_edges(slices, slice_tiles, n_item):
    e = set()
    for q in range(slices):
        a, b = q * slice_tiles * 32, min((q + 1) * slice_tiles * 32, n_item)
        if a < b:
            e |= {a, b - 1}
    return e


@pytest.mark.parametrize("n_item,n_rows,n_users,empty_rank,empty_topk", [
    (288, 100, 100, 3, 3),          # 9 tiles over 8 slices: the last 3 empty
    (16411, 40, 3, 1, 1),           # 513 tiles, 32 slices (both kernels), the last one empty, the last tile partial
    (262145, 100, 100, 30, 0),      # the rank kernel at its 512-slice maximum, 30 of them empty
])
def test_geometry_slices_and_seen_edges(n_item, n_rows, n_users, empty_rank, empty_topk):
    """Empty trailing slices, Seen on items 0, 31, 32, n_item - 1 and on the first and last item of every slice, a user
    whose Seen is a whole slice (its cand_n is 0 there), all items but one, and all items."""
    import _fp32_chain as F
    d = 32
    rng = np.random.RandomState(1200 + n_item % 1000)
    U = 120
    rs, rst, rempty = F.rank_plan(n_rows, n_item)
    tw, ts, tst, tempty = F.topk_plan(n_users, 20, n_item)
    assert (rempty, tempty) == (empty_rank, empty_topk)
    if n_item == 262145:
        assert rs == 512
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(n_item, d).astype(np.float32)
    edges = {0, 31, 32, n_item - 1} | _slice_edges(rs, rst, n_item) | _slice_edges(ts, tst, n_item)
    lists = {0: edges, 1: range(tst * 32, min(2 * tst * 32, n_item)), 2: range(rst * 32, min(2 * rst * 32, n_item)),
             3: [i for i in range(n_item) if i != n_item - 2], 4: range(n_item)}
    for u in range(5, U):
        lists[u] = rng.choice(n_item, size=min(n_item // 4, 50), replace=False)
    seen = F.seen_csr(U, n_item, lists)
    # positives on and next to the edges, and inside the users' own Seen
    pos = np.array(sorted(edges))
    pos = rng.permutation(np.concatenate([pos, np.clip(pos + 1, 0, n_item - 1), rng.randint(0, n_item, size=n_rows)]))[:n_rows]
    pos[0] = n_item - 1                     # user 0's positive, inside its own Seen
    rows = np.stack([np.arange(n_rows) % U, pos], 1).astype(np.int64)
    users = np.concatenate([np.arange(min(5, n_users)), rng.randint(0, U, size=max(0, n_users - 5))])
    on_gpu = n_item > 100000
    check_exact(engine(d), wu, wi, rows, users, (20, 128), seen, ref_device=DEV if on_gpu else "cpu")
    items, scores = engine(d).topk_items(gpu(wu), gpu(wi), gpu(np.arange(5)), 20, csr_dev(seen))
    items = items.cpu().numpy()
    assert (items[4] == -1).all() and items[3, 0] == n_item - 2 and (items[3, 1:] == -1).all()
    assert not (set(items[1].tolist()) & set(lists[1]))


def test_item_table_above_2_to_the_31_bytes():
    """d = 32, 2^24 + 4,099 items (2.15 GB): item rows and Seen past 2^31 bytes / 2^24 rows, near-ties planted at the far
    end; 64 rank rows and the top-20 of 64 users, exact through the float64 filter (on the device)."""
    import _fp32_chain as F
    d, U, I = 32, 256, (1 << 24) + 4099
    free, _ = torch.cuda.mem_get_info()
    assert free > 12 * (1 << 30), free
    g = torch.Generator(device=DEV)
    g.manual_seed(1300)
    ti = torch.randn(I, d, generator=g, device=DEV)
    rng = np.random.RandomState(1300)
    wu = rng.randn(U, d).astype(np.float32)
    n = 64
    far = (1 << 24) + rng.randint(0, 4099, size=n)
    rows = np.stack([rng.randint(0, U, size=n), far], 1).astype(np.int64)
    rows[: n // 2, 1] = rng.randint(0, I, size=n // 2)
    # exact and one-ulp copies of some positives, far and near
    src = torch.from_numpy(rows[:16, 1]).to(DEV)
    dst_far = torch.from_numpy(I - 1 - np.arange(16)).to(DEV)
    dst_near = torch.from_numpy(np.arange(16) * 1000 + 7).to(DEV)
    ti[dst_far] = ti[src]
    ti[dst_near] = torch.nextafter(ti[src], torch.full_like(ti[src], np.inf))
    lists = {u: np.concatenate([[I - 1, I - 17, (1 << 24) + 3], rng.randint(0, I, size=20)]) for u in range(U)}
    seen = F.seen_csr(U, I, lists)
    users = rng.choice(U, size=64, replace=False)
    check_exact(engine(d), gpu(wu), ti, rows, users, (20,), seen, ref_device=DEV, chunk=1 << 19)


def test_chunked_topk_equals_one_call(monkeypatch):
    """HipEngine.topk_items splits a call whose scratch exceeds TOPK_SCRATCH_BYTES: chunks of an odd user count (and a
    ragged last chunk) give the same bytes as one call."""
    import _fp32_chain as F
    from sml_amd.engine import HipEngine
    c = F.random_case(32, seed=1400, U=500, I=5000, n=300)
    eng = engine(32)
    tu, ti, csr = gpu(c["wu"]), gpu(c["wi"]), csr_dev(c["seen"])
    users = _sweep_users(c["rng"], 500, 300)
    k = 65
    one_i, one_s = eng.topk_items(tu, ti, gpu(users), k, csr)
    total = int(eng.lib.sml_topk_scratch_bytes(eng._ctx, len(users), k, c["wi"].shape[0]))
    monkeypatch.setattr(HipEngine, "TOPK_SCRATCH_BYTES", -(-37 * total // len(users)))
    calls = []
    real = eng.lib.sml_topk_items

    def counting(*a):
        calls.append(a[5])
        return real(*a)
    monkeypatch.setattr(eng.lib, "sml_topk_items", counting)
    ch_i, ch_s = eng.topk_items(tu, ti, gpu(users), k, csr)
    assert calls[0] == 37 and len(calls) == 9 and sum(calls) == 300, calls
    assert ch_i.cpu().numpy().tobytes() == one_i.cpu().numpy().tobytes()
    assert ch_s.cpu().numpy().tobytes() == one_s.cpu().numpy().tobytes()
    want_i, want_s = F.ref_topk(c["wu"], c["wi"], users, k, c["seen"])
    np.testing.assert_array_equal(ch_i.cpu().numpy(), want_i)
    assert ch_s.cpu().numpy().tobytes() == want_s.tobytes()


def test_host_layers_against_exact_reference():
    """evaluation.test_model_full over one array, a list of unequal batches and a DeviceRows; MFbasemode.recommend;
    recall / NDCG against the oracle's metrics on the exact ranks."""
    import _fp32_chain as F
    from oracle.sml_oracle import eval_metrics
    from sml_amd.evaluation import DeviceRows, test_model_full
    from sml_amd.retrieval import SeenItems
    c = F.near_tie_case(32, seed=5)
    wu, wi, rows = c["wu"], c["wi"], c["rows"]
    U, I = wu.shape[0], wi.shape[0]
    off, its = c["seen"]
    pairs = np.stack([np.repeat(np.arange(U), np.diff(off)), its], 1)
    seen = SeenItems(U, I).add(pairs)
    assert all((x == y).all() for x, y in zip(seen.host(), c["seen"]))
    mf = make_mf(U, I, 32, wu, wi, device=DEV)
    ranks = F.ref_full_rank(wu, wi, rows, c["seen"])
    for topK in (1, 10, 100):
        hits, ndcg = eval_metrics(torch.from_numpy(ranks), topK)
        want_r, want_n = hits / len(rows), ndcg / len(rows)
        cuts = [0, 1, 40, 41, 160, len(rows)]
        batches = [rows[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        for ts in (rows, batches, [gpu(b) for b in batches], DeviceRows(rows, DEV)):
            r, nd = test_model_full(mf, ts, seen=seen, topK=topK)
            assert r == want_r, (topK, type(ts))
            assert float(nd) == pytest.approx(want_n, rel=1e-6, abs=1e-7), (topK, type(ts))
    users = c["users"]
    for k in (1, 20, 128):
        ri, rs = mf.recommend(gpu(users), topK=k, exclude=seen)
        ti_, ts_ = engine(32).topk_items(gpu(wu), gpu(wi), gpu(users), k, csr_dev(c["seen"]))
        assert ri.cpu().numpy().tobytes() == ti_.cpu().numpy().tobytes()
        assert rs.cpu().numpy().tobytes() == ts_.cpu().numpy().tobytes()
        want_i, want_s = F.ref_topk(wu, wi, users, k, c["seen"])
        np.testing.assert_array_equal(ri.cpu().numpy(), want_i)
