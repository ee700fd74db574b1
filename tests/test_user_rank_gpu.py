"""Per-user ranking of held-out sets on the MI355X: sml_user_rank / sml_user_metrics through HipEngine.user_ranks,
MFbasemode.test_users and sml_amd.evaluation.test_model_users, exactly against the fp32-chain reference
(tests/_user_rank_ref.py), against sml_full_rank and against sml_topk_items."""
import numpy as np
import pytest
import torch

from conftest import make_mf
from _fp32_chain import near_tie_case, random_case
from _user_rank_ref import held_out_csr, ref_user_metrics, ref_user_rank, user_scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (1, 5, 20, 128)


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(eng, wu, wi, users, off, items, seen, ks=KS):
    csr = None if seen is None else (gpu(seen[0]), gpu(seen[1]))
    out = eng.user_ranks(gpu(wu), gpu(wi), users, off, items, csr, ks)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(out, wu, wi, users, off, items, seen, ks=KS):
    above, pos = ref_user_rank(wu, wi, users, off, items, seen)
    np.testing.assert_array_equal(out["above"], above)
    np.testing.assert_array_equal(out["pos"], pos)
    hits, dcg, ap, first = ref_user_metrics(pos, off, ks)
    np.testing.assert_array_equal(out["hits"], hits)
    np.testing.assert_array_equal(out["first"], first)
    np.testing.assert_allclose(out["dcg"], dcg, rtol=2e-6, atol=0)
    np.testing.assert_allclose(out["ap"], ap, rtol=2e-6, atol=0)
    return above, pos


def mixed_sets(c, rng, n_users=96, nan_items=()):
    """Held-out sets for the case's users: the planted rows' positives, random items, Seen items, NaN items, empty sets,
    one user listed twice."""
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    off, items = c["seen"]
    rows = c["rows"]
    lists = []
    for x, u in enumerate(rng.choice(U, size=n_users, replace=False)):
        it = set(rows[rows[:, 0] == u, 1].tolist())
        it.update(rng.choice(I, size=[0, 1, 4, 30, 200][x % 5], replace=False).tolist())
        s = items[off[u]:off[u + 1]]
        if len(s) and x % 4 == 1:
            it.update(s[:3].tolist())
        if x % 3 == 2:
            it.update(nan_items)
        if x % 11 == 10:
            it = set()
        lists.append((int(u), it))
    lists.insert(5, lists[20])
    return held_out_csr(U, lists)


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("kind", ["random", "near_tie"])
def test_exact_against_reference(d, kind):
    c = random_case(d, seed=40 + d) if kind == "random" else near_tie_case(d, seed=50 + d)
    rng = np.random.RandomState(d)
    nan_items = (7, 4000) if kind == "random" else ()
    for i in nan_items:
        c["wi"][i, 3] = np.nan
    wu, wi, seen = c["wu"], c["wi"], c["seen"]
    users, off, items = mixed_sets(c, rng, nan_items=nan_items)
    eng = engine(d)
    out = run(eng, wu, wi, users, off, items, seen)
    above, pos = check(out, wu, wi, users, off, items, seen)
    assert (pos == -1).any() and (np.diff(off) == 0).any() and len(set(users.tolist())) < len(users)
    # above is sml_full_rank's rank of every (u, p)
    rows = np.stack([np.repeat(users, np.diff(off)), items.astype(np.int64)], 1)
    rank = eng.full_rank(gpu(wu), gpu(wi), gpu(rows), (gpu(seen[0]), gpu(seen[1]))).cpu().numpy()
    np.testing.assert_array_equal(out["above"], rank)
    # pos < 128 exactly when p sits at index pos of u's top-128 list
    lists, _ = eng.topk_items(gpu(wu), gpu(wi), gpu(users), 128, (gpu(seen[0]), gpu(seen[1])))
    lists = lists.cpu().numpy()
    for x in range(len(users)):
        for e in range(off[x], off[x + 1]):
            at = np.nonzero(lists[x] == items[e])[0]
            if 0 <= pos[e] < 128:
                assert len(at) == 1 and at[0] == pos[e], (x, e)
            else:
                assert len(at) == 0, (x, e)
    # two calls, identical bytes
    again = run(eng, wu, wi, users, off, items, seen)
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize("d", [32, 64])
def test_large_held_out_sets(d):
    """m = 1, m = 5,000 and m = every eligible item (global-memory thresholds), beside short sets (LDS window)."""
    rng = np.random.RandomState(70 + d)
    U, I = 8, 6007
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(I, d).astype(np.float32)
    wi[rng.choice(I, size=40, replace=False)] = wi[rng.choice(I, size=40, replace=False)]     # exact ties
    wi[11, 0] = np.nan
    seen_l = {u: rng.choice(I, size=300, replace=False) for u in range(U)}
    from _fp32_chain import seen_csr
    seen = seen_csr(U, I, seen_l)
    S = user_scores(wu, wi, np.arange(U))
    every = [i for i in range(I) if i not in set(seen_l[2].tolist()) and not np.isnan(S[2, i])]
    lists = [(0, [int(rng.randint(I))]), (1, rng.choice(I, size=5000, replace=False)), (2, every),
             (3, rng.choice(I, size=33, replace=False)), (4, rng.choice(I, size=32, replace=False)), (2, [every[0]])]
    users, off, items = held_out_csr(U, lists)
    out = run(engine(d), wu, wi, users, off, items, seen)
    _, pos = check(out, wu, wi, users, off, items, seen)
    # every eligible item held out: the positions are exactly 0 .. m - 1
    assert sorted(pos[off[2]:off[3]].tolist()) == list(range(len(every)))


@pytest.mark.parametrize("n_item", [1, 2, 5, 31, 32, 33])
def test_small_catalogues(n_item):
    rng = np.random.RandomState(n_item)
    d, U = 32, 70
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(n_item, d).astype(np.float32)
    lists = [(u, rng.choice(n_item, size=rng.randint(0, n_item + 1), replace=False)) for u in range(U)]
    from _fp32_chain import seen_csr
    seen = seen_csr(U, n_item, {u: rng.choice(n_item, size=rng.randint(0, 2), replace=False) for u in range(U)})
    users, off, items = held_out_csr(U, lists)
    for s in (None, seen):
        out = run(engine(d), wu, wi, users, off, items, s)
        check(out, wu, wi, users, off, items, s)


def test_chunked_call_is_identical():
    c = random_case(32, seed=90)
    users, off, items = mixed_sets(c, np.random.RandomState(90))
    eng = engine(32)
    whole = run(eng, c["wu"], c["wi"], users, off, items, c["seen"])
    eng.USER_RANK_SCRATCH_BYTES = 4096          # a few users per call
    try:
        parts = run(eng, c["wu"], c["wi"], users, off, items, c["seen"])
    finally:
        del eng.USER_RANK_SCRATCH_BYTES
    for k in whole:
        assert whole[k].tobytes() == parts[k].tobytes(), k


def test_empty_calls():
    eng = engine(32)
    wu = torch.randn(10, 32, device=DEV)
    wi = torch.randn(20, 32, device=DEV)
    out = eng.user_ranks(wu, wi, np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert out["pos"].numel() == 0 and out["hits"].shape == (0, 1)
    out = eng.user_ranks(wu, wi, np.array([3, 4]), np.zeros(3, np.int64), np.zeros(0, np.int32), ks=(5, 10))
    assert out["hits"].cpu().tolist() == [[0, 0], [0, 0]] and out["first"].cpu().tolist() == [-1, -1]


def test_argument_checks():
    from sml_amd._lib import SmlError
    eng = engine(32)
    lib = eng.lib
    tu = torch.zeros(10, 32, device=DEV)
    ti = torch.zeros(20, 32, device=DEV)
    users = torch.zeros(1, dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    items = torch.zeros(1, dtype=torch.int32, device=DEV)
    soff = torch.zeros(11, dtype=torch.int64, device=DEV)
    o32 = torch.empty(1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(1 << 12, dtype=torch.uint8, device=DEV)
    args = lambda n_item, n_pos, so, si: (eng._ctx, tu.data_ptr(), ti.data_ptr(), n_item, users.data_ptr(), 1,  # noqa: E731
                                          off.data_ptr(), items.data_ptr(), n_pos, so, si, scratch.data_ptr(),
                                          o32.data_ptr(), o32.data_ptr(), None)
    assert lib.sml_user_rank(*args(20, 1, soff.data_ptr(), None)) != 0      # exactly one of the CSR arrays
    assert lib.sml_user_rank(*args(20, 1, None, items.data_ptr())) != 0
    assert lib.sml_user_rank(*args(0, 1, None, None)) != 0                  # n_item <= 0
    assert lib.sml_user_rank(*args(1 << 31, 1, None, None)) != 0            # n_item >= 2^31
    assert lib.sml_user_rank(*args(20, 1 << 31, None, None)) != 0           # n_pos >= 2^31
    assert lib.sml_user_rank(*args(20, -1, None, None)) != 0
    assert lib.sml_user_rank_scratch_bytes(eng._ctx, 1, 1 << 31, 20) < 0
    assert lib.sml_user_rank_scratch_bytes(eng._ctx, 1, 1, 0) < 0
    assert lib.sml_user_rank(eng._ctx, tu.data_ptr(), ti.data_ptr(), 20, users.data_ptr(), 1, off.data_ptr(),
                             items.data_ptr(), 1, None, None, None, o32.data_ptr(), o32.data_ptr(), None) != 0   # null scratch
    hits = torch.empty(1, dtype=torch.int32, device=DEV)
    f32 = torch.empty(1, dtype=torch.float32, device=DEV)
    ks1 = np.array([5], np.int32)
    margs = lambda p, n: (eng._ctx, p, off.data_ptr(), n, ks1.ctypes.data, 1, hits.data_ptr(), f32.data_ptr(),  # noqa: E731
                          f32.data_ptr(), o32.data_ptr(), None)
    assert lib.sml_user_metrics(*margs(None, 1)) != 0                        # null pos
    assert lib.sml_user_metrics(*margs(o32.data_ptr(), 1 << 31)) != 0        # n >= 2^31
    big = (eng._ctx, tu.data_ptr(), ti.data_ptr(), 20, users.data_ptr(), 1 << 31, off.data_ptr(), items.data_ptr(), 1,
           None, None, scratch.data_ptr(), o32.data_ptr(), o32.data_ptr(), None)
    assert lib.sml_user_rank(*big) != 0                                     # n >= 2^31
    assert lib.sml_user_rank_scratch_bytes(eng._ctx, 1 << 31, 1, 20) < 0
    for ks in ((0,), (5, -1), tuple(range(1, 10)), ()):
        with pytest.raises((SmlError, ValueError)):
            eng.user_ranks(tu, ti, users, np.array([0, 1]), items, ks=ks)
    with pytest.raises(ValueError):
        eng.user_ranks(tu, ti, users, np.array([0, 2]), items)                # pos_off does not end at n_pos
    e128 = engine(128)
    with pytest.raises(SmlError):
        e128.user_ranks(torch.zeros(10, 128, device=DEV), torch.zeros(20, 128, device=DEV), users, np.array([0, 1]), items)
    out = eng.user_ranks(tu, ti, users, np.array([0, 1]), items, (soff, torch.zeros(0, dtype=torch.int32)))
    assert out["above"].cpu().tolist() == [0] and out["pos"].cpu().tolist() == [0]


def test_model_layers_and_no_rng_draw():
    from sml_amd.evaluation import test_model_users, user_metrics
    from sml_amd.retrieval import SeenItems, held_out
    rng = np.random.RandomState(5)
    U, I, d = 120, 3000, 32
    wu = (rng.randn(U, d) * 0.3).astype(np.float32)
    wi = (rng.randn(I, d) * 0.3).astype(np.float32)
    mf = make_mf(U, I, d, wu, wi, device=DEV)
    seen = SeenItems(U, I).add(np.stack([rng.randint(0, U, 4000), rng.randint(0, I, 4000)], 1))
    test = np.stack([rng.randint(0, U, 900), rng.randint(0, I, 900), rng.randint(0, I, 900)], 1)
    old_user, old_item = set(range(0, U, 2)), np.arange(0, I, 3)
    t_state, n_state = torch.get_rng_state(), np.random.get_state()
    got = test_model_users(mf, test, seen=seen, topK=(20, 10, 5), old_user=old_user, old_item=old_item)
    assert torch.equal(t_state, torch.get_rng_state()) and np.random.get_state()[1].tolist() == n_state[1].tolist()
    sets = held_out(test, U, I)
    out = mf.test_users(sets, topK=(20, 10, 5), exclude=seen)
    users, off, items = out["users"], out["pos_off"], out["pos_items"]
    assert got["users"] == len(users) == len(np.unique(test[:, 0]))
    above, pos = ref_user_rank(wu, wi, users, off, items, seen.host())
    np.testing.assert_array_equal(out["pos"].cpu().numpy(), pos)
    hits, dcg, ap, first = ref_user_metrics(pos, off, (20, 10, 5))
    want = user_metrics(dict(users=users, pos_off=off, pos_items=items, ks=(20, 10, 5), pos=pos, hits=hits, dcg=dcg,
                             ap=ap, first=first), old_user, old_item)
    for k in ("recall", "precision", "ndcg", "ndcg_ref", "map", "mrr"):
        for K in (20, 10, 5):
            assert got[k][K] == pytest.approx(want[k][K], rel=1e-5), (k, K)
    assert got["hit_shares"] == want["hit_shares"]


@pytest.mark.parametrize("d", [32, 64])
def test_repeated_held_out_items_stay_in_bounds(d):
    """A range that repeats an item (against the header's precondition) is still sorted as a permutation: every copy
    gets the item's above / pos, and nothing is written outside the outputs or the scratch."""
    rng = np.random.RandomState(300 + d)
    U, I = 40, 3001
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(I, d).astype(np.float32)
    wi[17, 1] = np.nan
    from _fp32_chain import seen_csr
    seen = seen_csr(U, I, {u: rng.choice(I, size=50, replace=False) for u in range(U)})
    s_off, s_items = seen
    lists = [[3, 3, 7, 7, 7, 9], [17, 17, 17], [int(s_items[s_off[2]])] * 4 + [5], [11] * 40,
             np.repeat(rng.choice(I, size=700, replace=False), 3), rng.choice(I, size=200), [], [8]]
    users = np.arange(len(lists), dtype=np.int64)
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    items = np.concatenate([np.sort(np.asarray(x, np.int64)) for x in lists]).astype(np.int32)
    n, n_pos = len(users), len(items)
    eng = engine(d)
    lib = eng.lib
    G = 1024
    sentinel = -12345
    above = torch.full((n_pos + 2 * G,), sentinel, dtype=torch.int32, device=DEV)
    pos = torch.full((n_pos + 2 * G,), sentinel, dtype=torch.int32, device=DEV)
    nbytes = int(lib.sml_user_rank_scratch_bytes(eng._ctx, n, n_pos, I))
    scratch = torch.full((nbytes + 4 * G,), 0xAB, dtype=torch.uint8, device=DEV)
    tu, ti, tusers, toff, titems = gpu(wu), gpu(wi), gpu(users), gpu(off), gpu(items)
    tso, tsi = gpu(s_off), gpu(s_items)
    rc = lib.sml_user_rank(eng._ctx, tu.data_ptr(), ti.data_ptr(), I, tusers.data_ptr(), n, toff.data_ptr(), titems.data_ptr(),
                           n_pos, tso.data_ptr(), tsi.data_ptr(), scratch.data_ptr(), above[G:].data_ptr(), pos[G:].data_ptr(),
                           None)
    assert rc == 0
    torch.cuda.synchronize()
    a, p, sc = above.cpu().numpy(), pos.cpu().numpy(), scratch.cpu().numpy()
    assert (a[:G] == sentinel).all() and (a[G + n_pos:] == sentinel).all()
    assert (p[:G] == sentinel).all() and (p[G + n_pos:] == sentinel).all()
    assert (sc[nbytes:] == 0xAB).all()
    want_a, want_p = ref_user_rank(wu, wi, users, off, items, seen)
    np.testing.assert_array_equal(a[G:G + n_pos], want_a)
    np.testing.assert_array_equal(p[G:G + n_pos], want_p)
    # metrics over repeated pos values: every output written, repeated values summed once
    out = eng.user_ranks(tu, ti, users, off, items, (tso, tsi), KS)
    torch.cuda.synchronize()
    hits, dcg, ap, first = ref_user_metrics(want_p, off, KS)
    np.testing.assert_array_equal(out["hits"].cpu().numpy(), hits)
    np.testing.assert_array_equal(out["first"].cpu().numpy(), first)
    np.testing.assert_allclose(out["dcg"].cpu().numpy(), dcg, rtol=2e-6, atol=0)
    np.testing.assert_allclose(out["ap"].cpu().numpy(), ap, rtol=2e-6, atol=0)


def test_metrics_write_every_output_for_repeated_positions():
    eng = engine(32)
    off = np.array([0, 5, 9, 9, 12], np.int64)
    pos = np.array([2, 2, 0, 7, 7, -1, 3, 3, -1, 40, 1, 1], np.int32)
    ks = np.array([1, 3, 8, 50], np.int32)
    n = len(off) - 1
    hits = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    dcg = torch.full((n, 4), float("nan"), device=DEV)
    ap = torch.full((n, 4), float("nan"), device=DEV)
    first = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tpos, toff = gpu(pos), gpu(off)
    assert eng.lib.sml_user_metrics(eng._ctx, tpos.data_ptr(), toff.data_ptr(), n, ks.ctypes.data, 4, hits.data_ptr(),
                                    dcg.data_ptr(), ap.data_ptr(), first.data_ptr(), None) == 0
    torch.cuda.synchronize()
    h, dd, aa, ff = ref_user_metrics(pos, off, tuple(ks.tolist()))
    np.testing.assert_array_equal(hits.cpu().numpy(), h)
    np.testing.assert_array_equal(first.cpu().numpy(), ff)
    np.testing.assert_allclose(dcg.cpu().numpy(), dd, rtol=2e-6, atol=0)
    np.testing.assert_allclose(ap.cpu().numpy(), aa, rtol=2e-6, atol=0)
