"""The adjusted score A(u, i) = fmaf(S(u, i), scale[i], offset[i]) of full-catalogue retrieval on the MI355X
(sml_*_adjusted through HipEngine, MFbasemode / MF2 and sml_amd.evaluation).

Every comparison is exact: ranks, lists, score bits, above / pos against brute-force references over the adjusted score
matrix on the fp32 chain (tests/_item_score_cases.py).  Shapes: U = 300, I = 4,099 (129 tiles, 8 slices, a last tile of 3
items), n = 256, k in {1, 20, 128}."""
import functools

import numpy as np
import pytest
import torch

import _fp32_chain as F
import _item_score_cases as C
from _item_filter_cases import pack, random_mask, seen_prime
from _user_rank_ref import held_out_csr, ref_user_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (20, 10, 5)
TOPK = (1, 20, 128)
CASES = [("fp32", 32), ("fp32", 64), ("fp16", 32), ("fp16", 64), ("fp16", 128)]


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(seen):
    return None if seen is None else (gpu(seen[0]), gpu(seen[1]))


def words_dev(mask):
    return None if mask is None else gpu(pack(mask).view(np.int32))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(bits(a), bits(b)), what


@functools.lru_cache(maxsize=None)
def case(dtype, d, base="random"):
    """The seeded case, its tables on the device, the reference score matrices S and A, and held-out sets -- built once."""
    c = C.score_case(dtype, d, base=base)
    c["tu"], c["ti"] = gpu(c["wu"]), gpu(c["wi"])
    c["A"] = C.adjusted(C.case_scores(c), c["scale"][None], c["offset"][None])
    c["adj"] = gpu(C.pad_adj(c["scale"], c["offset"]))
    c["held"] = C.held_sets(c, 40)
    return c


def run_all(eng, c, seen, mask, adj, ks=TOPK, tables=None, n_users=64):
    """Every output of the three calls as a flat dict of device tensors."""
    tu, ti = tables or (c["tu"], c["ti"])
    seen, allow = csr_dev(seen), words_dev(mask)
    out = {"rank": eng.full_rank(tu, ti, gpu(c["rows"]), seen, allow=allow, adjust=adj)}
    for k in ks:
        out["items%d" % k], out["scores%d" % k] = eng.topk_items(tu, ti, gpu(c["users"][:n_users]), k, seen, allow=allow, adjust=adj)
    hu, hoff, hit = c["held"]
    ur = eng.user_ranks(tu, ti, hu, hoff, hit, seen, KS, allow=allow, adjust=adj)
    out.update(("ur_" + k, v) for k, v in ur.items())
    return out


def check_exact(got, c, A, seen, mask, ks=TOPK, n_users=64):
    """The outputs of run_all against the brute-force references on the score matrix A."""
    np.testing.assert_array_equal(got["rank"].cpu().numpy(), C.ref_rank(A, c["rows"], seen, mask))
    for k in ks:
        want_i, want_s = C.ref_topk(A, c["users"][:n_users], k, seen, mask)
        np.testing.assert_array_equal(got["items%d" % k].cpu().numpy(), want_i)
        np.testing.assert_array_equal(got["scores%d" % k].cpu().numpy().view(np.int32), want_s.view(np.int32))
    hu, hoff, hit = c["held"]
    above, pos = C.ref_user_rank(A, hu, hoff, hit, seen, mask)
    np.testing.assert_array_equal(got["ur_above"].cpu().numpy(), above)
    np.testing.assert_array_equal(got["ur_pos"].cpu().numpy(), pos)
    hits, dcg, ap, first = ref_user_metrics(pos, hoff, KS)
    np.testing.assert_array_equal(got["ur_hits"].cpu().numpy(), hits)
    np.testing.assert_array_equal(got["ur_first"].cpu().numpy(), first)
    # dcg / ap: fp32 sums of at most 20 terms in [0, 1] against float64 -- 20 roundings of 2^-24 relative, as the filter tests
    np.testing.assert_allclose(got["ur_dcg"].cpu().numpy(), dcg, rtol=2e-6, atol=0)
    np.testing.assert_allclose(got["ur_ap"].cpu().numpy(), ap, rtol=2e-6, atol=0)


# ---- exactness -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_seen", [True, False], ids=["seen", "noseen"])
@pytest.mark.parametrize("dtype,d", CASES)
def test_exact(dtype, d, with_seen):
    c = case(dtype, d)
    assert c["wi"].shape[0] == 4099 and c["wu"].shape[0] == 300 and len(c["rows"]) == 256
    seen = c["seen"] if with_seen else None
    check_exact(run_all(engine(d), c, seen, None, c["adj"]), c, c["A"], seen, None)


@pytest.mark.parametrize("base", ["near_tie", "near_tie_offset"])
def test_exact_on_near_ties(base):
    """near_tie_case (fp32, d = 32) with scales in [0.25, 4] and offset +0: the planted near-ties of S stay near-ties of A;
    near_tie_offset: copies of a positive share its scale and a small non-zero offset, so A's near-ties pass the fma's rounding."""
    c = case("fp32", 32, base)
    check_exact(run_all(engine(32), c, c["seen"], None, c["adj"]), c, c["A"], c["seen"], None)


def test_item_score_object_and_engine_builder_give_the_same_table():
    from sml_amd.retrieval import ItemScore
    c = case("fp32", 32)
    eng = engine(32)
    score = ItemScore(4099).scale(c["scale"]).offset(c["offset"])
    a = score.device(eng)
    assert a is score.device(eng, c["ti"])                                         # cached
    same_bytes(a, c["adj"], "ItemScore.device")
    same_bytes(eng.item_adjust(4099, gpu(c["scale"]), c["offset"]), c["adj"], "item_adjust")
    same_bytes(eng.item_adjust(4099), gpu(C.pad_adj(np.ones(4099), np.zeros(4099))), "neutral")
    rows = gpu(c["rows"])
    same_bytes(eng.full_rank(c["tu"], c["ti"], rows, adjust=score), eng.full_rank(c["tu"], c["ti"], rows, adjust=c["adj"]), "rank")
    score.offset(np.zeros(4099))
    assert score.device(eng) is not a
    odd = torch.empty(2 * 4128 + 1, device=DEV)[1:].view(2, 4128)                    # contiguous, right shape, 4 bytes off
    assert odd.data_ptr() % 16 == 4
    for bad in (c["adj"][:, :-32], c["adj"].double(), c["adj"].cpu(), c["adj"].t().contiguous().t(), "cosine", odd):
        with pytest.raises(ValueError):
            eng.full_rank(c["tu"], c["ti"], rows, adjust=bad)


# ---- the dispatch: every (width, element type, filter, terms) cell -------------------------------------------------------

@pytest.mark.parametrize("adjusted", [False, True], ids=["bare", "terms"])
@pytest.mark.parametrize("filtered", [False, True], ids=["all", "half"])
@pytest.mark.parametrize("dtype,d", CASES)
def test_every_instantiation_is_the_one_asked_for(dtype, d, filtered, adjusted):
    """One selector turns (d, element type, filter given, terms given) into a kernel instantiation; a cell wired to a
    neighbour's flags is how it can go wrong.  Every cell of 5 x 2 x 2 runs full_rank, topk_items (K = 20) and user_ranks
    on score_case (4,099 items: 129 tiles, 17 per slice, so the prefetch and the partial last tile run; 96 rows, 64 users, 40
    held-out sets) against the CPU references -- on Seen' for the filter, on A for the terms, on S without them -- exactly.
    That ignoring the random 50 % filter or these terms changes the references is what the host tests
    test_filters_have_teeth_on_the_cpu_references and test_terms_have_teeth_on_the_cpu_references show; here the cell's
    reference ranks are also checked to differ from those of the two neighbouring cells."""
    c = dict(case(dtype, d))
    c["rows"] = c["rows"][:96]
    assert c["wi"].shape[0] == 4099 and len(c["held"][0]) <= 60
    mask = random_mask(4099, 0.5, seed=7)

    def reference(f, a):                                    # (Seen or Seen', S or A) of the cell (f, a)
        return (seen_prime(c["seen"], mask, 300) if f else c["seen"]), (c["A"] if a else C.case_scores(c))

    seen, A = reference(filtered, adjusted)
    got = run_all(engine(d), c, c["seen"], mask if filtered else None, c["adj"] if adjusted else None, ks=(20,))
    check_exact(got, c, A, seen, None, ks=(20,))
    want = C.ref_rank(A, c["rows"], seen)
    for other in (reference(not filtered, adjusted), reference(filtered, not adjusted)):
        assert (C.ref_rank(other[1], c["rows"], other[0]) != want).sum() >= 48


# ---- neutral adjust ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "filtered"])
@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp32", 64), ("fp16", 128)])
def test_neutral_adjust_returns_the_unadjusted_outputs(dtype, d, filtered):
    c = case(dtype, d)
    eng = engine(d)
    mask = random_mask(4099, 0.5, seed=d) if filtered else None
    want = run_all(eng, c, c["seen"], mask, None)
    got = run_all(eng, c, c["seen"], mask, eng.item_adjust(4099))
    for key in want:
        if want[key].dtype == torch.float32 and key.startswith("scores"):
            assert torch.equal(got[key], want[key]), key                            # equal as values (-0 becomes +0)
        else:
            same_bytes(got[key], want[key], key)


# ---- filter composition --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep", [0.5, 0.05])
@pytest.mark.parametrize("dtype,d", [("fp32", 64), ("fp16", 32), ("fp16", 128)])
def test_adjusted_filter_equals_adjusted_seen_prime(dtype, d, keep):
    c = case(dtype, d)
    eng = engine(d)
    mask = random_mask(4099, keep, seed=d + 1)
    got = run_all(eng, c, c["seen"], mask, c["adj"])
    want = run_all(eng, c, seen_prime(c["seen"], mask, 300), None, c["adj"])
    for key in want:
        same_bytes(got[key], want[key], key)
    if keep == 0.5 and d != 32:
        check_exact(got, c, c["A"], c["seen"], mask, ks=(20,))


# ---- fp16 against fp32 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [32, 64])
def test_fp16_tables_equal_fp32_copies(d):
    c = case("fp16", d)
    eng = engine(d)
    mask = random_mask(4099, 0.5, seed=3)
    for m in (None, mask):
        h = run_all(eng, c, c["seen"], m, c["adj"])
        f = run_all(eng, c, c["seen"], m, c["adj"], tables=(c["tu"].float(), c["ti"].float()))
        for key in f:
            same_bytes(h[key], f[key], key)


# ---- pads ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_item", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp16", 128)])
def test_garbage_in_the_pads_changes_nothing(dtype, d, n_item):
    rng = np.random.RandomState(200 + n_item)
    U = 40
    wu = rng.randn(U, d).astype(np.float32 if dtype == "fp32" else np.float16)
    wi = rng.randn(n_item, d).astype(wu.dtype)
    rows = np.stack([rng.randint(0, U, 40), rng.randint(0, n_item, 40)], 1).astype(np.int64)
    seen = F.seen_csr(U, n_item, {u: rng.choice(n_item, size=rng.randint(0, min(n_item, 6) + 1), replace=False) for u in range(U)})
    scale, offset = rng.uniform(0.25, 4, n_item).astype(np.float32), rng.randn(n_item).astype(np.float32)
    c = dict(wu=wu, wi=wi, rows=rows, users=np.arange(U), seen=seen, tu=gpu(wu), ti=gpu(wi),
             held=held_out_csr(U, [(u, rng.choice(n_item, size=min(n_item, 3), replace=False)) for u in range(0, U, 2)]))
    eng = engine(d)
    A = C.adjusted(F.score_chain(wu.astype(np.float32), wi.astype(np.float32)), scale[None], offset[None])
    clean = run_all(eng, c, seen, None, gpu(C.pad_adj(scale, offset)), ks=(1, 20), n_users=U)
    check_exact(clean, c, A, seen, None, ks=(1, 20), n_users=U)
    for ps, po in ((np.nan, np.nan), (np.inf, -np.inf), (-np.inf, np.inf), (0.0, np.nan)):
        dirty = run_all(eng, c, seen, None, gpu(C.pad_adj(scale, offset, ps, po)), ks=(1, 20), n_users=U)
        for key in clean:
            same_bytes(dirty[key], clean[key], "%s with pads (%s, %s)" % (key, ps, po))
    mask = rng.rand(n_item) < 0.5
    a = run_all(eng, c, seen, mask, gpu(C.pad_adj(scale, offset, np.nan, np.inf)), ks=(20,), n_users=U)
    check_exact(a, c, A, seen, mask, ks=(20,), n_users=U)


# ---- skipped tiles -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp32", 64), ("fp16", 128)])
def test_skipped_tiles_do_not_let_the_adj_prefetch_drift(dtype, d):
    """The construction of test_item_filter_gpu.test_skipped_tiles_and_seen_cursor (empty slices, isolated tiles between long
    empty runs, one bit in a last tile) with terms that differ from tile to tile: a prefetch that fell behind or ran ahead by
    a tile would apply a neighbour's terms."""
    from test_item_filter_gpu import skip_filter
    from _half_cases import random_half_case, widen
    U, I, n = 70, 32 * 8 * 24 + 5, 64
    slices, slice_tiles, _ = F.rank_plan(n, I)
    assert (slices, slice_tiles) == (8, 25)
    c = F.random_case(d, 17, U=U, I=I, n=n) if dtype == "fp32" else random_half_case(d, 17, U=U, I=I, n=n)
    rng = np.random.RandomState(18)
    mask, tile_on = skip_filter(I, slice_tiles, slices, rng)
    tile = np.arange(I) // 32
    scale = (0.5 + (tile % 7)).astype(np.float32) * rng.uniform(0.9, 1.1, I).astype(np.float32)
    offset = ((tile % 5) - 2).astype(np.float32) + rng.randn(I).astype(np.float32) * np.float32(0.1)
    c.update(tu=gpu(c["wu"]), ti=gpu(c["wi"]))
    t_a = 3 * slice_tiles + 5
    c["held"] = held_out_csr(U, [(int(u), set(rng.choice(I, 6, replace=False).tolist()) | {t_a * 32, t_a * 32 + 31, I - 1})
                                 for u in rng.choice(U, 24, replace=False)])
    ru, ri = (c["wu"], c["wi"]) if dtype == "fp32" else (widen(c["wu"]), widen(c["wi"]))
    A = C.adjusted(F.score_chain(ru, ri), scale[None], offset[None])
    adj = gpu(C.pad_adj(scale, offset))
    eng = engine(d)
    for seen in (c["seen"], None):
        got = run_all(eng, c, seen, mask, adj, ks=(1, 20), n_users=n)
        check_exact(got, c, A, seen, mask, ks=(1, 20), n_users=n)


# ---- NaN / -inf / zero-scale rules ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp16", 128)])
def test_nan_neg_inf_and_zero_scale_rules(dtype, d):
    c = case(dtype, d)
    eng = engine(d)
    sp, rows, A = c["special"], c["rows"], c["A"]
    gone = np.concatenate([sp["nan_offset"], sp["nan_scale"]])
    assert np.isnan(A[:, gone]).all() and np.isneginf(A[:, sp["neg_inf"]]).all()
    assert (A[:, sp["zero_scale"]] == c["offset"][sp["zero_scale"]][None]).all()        # scale 0: A is the offset
    rank = eng.full_rank(c["tu"], c["ti"], gpu(rows), None, adjust=c["adj"]).cpu().numpy()
    is_nan, is_ninf = np.isin(rows[:, 1], gone), np.isin(rows[:, 1], sp["neg_inf"])
    assert is_nan.sum() >= 6 and is_ninf.sum() >= 4
    assert (rank[is_nan] == 0).all()                                                     # a NaN positive ranks 0
    n_real = 4099 - len(gone) - len(sp["neg_inf"])
    assert (rank[is_ninf] == n_real).all()                                               # every non-NaN, non -inf item is above; ties are not
    users = gpu(np.arange(8))
    K = 128
    it, sc = eng.topk_items(c["tu"], c["ti"], users, K, None, adjust=c["adj"])
    assert not np.isin(it.cpu().numpy(), gone).any()                                     # a NaN item enters no list
    # a catalogue of the special items and 20 others: the -inf items fill the tail by id, the NaN items leave padding
    keep = np.zeros(4099, bool)
    others = np.setdiff1d(np.arange(4099), np.concatenate(list(sp.values())))[:20]
    keep[np.concatenate([others, gone, sp["neg_inf"]])] = True
    it, sc = eng.topk_items(c["tu"], c["ti"], users, K, None, allow=keep, adjust=c["adj"])
    it, sc = it.cpu().numpy(), sc.cpu().numpy()
    n_inf = len(sp["neg_inf"])
    assert (np.sort(it[:, :20], 1) == np.sort(others)).all()
    assert (it[:, 20:20 + n_inf] == np.sort(sp["neg_inf"])).all() and np.isneginf(sc[:, 20:20 + n_inf]).all()
    assert (it[:, 20 + n_inf:] == -1).all() and np.isneginf(sc[:, 20 + n_inf:]).all()
    # held out: a NaN item has pos -1 and above 0; a -inf item keeps a pos, after every finite item
    held = held_out_csr(300, [(u, np.concatenate([gone[:3], sp["neg_inf"][:3], others[:2]])) for u in (0, 5)])
    out = eng.user_ranks(c["tu"], c["ti"], held[0], held[1], held[2], None, KS, adjust=c["adj"])
    pos, above = out["pos"].cpu().numpy(), out["above"].cpu().numpy()
    h_nan, h_inf = np.isin(held[2], gone), np.isin(held[2], sp["neg_inf"])
    assert (pos[h_nan] == -1).all() and (above[h_nan] == 0).all()
    assert (above[h_inf] == n_real).all() and (pos[h_inf] >= n_real).all() and (pos[h_inf] < n_real + n_inf).all()


# ---- cosine builder ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", CASES)
def test_cosine_builder_matches_numpy_bit_for_bit(dtype, d):
    from sml_amd.retrieval import ItemScore
    rng = np.random.RandomState(d)
    n_item = 4099
    wi = (rng.randn(n_item, d) * rng.uniform(0.01, 30, (n_item, 1))).astype(np.float32 if dtype == "fp32" else np.float16)
    wi[77] = 0                                                                           # the zero row
    wi[78] = wi.dtype.type(2.0 ** -20)                                                   # a tiny one
    ti = gpu(wi)
    eng = engine(d)
    want = C.cosine_scale(wi.astype(np.float32))
    assert want[77] == 0 and np.isfinite(want).all()
    adj = eng.item_adjust_cosine(ti)
    assert adj.shape == (2, 4128) and adj.dtype == torch.float32
    got = adj.cpu().numpy()
    np.testing.assert_array_equal(got[0, :n_item].view(np.int32), want.view(np.int32))
    assert (got[0, n_item:] == 1).all() and (got[1] == 0).all()
    # plane 1 is not touched when a table is given
    mine = eng.item_adjust(n_item, offset=np.arange(n_item, dtype=np.float32))
    assert eng.item_adjust_cosine(ti, mine) is mine
    np.testing.assert_array_equal(mine.cpu().numpy()[1, :n_item], np.arange(n_item, dtype=np.float32))
    np.testing.assert_array_equal(mine.cpu().numpy()[0].view(np.int32), got[0].view(np.int32))
    # a cosine ItemScore is resolved against the table at every call
    score = ItemScore(n_item).cosine()
    a = score.device(eng, ti)
    same_bytes(a, adj, "ItemScore.cosine")
    ti[5] *= 2
    b = score.device(eng, ti)
    assert float(b[0, 5]) != float(a[0, 5])
    # the zero row scores 0 against every user, not NaN
    tu = gpu(rng.randn(8, d).astype(wi.dtype))
    it, sc = eng.topk_items(tu, ti, gpu(np.arange(8)), 128, None, allow=np.isin(np.arange(n_item), [77, 78, 79]), adjust=b)
    assert (it[:, :3] >= 0).all() and (sc[(it == 77)] == 0).all() and (it == 77).sum() == 8


def test_cosine_item_score_follows_a_table_trained_in_place():
    """recommend with a cosine ItemScore, the item table changed in place the way training changes it (through .data: no
    version counter moves, the address stays), recommend again: the lists follow the new norms, as score="cosine" does."""
    from sml_amd.mf import MFbasemode
    from sml_amd.retrieval import ItemScore
    d, U, I = 32, 64, 1000
    mf = MFbasemode(U, I, d).to(DEV)
    users = gpu(np.arange(U))
    score = ItemScore(I).cosine()
    i0, s0 = mf.recommend(users, topK=20, score=score)
    w0, w1 = mf.recommend(users, topK=20, score="cosine")
    assert torch.equal(i0, w0) and torch.equal(bits(s0), bits(w1))
    ptr, ver = mf.item_laten.weight.data_ptr(), mf.item_laten.weight._version
    mf.item_laten.weight.data[::3] *= 5.0                                          # every third row five times as long
    opt = torch.optim.SGD([mf.item_laten.weight], lr=0.5)
    mf.item_laten.weight.grad = torch.randn_like(mf.item_laten.weight)
    opt.step()
    assert mf.item_laten.weight.data_ptr() == ptr and mf.item_laten.weight.data._version == 0
    i1, s1 = mf.recommend(users, topK=20, score=score)
    w0, w1 = mf.recommend(users, topK=20, score="cosine")
    assert torch.equal(i1, w0) and torch.equal(bits(s1), bits(w1))
    assert not torch.equal(i1, i0)
    out = mf.test_users((np.arange(U + 1) * 2, np.arange(2 * U) % I), topK=(20,), score=score)
    ref = mf.test_users((np.arange(U + 1) * 2, np.arange(2 * U) % I), topK=(20,), score="cosine")
    same_bytes(out["pos"], ref["pos"], "pos")


# ---- thresholds ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 64), ("fp16", 128)])
def test_positive_sits_at_rank_plus_smaller_id_ties(dtype, d):
    """The header's identity on A: with the same Seen and terms, the positive of an eligible row (u, p) sits at position
    rank + #{eligible i != p : A(u, i) == A(u, p), i < p} of u's adjusted list -- pos of sml_user_rank_adjusted says so at
    any depth, the list itself where that is < k.  rank and pos come from two kernels and two threshold sites; the planted
    copies (same row, same terms, other ids) make the tie term non-zero."""
    c = case(dtype, d)
    eng = engine(d)
    A, seen = c["A"], csr_dev(c["seen"])
    off, items = c["seen"]
    rows = c["rows"]
    # the positives of the planted rows, and for 64 users the items at places 0, 7 and 127 of their own lists
    K = 128
    lists, _ = eng.topk_items(c["tu"], c["ti"], gpu(c["users"][:64]), K, seen, adjust=c["adj"])
    lists = lists.cpu().numpy()
    extra = np.array([(u, lists[x, j]) for x, u in enumerate(c["users"][:64]) for j in (0, 7, 127)])
    rows = np.concatenate([rows[:, :2], extra])
    live = np.array([p not in items[off[u]:off[u + 1]] and not np.isnan(A[u, p]) for u, p in rows])
    rows = rows[live]
    rank = eng.full_rank(c["tu"], c["ti"], gpu(rows), seen, adjust=c["adj"]).cpu().numpy()
    hu, hoff, hit = held_out_csr(300, [(int(u), [int(p)]) for u, p in rows])               # one entry per row, in row order
    out = eng.user_ranks(c["tu"], c["ti"], hu, hoff, hit, seen, KS, adjust=c["adj"])
    pos, above = out["pos"].cpu().numpy(), out["above"].cpu().numpy()
    np.testing.assert_array_equal(above, rank)
    ties = np.zeros(len(rows), np.int64)
    for r, (u, p) in enumerate(rows):
        ok = np.ones(4099, bool)
        ok[items[off[u]:off[u + 1]]] = False
        ties[r] = int((ok[:p] & (A[u, :p] == A[u, p])).sum())
    np.testing.assert_array_equal(pos, rank + ties)
    assert (ties > 0).sum() >= 5                                                           # the planted copies with smaller ids
    it, _ = eng.topk_items(c["tu"], c["ti"], gpu(rows[:, 0]), K, seen, adjust=c["adj"])
    it = it.cpu().numpy()
    inside = pos < K
    assert inside.sum() >= 190 and (it[inside, pos[inside]] == rows[inside, 1]).all()


# ---- model surface -------------------------------------------------------------------------------------------------------

def test_model_surface():
    from sml_amd.evaluation import test_model_full, test_model_users, user_metrics
    from sml_amd.mf import MF2
    from sml_amd.retrieval import ItemFilter, ItemScore, SeenItems, held_out
    d, U, I = 32, 120, 3001
    rng = np.random.RandomState(71)
    mf = MF2(U, I, d)
    with torch.no_grad():                                            # dyadic tables and biases: every float64 score is exact and
        mf.user_laten.weight.copy_(torch.from_numpy(rng.randint(-8, 9, (U, d)) / 8.0))          # fp32 holds it, so fp32 == float64
        mf.item_laten.weight.copy_(torch.from_numpy(rng.randint(-8, 9, (I, d)) / 8.0))
        mf.item_bais.weight.copy_(torch.from_numpy(rng.permutation(I).reshape(I, 1) / 2.0 ** 18))   # distinct: a tie-free case
        mf.user_bais.weight.copy_(torch.from_numpy(rng.randint(-8, 9, (U, 1)) / 8.0))
    mf = mf.to(DEV)
    eng = engine(d)
    tu, ti = mf.user_laten.weight.data, mf.item_laten.weight.data
    users = gpu(np.arange(U))
    pairs = np.stack([rng.randint(0, U, 400), rng.randint(0, I, 400)], 1)
    seen = SeenItems(U, I).add(pairs)
    # MF2.recommend(score="bias") is the order of MF2.forward's score, computed in float64
    wu64, wi64 = tu.double().cpu().numpy(), ti.double().cpu().numpy()
    full = wu64 @ wi64.T + mf.item_bais.weight.data.double().cpu().numpy()[:, 0][None] + mf.user_bais.weight.data.double().cpu().numpy()
    off, its = seen.host()
    for u in range(U):
        full[u, its[off[u]:off[u + 1]]] = -np.inf
    assert all(len(np.unique(full[u])) >= I - 60 for u in range(0, U, 17))
    want = np.argsort(-full, axis=1, kind="stable")[:, :20]
    got_i, got_s = mf.recommend(users, topK=20, exclude=seen, score="bias")
    np.testing.assert_array_equal(got_i.cpu().numpy(), want)
    _, _, fwd = mf.forward(users[:, None].expand(-1, 20).reshape(-1), got_i.reshape(-1))
    ub = mf.user_bais.weight.data[:, 0]
    np.testing.assert_array_equal((got_s + ub[:, None]).cpu().numpy(), fwd.reshape(U, 20).cpu().numpy())     # exact on dyadic data
    # without score the call is what it was
    a_i, a_s = mf.recommend(users, topK=20, exclude=seen)
    b_i, b_s = eng.topk_items(tu, ti, users, 20, seen.device(DEV))
    assert torch.equal(a_i, b_i) and torch.equal(bits(a_s), bits(b_s))
    c_i, c_s = mf.recommend(users, topK=20, exclude=seen, score="dot")
    assert torch.equal(a_i, c_i) and torch.equal(bits(a_s), bits(c_s)) and not torch.equal(a_i, got_i)
    # an ItemScore with the bias is the same call
    e_i, e_s = mf.recommend(users, topK=20, exclude=seen, score=ItemScore(I).bias(mf.item_bais.weight.data))
    assert torch.equal(e_i, got_i) and torch.equal(bits(e_s), bits(got_s))
    # similar_items: real-valued tables
    with torch.no_grad():
        mf.item_laten.weight.copy_(torch.from_numpy(rng.randn(I, d).astype(np.float32)))
        mf.item_laten.weight[9] = 0
    ti = mf.item_laten.weight.data
    q = np.array([0, 5, 9, 700, I - 1, 5])
    wi = ti.cpu().numpy()
    scale = C.cosine_scale(wi)
    A = C.adjusted(F.score_chain(wi[q], wi), scale[None], np.zeros((1, I), np.float32))
    self_seen = (np.arange(len(q) + 1, dtype=np.int64), q.astype(np.int32))
    among = rng.rand(I) < 0.3
    for mask in (None, among):
        si, ss = mf.similar_items(q, topK=20, among=None if mask is None else ItemFilter.from_mask(mask))
        want_i, want_s = C.ref_topk(A, np.arange(len(q)), 20, self_seen, mask)
        np.testing.assert_array_equal(si.cpu().numpy(), want_i)
        assert not (si.cpu().numpy() == q[:, None]).any()                                  # the query is left out
        if mask is not None:
            assert mask[si.cpu().numpy()].all()
        np.testing.assert_array_equal(ss.cpu().numpy().view(np.int32), (want_s * scale[q][:, None]).astype(np.float32).view(np.int32))
    assert (ss[2] == 0).all()                                                              # the zero row: 0, not NaN
    wi_, ws_ = mf.similar_items(q, topK=5, exclude_self=False)
    assert (wi_[[0, 1, 3, 4, 5], 0].cpu().numpy() == q[[0, 1, 3, 4, 5]]).all()             # cosine 1 with itself comes first
    di, ds = mf.similar_items(q, topK=20, metric="dot")
    ei, es = eng.topk_items(ti, ti, gpu(q), 20, (gpu(np.arange(I + 1)), gpu(np.arange(I, dtype=np.int32))))
    assert torch.equal(di, ei) and torch.equal(bits(ds), bits(es))
    with pytest.raises(ValueError):
        mf.similar_items(q, metric="euclid")
    # evaluation: score= is passed on
    test = np.stack([rng.randint(0, U, 900), rng.randint(0, I, 900), rng.randint(0, I, 900)], 1)
    sets = held_out(test, U, I)
    for score in ("cosine", "bias"):
        out = mf.test_users(sets, topK=KS, exclude=seen, score=score)
        adj = eng.item_adjust_cosine(ti) if score == "cosine" else eng.item_adjust(I, offset=mf.item_bais.weight.data[:, 0])
        eo = eng.user_ranks(tu, ti, out["users"], out["pos_off"], out["pos_items"], seen.device(DEV), KS, adjust=adj)
        for key in ("above", "pos", "hits", "dcg", "ap", "first"):
            same_bytes(out[key], eo[key], key)
        assert test_model_users(mf, test, seen=seen, topK=KS, score=score) == user_metrics(out)
        ranks = eng.full_rank(tu, ti, gpu(test), seen.device(DEV), adjust=adj)
        h, nd, hit_rows = mf.test_full(gpu(test), topK=100, exclude=seen, score=score)
        assert torch.equal(hit_rows, (ranks < 100).nonzero()[:, 0]) and h == float((ranks < 100).sum())
        a = test_model_full(mf, [test[:400], test[400:]], seen=seen, topK=100, score=score)
        assert a[0] == h / len(test)
    assert test_model_users(mf, test, seen=seen, topK=KS, score=None) == test_model_users(mf, test, seen=seen, topK=KS)
