"""Per-user candidate lists on the MI355X: sml_topk_candidates through HipEngine.topk_candidates, MFbasemode.recommend(candidates=)
and MFbasemode.test_lists.

Every comparison is exact: item ids, score bits and n_elig against the CPU reference of tests/_candidates_cases.py (the
sibling suites' exact emulation with Seen' = Seen + (catalogue - list)), and row by row against the filtered topk_items call
on the device.  Shapes: U = 300, I = 4,099, at most 40 lists of at most a few hundred candidates, k in {1, 20, 128}."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _candidates_cases as K
import _item_score_cases as C
from _item_filter_cases import pack, random_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [("fp32", 32), ("fp32", 64), ("fp16", 32), ("fp16", 64), ("fp16", 128)]
TOPK = (1, 20, 128)
I = 4099


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(seen):
    return None if seen is None else (gpu(seen[0]), gpu(seen[1]))


def words_dev(mask):
    return gpu(pack(mask).view(np.int32))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bytes(a, b, what):
    for x, y, part in zip(a, b, ("items", "scores", "n_elig")):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, part)
        assert torch.equal(bits(x), bits(y)), (what, part)


def on_device(c):
    c["tu"], c["ti"] = gpu(c["wu"]), gpu(c["wi"])
    c["cand"] = tuple(gpu(t) for t in K.ragged(c["lists"], np.int64))
    return c


@functools.lru_cache(maxsize=None)
def boundary(dtype, d):
    """The case on the device and its reference at k = 128, computed once: the lists at smaller k are its prefixes."""
    c = on_device(K.boundary_case(dtype, d))
    c["want"] = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], K.KMAX, c["seen"])
    return c


def check_ref(got, want, k):
    """got of a call at k against the reference at KMAX."""
    it, sc, ne = want
    np.testing.assert_array_equal(got[0].cpu().numpy(), it[:, :k])
    np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), sc[:, :k].view(np.int32))
    np.testing.assert_array_equal(got[2].cpu().numpy(), ne)


# ---- 1. round boundaries --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", TOPK)
@pytest.mark.parametrize("dtype,d", CASES)
def test_round_boundaries(dtype, d, k):
    c = boundary(dtype, d)
    assert sorted(len(l) for l in c["lists"]) == sorted(K.LENGTHS * 3)
    eng = engine(d)
    got = eng.topk_candidates(c["tu"], c["ti"], c["users"], c["cand"], k, csr_dev(c["seen"]))
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    check_ref(got, c["want"], k)
    if dtype == "fp16" and d in (32, 64):             # the fp32 call on exact fp32 copies: the same bytes
        same_bytes(got, eng.topk_candidates(c["tu"].float(), c["ti"].float(), c["users"], c["cand"], k, csr_dev(c["seen"])), "fp16 vs fp32")


# ---- 2. the identity on the device ----------------------------------------------------------------------------------------

def identity(eng, c, k, seen, mask, adj, tables=None):
    """Row x of the call against topk_items for users[x] alone with the filter `mask AND bitmap(list x)`."""
    tu, ti = tables or (c["tu"], c["ti"])
    seen = csr_dev(seen)
    got = eng.topk_candidates(tu, ti, c["users"], c["cand"], k, seen, allow=None if mask is None else words_dev(mask), adjust=adj)
    for x, u in enumerate(c["users"]):
        m = K.list_mask(c["lists"][x], I)
        if mask is not None:
            m &= mask
        it, sc = eng.topk_items(tu, ti, gpu(np.array([u])), k, seen, allow=words_dev(m), adjust=adj)
        assert torch.equal(got[0][x], it[0]) and torch.equal(bits(got[1][x]), bits(sc[0])), x
    return got


@functools.lru_cache(maxsize=None)
def scored(dtype, d):
    """score_case (scale, offset, -inf / NaN offsets, zero / NaN scales) with the 40 mixed lists, the special items in
    every third of them."""
    s = C.score_case(dtype, d)
    special = np.concatenate(list(s["special"].values()))
    c = K.mixed_case(dtype, d, seed=C.SEED, with_special=special)
    assert c["wi"].shape == s["wi"].shape
    c["wu"], c["wi"], c["ru"], c["ri"] = s["wu"], s["wi"], s["ru"], s["ri"]         # (score_case plants rows of its own)
    c["scale"], c["offset"], c["special"] = s["scale"], s["offset"], special
    return on_device(c)


@pytest.mark.parametrize("variant", ["seen", "filter", "score", "bias", "cosine", "neutral"])
@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp16", 128)])
def test_identity_with_filtered_topk_items(dtype, d, variant):
    c = scored(dtype, d)
    eng = engine(d)
    assert len(c["lists"]) == 40
    mask = random_mask(I, 0.5, 11) if variant in ("filter", "score") else None
    adj = None
    if variant == "score":
        adj = gpu(C.pad_adj(c["scale"], c["offset"]))
    elif variant == "bias":
        adj = eng.item_adjust(I, offset=gpu(c["offset"]))
    elif variant == "cosine":
        adj = eng.item_adjust_cosine(c["ti"])
    elif variant == "neutral":
        adj = eng.item_adjust(I)
    got = identity(eng, c, 20, c["seen"], mask, adj)
    if variant == "score":
        # against the CPU too: the terms' -inf offsets fill after every finite score, the NaN terms remove their items
        want = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], 20, c["seen"], mask, (c["scale"], c["offset"]))
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
        np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), want[1].view(np.int32))
        np.testing.assert_array_equal(got[2].cpu().numpy(), want[2])
        listed = got[0][got[0] >= 0].cpu().numpy()
        nan_terms = c["special"][np.isnan(c["scale"][c["special"]]) | np.isnan(c["offset"][c["special"]])]
        assert len(nan_terms) and not np.isin(listed, nan_terms).any()
    if variant == "neutral":                          # the neutral table returns the unadjusted call's bytes
        same_bytes(got, eng.topk_candidates(c["tu"], c["ti"], c["users"], c["cand"], 20, csr_dev(c["seen"])), "neutral adj")


# ---- 3. repeats and padding -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def repeats():
    c = on_device(K.repeat_case())
    c["want"] = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], K.KMAX, c["seen"])
    return c


@pytest.mark.parametrize("k", TOPK)
def test_repeats_and_padding(k):
    c = repeats()
    eng = engine(32)
    seen = csr_dev(c["seen"])
    got = eng.topk_candidates(c["tu"], c["ti"], c["users"], c["cand"], k, seen)
    check_ref(got, c["want"], k)
    it = got[0].cpu().numpy()
    for row in it:                                    # a repeated id appears once
        live = row[row >= 0]
        assert len(np.unique(live)) == len(live)
    for name in ("all padding", "all Seen", "only the NaN row"):
        x = c["names"].index(name)
        assert (it[x] == -1).all() and torch.isinf(got[1][x]).all() and (got[1][x] < 0).all() and int(got[2][x]) == 0, name
    # the same lists as int32 entries: ids that do not fit become INT32_MAX / INT32_MIN, padding all the same
    clip = [np.clip(l, -2 ** 31, 2 ** 31 - 1) for l in c["lists"]]
    assert any((l == 2 ** 31 - 1).any() for l in clip)
    same_bytes(got, eng.topk_candidates(c["tu"], c["ti"], c["users"], tuple(gpu(t) for t in K.ragged(clip, np.int32)), k, seen), "int32")


# ---- 4. ties --------------------------------------------------------------------------------------------------------------

def test_ties_are_broken_by_id():
    c = on_device(K.tie_case())
    assert c["ties"] >= 24
    eng = engine(32)
    for k in (20, 128):
        got = eng.topk_candidates(c["tu"], c["ti"], c["users"], c["cand"], k, csr_dev(c["seen"]))
        want = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], k, c["seen"])
        check_ref(got, want, k)
    # bit-equal neighbours of the result are in ascending id order although the input was descending
    it, sc = got[0].cpu().numpy(), got[1].cpu().numpy().view(np.int32)
    eq = (sc[:, 1:] == sc[:, :-1]) & (it[:, 1:] >= 0)
    assert eq.sum() >= 24 and (it[:, 1:][eq] > it[:, :-1][eq]).all()


# ---- 5. forms -------------------------------------------------------------------------------------------------------------

def test_forms_repeated_users_and_the_empty_call():
    from conftest import make_mf
    from sml_amd.retrieval import CandidateRows
    c = boundary("fp32", 32)
    eng = engine(32)
    seen = csr_dev(c["seen"])
    users, lists = c["users"], c["lists"]
    assert len(np.unique(users)) < len(users)                              # a user repeats
    base = eng.topk_candidates(c["tu"], c["ti"], users, tuple(gpu(t) for t in K.ragged(lists, np.int32)), 20, seen)
    check_ref(base, c["want"], 20)
    same_bytes(base, eng.topk_candidates(c["tu"], c["ti"], users, c["cand"], 20, seen), "ragged int64")
    same_bytes(base, eng.topk_candidates(c["tu"], c["ti"], users, [l.tolist() for l in lists], 20, seen), "list of sequences")
    same_bytes(base, eng.topk_candidates(c["tu"], c["ti"], users, gpu(K.dense(lists, np.int32)), 20, seen), "dense int32")
    same_bytes(base, eng.topk_candidates(c["tu"], c["ti"], users, K.dense(lists, np.int64), 20, seen), "dense int64")
    # a test file's rows [user, candidates ...] read in place: stride C + 1, first 1
    rows = gpu(np.concatenate([users[:, None], K.dense(lists, np.int64)], 1))
    cr = CandidateRows(rows, first_col=1)
    assert cr.geometry == (301, 1, 300) and cr.rows.data_ptr() == rows.data_ptr()
    same_bytes(base, eng.topk_candidates(c["tu"], c["ti"], None, cr, 20, seen), "CandidateRows")
    mf = make_mf(300, I, 32, c["wu"], c["wi"], DEV)
    it, sc = mf.test_lists(rows, topK=20, exclude=c["seen"])
    assert torch.equal(it, base[0]) and torch.equal(bits(sc), bits(base[1]))
    it, sc = mf.test_lists(rows.cpu().numpy(), topK=20, exclude=c["seen"])
    assert torch.equal(it, base[0]) and torch.equal(bits(sc), bits(base[1]))
    # every list for one and the same user
    one = np.full(len(lists), users[0])
    got = eng.topk_candidates(c["tu"], c["ti"], one, c["cand"], 20, seen)
    check_ref(got, K.ref_topk_candidates(c["ru"], c["ri"], one, lists, 20, c["seen"]), 20)
    # n = 0 is a valid call
    it, sc, ne = eng.topk_candidates(c["tu"], c["ti"], np.zeros(0, np.int64), (np.zeros(1, np.int64), np.zeros(0, np.int32)), 20, seen)
    assert it.shape == (0, 20) and sc.shape == (0, 20) and ne.shape == (0,)
    it, sc, ne = eng.topk_candidates(c["tu"], c["ti"], np.zeros(0, np.int64), np.zeros((0, 7), np.int64), 20)
    assert it.shape == (0, 20)
    # lists that are all empty (nothing to read) and dense lists of no columns
    it, sc, ne = eng.topk_candidates(c["tu"], c["ti"], users[:3], [[], [], []], 20)
    assert (it == -1).all() and (ne == 0).all()
    it, sc, ne = eng.topk_candidates(c["tu"], c["ti"], users[:3], np.zeros((3, 0), np.int64), 20)
    assert (it == -1).all() and (ne == 0).all()


# ---- 6. launch geometry ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 64), ("fp16", 128)])
def test_launch_geometry_does_not_change_the_bytes(dtype, d):
    c = boundary(dtype, d)
    eng = engine(d)
    seen = csr_dev(c["seen"])
    base = eng.topk_candidates(c["tu"], c["ti"], c["users"], c["cand"], 20, seen, max_workgroups=0)
    check_ref(base, c["want"], 20)
    for g in (1, 3):
        same_bytes(base, eng.topk_candidates(c["tu"], c["ti"], c["users"], c["cand"], 20, seen, max_workgroups=g), g)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument_and_launch_nothing():
    from sml_amd._lib import load
    lib = load()
    n, k, C_ = 8, 20, 16
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)      # noqa: E731
    users = gpu(np.arange(n, dtype=np.int64))
    cand = gpu(np.random.RandomState(0).randint(0, I, size=(n, C_)).astype(np.int64))
    off, sitems = gpu(np.zeros(301, np.int64)), gpu(np.zeros(1, np.int32))
    items = torch.full((n, 129), -7, device=DEV, dtype=torch.int32)
    scores = torch.full((n, 129), 7.0, device=DEV, dtype=torch.float32)
    ne = torch.full((n,), -7, device=DEV, dtype=torch.int32)

    def call(d=32, half=False, k=k, cand_bytes=8, cols=C_, seen=(None, None), items_t=None, cand_t=None):
        eng = engine(d)
        dt = torch.float16 if half else torch.float32
        tu, ti = torch.zeros(300, d, device=DEV, dtype=dt), torch.zeros(I, d, device=DEV, dtype=dt)
        cand_t = cand if cand_t is None else cand_t
        rc = lib.sml_topk_candidates(eng._ctx, p(tu), p(ti), tu.element_size(), I, p(users), n, p(cand_t), cand_bytes, None, C_, 0, cols, k,
                                     p(seen[0]), p(seen[1]), None, None, 0, p(items if items_t is None else items_t), p(scores), p(ne),
                                     eng._stream())
        torch.cuda.synchronize()
        return rc, lib.sml_last_error().decode()

    for kw, word in ((dict(k=0), "1 <= k <= 128"), (dict(k=129), "1 <= k <= 128"), (dict(d=128), "128 for fp16 tables"),
                     (dict(cand_bytes=2), "cand_elem_bytes must be 4 or 8"), (dict(cols=-1), "must not be negative"),
                     (dict(seen=(off, None)), "seen_off and seen_items both or neither"),
                     (dict(seen=(None, sitems)), "seen_off and seen_items both or neither")):
        rc, msg = call(**kw)
        assert rc != 0 and "sml_topk_candidates" in msg and word in msg, (kw, msg)
    # `items` aliasing `cand`: the candidate matrix handed in as the output too
    alias = torch.full((n, C_), 5, device=DEV, dtype=torch.int64)
    rc, msg = call(items_t=alias, cand_t=alias)
    assert rc != 0 and "an output overlaps an input" in msg, msg
    assert (alias == 5).all()
    assert (items == -7).all() and (scores == 7.0).all() and (ne == -7).all()      # nothing was launched
    rc, msg = call(d=128, half=True)                                               # the same call, valid: it runs
    assert rc == 0, msg
    flat = items.reshape(-1)                                                       # (the call's items are [n, k], contiguous)
    assert (flat[:n * k] != -7).all() and (flat[n * k:] == -7).all() and (ne == C_).all()


# ---- 8. the model surface -------------------------------------------------------------------------------------------------

def test_model_surface():
    from conftest import make_mf
    from sml_amd.mf import MF2
    c = boundary("fp32", 32)
    users, lists = c["users"], c["lists"]
    mf = make_mf(300, I, 32, c["wu"], c["wi"], DEV)
    it, sc = mf.recommend(users, topK=20, exclude=c["seen"], candidates=[l.tolist() for l in lists])
    np.testing.assert_array_equal(it.cpu().numpy(), c["want"][0][:, :20])
    np.testing.assert_array_equal(sc.cpu().numpy().view(np.int32), c["want"][1][:, :20].view(np.int32))
    with pytest.raises(ValueError):
        mf.recommend(None, candidates=[l.tolist() for l in lists])
    # without candidates: the bytes of the catalogue walk, as before
    eng = engine(32)
    it, sc = mf.recommend(users, topK=20, exclude=c["seen"])
    it0, sc0 = eng.topk_items(c["tu"], c["ti"], gpu(users), 20, csr_dev(c["seen"]))
    assert torch.equal(it, it0) and torch.equal(bits(sc), bits(sc0))
    # a .half() model at d = 128
    h = boundary("fp16", 128)
    mh = make_mf(300, I, 128, device=DEV).half()
    with torch.no_grad():
        mh.user_laten.weight.copy_(h["tu"])
        mh.item_laten.weight.copy_(h["ti"])
    it, sc = mh.recommend(h["users"], topK=20, exclude=h["seen"], candidates=h["cand"])
    np.testing.assert_array_equal(it.cpu().numpy(), h["want"][0][:, :20])
    np.testing.assert_array_equal(sc.cpu().numpy().view(np.int32), h["want"][1][:, :20].view(np.int32))
    # MF2 with score="bias": the item bias as the offset
    m2 = MF2(300, I, 32).to(DEV)
    with torch.no_grad():
        m2.user_laten.weight.copy_(c["tu"])
        m2.item_laten.weight.copy_(c["ti"])
    bias = m2.item_bais.weight.data[:, 0].cpu().numpy()
    it, sc = m2.recommend(users, topK=20, exclude=c["seen"], score="bias", candidates=c["cand"])
    want = K.ref_topk_candidates(c["ru"], c["ri"], users, lists, 20, c["seen"], None, (np.ones(I, np.float32), bias))
    np.testing.assert_array_equal(it.cpu().numpy(), want[0])
    np.testing.assert_array_equal(sc.cpu().numpy().view(np.int32), want[1].view(np.int32))
    assert (it.cpu().numpy() != c["want"][0][:, :20]).any()                        # the bias reorders the lists
