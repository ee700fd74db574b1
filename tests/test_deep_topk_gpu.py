"""Deep lists on the MI355X: sml_topk_deep through HipEngine.topk_deep, MFbasemode.recommend / similar_items above 128 and
sml_amd.evaluation.recall_curve.

Every comparison is of bytes or integers: item ids, score bits and n_elig against the exact CPU reference of
tests/_deep_topk_cases.py (ref_topk of tests/_fp32_chain.py, a filter as Seen', terms as one fma32), against the host walk
sml_host_topk_items, across launch geometries, and against the family's other calls on the device (topk_items, full_rank).
Shapes: U = 300, I = 4,099 (129 tiles, the last of 3 items), n in {1, 33, 97, 257}, k in {1, 128, 129, 500, 1024}; `long` is
40 x 70,001."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _deep_topk_cases as D
from _item_filter_cases import seen_prime
from conftest import make_mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(seen):
    return None if seen is None else (gpu(seen[0]), gpu(seen[1]))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bytes(a, b, what):
    for x, y, part in zip(a, b, ("items", "scores", "n_elig")):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, part)
        assert torch.equal(bits(x), bits(y)), (what, part)


@functools.lru_cache(maxsize=None)
def on_device(name, dtype, d):
    c = dict(D.case(name, dtype, d))
    c["tu"], c["ti"], c["csr"] = gpu(c["wu"]), gpu(c["wi"]), csr_dev(c["seen"])
    c["allow"] = gpu(D.words(c).view(np.int32))
    c["adj"] = gpu(D.adj_table(c))
    return c


def deep(c, users, k, variant="none", slices=0, seen="case"):
    return engine(c["d"]).topk_deep(c["tu"], c["ti"], users, k, c["csr"] if seen == "case" else seen,
                                    c["allow"] if variant in ("filter", "both") else None,
                                    c["adj"] if variant in ("terms", "both") else None, slices)


def check_ref(got, want, what):
    items, scores, n_elig = want
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    np.testing.assert_array_equal(got[0].cpu().numpy(), items, err_msg=str(what))
    np.testing.assert_array_equal(got[1].cpu().numpy().view(np.int32), np.ascontiguousarray(scores).view(np.int32), err_msg=str(what))
    np.testing.assert_array_equal(got[2].cpu().numpy(), n_elig, err_msg=str(what))


# ---- 1. the reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype,d,variant,n", D.GRID, ids=D.GRID_IDS)
def test_reference(name, dtype, d, variant, n):
    c = on_device(name, dtype, d)
    ref = D.reference(name, dtype, d, variant, n)
    users = gpu(c["users"][:n])
    for k in D.KS:
        check_ref(deep(c, users, k, variant), D.cut(ref, k), (name, dtype, d, variant, n, k))


def test_cases_cover_what_they_claim():
    """Negative and positive scores both present in `wide`; -0 scores in `all_tie` keep their sign bit on the device."""
    c = on_device("wide", "fp32", 32)
    it, sc, _ = deep(c, gpu(c["users"][:97]), 1024, "terms")
    live = sc[it >= 0]
    assert (live > 0).any() and (live < 0).any() and torch.isinf(live).any() and not torch.isnan(sc).any()
    c = on_device("all_tie", "fp16", 128)
    it, sc, _ = deep(c, gpu(c["users"][:97]), 1024, "both")
    assert (sc == 0).all() and torch.equal(torch.signbit(sc), it % 3 == 0) and (it[:, 1:] > it[:, :-1]).all()


# ---- 2. the host walk --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype,d,variant", [("random", "fp32", 64, "both"), ("near_tie", "fp32", 32, "none"), ("all_tie", "fp16", 128, "both"),
                                                  ("wide", "fp16", 32, "terms"), ("sorted_asc", "fp16", 64, "filter")])
def test_host_walk_gives_the_same_bytes(name, dtype, d, variant):
    from sml_amd import _lib
    lib = _lib.load()
    c = on_device(name, dtype, d)
    users = np.ascontiguousarray(c["users"][:33])
    off, seen_items = c["seen"]
    allow = D.words(c) if variant in ("filter", "both") else None
    adj = D.adj_table(c) if variant in ("terms", "both") else None
    p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    for k in (129, 1024):
        items, scores, n_elig = np.full((33, k), 77, np.int32), np.full((33, k), 7.0, np.float32), np.full(33, 77, np.int32)
        _lib.check(lib.sml_host_topk_items(p(c["wu"]), p(c["wi"]), c["wu"].itemsize, d, D.I, p(users), 33, k, p(off), p(seen_items), p(allow),
                                           p(adj), p(items), p(scores), p(n_elig)), "sml_host_topk_items")
        got = deep(c, gpu(users), k, variant)
        same_bytes((got[0].int(), got[1], got[2]), (gpu(items), gpu(scores), gpu(n_elig)), (name, k))


# ---- 3. geometry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype,d,variant", [("random", "fp32", 32, "none"), ("all_tie", "fp32", 64, "filter"), ("all_tie", "fp16", 32, "terms"),
                                                  ("sorted_desc", "fp16", 32, "none"), ("sorted_asc", "fp32", 32, "both")])
def test_geometry_does_not_change_the_bytes(name, dtype, d, variant):
    """slices = 200 exceeds the 129 tiles, so some slices are empty; 1 puts a user's whole catalogue in one wave."""
    c = on_device(name, dtype, d)
    users = gpu(c["users"][:97])
    for k in (129, 1024):
        base = deep(c, users, k, variant, 0)
        for slices in (1, 8, 24, 200):
            same_bytes(deep(c, users, k, variant, slices), base, (name, k, slices))


# ---- 4. the family's identities ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", D.WIDTHS)
def test_equals_topk_items_up_to_128(dtype, d, monkeypatch):
    """The partner is the sorted-list kernel at every k: DEEP_FROM = 129 keeps HipEngine.topk_items on sml_topk_items[_adjusted][_f16]
    (counted), whatever the committed routing is."""
    from sml_amd import retrieval
    monkeypatch.setattr(retrieval, "DEEP_FROM", 129)
    c = on_device("random", dtype, d)
    eng = engine(d)
    users = gpu(c["users"])
    sorted_calls = []
    for name in ("sml_topk_items", "sml_topk_items_f16", "sml_topk_items_filtered", "sml_topk_items_filtered_f16", "sml_topk_items_adjusted"):
        def counting(*a, _real=getattr(eng.lib, name), _name=name):
            sorted_calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(eng.lib, name, counting)
    for variant, allow, adj in (("none", None, None), ("filter", c["allow"], None), ("both", c["allow"], c["adj"])):
        deep1024 = deep(c, users, 1024, variant)
        for k in (1, 20, 128):
            before = len(sorted_calls)
            it, sc = eng.topk_items(c["tu"], c["ti"], users, k, c["csr"], allow, adj)
            assert len(sorted_calls) > before, "topk_items must have run the sorted-list entry point"
            got = deep(c, users, k, variant)
            same_bytes(got[:2], (it, sc), (variant, k))
            same_bytes((deep1024[0][:, :k].contiguous(), deep1024[1][:, :k].contiguous()), (it, sc), (variant, "prefix", k))


def test_filter_is_seen_prime():
    c = on_device("random", "fp32", 32)
    users = gpu(c["users"][:97])
    prime = csr_dev(seen_prime(c["seen"], c["mask"], D.U))
    for k in (129, 1024):
        same_bytes(deep(c, users, k, "filter"), deep(c, users, k, "none", seen=prime), k)
        same_bytes(deep(c, users, k, "both"), deep(c, users, k, "terms", seen=prime), k)


@pytest.mark.parametrize("d", (32, 64))
def test_fp16_equals_fp32_on_widened_copies(d):
    c = on_device("random", "fp16", d)
    eng = engine(d)
    users = gpu(c["users"][:97])
    for k in (129, 1024):
        for allow, adj in ((None, None), (c["allow"], c["adj"])):
            same_bytes(eng.topk_deep(c["tu"], c["ti"], users, k, c["csr"], allow, adj),
                       eng.topk_deep(c["tu"].float(), c["ti"].float(), users, k, c["csr"], allow, adj), (d, k))


def test_neutral_terms_equal_no_terms_in_every_integer():
    c = on_device("near_tie", "fp32", 32)
    eng = engine(32)
    users = gpu(c["users"])
    neutral = eng.item_adjust(D.I)
    for k in (129, 1024):
        a, b = deep(c, users, k), eng.topk_deep(c["tu"], c["ti"], users, k, c["csr"], None, neutral)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and (a[1] == b[1]).all()


# ---- 5. the positive's position -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", (32, 64))
def test_positive_sits_at_rank_plus_ties_before_it(d):
    """Dyadic tables (every score exact, many exact ties): with full_rank's rank, the positive of a row sits at rank + #{eligible ties
    with a smaller id} of the deep list whenever that is < 1,024."""
    rng = np.random.RandomState(300 + d)
    U, I, n = 300, 2053, 257
    wu = (rng.randint(-16, 17, size=(U, d)) / 8.0).astype(np.float32)
    wi = (rng.randint(-4, 5, size=(I, d)) / 8.0).astype(np.float32)
    wi[:, 4:] = 0                                              # few distinct scores: long runs of ties
    rows = np.stack([rng.randint(0, U, size=n), rng.randint(0, I, size=n)], 1).astype(np.int64)
    lists = {u: rng.choice(I, size=rng.randint(0, 60), replace=False) for u in range(U)}
    from _fp32_chain import seen_csr
    seen = seen_csr(U, I, lists)
    for r in range(n):                                         # (a positive inside Seen(u) has no place in the list)
        while rows[r, 1] in set(lists[rows[r, 0]].tolist()):
            rows[r, 1] = rng.randint(0, I)
    eng = engine(d)
    tu, ti, csr = gpu(wu), gpu(wi), csr_dev(seen)
    rank = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
    it, sc, _ = eng.topk_deep(tu, ti, gpu(rows[:, 0]), 1024, csr)
    it = it.cpu().numpy()
    S = wu.astype(np.float64) @ wi.astype(np.float64).T
    checked = 0
    for r, (u, p) in enumerate(rows):
        ok = np.ones(I, bool)
        ok[lists[u]] = False
        before = int((ok & (S[u] == S[u, p]) & (np.arange(I) < p)).sum())
        if rank[r] + before < 1024:
            assert it[r, rank[r] + before] == p, r
            checked += 1
        else:
            assert p not in it[r]
    assert checked > 100 and checked < n


# ---- 6. the surface ----------------------------------------------------------------------------------------------------

def test_recommend_and_similar_items_go_deep():
    from sml_amd.retrieval import ItemFilter, SeenItems
    c = on_device("random", "fp32", 32)
    model = make_mf(D.U, D.I, 32, c["wu"], c["wi"], DEV)
    eng = engine(32)
    users = gpu(c["users"][:97])
    flt = ItemFilter.from_mask(c["mask"])
    tab = model.item_laten.weight.data
    got = model.recommend(users, 500, exclude=c["csr"], items=flt, score="cosine")
    want = eng.topk_deep(model.user_laten.weight.data, tab, users, 500, c["csr"], c["allow"], eng.item_adjust_cosine(tab))
    same_bytes(got, want[:2], "recommend")
    assert got[0].shape == (97, 500)
    q = gpu(np.arange(0, 4099, 61))
    from sml_amd.retrieval import self_seen
    got = model.similar_items(q, 300, metric="dot")
    same_bytes(got, eng.topk_deep(tab, tab, q, 300, self_seen(D.I, tab.device))[:2], "similar_items dot")
    got = model.similar_items(q, 300)
    adj = eng.item_adjust_cosine(tab)
    it, sc, _ = eng.topk_deep(tab, tab, q, 300, self_seen(D.I, tab.device), None, adj)
    same_bytes(got, (it, torch.where(it >= 0, sc * adj[0, q].unsqueeze(1), sc)), "similar_items cosine")
    assert not (got[0] == q.unsqueeze(1)).any()
    with pytest.raises(ValueError):
        model.recommend(users, 129, diversify=0.5)
    with pytest.raises(Exception):
        model.recommend(users, 1025)
    assert isinstance(SeenItems(2, 2), SeenItems)


def test_recall_curve_agrees_with_test_model_users():
    from sml_amd.evaluation import recall_curve, test_model_users
    from sml_amd.retrieval import SeenItems, held_out
    c = on_device("random", "fp32", 64)
    model = make_mf(D.U, D.I, 64, c["wu"], c["wi"], DEV)
    rng = np.random.RandomState(9)
    # held-out sets around each user's best items, so that recall at small K is not 0
    best = engine(64).topk_deep(c["tu"], c["ti"], gpu(np.arange(D.U)), 40, c["csr"])[0].cpu().numpy()
    pairs = np.concatenate([np.stack([np.full(6, u), rng.choice(best[u][best[u] >= 0], size=6, replace=False)], 1) for u in range(0, D.U, 2)] +
                           [np.stack([rng.randint(0, D.U, 400), rng.randint(0, D.I, 400)], 1)]).astype(np.int64)
    seen = SeenItems(D.U, D.I)
    off, items = c["seen"]
    seen.add(np.stack([np.repeat(np.arange(D.U), np.diff(off)), items.astype(np.int64)], 1))
    want = test_model_users(model, pairs, seen, topK=(20, 10, 5))
    got = recall_curve(model, held_out(pairs, D.U, D.I), (5, 10, 20, 500), exclude=seen)
    assert got[:3] == [want["recall"][5], want["recall"][10], want["recall"][20]]
    assert 0 < got[0] <= got[1] <= got[2] <= got[3] <= 1


def test_refusals_and_edges():
    from sml_amd._lib import SmlError
    c = on_device("random", "fp32", 32)
    eng = engine(32)
    users = gpu(c["users"][:33])
    with pytest.raises(SmlError, match="1 <= k <= 128"):
        eng.topk_items(c["tu"], c["ti"], users, 129, c["csr"])
    for k in (0, 1025):
        with pytest.raises(ValueError, match="1..1024"):
            deep(c, users, k)
    with pytest.raises(SmlError, match="slices"):
        deep(c, users, 200, slices=-1)
    with pytest.raises(SmlError, match="slices"):
        deep(c, users, 200, slices=257)
    with pytest.raises(ValueError, match="16-byte aligned"):
        eng.topk_deep(c["tu"], c["ti"], users, 200, c["csr"], None, torch.zeros(2 * 4128 + 1, device=DEV)[1:].view(2, 4128))
    # the library's own words, past the Python checks
    lib, ctx = eng.lib, eng._ctx
    assert lib.sml_topk_deep_scratch_bytes(ctx, 33, 0, D.I, 0) < 0 and lib.sml_topk_deep_scratch_bytes(ctx, 33, 1025, D.I, 0) < 0
    assert lib.sml_topk_deep_scratch_bytes(ctx, 33, 200, D.I, -1) < 0 and lib.sml_topk_deep_scratch_bytes(ctx, 33, 200, 0, 0) < 0
    assert lib.sml_topk_deep_scratch_bytes(ctx, 0, 200, D.I, 0) == 0 and lib.sml_topk_deep_scratch_bytes(ctx, 33, 200, D.I, 200) > 33 * 1024
    nbytes = lib.sml_topk_deep_scratch_bytes(ctx, 33, 200, D.I, 0)
    scratch = torch.empty(nbytes + 256, device=DEV, dtype=torch.uint8)
    items = torch.full((33, 200), 77, device=DEV, dtype=torch.int32)
    scores = torch.full((33, 200), 7.0, device=DEV, dtype=torch.float32)
    n_elig = torch.full((33,), 77, device=DEV, dtype=torch.int32)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731

    def call(k=200, slices=0, adj=None, scratch_ptr=None, seen_items=c["csr"][1], out=items):
        return lib.sml_topk_deep(ctx, P(c["tu"]), P(c["ti"]), 4, D.I, P(users), 33, k, P(c["csr"][0]), P(seen_items), None, adj, slices,
                                 scratch_ptr or P(scratch), P(out), P(scores), P(n_elig), None)
    for bad, word in ((dict(k=0), "1 <= k <= 1024"), (dict(k=1025), "1 <= k <= 1024"), (dict(slices=-1), "0 <= slices <= 256"),
                      (dict(adj=ctypes.c_void_p(c["adj"].data_ptr() + 4)), "adj must be 16-byte aligned"),
                      (dict(scratch_ptr=ctypes.c_void_p(scratch.data_ptr() + 16)), "scratch must be 256-byte aligned"),
                      (dict(seen_items=None), "both or neither"), (dict(out=scores), "outputs overlap"), (dict(out=users), "overlaps an input")):
        assert call(**bad) != 0, bad
        assert word in lib.sml_last_error().decode(), (bad, lib.sml_last_error())
    assert (items == 77).all() and (scores == 7.0).all() and (n_elig == 77).all(), "a refused call launches nothing"
    # junk-prefilled outputs are fully overwritten
    assert call() == 0
    want = deep(c, users, 200)
    same_bytes((items, scores, n_elig), (want[0].int(), want[1], want[2]), "raw call")
    # n == 0
    it, sc, ne = deep(c, gpu(np.zeros(0, np.int64)), 500)
    assert it.shape == (0, 500) and sc.shape == (0, 500) and ne.shape == (0,) and it.dtype == torch.int64


def test_long_catalogue_in_chunks(monkeypatch):
    """The engine walks the users in chunks sized by the scratch: a tiny budget (chunks of 9 users) gives the same bytes."""
    from sml_amd.engine import HipEngine
    c = on_device("long", "fp32", 32)
    eng = engine(32)
    users = gpu(c["users"])
    base = deep(c, users, 500, "both")
    calls = []
    real = eng.lib.sml_topk_deep

    def counting(*a):
        calls.append(a[6])
        return real(*a)
    monkeypatch.setattr(HipEngine, "TOPK_SCRATCH_BYTES", 16 << 10)
    monkeypatch.setattr(eng.lib, "sml_topk_deep", counting)
    same_bytes(deep(c, users, 500, "both"), base, "chunks")
    assert len(calls) > 1 and sum(calls) == 40 and max(calls) < 40, calls
