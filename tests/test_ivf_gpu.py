"""The clustered item index on the MI355X: sml_ivf_search / sml_ivf_centroids through HipEngine.ivf_search / ivf_centroids,
sml_amd.retrieval.ItemIndex, MFbasemode.recommend(index=) / similar_items(index=) and sml_amd.evaluation.index_recall.

Every comparison is byte equality (item ids, score bits, n_elig, centroid bytes): against the host walks of the same definitions,
against HipEngine.topk_candidates on the concatenated probed lists, and against topk_items when every list is probed.  Shapes:
U = 40, I = 420, 12 hand-made lists (tests/_ivf_cases.py) and 130 tiny ones, nprobe in {1, 3, 12, 128}, k in {1, 20, 128}."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _candidates_cases as K
import _item_score_cases as C
import _ivf_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, what):
    for x, y, part in zip(a, b, ("items", "scores", "n_elig")):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, part)
        assert torch.equal(bits(x), bits(y)), (what, part)


@functools.lru_cache(maxsize=None)
def dev_case(dtype, d):
    c = dict(V.case(dtype, d))
    c["tu"], c["ti"] = gpu(c["wu"]), gpu(c["wi"])
    c["idx_a"] = tuple(gpu(t) for t in V.csr(c["lists_a"]))
    c["idx_b"] = tuple(gpu(t) for t in V.csr(c["lists_b"]))
    c["seen_dev"] = (gpu(c["csr"][0]), gpu(c["csr"][1]))
    n, wi, ri, seen, mask, terms = V.sub_b(c)
    c["b"] = dict(n=n, wi=wi, ti=gpu(wi), seen=seen, seen_dev=(gpu(seen[0]), gpu(seen[1])), mask=mask, terms=terms)
    return c


def dev_variant(variant, mask, terms):
    m, t = V.variant_args(variant, mask, terms)
    return m, t, (None if m is None else gpu(V.filter_words(m).view(np.int32))), (None if t is None else gpu(C.pad_adj(*t)))


def search(c, d, probes, k, variant, part="a", max_workgroups=0, tables=None):
    """(device result, host-walk result) of one case."""
    eng = engine(d)
    if part == "a":
        wi, ti, lists, idx, seen, seen_dev, mask, terms = c["wi"], c["ti"], c["lists_a"], c["idx_a"], c["csr"], c["seen_dev"], c["mask"], c["terms"]
    else:
        b = c["b"]
        wi, ti, lists, idx, seen, seen_dev, mask, terms = b["wi"], b["ti"], c["lists_b"], c["idx_b"], b["seen"], b["seen_dev"], b["mask"], b["terms"]
    m, t, allow, adj = dev_variant(variant, mask, terms)
    tu, ti = tables or (c["tu"], ti)
    got = eng.ivf_search(tu, ti, gpu(V.USERS), idx, gpu(probes), k, seen_dev, allow, adj, max_workgroups=max_workgroups)
    host = V.host_search(c["wu"], wi, d, V.USERS, lists, probes, k, seen, m, t)
    return got, host, (tu, ti, idx, seen_dev, allow, adj, lists)


@pytest.mark.parametrize("variant", V.VARIANTS)
@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_device_search_equals_host_walk_and_candidates(dtype, d, variant):
    """Every (nprobe, k) of the hand-made partition: the host walk's bytes, topk_candidates' bytes on the concatenated lists,
    the same bytes from one workgroup, and (fp16, d = 32 / 64) from fp32 copies of the tables."""
    c = dev_case(dtype, d)
    eng = engine(d)
    for nprobe in V.NPROBES:
        probes = V.probes_a(nprobe)
        for k in V.KS:
            got, host, (tu, ti, idx, seen_dev, allow, adj, lists) = search(c, d, probes, k, variant)
            assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
            V.same_bytes([t.cpu().numpy() for t in got], host, (dtype, d, nprobe, k, variant))
            cand = tuple(gpu(t) for t in K.ragged(V.concat_lists(lists, probes), np.int32))
            same(got, eng.topk_candidates(tu, ti, gpu(V.USERS), cand, k, seen_dev, allow, adj), ("candidates", nprobe, k))
            same(got, search(c, d, probes, k, variant, max_workgroups=1)[0], ("one workgroup", nprobe, k))
        if dtype == "fp16" and d in (32, 64):
            same(got, search(c, d, probes, V.KS[-1], variant, tables=(c["tu"].float(), c["ti"].float()))[0], ("fp32 copies", nprobe))


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_many_tiny_lists(dtype, d):
    """130 lists of 0 .. 3 items, 128 probes per user: both probes of every lane, a virtual sequence shorter than one round."""
    c = dev_case(dtype, d)
    probes = V.probes_b()
    for variant in ("none", "both"):
        for k in V.KS:
            got, host, _ = search(c, d, probes, k, variant, part="b")
            V.same_bytes([t.cpu().numpy() for t in got], host, (dtype, d, k, variant))
            same(got, search(c, d, probes, k, variant, part="b", max_workgroups=1)[0], ("one workgroup", k))


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_every_list_probed_equals_topk_items(dtype, d):
    c = dev_case(dtype, d)
    eng = engine(d)
    every = np.tile(np.arange(12, dtype=np.int32), (len(V.USERS), 1))
    for variant in V.VARIANTS:
        for k in V.KS:
            got, _, (tu, ti, idx, seen_dev, allow, adj, _) = search(c, d, every, k, variant)
            it, sc = eng.topk_items(tu, ti, gpu(V.USERS), k, seen_dev, allow, adj)
            assert torch.equal(got[0], it) and torch.equal(bits(got[1]), bits(sc)), (dtype, d, variant, k)


def test_outputs_are_fully_overwritten():
    c = dev_case("fp32", 32)
    eng = engine(32)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    users, probes = gpu(V.USERS), gpu(V.probes_a(3))
    for k in (1, 20, 128):
        items = torch.full((7, k), 77, device=DEV, dtype=torch.int32)
        scores = torch.full((7, k), 7.0, device=DEV, dtype=torch.float32)
        n_elig = torch.full((7,), 77, device=DEV, dtype=torch.int32)
        rc = eng.lib.sml_ivf_search(eng._ctx, P(c["tu"]), P(c["ti"]), 4, V.I, P(users), 7, P(c["idx_a"][0]), P(c["idx_a"][1]), 12, P(probes), 3, k,
                                    P(c["seen_dev"][0]), P(c["seen_dev"][1]), None, None, 0, P(items), P(scores), P(n_elig), eng._stream())
        assert rc == 0, eng.lib.sml_last_error()
        host = V.host_search(c["wu"], c["wi"], 32, V.USERS, c["lists_a"], V.probes_a(3), k, c["csr"])
        V.same_bytes((items.cpu().numpy(), scores.cpu().numpy(), n_elig.cpu().numpy()), host, k)
        assert (items[3] == -1).all() and torch.isinf(scores[3]).all() and n_elig[3] == 0          # the all-padding row
    # the device call's own refusals
    bad = eng.lib.sml_ivf_search(eng._ctx, P(c["tu"]), P(c["ti"]), 4, V.I, P(users), 7, P(c["idx_a"][0]), P(c["idx_a"][1]), 12, P(probes), 129, 20,
                                 None, None, None, None, 0, P(items), P(scores), P(n_elig), eng._stream())
    assert bad != 0 and "nprobe" in eng.lib.sml_last_error().decode()
    bad = eng.lib.sml_ivf_search(eng._ctx, ctypes.c_void_p(c["tu"].data_ptr() + 4), P(c["ti"]), 4, V.I, P(users), 7, P(c["idx_a"][0]),
                                 P(c["idx_a"][1]), 12, P(probes), 3, 20, None, None, None, None, 0, P(items), P(scores), P(n_elig), eng._stream())
    assert bad != 0 and "16-byte aligned" in eng.lib.sml_last_error().decode()


def _clean(c):
    wi = c["wi"].copy()
    wi[c["lists_a"][V.NAN_LIST]] = wi[:2]
    return wi


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_device_centroids_equal_host_walk(dtype, d):
    c = dev_case(dtype, d)
    eng = engine(d)
    wi = _clean(c)
    rng = np.random.RandomState(5)
    for lists, idx in ((c["lists_a"], c["idx_a"]), (c["lists_b"], c["idx_b"])):
        tab = wi if lists is c["lists_a"] else wi[:c["b"]["n"]]
        cin = rng.randn(len(lists), d).astype(wi.dtype)
        want = V.host_centroids(tab, d, lists, cin)
        t_in = gpu(cin)
        got = eng.ivf_centroids(gpu(tab), idx[0], idx[1], t_in)
        assert got.data_ptr() != t_in.data_ptr() and got.cpu().numpy().tobytes() == want.tobytes(), (dtype, d, len(lists))
        assert eng.ivf_centroids(gpu(tab), idx[0], idx[1], t_in, out=t_in) is t_in and t_in.cpu().numpy().tobytes() == want.tobytes()


def _table(dtype, d):
    """A clean random table [420, d] on the device (the k-means tests: no NaN rows)."""
    rng = np.random.RandomState(31 + d)
    return gpu(rng.randn(V.I, d).astype(np.float32 if dtype == "fp32" else np.float16))


def _index_bytes(idx):
    return tuple(v.tobytes() for _, v in sorted(idx.host().items()))


@pytest.mark.parametrize("metric", ("cosine", "dot"))
@pytest.mark.parametrize("dtype,d", (("fp32", 32), ("fp16", 128)))
def test_build_is_reproducible_and_refresh_continues(dtype, d, metric):
    from sml_amd.retrieval import ItemIndex
    tab = _table(dtype, d)
    a = ItemIndex.build(tab, iters=3, seed=4, metric=metric)
    b = ItemIndex.build(tab, iters=3, seed=4, metric=metric)
    assert a.n_list == 20 and a.n_item == V.I and a.dtype == tab.dtype          # round(sqrt(420))
    assert _index_bytes(a) == _index_bytes(b)
    h = a.host()
    assert h["list_off"][0] == 0 and h["list_off"][-1] == V.I and (np.diff(h["list_off"]) >= 0).all()
    assert sorted(h["list_items"].tolist()) == list(range(V.I))
    for q in range(a.n_list):
        assert (np.diff(h["list_items"][h["list_off"][q]:h["list_off"][q + 1]]) > 0).all()
    assert a.sizes().cpu().tolist() == np.diff(h["list_off"]).tolist()
    assert _index_bytes(ItemIndex.build(tab, iters=3, seed=5, metric=metric)) != _index_bytes(a)
    two = ItemIndex.build(tab, iters=2, seed=4, metric=metric)
    assert _index_bytes(two.refresh(tab, iters=1)) == _index_bytes(a)
    # the lists are the assignment the definition states: every item sits in the list of its best centroid of the LAST assign
    pr = a.probe(tab, torch.arange(V.I, device=DEV), 3)
    assert pr.dtype == torch.int32 and tuple(pr.shape) == (V.I, 3) and int(pr.min()) >= 0 and int(pr.max()) < a.n_list


@functools.lru_cache(maxsize=None)
def model_case():
    """An fp32 model of width 32 over the case's tables (NaN rows, zero rows and all), its Seen set, and an index over it."""
    from sml_amd.mf import MFbasemode
    from sml_amd.retrieval import ItemIndex
    c = dev_case("fp32", 32)
    torch.manual_seed(0)
    model = MFbasemode(V.U, V.I, 32).to(DEV)
    model.user_laten.weight.data.copy_(c["tu"])
    model.item_laten.weight.data.copy_(c["ti"])
    idx = ItemIndex.build(model.item_laten.weight.data, n_list=12, iters=3, seed=1)
    return c, model, idx


def test_recommend_with_every_list_equals_recommend():
    from sml_amd.retrieval import ItemFilter, ItemIndex
    c, model, idx = model_case()
    users = gpu(V.USERS)
    assert sorted(idx.host()["list_items"].tolist()) == list(range(V.I))          # NaN rows and all: still a partition
    for extra in (dict(), dict(exclude=c["csr"]), dict(items=ItemFilter.from_mask(c["mask"])), dict(score="cosine"), dict(score="bias")):
        for k in (20, 128):
            want = model.recommend(users, k, **extra)
            got = model.recommend(users, k, index=idx, nprobe=idx.n_list, **extra)
            assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1])), (extra.keys(), k)
            none = model.recommend(users, k, index=None, **extra)
            assert torch.equal(none[0], want[0]) and torch.equal(bits(none[1]), bits(want[1]))
    # fewer probes: an exact answer over fewer items -- each row is topk_candidates on its probed lists
    eng = engine(32)
    probes = idx.probe(c["tu"], users, 2)
    got = model.recommend(users, 20, index=idx, nprobe=2, exclude=c["csr"])
    lists = V.concat_lists([l.astype(np.int64) for l in np.split(idx.host()["list_items"], idx.host()["list_off"][1:-1])], probes.cpu().numpy())
    want = eng.topk_candidates(c["tu"], c["ti"], users, tuple(gpu(t) for t in K.ragged(lists, np.int32)), 20, c["seen_dev"])
    assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))
    assert not torch.equal(got[0], model.recommend(users, 20, exclude=c["csr"])[0])
    assert model.recommend(users, 20, index=idx)[0].shape == (7, 20)               # the default nprobe: min(8, n_list)
    # diversify takes its pool from the indexed call; similar_items takes the same route
    a = model.recommend(users, 10, diversify=0.5, index=idx, nprobe=idx.n_list)
    b = model.recommend(users, 10, diversify=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))
    q = gpu(np.array([5, 17, 300], np.int64))
    for metric in ("dot", "cosine"):
        a = model.similar_items(q, 20, metric=metric, index=idx, nprobe=idx.n_list)
        b = model.similar_items(q, 20, metric=metric)
        assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1])), metric
    with pytest.raises(ValueError):
        model.recommend(users, 20, index=idx, candidates=[[1, 2]] * 7)
    with pytest.raises(ValueError):
        model.recommend(users, 20, index=ItemIndex.build(c["ti"][:100].contiguous(), n_list=4, iters=1))


def test_index_recall():
    from sml_amd.evaluation import index_recall
    c, model, idx = model_case()
    users = gpu(np.arange(V.U, dtype=np.int64))
    assert index_recall(model, idx, users, 20, nprobe=idx.n_list, exclude=c["csr"]) == 1.0
    got = index_recall(model, idx, users, 20, nprobe=2, exclude=c["csr"])
    exact = model.recommend(users, 20, exclude=c["csr"])[0].cpu().numpy()
    part = model.recommend(users, 20, exclude=c["csr"], index=idx, nprobe=2)[0].cpu().numpy()
    shares = [len(set(p[p >= 0]) & set(e[e >= 0])) / float((e >= 0).sum()) for p, e in zip(part, exact) if (e >= 0).any()]
    assert got == float(np.mean(np.array(shares, np.float64))) and 0.0 < got < 1.0
