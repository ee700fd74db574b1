"""The weighted neighbours of items on the MI355X: sml_cooc_topk_weighted through HipEngine.cooc_topk_weighted and the weighted
forms of sml_amd.knn.ItemNeighbours.

Every comparison of items, sims and counts is byte equality against the host walk of the same definition, which
tests/test_cooc_weighted_host.py holds to a restatement of the header.  Shapes: U = 48 users over I = 300 items
(tests/_knn_cases.py) with the planted weights of tests/_cooc_weighted_cases.py; rows on both sides of the on-chip limit, so both
accumulators run in every call."""
import functools

import numpy as np
import pytest
import torch

import _cooc_weighted_cases as W
import _knn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d=32):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same3(got, want, what):
    """(items int64, sims, n_elig) device tensors against the host walk's numpy triple, byte for byte."""
    C.same_bytes(got[0].cpu().numpy().astype(np.int32), want[0], (what, "items"))
    C.same_bytes(got[1].cpu().numpy(), want[1], (what, "sims"))
    C.same_bytes(got[2].cpu().numpy(), want[2], (what, "n_elig"))


@functools.lru_cache(maxsize=None)
def dev_case():
    c = dict(C.case())
    for name in ("by_user_csr", "by_item_csr"):
        c[name + "_dev"] = tuple(gpu(t) for t in c[name])
    c["allow_dev"] = gpu(c["allow_words"].view(np.int32))
    return c


def dev_norm(norm):
    na, nb = W.norms(norm, C.case()["by_item"])
    return None if na is None else (gpu(na), gpu(nb))


@pytest.mark.parametrize("F", W.FS)
@pytest.mark.parametrize("norm,shrink", ((None, 0.0), ("cosine", 0.0), ("cosine", 10.0), ("rp3", 0.0), ("rp3", 10.0)))
def test_device_equals_the_host_walk(norm, shrink, F):
    c = dev_case()
    eng = engine()
    w = W.weights(F)
    for k in (64, 128):
        want = W.host(k, w, F, norm=norm, shrink=shrink)
        got = eng.cooc_topk_weighted(c["by_item_csr_dev"], c["by_user_csr_dev"], k, gpu(w), frac_bits=F, norm=dev_norm(norm), shrink=shrink)
        same3(got, want, (norm, shrink, F, k))
    want = W.host(64, w, F, norm=norm, shrink=shrink, allow_words=c["allow_words"])
    got = eng.cooc_topk_weighted(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, gpu(w), frac_bits=F, norm=dev_norm(norm), shrink=shrink,
                                 allow=c["allow_dev"])
    same3(got, want, (norm, shrink, F, "filtered"))


def test_geometry_and_path_never_change_a_byte():
    c = dev_case()
    eng = engine(64)                                     # (any engine's context serves)
    w = W.weights(30)
    want = W.host(64, w, 30, norm="rp3")
    for mw in (1, 3, 0):
        for path in (0, 1, 2):
            got = eng.cooc_topk_weighted(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, gpu(w), frac_bits=30, norm=dev_norm("rp3"),
                                         max_workgroups=mw, path=path)
            same3(got, want, (mw, path))
    rows = np.array([17, 3, 0, 299, 3, 250, 17, 1, 42], np.int64)        # permuted, with repeats
    for path in (1, 2):
        got = eng.cooc_topk_weighted(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, gpu(w), frac_bits=30, rows=gpu(rows),
                                     norm=dev_norm("rp3"), path=path)
        same3(got, tuple(x[rows] for x in want), ("rows", path))


@pytest.mark.parametrize("norm", (None, "cosine"))
def test_unit_weights_return_cooc_topk_bytes_on_the_device(norm):
    c = dev_case()
    eng = engine()
    ones = torch.ones(C.U, device=DEV)
    for path in (1, 2):
        for kw in (dict(), dict(shrink=10.0), dict(allow=c["allow_dev"])):
            want = eng.cooc_topk(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, norm=dev_norm(norm), min_co=1, **kw)
            got = eng.cooc_topk_weighted(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, ones, frac_bits=0, norm=dev_norm(norm),
                                         path=path, **kw)
            for g, x in zip(got, want):
                C.same_bytes(g.cpu().numpy(), x.cpu().numpy(), (norm, path, sorted(kw)))


def _raw(eng, c, w, scratch, items, sims, ne, k, path=0, F=30, mw=0, user_w=True):
    from sml_amd.engine import _ptr
    (i_off, i_users), (u_off, u_items) = c["by_item_csr_dev"], c["by_user_csr_dev"]
    return eng.lib.sml_cooc_topk_weighted(eng._ctx, _ptr(i_off), _ptr(i_users), _ptr(u_off), _ptr(u_items), C.U, C.I, None, C.I,
                                          _ptr(w) if user_w else None, F, None, None, 0.0, None, k, mw, path, _ptr(scratch), _ptr(items),
                                          _ptr(sims), _ptr(ne), eng._stream())


def test_scratch_is_left_zero_and_a_refused_call_writes_nothing():
    c = dev_case()
    eng = engine()
    k = 16
    w_host = W.weights(30)
    w = gpu(w_host)
    nbytes = eng.lib.sml_cooc_weighted_scratch_bytes(eng._ctx, C.I, 0)
    assert nbytes > 0 and 0 < eng.lib.sml_cooc_weighted_scratch_bytes(eng._ctx, C.I, 3) < nbytes
    assert eng.lib.sml_cooc_weighted_scratch_bytes(eng._ctx, 0, 0) < 0 and eng.lib.sml_cooc_weighted_scratch_bytes(eng._ctx, C.I, -1) < 0
    scratch = torch.full((nbytes,), 0x5a, device=DEV, dtype=torch.uint8)          # the call zeroes it itself
    items = torch.full((C.I, k), 77, device=DEV, dtype=torch.int32)
    sims = torch.full((C.I, k), 7.0, device=DEV, dtype=torch.float32)
    ne = torch.full((C.I,), 77, device=DEV, dtype=torch.int32)
    for kw in (dict(k=0), dict(k=129), dict(path=3), dict(path=-1), dict(mw=-1), dict(F=-1), dict(F=33), dict(user_w=False)):
        assert _raw(eng, c, w, scratch, items, sims, ne, **dict(dict(k=k), **kw)) != 0 and eng.lib.sml_last_error(), kw
    assert _raw(eng, c, w, scratch[16:], items, sims, ne, k) != 0                   # a misaligned scratch
    assert _raw(eng, c, w, scratch, items, items.view(torch.float32), ne, k) != 0   # overlapping outputs
    assert _raw(eng, c, sims.view(-1), scratch, items, sims, ne, k) != 0            # an output on the weights
    torch.cuda.synchronize()
    assert (items == 77).all() and (sims == 7.0).all() and (ne == 77).all() and (scratch == 0x5a).all()
    want = W.host(k, w_host, 30)
    one = eng.lib.sml_cooc_weighted_scratch_bytes(eng._ctx, C.I, 1)                 # one workgroup's share
    for path in (1, 2):
        # the whole of a one-workgroup scratch is used, and is zero afterwards
        small = torch.full((one,), 0x5a, device=DEV, dtype=torch.uint8)
        assert _raw(eng, c, w, small, items, sims, ne, k, path=path, mw=1) == 0
        torch.cuda.synchronize()
        assert (small == 0).all(), path
        same3((items.long(), sims, ne), want, (path, "one workgroup"))
        # the grid's own choice: what it uses (the first workgroup's share at least) is zero, the rest is untouched
        scratch.fill_(0x5a)
        assert _raw(eng, c, w, scratch, items, sims, ne, k, path=path) == 0
        torch.cuda.synchronize()
        assert (scratch[:one] == 0).all() and ((scratch == 0) | (scratch == 0x5a)).all(), path
        same3((items.long(), sims, ne), want, path)


def test_engine_refuses_a_weight_tensor_of_the_wrong_kind():
    c = dev_case()
    eng = engine()
    for bad in (torch.ones(C.U, device=DEV, dtype=torch.float64), torch.ones(C.U + 1, device=DEV), torch.ones(C.U),
                torch.ones(2 * C.U, device=DEV)[::2], np.ones(C.U, np.float32)):
        with pytest.raises(ValueError):
            eng.cooc_topk_weighted(c["by_item_csr_dev"], c["by_user_csr_dev"], 8, bad)


def _pairs():
    return np.array([(u, i) for u, s in enumerate(C.case()["sets"]) for i in s], np.int64)


@pytest.mark.parametrize("metric", ("rp3beta", "p3alpha"))
def test_item_neighbours_from_a_device_set_equals_the_host_route(metric):
    from sml_amd import knn
    from sml_amd.retrieval import DeviceSeen, SeenItems
    eng = engine()
    seen = DeviceSeen(C.U, C.I, eng).add(_pairs())
    host_seen = SeenItems(C.U, C.I).add(_pairs())
    nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=C.K_NBR, metric=metric, shrink=0.5, engine=eng)
    hb = knn.ItemNeighbours.build(host_seen, C.U, C.I, k=C.K_NBR, metric=metric, shrink=0.5, engine="host")
    same3((nb.items, nb.sims, nb.n_nbr), (hb.items.numpy().astype(np.int32), hb.sims.numpy(), hb.n_nbr.numpy()), metric)
    assert nb.frac_bits == hb.frac_bits and nb.metric == metric and nb.items.dtype == torch.int64
    users = np.array([5, 1, 30, 0, 5], np.int64)
    it, sc = nb.recommend(seen, users=users, topK=20, exclude=seen)
    hi, hs = hb.recommend(host_seen, users=users, topK=20, exclude=host_seen)
    C.same_bytes(it.cpu().numpy(), hi.numpy())
    C.same_bytes(sc.cpu().numpy(), hs.numpy())


def test_item_neighbours_with_a_user_weight_from_a_device_set():
    from sml_amd import knn
    from sml_amd.retrieval import DeviceSeen, SeenItems
    eng = engine()
    seen = DeviceSeen(C.U, C.I, eng).add(_pairs())
    host_seen = SeenItems(C.U, C.I).add(_pairs())
    uw = torch.from_numpy(W.weights(30))
    nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=32, metric="cosine", user_weight=uw, engine=eng)
    hb = knn.ItemNeighbours.build(host_seen, C.U, C.I, k=32, metric="cosine", user_weight=uw, engine="host")
    same3((nb.items, nb.sims, nb.n_nbr), (hb.items.numpy().astype(np.int32), hb.sims.numpy(), hb.n_nbr.numpy()), "user_weight")
    assert nb.frac_bits == hb.frac_bits
