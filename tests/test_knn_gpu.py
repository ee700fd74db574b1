"""The neighbourhood model on the MI355X: sml_cooc_topk / sml_knn_topk through HipEngine.cooc_topk / knn_topk,
sml_amd.knn.ItemNeighbours and evaluation.recall_of_lists.

Every comparison of items, similarities, scores and counts is byte equality against the host walks of the same definitions,
which tests/test_knn_host.py holds to a restatement of the header.  Shapes: U = 48 users over I = 300 items
(tests/_knn_cases.py), rows on both sides of the on-chip limit, so both accumulators run in every call."""
import functools

import numpy as np
import pytest
import torch

import _knn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d=32):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same3(got, want, what):
    """(items int64, scores, n_elig) device tensors against the host walk's numpy triple, byte for byte."""
    C.same_bytes(got[0].cpu().numpy().astype(np.int32), want[0], (what, "items"))
    C.same_bytes(got[1].cpu().numpy(), want[1], (what, "scores"))
    C.same_bytes(got[2].cpu().numpy(), want[2], (what, "n_elig"))


@functools.lru_cache(maxsize=None)
def dev_case():
    c = dict(C.case())
    for name in ("by_user_csr", "by_item_csr", "seen_csr"):
        c[name + "_dev"] = tuple(gpu(t) for t in c[name])
    c["allow_dev"] = gpu(c["allow_words"].view(np.int32))
    return c


def dev_norm(norm):
    na, nb = C.norms(norm, C.case()["by_item"])
    return None if na is None else (gpu(na), gpu(nb))


@pytest.mark.parametrize("norm,shrink,min_co", ((None, 0.0, 1), (None, 0.0, 2), ("cosine", 0.0, 1), ("cosine", 10.0, 2),
                                                ("asymmetric", 10.0, 1)))
def test_cooc_equals_the_host_walk(norm, shrink, min_co):
    c = dev_case()
    eng = engine()
    for k in (1, 64, 128):
        want = C.host_cooc(k, norm=norm, shrink=shrink, min_co=min_co)
        got = eng.cooc_topk(c["by_item_csr_dev"], c["by_user_csr_dev"], k, norm=dev_norm(norm), shrink=shrink, min_co=min_co)
        same3(got, want, (norm, shrink, min_co, k))
    want = C.host_cooc(5, norm=norm, shrink=shrink, min_co=min_co, allow_words=c["allow_words"])
    got = eng.cooc_topk(c["by_item_csr_dev"], c["by_user_csr_dev"], 5, norm=dev_norm(norm), shrink=shrink, min_co=min_co,
                        allow=c["allow_dev"])
    same3(got, want, (norm, shrink, min_co, "filtered"))


def test_cooc_geometry_and_path_never_change_a_byte():
    c = dev_case()
    eng = engine(64)                                     # (any engine's context serves)
    want = C.host_cooc(64, norm="cosine")
    for mw in (0, 1, 7):
        for path in (0, 1, 2):
            got = eng.cooc_topk(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, norm=dev_norm("cosine"), max_workgroups=mw, path=path)
            same3(got, want, (mw, path))
    rows = np.array([17, 3, 0, 299, 3, 250, 17, 1, 42], np.int64)        # permuted, with repeats
    for path in (1, 2):
        got = eng.cooc_topk(c["by_item_csr_dev"], c["by_user_csr_dev"], 64, rows=gpu(rows), norm=dev_norm("cosine"), path=path)
        same3(got, tuple(w[rows] for w in want), ("rows", path))


@pytest.mark.parametrize("norm,F", ((None, 0), ("cosine", 30), ("cosine", 0), ("asymmetric", 30)))
def test_knn_equals_the_host_walk(norm, F):
    c = dev_case()
    eng = engine()
    ti, ts = C.table(norm)
    t_items, t_sims = gpu(ti), gpu(ts)
    for k in (1, 5, 128):
        want = C.host_knn(ti, ts, C.I, c["by_user_csr"], k, frac_bits=F)
        got = eng.knn_topk(t_items, t_sims, C.I, c["by_user_csr_dev"], k, frac_bits=F)
        same3(got, want, (norm, F, k))
    want = C.host_knn(ti, ts, C.I, c["by_user_csr"], 64, frac_bits=F, seen_csr=c["seen_csr"], allow_words=c["allow_words"])
    got = eng.knn_topk(t_items, t_sims, C.I, c["by_user_csr_dev"], 64, frac_bits=F, seen=c["seen_csr_dev"], allow=c["allow_dev"])
    same3(got, want, (norm, F, "seen and filter"))


def test_knn_geometry_and_path_never_change_a_byte():
    c = dev_case()
    eng = engine(128)
    ti, ts = C.table("cosine")
    t_items, t_sims = gpu(ti), gpu(ts)
    want = C.host_knn(ti, ts, C.I, c["by_user_csr"], 20, seen_csr=c["by_user_csr"])
    for mw in (0, 1, 5):
        for path in (0, 1, 2):
            got = eng.knn_topk(t_items, t_sims, C.I, c["by_user_csr_dev"], 20, seen=c["by_user_csr_dev"], max_workgroups=mw, path=path)
            same3(got, want, (mw, path))
    users = np.array([40, 2, 1, 0, 2, 47, 40, 9, 13], np.int64)          # permuted, with repeats
    for path in (1, 2):
        got = eng.knn_topk(t_items, t_sims, C.I, c["by_user_csr_dev"], 20, users=gpu(users), seen=c["by_user_csr_dev"], path=path)
        same3(got, tuple(w[users] for w in want), ("users", path))


def test_knn_narrow_tables_cancelling_sums_and_junk():
    """k_nbr = 4 (sixteen members per round) and k_nbr = 128 (two rounds per member); a sum that cancels to 0 is listed; members,
    ids and sims out of range contribute nothing -- on both paths."""
    eng = engine()
    ti = np.full((4, 4), -1, np.int32)
    ts = np.full((4, 4), -np.inf, np.float32)
    ti[0], ts[0] = [9, 3, 40, -5], [0.5, 0.25, 1.0, 1.0]
    ti[1], ts[1] = [9, 4, 5, 6], [-0.5, np.nan, np.inf, -np.inf]
    ti[2], ts[2] = [7, 8, 3, 2], [8.0, 4.0, 0.25, 2.0 ** 33]
    ti[3], ts[3] = [1, 1, 1, 1], [1.0, 1.0, 1.0, 1.0]
    # (the last two: 40 and 44 slots over 40 items, on either side of "more slots than items", where the dense path claims its
    # candidates from the touched bitmap instead of a second walk)
    sets = [[0, 1, 2, -1, 4, 2 ** 31 - 1], [2], [], [0, 1], [3, 3, 0], [0, 1, 2, 3, 2, 0, 3, 2, 1, 0], [0, 1, 2, 3, 2, 0, 3, 2, 1, 0, 2]]
    hist = C.csr(sets)
    hist_dev = tuple(gpu(t) for t in hist)
    for F in (30, 0):
        want = C.host_knn(ti, ts, 40, hist, 8, frac_bits=F)
        for path in (1, 2):
            got = eng.knn_topk(gpu(ti), gpu(ts), 40, hist_dev, 8, frac_bits=F, path=path)
            same3(got, want, (F, path))
    assert want is not None and C.host_knn(ti, ts, 40, hist, 8, frac_bits=30)[0][3].tolist()[:3] == [3, 9, -1]
    wide_i, wide_s = C.host_cooc(128, norm="cosine")[:2]
    c = dev_case()
    want = C.host_knn(wide_i, wide_s, C.I, c["by_user_csr"], 33)
    for path in (1, 2):
        same3(eng.knn_topk(gpu(wide_i), gpu(wide_s), C.I, c["by_user_csr_dev"], 33, path=path), want, ("k_nbr 128", path))


def _raw_cooc(eng, c, scratch, items, sims, ne, k, path=0, min_co=1, mw=0):
    from sml_amd.engine import _ptr
    (i_off, i_users), (u_off, u_items) = c["by_item_csr_dev"], c["by_user_csr_dev"]
    return eng.lib.sml_cooc_topk(eng._ctx, _ptr(i_off), _ptr(i_users), _ptr(u_off), _ptr(u_items), C.U, C.I, None, C.I, None, None, 0.0,
                                 min_co, None, k, mw, path, _ptr(scratch), _ptr(items), _ptr(sims), _ptr(ne), eng._stream())


def _raw_knn(eng, c, t_items, t_sims, scratch, items, scores, ne, k, path=0, F=30, mw=0):
    from sml_amd.engine import _ptr
    h_off, h_items = c["by_user_csr_dev"]
    return eng.lib.sml_knn_topk(eng._ctx, _ptr(t_items), _ptr(t_sims), C.I, C.K_NBR, C.I, _ptr(h_off), _ptr(h_items), None, C.U, F, None,
                                None, None, k, mw, path, _ptr(scratch), _ptr(items), _ptr(scores), _ptr(ne), eng._stream())


def test_scratch_is_left_zero_and_a_refused_call_writes_nothing():
    c = dev_case()
    eng = engine()
    k = 16
    ti, ts = C.table("cosine")
    t_items, t_sims = gpu(ti), gpu(ts)
    for kind in (0, 1):
        n = C.I if kind == 0 else C.U
        nbytes = eng.lib.sml_knn_scratch_bytes(eng._ctx, C.I, 0, kind)
        assert nbytes > 0 and eng.lib.sml_knn_scratch_bytes(eng._ctx, C.I, 3, kind) < nbytes
        assert eng.lib.sml_knn_scratch_bytes(eng._ctx, 0, 0, kind) < 0 and eng.lib.sml_knn_scratch_bytes(eng._ctx, C.I, 0, 2) < 0
        scratch = torch.full((nbytes,), 0x5a, device=DEV, dtype=torch.uint8)          # the call zeroes it itself
        items = torch.full((n, k), 77, device=DEV, dtype=torch.int32)
        sims = torch.full((n, k), 7.0, device=DEV, dtype=torch.float32)
        ne = torch.full((n,), 77, device=DEV, dtype=torch.int32)

        def call(scr, **kw):
            if kind == 0:
                return _raw_cooc(eng, c, scr, items, sims, ne, **dict(dict(k=k), **kw))
            return _raw_knn(eng, c, t_items, t_sims, scr, items, sims, ne, **dict(dict(k=k), **kw))

        for kw in (dict(k=0), dict(k=129), dict(path=3), dict(path=-1), dict(mw=-1)) + \
                ((dict(min_co=0),) if kind == 0 else (dict(F=33), dict(F=-1))):
            assert call(scratch, **kw) != 0 and eng.lib.sml_last_error(), (kind, kw)
        odd = scratch[16:]
        if kind == 0:
            assert _raw_cooc(eng, c, odd, items, sims, ne, k) != 0              # a misaligned scratch
            assert _raw_cooc(eng, c, scratch, items, items.view(torch.float32), ne, k) != 0          # overlapping outputs
        else:
            assert _raw_knn(eng, c, t_items, t_sims, odd, items, sims, ne, k) != 0
            assert _raw_knn(eng, c, t_items, t_sims, scratch, items, t_sims, ne, k) != 0             # an output on an input
        torch.cuda.synchronize()
        assert (items == 77).all() and (sims == 7.0).all() and (ne == 77).all() and (scratch == 0x5a).all(), kind
        want = C.host_cooc(k) if kind == 0 else C.host_knn(ti, ts, C.I, c["by_user_csr"], k)
        one = eng.lib.sml_knn_scratch_bytes(eng._ctx, C.I, 1, kind)             # one workgroup's share
        for path in (1, 2):
            # the whole of a one-workgroup scratch is used, and is zero afterwards
            small = torch.full((one,), 0x5a, device=DEV, dtype=torch.uint8)
            assert call(small, path=path, mw=1) == 0
            torch.cuda.synchronize()
            assert (small == 0).all(), (kind, path)
            same3((items.long(), sims, ne), want, (kind, path, "one workgroup"))
            # the grid's own choice: what it uses (the first workgroup's share at least) is zero, the rest is untouched
            scratch.fill_(0x5a)
            assert call(scratch, path=path) == 0
            torch.cuda.synchronize()
            assert (scratch[:one] == 0).all() and ((scratch == 0) | (scratch == 0x5a)).all(), (kind, path)
            same3((items.long(), sims, ne), want, (kind, path))


def _pairs():
    return np.array([(u, i) for u, s in enumerate(C.case()["sets"]) for i in s], np.int64)


@pytest.mark.parametrize("metric", ("cosine", "asymmetric", "count"))
def test_item_neighbours_end_to_end_on_a_device_set(metric):
    from sml_amd import knn
    from sml_amd.retrieval import DeviceSeen, ItemFilter
    c = dev_case()
    eng = engine()
    seen = DeviceSeen(C.U, C.I, eng).add(_pairs())
    among = ItemFilter.from_mask(c["allow"])
    nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=C.K_NBR, metric=metric, alpha=C.ALPHA, shrink=1.0, engine=eng)
    deg = torch.tensor([len(s) for s in c["by_item"]], dtype=torch.float64, device=DEV)          # the tables as build makes them
    tables = None if metric == "count" else (deg.sqrt().cpu().numpy(),) * 2 if metric == "cosine" else \
        (deg.pow(C.ALPHA).cpu().numpy(), deg.pow(1.0 - C.ALPHA).cpu().numpy())
    want = C.host_cooc(C.K_NBR, shrink=1.0, norm_tables=tables)
    same3((nb.items, nb.sims, nb.n_nbr), (want[0], want[1], np.minimum(want[2], C.K_NBR).astype(np.int32)), metric)
    assert nb.frac_bits == (0 if metric == "count" else 30) and nb.items.dtype == torch.int64
    it, sc = nb.recommend(seen, topK=20)
    w = C.host_knn(want[0], want[1], C.I, c["by_user_csr"], 20, frac_bits=nb.frac_bits)
    C.same_bytes(it.cpu().numpy().astype(np.int32), w[0])
    C.same_bytes(sc.cpu().numpy(), w[1])
    users = np.array([5, 1, 30, 0, 5], np.int64)
    it, sc = nb.recommend(seen, users=users, topK=20, exclude=seen, items=among)
    w = C.host_knn(want[0], want[1], C.I, c["by_user_csr"], 20, users=users, frac_bits=nb.frac_bits, seen_csr=c["by_user_csr"],
                   allow_words=c["allow_words"])
    C.same_bytes(it.cpu().numpy().astype(np.int32), w[0])
    C.same_bytes(sc.cpu().numpy(), w[1])
    si, ss = nb.similar_items([3, 299, 3], 7)
    C.same_bytes(si.cpu().numpy().astype(np.int32), want[0][[3, 299, 3], :7])
    among_nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=8, metric=metric, alpha=C.ALPHA, min_co=2, among=among, engine=eng)
    w = C.host_cooc(8, min_co=2, allow_words=c["allow_words"],
                    norm_tables=None if tables is None else tables)
    C.same_bytes(among_nb.items.cpu().numpy().astype(np.int32), w[0])
    C.same_bytes(among_nb.sims.cpu().numpy(), w[1])


@functools.lru_cache(maxsize=None)
def model32():
    from sml_amd.mf import MFbasemode
    torch.manual_seed(23)
    return MFbasemode(C.U, C.I, 32).to(DEV)


def test_from_model_on_a_d32_model():
    from sml_amd import knn
    c = dev_case()
    m = model32()
    nb = knn.ItemNeighbours.from_model(m, 16)
    it, sc = m.similar_items(torch.arange(C.I), 16)
    assert torch.equal(nb.items, it) and torch.equal(nb.sims, sc) and (nb.n_nbr == 16).all() and nb.metric == "model:cosine"
    top = float(sc.abs().max())
    assert 0 <= nb.frac_bits <= 32 and top * 2.0 ** nb.frac_bits <= 2.0 ** 32
    assert nb.frac_bits == 32 or top * 2.0 ** (nb.frac_bits + 1) > 2.0 ** 32
    got = nb.recommend(c["by_user_csr_dev"], topK=20, exclude=c["by_user_csr_dev"])
    w = C.host_knn(it.cpu().numpy().astype(np.int32), sc.cpu().numpy(), C.I, c["by_user_csr"], 20, frac_bits=nb.frac_bits,
                   seen_csr=c["by_user_csr"])
    C.same_bytes(got[0].cpu().numpy().astype(np.int32), w[0])
    C.same_bytes(got[1].cpu().numpy(), w[1])
    single = nb.recommend(C.csr([[i] for i in range(C.I)]), topK=16)[0]
    assert torch.equal(single.sort(1)[0], it.sort(1)[0])                   # a history {i}: item i's neighbours, as a set


def test_recall_of_lists_is_the_list_half_of_recall_curve():
    from sml_amd import evaluation as E, knn
    from sml_amd.retrieval import SeenItems, held_out, nonempty_users
    c = dev_case()
    m = model32()
    rng = np.random.RandomState(5)
    pairs = np.stack([rng.randint(0, C.U, 200), rng.randint(0, C.I, 200)], 1).astype(np.int64)
    pairs = pairs[pairs[:, 0] % 5 != 0]                                    # some users have no held-out item
    held = held_out(pairs, C.U, C.I)
    e = SeenItems(C.U, C.I).add(_pairs()[::3])
    ks = (1, 5, 20, 100)
    users = nonempty_users(held)[0]
    lists = m.recommend(torch.from_numpy(users), max(ks), exclude=e)[0]
    assert E.recall_of_lists(lists, users, held, ks) == E.recall_curve(m, held, ks, exclude=e)
    nb = knn.ItemNeighbours.build(e, C.U, C.I, k=32, engine=engine())
    r = E.recall_of_lists(nb.recommend(e, users=users, topK=100, exclude=e)[0], users, held, ks)
    assert len(r) == 4 and all(0.0 <= a <= b <= 1.0 for a, b in zip(r, r[1:]))
