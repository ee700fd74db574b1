"""The neighbourhood model, the parts that need no GPU: the C ABI surface, sml_host_cooc_topk and sml_host_knn_topk -- the
definitions of sml_cooc_topk and sml_knn_topk as single-threaded walks over host memory -- against a numpy restatement of the
header's text (byte equality), the defining identities, every refusal of the host entry points, ItemNeighbours on the host route
and recall_of_lists."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _knn_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sml_knn_lds_limit": 0, "sml_knn_scratch_bytes": 4, "sml_cooc_topk": 22, "sml_host_cooc_topk": 17, "sml_knn_topk": 22,
         "sml_host_knn_topk": 17}


def test_abi_surface():
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "knn.hip" in build.SOURCES and "topk_list.h" in build.HEADERS
    for name, n_args in NAMES.items():
        res_c = "int64_t " if name == "sml_knn_scratch_bytes" else "int "
        assert res_c + name + "(" in header and name in _lib.SIGNATURES and name in syms, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int64 if res_c == "int64_t " else ctypes.c_int) and len(args) == n_args, name
        decl = header[header.index(res_c + name + "("):]
        decl = decl[:decl.index(");")]
        params = [p.strip() for p in decl[decl.index("(") + 1:].split(",") if p.strip() != "void"]
        assert len(params) == n_args, (name, params)
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else \
                ctypes.c_double if p.startswith("double") else ctypes.c_int
            assert a is want, (name, p, a)
    for phrase in ("NEIGHBOURS", "c(j) = #{u in U(i) : j in S(u)}, an integer", "den = norm_a[i] * norm_b[j], one fp64 rounding",
                   "the correctly rounded fp64 division", "The definition contains no square root",
                   "sim(i, j) and sim(j, i) are the same bits", "q = llrint(ldexp((double)sim, F)), round to nearest even",
                   "is skipped before any address is formed", "a j whose sum cancels to 0 is still a candidate",
                   "Score A = (float)ldexp((double)acc, -F)", "a k'-call is the prefix of a k-call",
                   "max_workgroups and path never change a byte", "a row named twice is written twice with the same bytes",
                   "which therefore can never fill", "a refused call writes nothing", "Not measured: real periods"):
        assert phrase in header, phrase
    with open(os.path.join(REPO, "sml_amd", "csrc", "knn.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src
    assert _lib.load().sml_knn_lds_limit() > 0


def test_rows_fall_on_both_sides_of_the_limit():
    from sml_amd import _lib
    limit = _lib.load().sml_knn_lds_limit()
    c = C.case()
    below, above = C.sides([C.cooc_total(c, i) for i in range(C.I)], limit)
    assert len(below) >= 10 and len(above) >= 10, (limit, len(below), len(above))
    below, above = C.sides([len(s) * C.K_NBR for s in c["sets"]], limit)
    assert len(below) >= 5 and len(above) >= 5, (limit, len(below), len(above))
    assert sum(1 for s in c["sets"] if 1 <= len(s) <= 5) >= 10 and len(c["sets"][0]) == 0 and len(c["sets"][1]) == C.I - 1


# ---- neighbours of items -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_co", (1, 2))
@pytest.mark.parametrize("shrink", (0.0, 10.0))
@pytest.mark.parametrize("norm", C.NORMS)
def test_host_cooc_equals_the_restatement(norm, shrink, min_co):
    c = C.case()
    want = C.ref_cooc(None, 128, norm, shrink, min_co)
    for k in C.KS:
        got = C.host_cooc(k, norm=norm, shrink=shrink, min_co=min_co)
        for g, w, what in zip(got, (want[0][:, :k], want[1][:, :k], want[2]), ("items", "sims", "n_elig")):
            C.same_bytes(g, w, (what, norm, shrink, min_co, k))                 # (also: a k'-call is the prefix of a k-call)
    got = C.host_cooc(64, norm=norm, shrink=shrink, min_co=min_co, allow_words=c["allow_words"])
    want = C.ref_cooc(None, 64, norm, shrink, min_co, allow=c["allow"])
    for g, w in zip(got, want):
        C.same_bytes(g, w, ("filtered", norm, shrink, min_co))
    assert (got[0][C.I - 1] == -1).all() and np.isneginf(got[1][C.I - 1]).all() and got[2][C.I - 1] == 0      # the item with no user


def test_cooc_counts_are_the_gram_of_the_interaction_matrix():
    c = C.case()
    x = np.zeros((C.U, C.I), np.int64)
    for u, s in enumerate(c["sets"]):
        x[u, s] = 1
    g = x.T @ x
    np.fill_diagonal(g, 0)
    k = 128
    items, sims, n_elig = C.host_cooc(k)
    heavy = 0
    for i in range(C.I):
        nz = np.nonzero(g[i])[0]
        if len(nz) > k:                                  # (the rows of the heavy user: more neighbours than a list holds)
            heavy += 1
            assert n_elig[i] == len(nz)
            continue
        assert n_elig[i] == len(nz)
        got = dict(zip(items[i, :len(nz)].tolist(), sims[i, :len(nz)].tolist()))
        assert got == {int(j): float(g[i, j]) for j in nz} and (items[i, len(nz):] == -1).all(), i
    assert heavy == C.I - 1
    # with the heavy user left out, whole rows fit: the row IS the non-zero off-diagonal of X^T X
    sets = [s if u != 1 else np.zeros(0, np.int64) for u, s in enumerate(c["sets"])]
    x[1] = 0
    g = x.T @ x
    np.fill_diagonal(g, 0)
    by_item = C.transpose(sets, C.I)
    from sml_amd import _lib
    (i_off, i_users), (u_off, u_items) = C.csr(by_item), C.csr(sets)
    i_users, u_items = C._tail(i_users), C._tail(u_items)
    k = 128
    items, sims, n_elig = np.zeros((C.I, k), np.int32), np.zeros((C.I, k), np.float32), np.zeros(C.I, np.int32)
    _lib.check(_lib.load().sml_host_cooc_topk(C._p(i_off), C._p(i_users), C._p(u_off), C._p(u_items), C.U, C.I, None, C.I, None, None, 0.0,
                                              1, None, k, C._p(items), C._p(sims), C._p(n_elig)), "sml_host_cooc_topk")
    whole = 0
    for i in range(C.I):
        nz = np.nonzero(g[i])[0]
        assert n_elig[i] == len(nz)
        if len(nz) <= k:
            whole += 1
            got = dict(zip(items[i, :len(nz)].tolist(), sims[i, :len(nz)].tolist()))
            assert got == {int(j): float(g[i, j]) for j in nz} and (items[i, len(nz):] == -1).all(), i
    assert whole >= 100, whole


@pytest.mark.parametrize("shrink", (0.0, 10.0))
def test_cosine_is_symmetric_in_bits(shrink):
    among = np.zeros(C.I, bool)
    among[100:200] = True                                # (a filter of 100 items: the whole filtered row fits a list of 128)
    items, sims, n_elig = C.host_cooc(128, norm="cosine", shrink=shrink, rows=np.arange(100, 200), allow_words=C.words(among))
    assert (n_elig == 99).all()                          # the heavy user makes every pair co-occur
    sim = {}
    for x, i in enumerate(range(100, 200)):
        for j, s in zip(items[x, :99].tolist(), sims[x, :99]):
            sim[(i, j)] = s.tobytes()
    assert len(sim) == 9900 and all(sim[(i, j)] == sim[(j, i)] for i, j in sim)


def test_cooc_rows_permuted_with_a_repeat():
    full = C.host_cooc(64, norm="cosine")
    rows = np.array([17, 3, 0, 299, 3, 250, 17, 1], np.int64)
    got = C.host_cooc(64, rows=rows, norm="cosine")
    for g, f in zip(got, full):
        C.same_bytes(g, f[rows])
    got = C.host_cooc(64, rows=np.zeros(0, np.int64))
    assert got[0].shape == (0, 64)


def test_cooc_nan_is_not_eligible_and_inf_is():
    c = C.case()
    a = np.sqrt(np.array([len(s) for s in c["by_item"]], np.float64))
    b = a.copy()
    b[5], b[7] = np.nan, 0.0
    items, sims, n_elig = C.host_cooc(128, rows=np.array([200], np.int64), norm_tables=(a, b))
    plain = C.host_cooc(128, rows=np.array([200], np.int64), norm="cosine")
    co = C.counts()[200]
    assert co[5] > 0 and co[7] > 0
    assert 5 not in items[0] and items[0, 0] == 7 and np.isposinf(sims[0, 0]) and n_elig[0] == plain[2][0] - 1


# ---- the list of a history -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,F", ((None, 0), ("cosine", 30), ("cosine", 0), ("asymmetric", 30)))
def test_host_knn_equals_the_restatement(norm, F):
    c = C.case()
    ti, ts = C.table(norm)
    want = C.ref_knn(ti, ts, C.I, c["sets"], None, 128, F)
    for k in C.KS:
        got = C.host_knn(ti, ts, C.I, c["by_user_csr"], k, frac_bits=F)
        for g, w, what in zip(got, (want[0][:, :k], want[1][:, :k], want[2]), ("items", "scores", "n_elig")):
            C.same_bytes(g, w, (what, norm, F, k))
    got = C.host_knn(ti, ts, C.I, c["by_user_csr"], 64, frac_bits=F, seen_csr=c["seen_csr"], allow_words=c["allow_words"])
    want = C.ref_knn(ti, ts, C.I, c["sets"], None, 64, F, seen=c["seen"], allow=c["allow"])
    for g, w in zip(got, want):
        C.same_bytes(g, w, ("seen and filter", norm, F))
    assert got[2][0] == 0 and (got[0][0] == -1).all()                      # the empty history


def test_knn_filter_is_the_complement_added_to_seen():
    c = C.case()
    ti, ts = C.table("cosine")
    filtered = C.host_knn(ti, ts, C.I, c["by_user_csr"], 64, seen_csr=c["seen_csr"], allow_words=c["allow_words"])
    denied = np.nonzero(~c["allow"])[0]
    seen2 = [np.union1d(s, denied) for s in c["seen"]]
    plain = C.host_knn(ti, ts, C.I, c["by_user_csr"], 64, seen_csr=C.csr(seen2))
    for f, p in zip(filtered, plain):
        C.same_bytes(f, p)


def test_knn_exclude_history_and_users_with_a_repeat():
    c = C.case()
    ti, ts = C.table("cosine")
    full = C.host_knn(ti, ts, C.I, c["by_user_csr"], 20, seen_csr=c["by_user_csr"])
    for u, s in enumerate(c["sets"]):
        assert not set(full[0][u].tolist()) & set(s.tolist())
    assert full[2][1] == 0                                                 # the user who holds everything has nothing left
    users = np.array([40, 2, 1, 0, 2, 47, 40], np.int64)
    got = C.host_knn(ti, ts, C.I, c["by_user_csr"], 20, users=users, seen_csr=c["by_user_csr"])
    for g, f in zip(got, full):
        C.same_bytes(g, f[users])


def test_single_item_history_returns_the_neighbour_list():
    """A history {i} with no Seen and no filter returns item i's list, ids in the same order.  The scores are bit-equal because
    every sim is a multiple of 2^-30: cosine sims of this case are count / sqrt(deg_i deg_j) >= 1 / 48 >= 2^-7, and a float32 at
    or above 2^-7 has an ulp of at least 2^-30.  Counts (F = 0) are integers."""
    for norm in (None, "cosine"):
        ti, ts = C.table(norm)
        live = ti >= 0
        assert np.isfinite(ts[live]).all() and (ts[live] >= 1.0 / 48 - 1e-9).all()
        hist = C.csr([[i] for i in range(C.I)])
        items, scores, n_elig = C.host_knn(ti, ts, C.I, hist, C.K_NBR, frac_bits=C.frac_bits(norm))
        C.same_bytes(items, ti, norm)
        C.same_bytes(scores, ts, norm)
        assert (n_elig == live.sum(1)).all()


def _planted():
    """Three table rows over 40 items: +0.5 and -0.5 on item 9 cancel; junk ids and sims contribute nothing."""
    ti = np.full((4, 4), -1, np.int32)
    ts = np.full((4, 4), -np.inf, np.float32)
    ti[0], ts[0] = [9, 3, 40, -5], [0.5, 0.25, 1.0, 1.0]                   # ids 40 and -5 are outside [0, 40)
    ti[1], ts[1] = [9, 4, 5, 6], [-0.5, np.nan, np.inf, -np.inf]            # non-finite sims
    ti[2], ts[2] = [7, 8, 3, 2], [8.0, 4.0 + 2.0 ** -29, 0.25, 2.0 ** 33]   # 8 * 2^30 > 2^32; 4 + 2^-29 is not (float32: 4.0); 2^33
    ti[3], ts[3] = [1, 1, 1, 1], [1.0, 1.0, 1.0, 1.0]
    return ti, ts


def test_a_sum_that_cancels_to_zero_is_still_listed():
    ti, ts = _planted()
    hist = C.csr([[0, 1]])
    items, scores, n_elig = C.host_knn(ti, ts, 40, hist, 4, frac_bits=30)
    assert items[0].tolist() == [3, 9, -1, -1] and scores[0, :2].tolist() == [0.25, 0.0] and n_elig[0] == 2
    assert scores[0, 1].tobytes() == np.float32(0.0).tobytes()             # +0, from the integer 0


def test_out_of_range_members_ids_and_bad_sims_contribute_nothing():
    ti, ts = _planted()
    hist = C.csr([[0, 1, 2, -1, 4, 2 ** 31 - 1], [2], []])
    items, scores, n_elig = C.host_knn(ti, ts, 40, hist, 8, frac_bits=30)
    want = C.ref_knn(ti, ts, 40, [[0, 1, 2, -1, 4, 2 ** 31 - 1], [2], []], None, 8, 30)
    for g, w in zip((items, scores, n_elig), want):
        C.same_bytes(g, w)
    # row 1: 8.0 * 2^30 = 2^33 is out of range, 4.0 * 2^30 = 2^32 is the last value in range, 2^33 is out
    assert items[1].tolist()[:3] == [8, 3, -1] and scores[1, 0] == 4.0 and n_elig[1] == 2
    assert items[0].tolist()[:4] == [8, 3, 9, -1] and scores[0, 1] == 0.5
    # the same table at F = 0: everything finite is in range; rint(0.5) = 0, rint(0.25) = 0: still candidates, score 0
    items, scores, n_elig = C.host_knn(ti, ts, 40, hist, 8, frac_bits=0)
    want = C.ref_knn(ti, ts, 40, [[0, 1, 2, -1, 4, 2 ** 31 - 1], [2], []], None, 8, 0)
    for g, w in zip((items, scores, n_elig), want):
        C.same_bytes(g, w)
    assert items[1].tolist()[:4] == [7, 8, 3, -1] and n_elig[1] == 3       # 2^33 * 2^0 > 2^32 is still out of range


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = C.case()
    p = C._p
    (i_off, i_users), (u_off, u_items) = c["by_item_csr"], c["by_user_csr"]
    i_users, u_items = C._tail(i_users), C._tail(u_items)
    na = np.ones(C.I, np.float64)
    k = 8
    items, sims, ne = np.full((C.I, k), 77, np.int32), np.full((C.I, k), 7.0, np.float32), np.full(C.I, 77, np.int32)
    rows = np.arange(C.I, dtype=np.int64)

    def cooc(**kw):
        a = dict(i_off=p(i_off), i_users=p(i_users), u_off=p(u_off), u_items=p(u_items), n_user=C.U, n_item=C.I, rows=p(rows), n=C.I,
                 na=p(na), nb=p(na), shrink=0.0, min_co=1, allow=None, k=k, items=p(items), sims=p(sims), ne=p(ne))
        a.update(kw)
        return lib.sml_host_cooc_topk(a["i_off"], a["i_users"], a["u_off"], a["u_items"], a["n_user"], a["n_item"], a["rows"], a["n"],
                                      a["na"], a["nb"], a["shrink"], a["min_co"], a["allow"], a["k"], a["items"], a["sims"], a["ne"])

    for kw in (dict(k=0), dict(k=129), dict(min_co=0), dict(shrink=-1.0), dict(shrink=float("nan")), dict(i_off=None), dict(i_users=None),
               dict(u_off=None), dict(u_items=None), dict(na=None), dict(nb=None), dict(n_item=0), dict(n_item=2 ** 31), dict(n_user=0),
               dict(n_user=2 ** 31), dict(n=-1), dict(items=None), dict(sims=None), dict(items=p(i_off)), dict(sims=p(u_items)),
               dict(ne=p(rows)), dict(sims=p(items)), dict(ne=p(items)), dict(items=p(na)), dict(u_off=None, u_items=None)):
        assert cooc(**kw) != 0 and lib.sml_last_error(), kw
    assert (items == 77).all() and (sims == 7.0).all() and (ne == 77).all()          # a refused call writes nothing
    assert cooc(n=0, items=None, sims=None) == 0                                     # n == 0 does nothing
    assert cooc(i_off=None, i_users=None) == 0 and (items == -1).all()               # no set at all: every row is empty
    assert cooc() == 0

    ti, ts = C.table("cosine")
    ti, ts = np.ascontiguousarray(ti), np.ascontiguousarray(ts)
    items[:], sims[:], ne[:] = 77, 7.0, 77
    users = np.arange(C.U, dtype=np.int64)

    def knn(**kw):
        a = dict(ti=p(ti), ts=p(ts), n_rows=C.I, k_nbr=C.K_NBR, n_item=C.I, h_off=p(u_off), h_items=p(u_items), users=p(users), n=C.U,
                 F=30, s_off=None, s_items=None, allow=None, k=k, items=p(items), scores=p(sims), ne=p(ne))
        a.update(kw)
        return lib.sml_host_knn_topk(a["ti"], a["ts"], a["n_rows"], a["k_nbr"], a["n_item"], a["h_off"], a["h_items"], a["users"], a["n"],
                                     a["F"], a["s_off"], a["s_items"], a["allow"], a["k"], a["items"], a["scores"], a["ne"])

    for kw in (dict(k=0), dict(k=129), dict(k_nbr=0), dict(k_nbr=129), dict(F=-1), dict(F=33), dict(h_off=None), dict(h_items=None),
               dict(s_off=p(u_off)), dict(s_items=p(u_items)), dict(n_item=0), dict(n_item=2 ** 31), dict(n=-1), dict(ti=None),
               dict(ts=None), dict(items=None), dict(scores=None), dict(items=p(ti)), dict(scores=p(ts)), dict(ne=p(users)),
               dict(scores=p(items)), dict(ne=p(items)), dict(items=p(u_items))):
        assert knn(**kw) != 0 and lib.sml_last_error(), kw
    assert (items == 77).all() and (sims == 7.0).all() and (ne == 77).all()
    assert knn(n=0, items=None, scores=None) == 0
    assert knn() == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,norm", (("cosine", "cosine"), ("count", None), ("asymmetric", "asymmetric")))
def test_item_neighbours_on_the_host_route(metric, norm):
    from sml_amd import knn
    from sml_amd.retrieval import ItemFilter, SeenItems
    c = C.case()
    pairs = np.array([(u, i) for u, s in enumerate(c["sets"]) for i in s], np.int64)
    seen = SeenItems(C.U, C.I).add(pairs)
    among = ItemFilter.from_mask(c["allow"])
    nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=C.K_NBR, metric=metric, alpha=C.ALPHA, shrink=10.0, min_co=2, among=among,
                                  engine="host")
    if metric == "asymmetric":                          # (the tables by torch's pow, as build makes them)
        deg = torch.tensor([len(s) for s in c["by_item"]], dtype=torch.float64)
        tables = (deg.pow(C.ALPHA).numpy(), deg.pow(1.0 - C.ALPHA).numpy())
    else:
        tables = C.norms(norm, c["by_item"])
    want = C.host_cooc(C.K_NBR, shrink=10.0, min_co=2, allow_words=c["allow_words"], norm_tables=tables)
    C.same_bytes(nb.items.numpy().astype(np.int32), want[0])
    C.same_bytes(nb.sims.numpy(), want[1])
    assert (nb.n_nbr.numpy() == np.minimum(want[2], C.K_NBR)).all()
    assert nb.metric == metric and nb.frac_bits == (0 if metric == "count" else 30) and nb.k == C.K_NBR and nb.n_item == C.I
    users = np.array([5, 1, 30, 0, 5], np.int64)
    it, sc = nb.recommend(seen, users=users, topK=20, exclude=seen, items=among)
    w = C.host_knn(want[0], want[1], C.I, c["by_user_csr"], 20, users=users, frac_bits=nb.frac_bits, seen_csr=c["by_user_csr"],
                   allow_words=c["allow_words"])
    C.same_bytes(it.numpy().astype(np.int32), w[0])
    C.same_bytes(sc.numpy(), w[1])
    it, sc = nb.recommend(c["by_user_csr"], topK=5)
    w = C.host_knn(want[0], want[1], C.I, c["by_user_csr"], 5, frac_bits=nb.frac_bits)
    C.same_bytes(it.numpy().astype(np.int32), w[0])
    si, ss = nb.similar_items([3, 299, 3], 7)
    C.same_bytes(si.numpy().astype(np.int32), want[0][[3, 299, 3], :7])
    C.same_bytes(ss.numpy(), want[1][[3, 299, 3], :7])
    with pytest.raises(ValueError):
        knn.ItemNeighbours.build(seen, C.U, C.I, metric="jaccard", engine="host")


def test_frac_bits_for():
    from sml_amd import knn
    for top, want in ((0.0, 32), (1.0, 32), (0.99, 32), (1.5, 31), (2.0, 31), (3.5, 30), (2.0 ** 31, 1), (2.0 ** 32, 0),
                      (2.0 ** 32 + 2.0 ** 20, 0), (2.0 ** -9, 32)):
        f = knn.frac_bits_for(top)
        assert f == want and (top * 2.0 ** f <= 2.0 ** 32 or f == 0) and (f == 32 or top * 2.0 ** (f + 1) > 2.0 ** 32), (top, f)


def test_recall_of_lists():
    from sml_amd import evaluation as E
    from sml_amd.retrieval import SeenItems
    held = SeenItems(5, 50).add(np.array([(0, 3), (0, 9), (2, 7), (4, 1), (4, 2), (4, 3), (4, 49)], np.int64))
    users = np.array([0, 1, 2, 4], np.int64)
    lists = np.array([[9, 5, 3, -1], [1, 2, 3, 4], [0, 1, 2, 3], [49, 7, 1, -1]], np.int64)
    got = E.recall_of_lists(lists, users, held, (1, 2, 4))
    # user 1 has no held-out item and does not count
    want = [np.mean([1 / 2, 0 / 1, 1 / 4]), np.mean([1 / 2, 0, 1 / 4]), np.mean([2 / 2, 0, 2 / 4])]
    assert got == [float(w) for w in want], (got, want)
    assert E.recall_of_lists(torch.from_numpy(lists), torch.from_numpy(users), held.host(), (4,)) == [got[2]]
    assert E.recall_of_lists(lists[:1], np.array([1]), held, (1,)) == [0.0]
    with pytest.raises(ValueError):
        E.recall_of_lists(lists, users, held, (5,))
