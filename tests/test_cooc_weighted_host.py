"""The weighted neighbours of items, the parts that need no GPU: the C ABI surface, sml_host_cooc_topk_weighted -- the definition
of sml_cooc_topk_weighted as a single-threaded walk over host memory -- against a numpy restatement of the header's text (byte
equality), the defining identities (a) .. (g) of the header, a dense float64 reference under the derived bound, every refusal of
the host entry point, ItemNeighbours' weighted forms on the host route and popularity_of_lists."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _cooc_weighted_cases as W
import _knn_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sml_cooc_weighted_scratch_bytes": 3, "sml_cooc_topk_weighted": 23, "sml_host_cooc_topk_weighted": 18}


def test_abi_surface():
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, n_args in NAMES.items():
        res_c = "int64_t " if name == "sml_cooc_weighted_scratch_bytes" else "int "
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
    for phrase in ("WEIGHTED NEIGHBOURS OF ITEMS", "q(u) = llrint(ldexp((double)user_w[u], F)), round to nearest even",
                   "a user that contributes nothing\n *     creates no candidate", "cw(j) = sum of q(u) over the contributing u in U(i)",
                   "num = ldexp((double)cw, -F)", "is exact below 2^53", "a NaN score is not eligible, an inf score is",
                   "(a) unit weights", "(b) dropped users", "(c) power-of-two scaling", "(d) symmetry", "(e) prefix", "(f) geometry",
                   "(g) filter", "user_w NULL; F outside [0, 32]; a misaligned scratch", "sums above 2^53"):
        assert phrase in header, phrase
    with open(os.path.join(REPO, "sml_amd", "csrc", "knn.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src
    assert "k_cooc_topk_weighted" in src and "fp contract(fast)" not in src and "fp contract(on)" not in src


def test_rows_fall_on_both_sides_of_the_limit_and_the_weights_are_planted():
    from sml_amd import _lib
    limit = _lib.load().sml_knn_lds_limit()
    c = C.case()
    below, above = C.sides([C.cooc_total(c, i) for i in range(C.I)], limit)
    assert len(below) >= 10 and len(above) >= 10, (limit, len(below), len(above))
    assert len(c["sets"][1]) == C.I - 1 and all(len(c["sets"][u]) > 0 for u in range(12, 22))
    for F in W.FS:
        w, q = W.weights(F), W.quant(W.weights(F), F)
        assert all(q[u] is None for u in W.DROPPED_ALWAYS) and q[17] == 2 ** 32 and q[20] == 2 and q[21] == 2, (F, q)
        assert w[1] == 0.125 and q[1] == (None if F == 0 else 2 ** (F - 3))
        assert w[16] * 2.0 ** F == 2.0 ** 33 and w[18] * 2.0 ** F == 0.25 and w[19] * 2.0 ** F == 0.5
    assert W.weights(0)[16] == 2.0 ** 33 and W.weights(0)[17] == 2.0 ** 32 and W.weights(30)[18] == 2.0 ** -32


# ---- the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", W.FS)
@pytest.mark.parametrize("shrink", (0.0, 10.0))
@pytest.mark.parametrize("norm", W.NORMS)
def test_host_walk_equals_the_restatement(norm, shrink, F):
    c = C.case()
    w, cw, tables = W.weights(F), W.planted_counts(F), W.norms(norm, c["by_item"])
    want = W.ref_rows(cw, F, 128, norm_tables=tables, shrink=shrink)
    for k in W.KS:
        got = W.host(k, w, F, norm=norm, shrink=shrink)
        for g, x, what in zip(got, (want[0][:, :k], want[1][:, :k], want[2]), ("items", "sims", "n_elig")):
            W.same_bytes(g, x, (what, norm, shrink, F, k))                     # (e): a k'-call is the prefix of a k-call
    got = W.host(64, w, F, norm=norm, shrink=shrink, allow_words=c["allow_words"])
    want = W.ref_rows(cw, F, 64, norm_tables=tables, shrink=shrink, allow=c["allow"])
    for g, x in zip(got, want):
        W.same_bytes(g, x, ("filtered", norm, shrink, F))
    assert (got[0][C.I - 1] == -1).all() and np.isneginf(got[1][C.I - 1]).all() and got[2][C.I - 1] == 0      # the item with no user
    assert want[2].max() > 0


@pytest.mark.parametrize("norm", (None, "cosine", "asymmetric"))
def test_a_unit_weights_return_the_unweighted_bytes(norm):
    c = C.case()
    tables = C.norms(norm, c["by_item"])
    ones = np.ones(C.U, np.float32)
    for shrink in (0.0, 10.0):
        for k in (5, 128):
            got = W.host(k, ones, 0, norm_tables=tables, shrink=shrink)
            want = C.host_cooc(k, norm=norm, shrink=shrink, min_co=1)
            for g, x in zip(got, want):
                W.same_bytes(g, x, ("unit", norm, shrink, k))
    got = W.host(64, ones, 0, norm_tables=tables, allow_words=c["allow_words"])
    want = C.host_cooc(64, norm=norm, allow_words=c["allow_words"])
    for g, x in zip(got, want):
        W.same_bytes(g, x, ("unit, filtered", norm))


@pytest.mark.parametrize("F", W.FS)
def test_b_a_dropped_user_is_a_user_removed_from_both_csrs(F):
    c = C.case()
    w = W.weights(F)
    q = W.quant(w, F)
    dropped = [u for u in range(C.U) if q[u] is None]
    assert set(W.DROPPED_ALWAYS) <= set(dropped) and (1 in dropped) == (F == 0)
    sets = [np.zeros(0, np.int64) if u in dropped else s for u, s in enumerate(c["sets"])]
    w2 = w.copy()
    w2[dropped] = 1.0                                    # (a weight that would contribute: the user has nothing left to add)
    tables = W.norms("rp3", c["by_item"])                # the tables stay those of the whole set: only the walk loses the users
    for norm_tables in ((None, None), tables):
        got = W.host(64, w, F, norm_tables=norm_tables)
        want = W.host(64, w2, F, norm_tables=norm_tables, sets=sets)
        for g, x in zip(got, want):
            W.same_bytes(g, x, ("dropped", F))


@pytest.mark.parametrize("F", (30, 32, 1))
def test_c_doubling_the_weights_and_lowering_f_by_one(F):
    """q(2w, F - 1) = q(w, F) for every user, so the sums, the items and n_elig are the same bytes; num = ldexp(cw, -F) carries the
    scale, so every sim is exactly doubled (no sim of the case is near the overflow or the subnormal range): the same bytes once
    halved."""
    w = W.weights(F)
    with np.errstate(over="ignore", invalid="ignore"):
        w2 = (w * np.float32(2.0)).astype(np.float32)
    assert W.quant(w2, F - 1) == W.quant(w, F)
    for norm in (None, "rp3"):
        a = W.host(64, w, F, norm=norm, shrink=10.0)
        b = W.host(64, w2, F - 1, norm=norm, shrink=10.0)
        W.same_bytes(a[0], b[0], ("items", F, norm))
        W.same_bytes(a[2], b[2], ("n_elig", F, norm))
        W.same_bytes(a[1], b[1] * np.float32(0.5), ("sims", F, norm))
        live = a[0] >= 0
        assert live.any() and (np.abs(b[1][live]) < 2.0 ** 100).all() and (np.abs(a[1][live]) > 2.0 ** -100).all()


@pytest.mark.parametrize("F,shrink", ((30, 0.0), (30, 10.0), (32, 0.0)))
def test_d_equal_norm_tables_make_the_similarity_symmetric_in_bits(F, shrink):
    among = np.zeros(C.I, bool)
    among[100:200] = True                                # (a filter of 100 items: the whole filtered row fits a list of 128)
    items, sims, n_elig = W.host(128, W.weights(F), F, norm="cosine", shrink=shrink, rows=np.arange(100, 200), allow_words=C.words(among))
    assert (n_elig == 99).all()                          # the heavy user contributes at F >= 3 and makes every pair co-occur
    sim = {}
    for x, i in enumerate(range(100, 200)):
        for j, s in zip(items[x, :99].tolist(), sims[x, :99]):
            sim[(i, j)] = s.tobytes()
    assert len(sim) == 9900 and all(sim[(i, j)] == sim[(j, i)] for i, j in sim)


def test_g_a_filtered_row_is_the_unfiltered_row_without_the_disallowed():
    c = C.case()
    checked = 0
    for F, heavy in ((0, True), (30, True), (30, False), (32, False)):
        w = W.weights(F)
        if not heavy:
            w[1] = 0.0                                   # without the user who holds everything, whole rows fit a list of 128
        full = W.host(128, w, F, norm="rp3")
        filt = W.host(128, w, F, norm="rp3", allow_words=c["allow_words"])
        for i in range(C.I):
            if full[2][i] > 128:                         # (the unfiltered row does not fit a list: nothing to compare it with)
                continue
            keep = [q for q in range(full[2][i]) if c["allow"][full[0][i, q]]]
            assert filt[2][i] == len(keep)
            assert filt[0][i, :len(keep)].tobytes() == full[0][i, keep].tobytes() and (filt[0][i, len(keep):] == -1).all()
            assert filt[1][i, :len(keep)].tobytes() == full[1][i, keep].tobytes() and np.isneginf(filt[1][i, len(keep):]).all()
            checked += full[2][i] > 0
    assert checked >= 100, checked                       # (a guard on the case, not on the walk: enough rows fit to be compared)


def test_rows_permuted_with_a_repeat():
    w = W.weights(30)
    full = W.host(64, w, 30, norm="rp3")
    rows = np.array([17, 3, 0, 299, 3, 250, 17, 1], np.int64)
    got = W.host(64, w, 30, rows=rows, norm="rp3")
    for g, f in zip(got, full):
        W.same_bytes(g, f[rows])
    got = W.host(64, w, 30, rows=np.zeros(0, np.int64))
    assert got[0].shape == (0, 64)


def test_nan_is_not_eligible_and_inf_is():
    c = C.case()
    a = np.sqrt(np.array([len(s) for s in c["by_item"]], np.float64))
    b = a.copy()
    b[5], b[7] = np.nan, 0.0
    w = W.weights(30)
    items, sims, n_elig = W.host(128, w, 30, rows=np.array([200], np.int64), norm_tables=(a, b))
    plain = W.host(128, w, 30, rows=np.array([200], np.int64), norm="cosine")
    cw = W.planted_counts(30)[200]
    assert cw[5] > 0 and cw[7] > 0
    assert 5 not in items[0] and items[0, 0] == 7 and np.isposinf(sims[0, 0]) and n_elig[0] == plain[2][0] - 1


# ---- against real arithmetic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", W.FS)
def test_against_a_dense_float64_reference_under_the_derived_bound(F):
    """R = X^T diag(w) X / (deg^alpha (x) deg^beta) in float64, w the weights that contribute by the definition's rules that are
    not roundings (finite, positive, at most 2^32 in fixed point), 0 otherwise.  The bound on |sim - R[i, j]|, derived and not
    fitted: each of the L users of row i is quantised with an error of at most 2^-(F+1) (a user rounded to 0 included), so the
    numerator is off by at most L * 2^-(F+1); the walk's sum itself is exact (integers below 2^53), the denominator is the same
    float64 text in both, and what remains is one fp64 rounding (the division) and one fp32 rounding (the result); the reference's
    own sum of L float64 terms adds at most L * 2^-53 relative.  So
      eps(i, j) = L * 2^-(F+1) / den + |R| * (2^-24 + (L + 1) * 2^-53).
    Held: every listed sim is within eps of R; no unlisted candidate of R beats a listed one by more than the two eps; when the
    list is not full, every j whose R exceeds its eps is listed."""
    c = C.case()
    w = W.weights(F)
    wr = np.zeros(C.U, np.float64)
    for u in range(C.U):
        if np.isfinite(w[u]) and w[u] > 0 and np.rint(np.ldexp(np.float64(w[u]), F)) <= 2.0 ** 32:
            wr[u] = np.float64(w[u])
    x = np.zeros((C.U, C.I), np.float64)
    for u, s in enumerate(c["sets"]):
        x[u, s] = 1.0
    na, nb = W.norms("rp3", c["by_item"])
    k = 64
    items, sims, n_elig = W.host(k, w, F, norm="rp3")
    num = x.T @ (wr[:, None] * x)
    listed_rows = 0
    for i in range(C.I):
        L = len(c["by_item"][i])
        with np.errstate(all="ignore"):
            den = na[i] * nb
            r = np.where(den > 0, num[i] / den, 0.0)
            eps = np.where(den > 0, L * 2.0 ** -(F + 1) / den, 0.0) + np.abs(r) * (2.0 ** -24 + (L + 1) * 2.0 ** -53)
        live = int(min(n_elig[i], k))
        got = items[i, :live]
        assert (np.abs(sims[i, :live].astype(np.float64) - r[got]) <= eps[got]).all(), (F, i)
        rest = np.ones(C.I, bool)
        rest[got] = False
        rest[i] = False
        if live:
            listed_rows += 1
            worst = (r[got] + eps[got]).min()
            assert ((r - eps)[rest] <= worst).all(), (F, i)
        if live < k:
            assert ((r - eps)[rest] <= 0).all(), (F, i)
    # (a guard on the case: with the heavy user contributing every item with a user has a list; at F = 0 user 17's items at least)
    assert listed_rows == C.I - 1 if F else listed_rows >= len(c["sets"][17]) >= 6, listed_rows


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = C.case()
    p = C._p
    (i_off, i_users), (u_off, u_items) = c["by_item_csr"], c["by_user_csr"]
    i_users, u_items = C._tail(i_users), C._tail(u_items)
    na = np.ones(C.I, np.float64)
    w = np.ascontiguousarray(W.weights(30))
    k = 8
    items, sims, ne = np.full((C.I, k), 77, np.int32), np.full((C.I, k), 7.0, np.float32), np.full(C.I, 77, np.int32)
    rows = np.arange(C.I, dtype=np.int64)

    def call(**kw):
        a = dict(i_off=p(i_off), i_users=p(i_users), u_off=p(u_off), u_items=p(u_items), n_user=C.U, n_item=C.I, rows=p(rows), n=C.I,
                 w=p(w), F=30, na=p(na), nb=p(na), shrink=0.0, allow=None, k=k, items=p(items), sims=p(sims), ne=p(ne))
        a.update(kw)
        return lib.sml_host_cooc_topk_weighted(a["i_off"], a["i_users"], a["u_off"], a["u_items"], a["n_user"], a["n_item"], a["rows"],
                                               a["n"], a["w"], a["F"], a["na"], a["nb"], a["shrink"], a["allow"], a["k"], a["items"],
                                               a["sims"], a["ne"])

    for kw in (dict(k=0), dict(k=129), dict(shrink=-1.0), dict(shrink=float("nan")), dict(i_off=None), dict(i_users=None),
               dict(u_off=None), dict(u_items=None), dict(na=None), dict(nb=None), dict(n_item=0), dict(n_item=2 ** 31), dict(n_user=0),
               dict(n_user=2 ** 31), dict(n=-1), dict(items=None), dict(sims=None), dict(items=p(i_off)), dict(sims=p(u_items)),
               dict(ne=p(rows)), dict(sims=p(items)), dict(ne=p(items)), dict(items=p(na)), dict(u_off=None, u_items=None),
               dict(w=None), dict(F=-1), dict(F=33), dict(items=p(w)), dict(sims=p(w)), dict(ne=p(w))):
        assert call(**kw) != 0 and lib.sml_last_error(), kw
    assert (items == 77).all() and (sims == 7.0).all() and (ne == 77).all()          # a refused call writes nothing
    assert np.array_equal(w, W.weights(30), equal_nan=True)
    assert call(n=0, items=None, sims=None) == 0                                     # n == 0 does nothing
    assert (items == 77).all()
    assert call(i_off=None, i_users=None) == 0 and (items == -1).all()               # no set at all: every row is empty
    assert call(F=0) == 0 and call(F=32) == 0 and call() == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def _seen():
    from sml_amd.retrieval import SeenItems
    pairs = np.array([(u, i) for u, s in enumerate(C.case()["sets"]) for i in s], np.int64)
    return SeenItems(C.U, C.I).add(pairs)


def _build_tables(metric, alpha, beta):
    """(user_w float32, norm tables) as ItemNeighbours.build makes them: float64 torch, the weights cast to float32."""
    c = C.case()
    deg_i = torch.tensor([len(s) for s in c["by_item"]], dtype=torch.float64)
    deg_u = torch.tensor([len(s) for s in c["sets"]], dtype=torch.float64)
    w = torch.where(deg_u > 0, deg_u.clamp(min=1.0).pow(-alpha), torch.zeros_like(deg_u)).to(torch.float32).numpy()
    return w, (deg_i.pow(alpha).numpy(), deg_i.pow(0.0 if metric == "p3alpha" else beta).numpy())


@pytest.mark.parametrize("metric,alpha,beta", (("rp3beta", 1.0, 0.6), ("rp3beta", 0.8, 0.3), ("p3alpha", 1.0, 0.6)))
def test_item_neighbours_random_walk_metrics_on_the_host_route(metric, alpha, beta):
    from sml_amd import knn
    from sml_amd.retrieval import ItemFilter
    c = C.case()
    seen = _seen()
    among = ItemFilter.from_mask(c["allow"])
    kw = {} if (alpha, beta) == (1.0, 0.6) else dict(alpha=alpha, beta=beta)          # (the defaults are the literature's 1 and 0.6)
    nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=C.K_NBR, metric=metric, shrink=0.5, among=among, engine="host", **kw)
    w, tables = _build_tables(metric, alpha, beta)
    assert w[0] == 0.0 and w[1] == np.float32(299.0 ** -alpha) and w.max() == 1.0
    F = knn.frac_bits_for(float(w.max()))
    assert F == 32                                       # the largest weight is 1
    want = W.host(C.K_NBR, w, F, shrink=0.5, allow_words=c["allow_words"], norm_tables=tables)
    C.same_bytes(nb.items.numpy().astype(np.int32), want[0])
    C.same_bytes(nb.sims.numpy(), want[1])
    assert (nb.n_nbr.numpy() == np.minimum(want[2], C.K_NBR)).all()
    top = float(np.abs(want[1][want[0] >= 0]).max())
    assert nb.metric == metric and nb.frac_bits == knn.frac_bits_for(top) and nb.k == C.K_NBR
    users = np.array([5, 1, 30, 0, 5], np.int64)
    it, sc = nb.recommend(seen, users=users, topK=20, exclude=seen, items=among)
    r = C.ref_knn(want[0], want[1], C.I, c["sets"], users, 20, nb.frac_bits, seen=c["sets"], allow=c["allow"])
    C.same_bytes(it.numpy().astype(np.int32), r[0])
    C.same_bytes(sc.numpy(), r[1])
    si, ss = nb.similar_items([3, 299, 3], 7)
    C.same_bytes(si.numpy().astype(np.int32), want[0][[3, 299, 3], :7])
    C.same_bytes(ss.numpy(), want[1][[3, 299, 3], :7])


def test_p3alpha_is_rp3beta_with_beta_zero():
    from sml_amd import knn
    seen = _seen()
    a = knn.ItemNeighbours.build(seen, C.U, C.I, k=32, metric="p3alpha", engine="host")
    b = knn.ItemNeighbours.build(seen, C.U, C.I, k=32, metric="rp3beta", beta=0.0, engine="host")
    C.same_bytes(a.items.numpy(), b.items.numpy())
    C.same_bytes(a.sims.numpy(), b.sims.numpy())
    C.same_bytes(a.n_nbr.numpy(), b.n_nbr.numpy())
    assert a.frac_bits == b.frac_bits
    c = knn.ItemNeighbours.build(seen, C.U, C.I, k=32, metric="rp3beta", engine="host")
    assert not torch.equal(c.sims, b.sims)                                           # beta does something


@pytest.mark.parametrize("metric,norm", (("cosine", "cosine"), ("count", None), ("asymmetric", "asymmetric")))
def test_item_neighbours_with_a_user_weight_on_the_host_route(metric, norm):
    """user_weight= on the three plain metrics: here inverse user frequency, log(I / deg_u), with junk planted."""
    from sml_amd import knn
    c = C.case()
    seen = _seen()
    deg_u = np.array([len(s) for s in c["sets"]], np.float64)
    with np.errstate(divide="ignore"):
        iuf = np.log(C.I / deg_u)                        # user 0: +inf, contributes nothing (and has no item anyway)
    iuf[14], iuf[15] = np.nan, -2.0
    uw = torch.from_numpy(iuf)                           # float64 is accepted and cast
    nb = knn.ItemNeighbours.build(seen, C.U, C.I, k=C.K_NBR, metric=metric, alpha=C.ALPHA, shrink=2.0, user_weight=uw, engine="host")
    w = iuf.astype(np.float32)
    F = knn.frac_bits_for(float(np.abs(w[np.isfinite(w)]).max()))
    assert 0 < F < 32
    if metric == "asymmetric":
        deg = torch.tensor([len(s) for s in c["by_item"]], dtype=torch.float64)
        tables = (deg.pow(C.ALPHA).numpy(), deg.pow(1.0 - C.ALPHA).numpy())
    else:
        tables = C.norms(norm, c["by_item"])
    want = W.host(C.K_NBR, w, F, shrink=2.0, norm_tables=tables)
    C.same_bytes(nb.items.numpy().astype(np.int32), want[0])
    C.same_bytes(nb.sims.numpy(), want[1])
    top = float(np.abs(want[1][want[0] >= 0]).max())
    assert nb.frac_bits == knn.frac_bits_for(top) and nb.metric == metric
    it, sc = nb.recommend(seen, users=np.array([7, 40], np.int64), topK=10, exclude=seen)
    r = C.ref_knn(want[0], want[1], C.I, c["sets"], [7, 40], 10, nb.frac_bits, seen=c["sets"])
    C.same_bytes(it.numpy().astype(np.int32), r[0])
    C.same_bytes(sc.numpy(), r[1])


def test_value_errors():
    from sml_amd import knn
    seen = _seen()
    c = C.case()
    uw = torch.ones(C.U)
    for kw in (dict(metric="jaccard"), dict(metric="rp3beta", min_co=2), dict(metric="p3alpha", min_co=0),
               dict(metric="cosine", user_weight=uw, min_co=2), dict(metric="rp3beta", user_weight=uw),
               dict(metric="count", user_weight=torch.ones(C.U - 1)), dict(metric="count", user_weight=torch.ones(C.U, dtype=torch.int64))):
        with pytest.raises(ValueError):
            knn.ItemNeighbours.build(seen, C.U, C.I, engine="host", **kw)
    h = knn.HostWalks()
    by_user = tuple(torch.from_numpy(t) for t in c["by_user_csr"])
    by_item = tuple(torch.from_numpy(t) for t in c["by_item_csr"])
    for bad in (torch.ones(C.U, dtype=torch.float64), torch.ones(C.U + 1), torch.ones(2 * C.U)[::2], np.ones(C.U, np.float32), None):
        with pytest.raises(ValueError):
            h.cooc_topk_weighted(by_item, by_user, 8, bad)
    got = h.cooc_topk_weighted(by_item, by_user, 8, torch.ones(C.U), frac_bits=0)
    want = h.cooc_topk(by_item, by_user, 8)
    assert all(torch.equal(g, x) for g, x in zip(got, want))
    with pytest.raises(RuntimeError):
        h.cooc_topk_weighted(by_item, by_user, 8, torch.ones(C.U), frac_bits=33)


def test_popularity_of_lists():
    from sml_amd import evaluation as E
    count = np.array([10, 0, 4, 1, 7, 100], np.int64)
    lists = np.array([[0, 2, -1], [5, 0, 4], [-1, -1, -1]], np.int64)
    got = E.popularity_of_lists(lists, count)
    assert got == {"mean_count": (10 + 4 + 100 + 10 + 7) / 5.0, "coverage": 4 / 6.0}
    assert E.popularity_of_lists(torch.from_numpy(lists), torch.from_numpy(count)) == got
    assert E.popularity_of_lists(np.full((2, 3), -1, np.int64), count) == {"mean_count": 0.0, "coverage": 0.0}
    with pytest.raises(ValueError):
        E.popularity_of_lists(np.array([[6]], np.int64), count)
    with pytest.raises(ValueError):
        E.popularity_of_lists(np.array([1, 2], np.int64), count)
