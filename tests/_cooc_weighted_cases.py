"""Seeded cases of the weighted neighbours of items (sml_cooc_topk_weighted, include/sml_hip.h "WEIGHTED NEIGHBOURS OF ITEMS"),
shared by test_cooc_weighted_host.py and test_cooc_weighted_gpu.py, with a plain numpy restatement of the header's text to compare
the host walk against.  Every comparison of items, sims and counts made on them is byte equality.

The sets are those of _knn_cases.case(): U = 48 users over I = 300 items, rows on both sides of the on-chip limit.  weights(F) is
the planted weight vector for F fractional bits (user ids 0-based, as _knn_cases numbers them):
  most users       deg_u^-1 as float32 (user 0, who has no item, gets 0)
  user 1           2^-3: the user who holds 299 items (at F = 0 it rounds to 0 and the user is dropped)
  users 12 .. 15   +0.0, -1.0, NaN, +inf: all four contribute nothing
  user 16          2^33 * 2^-F: 2^33 in fixed point, out of range, dropped (F = 0: the weight 2^33 itself)
  user 17          2^32 * 2^-F: exactly 2^32 in fixed point, the last value in range, kept
  user 18          2^-2 * 2^-F: rounds to 0, dropped (F = 30: the weight 2^-32)
  users 19, 20, 21 0.5, 1.5, 2.5 times 2^-F: ties to even give q = 0 (dropped), 2 and 2
All planted values are powers of two times small integers, exact in float32 for every F in FS.

The restatement: the call as loops over dense arrays with Python-int sums; the quantisation is np.rint(np.ldexp(.)) on float64
and the floats go through the named numpy float64 / float32 operations (an elementwise numpy operation rounds once, to nearest
even; a Python int converts to float64 correctly rounded, to nearest even)."""
import functools

import numpy as np

import _knn_cases as C

U, I = C.U, C.I
FS = (0, 30, 32)
KS = C.KS
NORMS = (None, "cosine", "rp3")
ALPHA, BETA = 1.0, 0.6
JUNK = (12, 13, 14, 15)
DROPPED_ALWAYS = JUNK + (16, 18, 19)                   # at every F; F = 0 drops more (every deg^-1 below or at 1/2, and user 1)


def weights(F):
    c = C.case()
    deg = np.array([len(s) for s in c["sets"]], np.float64)
    with np.errstate(divide="ignore"):
        w = np.where(deg > 0, 1.0 / deg, 0.0).astype(np.float32)
    w[1] = 2.0 ** -3
    w[12], w[13], w[14], w[15] = 0.0, -1.0, np.nan, np.inf
    s = 2.0 ** -F
    w[16], w[17], w[18] = 2.0 ** 33 * s, 2.0 ** 32 * s, 2.0 ** -2 * s
    w[19], w[20], w[21] = 0.5 * s, 1.5 * s, 2.5 * s
    return w


def quant(w, F):
    """q(u) as Python ints, None where the user contributes nothing."""
    out = []
    for x in np.asarray(w, np.float32):
        q = None
        if np.isfinite(x):
            r = np.rint(np.ldexp(np.float64(x), F))                        # to nearest even
            if abs(r) <= 2.0 ** 32 and r > 0:
                q = int(r)
        out.append(q)
    return out


def norms(kind, by_item):
    """(norm_a, norm_b) float64 [I]: None, the cosine table, or the random walk's (deg^ALPHA, deg^BETA)."""
    if kind == "rp3":
        deg = np.array([len(s) for s in by_item], np.float64)
        return np.power(deg, ALPHA), np.power(deg, BETA)
    return C.norms(kind, by_item)


def weighted_counts(w, F, sets=None):
    """cw[i][j] = sum of q(u) over the contributing u in U(i) with j in S(u), as Python ints, by the loops of the definition."""
    sets = C.case()["sets"] if sets is None else sets
    by_item = C.transpose(sets, I)
    q = quant(w, F)
    out = []
    for i in range(I):
        row = [0] * I
        for u in by_item[i]:
            if q[int(u)] is None:
                continue
            for j in sets[int(u)]:
                row[int(j)] += q[int(u)]
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def planted_counts(F):
    return weighted_counts(weights(F), F)


def ref_rows(cw, F, k, rows=None, norm_tables=(None, None), shrink=0.0, allow=None):
    """The restatement from the integer sums on: (items int32 [n, k], sims float32 [n, k], n_elig int32 [n])."""
    na, nb = norm_tables
    rows = range(I) if rows is None else rows
    items, sims, n_elig = [], [], []
    for i in rows:
        i = int(i)
        num = np.ldexp(np.array([float(c) for c in cw[i]], np.float64), -F)      # int -> float64 to nearest even; the scaling is exact
        if na is None:
            s = num.astype(np.float32)
        else:
            with np.errstate(all="ignore"):
                den = na[i] * nb                                       # one fp64 rounding
                den = den + np.float64(shrink)
                s64 = num / den                                        # the correctly rounded fp64 division
                s = s64.astype(np.float32)
        pairs = [(s[j], j) for j in range(I) if j != i and cw[i][j] > 0 and (allow is None or allow[j]) and not np.isnan(s[j])]
        it, sc = C._ranked(pairs, k)
        items.append(it)
        sims.append(sc)
        n_elig.append(len(pairs))
    return np.array(items, np.int32).reshape(-1, k), np.array(sims, np.float32).reshape(-1, k), np.array(n_elig, np.int32)


def host(k, w, F, rows=None, norm=None, shrink=0.0, allow_words=None, norm_tables=None, sets=None):
    """(items int32 [n, k], sims float32 [n, k], n_elig int32 [n]) of sml_host_cooc_topk_weighted on the case (or on `sets`)."""
    from sml_amd import _lib
    c = C.case()
    sets = c["sets"] if sets is None else sets
    by_item = C.transpose(sets, I)
    (i_off, i_users), (u_off, u_items) = C.csr(by_item), C.csr(sets)
    i_users, u_items = C._tail(i_users), C._tail(u_items)
    na, nb = norm_tables if norm_tables is not None else norms(norm, by_item)
    na, nb = C._arr(na, np.float64), C._arr(nb, np.float64)
    rows = C._arr(rows, np.int64)
    n = I if rows is None else len(rows)
    aw = C._arr(allow_words, np.uint32)
    w = C._arr(w, np.float32)
    items, sims, n_elig = np.full((n, k), 77, np.int32), np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32)
    p = C._p
    _lib.check(_lib.load().sml_host_cooc_topk_weighted(p(i_off), p(i_users), p(u_off), p(u_items), U, I, p(rows), n, p(w), int(F), p(na),
                                                       p(nb), float(shrink), p(aw), k, p(items), p(sims), p(n_elig)),
               "sml_host_cooc_topk_weighted")
    return items, sims, n_elig


same_bytes = C.same_bytes
