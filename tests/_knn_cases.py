"""Seeded cases of the neighbourhood model (sml_cooc_topk / sml_knn_topk, include/sml_hip.h "NEIGHBOURS"), shared by
test_knn_host.py and test_knn_gpu.py, with a plain numpy restatement of the header's text to compare the host walks against.
Every comparison of items, similarities, scores and counts made on them is byte equality.

U = 48 users over I = 300 items.  User 0 has no item; user 1 holds every item that has a user at all (299 of them: item 299 has
none), so every row it is in is heavy; users 2 .. 11 have one to five items; the other 36 have 6 .. 40 items drawn with a skew
towards the low ids, so that the popular items' rows are long and the rare items' rows short.  Counts are small integers, so ties
are everywhere and the id order decides them.  The rows fall on both sides of the library's on-chip limit (sml_knn_lds_limit, read
from the library): `sides` says which, and the tests assert that both sides are populated.

The restatement: both calls as loops over dense arrays with Python-int sums; the floats go through the named numpy float64 /
float32 operations (an elementwise numpy operation rounds once, to nearest even)."""
import functools

import numpy as np

U, I = 48, 300
K_NBR = 64
KS = (1, 5, 64, 128)
NORMS = (None, "cosine", "asymmetric")
ALPHA = 0.3


def csr(sets):
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=off[1:])
    items = np.concatenate([np.asarray(s, np.int64) for s in sets] + [np.zeros(0, np.int64)]).astype(np.int32)
    return off, items


def transpose(sets, n_other):
    out = [[] for _ in range(n_other)]
    for u, s in enumerate(sets):
        for i in s:
            out[int(i)].append(u)
    return [np.asarray(s, np.int64) for s in out]


def words(mask):
    """bool [n_item] -> the filter words uint32 [ceil(n_item / 32)]."""
    b = np.packbits(np.asarray(mask, bool), bitorder="little")
    return np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)]).view("<u4").astype(np.uint32)


def norms(kind, by_item):
    """(norm_a, norm_b) float64 [I] of a metric, or (None, None): made in numpy float64 from the degrees."""
    if kind is None:
        return None, None
    deg = np.array([len(s) for s in by_item], np.float64)
    if kind == "cosine":
        a = np.sqrt(deg)
        return a, a
    return np.power(deg, ALPHA), np.power(deg, 1.0 - ALPHA)


@functools.lru_cache(maxsize=None)
def case():
    rng = np.random.RandomState(2300)
    p = 1.0 / (1.0 + np.arange(I - 1)) ** 0.8
    p /= p.sum()
    sizes = [0, I - 1] + [1 + q % 5 for q in range(10)] + [6 + (5 * q + 1) % 35 for q in range(36)]
    assert len(sizes) == U
    sets = [np.zeros(0, np.int64), np.arange(I - 1, dtype=np.int64)]
    for s in sizes[2:]:
        sets.append(np.sort(rng.choice(I - 1, size=s, replace=False, p=p)).astype(np.int64))
    by_item = transpose(sets, I)
    assert len(by_item[I - 1]) == 0
    allow = rng.rand(I) < 0.6
    seen = [np.sort(rng.choice(I, size=int(s), replace=False)).astype(np.int64) for s in rng.randint(0, 30, size=U)]
    seen[3] = np.zeros(0, np.int64)
    return dict(sets=sets, by_item=by_item, by_user_csr=csr(sets), by_item_csr=csr(by_item), allow=allow, allow_words=words(allow),
                seen=seen, seen_csr=csr(seen))


def cooc_total(c, i):
    """The total list length of row i of the co-occurrence call."""
    return sum(len(c["sets"][int(u)]) for u in c["by_item"][i])


def sides(totals, limit):
    below = [x for x, t in enumerate(totals) if 0 < t <= limit]
    above = [x for x, t in enumerate(totals) if t > limit]
    return below, above


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts():
    """c[i][j] = #{u in U(i) : j in S(u)} as Python ints, by the loops of the definition."""
    c = case()
    out = []
    for i in range(I):
        row = [0] * I
        for u in c["by_item"][i]:
            for j in c["sets"][int(u)]:
                row[int(j)] += 1
        out.append(row)
    return out


def _ranked(pairs, k):
    """(score float32, id) pairs -> (items int32 [k], scores float32 [k]) in the family's order, (-1, -inf) behind."""
    pairs = sorted(pairs, key=lambda p: (-float(p[0]), p[1]))
    items, scores = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float32)
    for q, (s, j) in enumerate(pairs[:k]):
        items[q], scores[q] = j, s
    return items, scores


def ref_cooc(rows, k, norm=None, shrink=0.0, min_co=1, allow=None):
    c = case()
    na, nb = norms(norm, c["by_item"])
    rows = range(I) if rows is None else rows
    items, sims, n_elig = [], [], []
    for i in rows:
        i = int(i)
        cnt = np.array(counts()[i], np.int64)
        if na is None:
            s = cnt.astype(np.float32)
        else:
            with np.errstate(all="ignore"):
                den = na[i] * nb                                   # one fp64 rounding
                den = den + np.float64(shrink)
                s64 = cnt.astype(np.float64) / den                 # the correctly rounded fp64 division
                s = s64.astype(np.float32)
        pairs = [(s[j], j) for j in range(I)
                 if j != i and cnt[j] >= min_co and (allow is None or allow[j]) and not np.isnan(s[j])]
        it, sc = _ranked(pairs, k)
        items.append(it)
        sims.append(sc)
        n_elig.append(len(pairs))
    return np.array(items, np.int32).reshape(-1, k), np.array(sims, np.float32).reshape(-1, k), np.array(n_elig, np.int32)


def ref_knn(nbr_items, nbr_sims, n_item, hist, users, k, frac_bits, seen=None, allow=None):
    users = range(len(hist)) if users is None else users
    items, scores, n_elig = [], [], []
    for u in users:
        u = int(u)
        acc, touched = [0] * n_item, [False] * n_item
        for m in hist[u]:
            m = int(m)
            if m < 0 or m >= nbr_items.shape[0]:
                continue
            for slot in range(nbr_items.shape[1]):
                j, sim = int(nbr_items[m, slot]), nbr_sims[m, slot]
                if j < 0 or j >= n_item or not np.isfinite(sim):
                    continue
                r = np.rint(np.ldexp(np.float64(sim), frac_bits))      # to nearest even
                if abs(r) > 2.0 ** 32:
                    continue
                acc[j] += int(r)
                touched[j] = True
        gone = set() if seen is None else set(int(x) for x in seen[u])
        pairs = [(np.float32(np.ldexp(np.float64(acc[j]), -frac_bits)), j) for j in range(n_item)
                 if touched[j] and j not in gone and (allow is None or allow[j])]
        it, sc = _ranked(pairs, k)
        items.append(it)
        scores.append(sc)
        n_elig.append(len(pairs))
    return np.array(items, np.int32).reshape(-1, k), np.array(scores, np.float32).reshape(-1, k), np.array(n_elig, np.int32)


# ---- the library's host walks --------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _tail(items):
    """A CSR's entries with one spare element behind them, so that an empty set still has an address."""
    return np.ascontiguousarray(np.concatenate([items, [0]]), np.int32)


def host_cooc(k, rows=None, norm=None, shrink=0.0, min_co=1, allow_words=None, norm_tables=None):
    """(items int32 [n, k], sims float32 [n, k], n_elig int32 [n]) of sml_host_cooc_topk on the case."""
    from sml_amd import _lib
    c = case()
    (i_off, i_users), (u_off, u_items) = c["by_item_csr"], c["by_user_csr"]
    i_users, u_items = _tail(i_users), _tail(u_items)
    na, nb = norm_tables if norm_tables is not None else norms(norm, c["by_item"])
    na, nb = _arr(na, np.float64), _arr(nb, np.float64)
    rows = _arr(rows, np.int64)
    n = I if rows is None else len(rows)
    aw = _arr(allow_words, np.uint32)
    items, sims, n_elig = np.full((n, k), 77, np.int32), np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32)
    _lib.check(_lib.load().sml_host_cooc_topk(_p(i_off), _p(i_users), _p(u_off), _p(u_items), U, I, _p(rows), n, _p(na), _p(nb),
                                              float(shrink), int(min_co), _p(aw), k, _p(items), _p(sims), _p(n_elig)),
               "sml_host_cooc_topk")
    return items, sims, n_elig


def host_knn(nbr_items, nbr_sims, n_item, hist_csr, k, users=None, frac_bits=30, seen_csr=None, allow_words=None):
    """(items int32 [n, k], scores float32 [n, k], n_elig int32 [n]) of sml_host_knn_topk."""
    from sml_amd import _lib
    nbr_items, nbr_sims = _arr(nbr_items, np.int32), _arr(nbr_sims, np.float32)
    h_off, h_items = _arr(hist_csr[0], np.int64), _tail(hist_csr[1])
    s_off, s_items = (None, None) if seen_csr is None else (_arr(seen_csr[0], np.int64), _tail(seen_csr[1]))
    users = _arr(users, np.int64)
    n = len(h_off) - 1 if users is None else len(users)
    aw = _arr(allow_words, np.uint32)
    items, scores, n_elig = np.full((n, k), 77, np.int32), np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32)
    _lib.check(_lib.load().sml_host_knn_topk(_p(nbr_items), _p(nbr_sims), nbr_items.shape[0], nbr_items.shape[1], n_item, _p(h_off),
                                             _p(h_items), _p(users), n, int(frac_bits), _p(s_off), _p(s_items), _p(aw), k, _p(items),
                                             _p(scores), _p(n_elig)), "sml_host_knn_topk")
    return items, scores, n_elig


@functools.lru_cache(maxsize=None)
def table(norm):
    """The neighbour table of the case under a metric, k_nbr = 64, by the host walk: (items int32 [I, 64], sims float32 [I, 64])."""
    items, sims, _ = host_cooc(K_NBR, norm=norm)
    return items, sims


def frac_bits(norm):
    return 0 if norm is None else 30


def same_bytes(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        diff = np.argwhere(a.view("u%d" % a.itemsize) != b.view("u%d" % b.itemsize))
        raise AssertionError("%s: %d entries differ, first at %s: %r vs %r" % (what, len(diff), tuple(diff[0]), a[tuple(diff[0])],
                                                                            b[tuple(diff[0])]))
