"""Seeded cases and exact references for the deep lists (sml_topk_deep / sml_host_topk_items, include/sml_hip.h "DEEP LISTS"),
shared by test_deep_topk_host.py and test_deep_topk_gpu.py.

The reference is tests/_fp32_chain.py's ref_topk, exact at any k; an item filter goes in as Seen' = Seen + complement
(_item_filter_cases.seen_prime) and per-item terms as one fma32 on the chain's value, the way the item-filter and item-score
suites put them.  A reference is computed once per (case, variant, users) at k = 1,024; the list at a smaller k is its prefix.
Every case has U = 300 users and I = 4,099 items (129 tiles, a last tile of 3 items) except `long` and `long_tie` (40 x 70,001)."""
import functools

import numpy as np

import _fp32_chain as F
from _half_cases import widen
from _item_filter_cases import pack, seen_prime

U, I = 300, 4099
KMAX = 1024
KS = (1, 128, 129, 500, 1024)
NS = (1, 33, 97, 257)
WIDTHS = (("fp32", 32), ("fp32", 64), ("fp16", 32), ("fp16", 64), ("fp16", 128))
VARIANTS = ("none", "filter", "terms", "both")
EXACT = ((1, 129), (2, 500), (3, 1024))          # (place among the case's users, number of eligible items left)


def _csr_lists(seen, n_user):
    off, items = seen
    return {u: items[off[u]:off[u + 1]].astype(np.int64) for u in range(n_user)}


def _finish(c, dtype, d, users, mask, scale, offset):
    np_t = np.float32 if dtype == "fp32" else np.float16
    c["wu"], c["wi"] = np.ascontiguousarray(c["wu"], dtype=np_t), np.ascontiguousarray(c["wi"], dtype=np_t)
    c.update(dtype=dtype, d=d, users=np.asarray(users, np.int64), mask=mask, scale=scale.astype(np.float32),
             offset=offset.astype(np.float32), ru=widen(c["wu"]) if dtype == "fp16" else c["wu"],
             ri=widen(c["wi"]) if dtype == "fp16" else c["wi"])
    return c


def _users257(c):
    """257 users: the case's 256 distinct ones and the first once more (a user may repeat)."""
    return np.concatenate([c["users"], c["users"][:1]])


def _random_terms(rng, n_item):
    return rng.uniform(0.25, 4.0, n_item).astype(np.float32), rng.randn(n_item).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, dtype, d):
    """The named case as a dict: wu / wi (the tables in their element type), ru / ri (the fp32 tables the references score),
    seen (CSR), users (257, or 40 for `long`), mask (the item filter, bool [I]), scale / offset (the terms)."""
    rng = np.random.RandomState(77)
    if name == "random":
        # users[0] keeps 50 eligible items (padding at every k above 50); users[1..3] keep exactly 129, 500 and 1,024
        c = F.random_case(d)
        users = _users257(c)
        lists = _csr_lists(c["seen"], U)
        for place, left in ((0, 50),) + EXACT:
            lists[int(users[place])] = rng.permutation(I)[left:]
        c["seen"] = F.seen_csr(U, I, lists)
        scale, offset = _random_terms(rng, I)
        return _finish(c, dtype, d, users, rng.rand(I) < 0.6, scale, offset)
    if name == "near_tie":
        # copies of the k-th item planted in other slices, near-ties, subnormal users (fp32 only: the scores are subnormal)
        assert dtype == "fp32"
        c = F.near_tie_case(d, ks=(129, 500, 1024))
        return _finish(c, dtype, d, _users257(c), rng.rand(I) < 0.8, np.ones(I), np.zeros(I))
    if name == "all_tie":
        # every score +0: the list is the first k eligible ids.  Terms: scale -1, offset -0 on every third item, whose scores
        # are then -0 -- they tie with +0 by id and keep their sign bit
        c = F.random_case(d)
        c["wu"][:], c["wi"][:] = 0.0, 0.0
        third = np.arange(I) % 3 == 0
        return _finish(c, dtype, d, _users257(c), np.arange(I) % 5 != 2, np.where(third, -1.0, 1.0), np.where(third, -0.0, 0.0))
    if name in ("sorted_desc", "sorted_asc"):
        # wi[i] = c_i e_0, wu[u] = e_0, c strictly monotonic in i (consecutive fp16 values, exact in both element types): every
        # top entry lies in slice 0 -- or in the last slice and the last, partial tile
        c = F.random_case(d)
        c["wu"][:], c["wi"][:] = 0.0, 0.0
        c["wu"][:, 0] = 1.0
        asc = (0x3000 + np.arange(I)).astype(np.uint16).view(np.float16).astype(np.float32)
        assert (np.diff(asc) > 0).all()
        c["wi"][:, 0] = asc if name == "sorted_asc" else asc[::-1]
        scale, offset = _random_terms(rng, I)
        return _finish(c, dtype, d, _users257(c), rng.rand(I) < 0.6, scale, offset)
    if name == "wide":
        # NaN item rows, and terms with offsets of +inf, -inf and NaN on planted items
        c = F.random_case(d)
        # the first 20 users keep 1,200 unseen items, so that their lists of 1,024 run from the positive scores into the negative
        lists = _csr_lists(c["seen"], U)
        for u in c["users"][:20]:
            lists[int(u)] = rng.permutation(I)[1200:]
        c["seen"] = F.seen_csr(U, I, lists)
        ids = rng.permutation(I)
        c["wi"][ids[:12]] = np.nan
        scale, offset = _random_terms(rng, I)
        offset[ids[12:24]] = np.inf
        offset[ids[24:36]] = -np.inf
        offset[ids[36:48]] = np.nan
        c["planted"] = dict(nan_rows=ids[:12], pos_inf=ids[12:24], neg_inf=ids[24:36], nan_offset=ids[36:48])
        return _finish(c, dtype, d, _users257(c), rng.rand(I) < 0.6, scale, offset)
    if name == "long_tie":
        # every score +0 over 70,001 items: ONE bin of every radix pass, in LDS and in the global histogram, holds more than
        # 65,535 (a 16-bit or packed bin counter would wrap), and the tie walk places 1,024 of some 70,000 ties
        c = F.random_case(d, 0, 40, 70001, 40)
        c["wu"][:], c["wi"][:] = 0.0, 0.0
        n_item = c["wi"].shape[0]
        return _finish(c, dtype, d, np.arange(40), np.arange(n_item) % 5 != 2, np.ones(n_item), np.zeros(n_item))
    if name == "long":
        # eligible counts (the pass-0 totals, n_elig) beyond 65,535; the scores spread over many bins
        c = F.random_case(d, 0, 40, 70001, 40)
        n_item = c["wi"].shape[0]
        scale, offset = _random_terms(rng, n_item)
        return _finish(c, dtype, d, np.arange(40), rng.rand(n_item) < 0.6, scale, offset)
    raise ValueError(name)


def words(c):
    """The case's filter as uint32 words."""
    return pack(c["mask"])


def adj_table(c):
    """The case's terms as the padded float32 [2, n_pad] table (pads (1, 0))."""
    n_item = c["wi"].shape[0]
    adj = np.zeros((2, (n_item + 31) // 32 * 32), np.float32)
    adj[0] = 1.0
    adj[0, :n_item], adj[1, :n_item] = c["scale"], c["offset"]
    return adj


def effective_seen(c, variant):
    """The Seen CSR the reference sees: the case's, with the filter's complement added for `filter` / `both`."""
    if variant in ("filter", "both"):
        return seen_prime(c["seen"], c["mask"], c["wu"].shape[0])
    return c["seen"]


@functools.lru_cache(maxsize=None)
def reference(name, dtype, d, variant, n):
    """(items int64 [n, 1024], scores float32 [n, 1024], n_elig int64 [n]) of the case's first n users."""
    c = case(name, dtype, d)
    users = c["users"][:n]
    n_item = c["wi"].shape[0]
    seen = effective_seen(c, variant)
    off, seen_items = seen
    if variant in ("none", "filter") and np.isfinite(c["ru"]).all() and np.isfinite(c["ri"]).all():
        # finite tables of moderate entries: no score is NaN, so every unseen item is eligible
        assert np.abs(c["ru"]).max() < 2.0 ** 20 and np.abs(c["ri"]).max() < 2.0 ** 20
        items, scores = F.ref_topk(c["ru"], c["ri"], users, KMAX, seen)
        return items, scores, (n_item - (off[users + 1] - off[users])).astype(np.int64)
    # the whole score matrix of these users, exactly: the chain, then one fma32 for the terms
    A = F.score_chain(c["ru"][users], c["ri"])
    if variant in ("terms", "both"):
        A = F.fma32(A, c["scale"][None, :], c["offset"][None, :])
    items = np.full((n, KMAX), -1, np.int64)
    scores = np.full((n, KMAX), -np.inf, np.float32)
    n_elig = np.zeros(n, np.int64)
    for x, u in enumerate(users):
        ok = ~np.isnan(A[x])
        ok[seen_items[off[u]:off[u + 1]].astype(np.int64)] = False
        ids = np.nonzero(ok)[0]
        n_elig[x] = len(ids)
        o = ids[np.lexsort((ids, -A[x, ids].astype(np.float64)))][:KMAX]      # (-0 and +0 compare equal: the id decides)
        items[x, :len(o)] = o
        scores[x, :len(o)] = A[x, o]
    return items, scores, n_elig


def cut(ref, k):
    """The reference at k <= 1,024: the first k slots."""
    return ref[0][:, :k], ref[1][:, :k], ref[2]


# (case, element type, d, variant, users): every case; both element types, fp16 at d = 32 / 64 / 128; each of none, filter,
# terms and both at every width; n = 1, 33, 97, 257
GRID = []
for _q, (_t, _d) in enumerate(WIDTHS):
    for _v, _variant in enumerate(VARIANTS):
        GRID.append(("random", _t, _d, _variant, NS[(_q + 3 - _v) % 4]))
GRID += [("near_tie", "fp32", 32, "none", 257), ("near_tie", "fp32", 64, "filter", 97), ("near_tie", "fp32", 32, "terms", 33),
         ("all_tie", "fp32", 32, "none", 97), ("all_tie", "fp32", 64, "filter", 257), ("all_tie", "fp16", 128, "both", 97),
         ("all_tie", "fp16", 32, "terms", 33),
         ("sorted_desc", "fp32", 64, "none", 33), ("sorted_desc", "fp16", 32, "filter", 97), ("sorted_asc", "fp32", 32, "none", 97),
         ("sorted_asc", "fp16", 64, "both", 33), ("sorted_asc", "fp16", 128, "none", 257),
         ("wide", "fp32", 32, "terms", 97), ("wide", "fp16", 128, "both", 33), ("wide", "fp32", 64, "none", 33),
         ("long", "fp32", 32, "none", 40), ("long", "fp32", 32, "filter", 40),
         ("long_tie", "fp32", 32, "none", 8), ("long_tie", "fp16", 64, "filter", 8)]
GRID_IDS = ["%s-%s-d%d-%s-n%d" % g for g in GRID]
