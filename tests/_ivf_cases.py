"""Seeded cases of the clustered item index (sml_ivf_search / sml_ivf_centroids, include/sml_hip.h "CLUSTERED INDEX"), shared by
test_ivf_host.py and test_ivf_gpu.py.  Every comparison made on them is byte equality.

The catalogue has I = 420 items and U = 40 users at every (element type, width) pair of the family.  PARTITION A is hand-made, 12
lists of the sizes SIZES_A: two tiny lists (1, 1) followed by an empty one and a 70, so that one round of 64 candidates spans
four lists; 63 / 64 / 65 around the round; 127 just short of the two-round step; list 9 (2 items) holds NaN rows only.  PARTITION
B has 130 lists of 0 .. 3 items over the first I_B items: probed with nprobe = 128 it takes both probes of every lane, and one
of its users probes fewer than 64 items in all.  The reference is tests/_candidates_cases.py's ref_topk_candidates on the
concatenated lists, the defining identity of the header."""
import functools

import numpy as np

import _candidates_cases as K
import _item_score_cases as C
from _half_cases import widen

I, U = 420, 40
PAIRS = (("fp32", 32), ("fp32", 64), ("fp16", 32), ("fp16", 64), ("fp16", 128))
SIZES_A = (0, 1, 1, 0, 70, 63, 64, 65, 127, 2, 20, 7)       # sums to I
NAN_LIST = 9
USERS = np.array([3, 7, 3, 11, 0, 39, 20], np.int64)          # user 3 repeats
KS = (1, 20, 128)
NPROBES = (1, 3, 12)
VARIANTS = ("none", "filter", "terms", "both")
NEG_INF_ITEM_LIST, ZERO_LISTS = 8, (5, 6)
assert sum(SIZES_A) == I


def csr(lists):
    """(list_off int64 [n_list + 1], list_items int32) of lists of ascending ids."""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return off, np.concatenate([np.asarray(l, np.int64) for l in lists]).astype(np.int32)


def partition_a(rng):
    order = rng.permutation(I)
    cuts = np.cumsum((0,) + SIZES_A)
    return [np.sort(order[cuts[c]:cuts[c + 1]]) for c in range(len(SIZES_A))]


def partition_b(rng):
    sizes = np.array([(c * 7 + 3) % 4 for c in range(130)])           # 0 .. 3, every value often
    order = rng.permutation(int(sizes.sum()))
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return [np.sort(order[cuts[c]:cuts[c + 1]]) for c in range(130)]


def probes_a(nprobe):
    """int32 [7, nprobe] over partition A (12 lists): padding by -1 and by n_list + 5, a list probed twice, an all-padding row."""
    pad = 12 + 5
    if nprobe == 1:
        rows = [[4], [1], [-1], [8], [pad], [NAN_LIST], [0]]
    elif nprobe == 3:
        rows = [[1, 2, 3], [3, 4, -1], [8, 8, pad], [-1, pad, -1], [NAN_LIST, 5, 6], [10, 11, 0], [2, 1, 4]]
    else:
        rows = [list(range(12)),                                      # every list once: the whole catalogue
                [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0],
                [1, 2, 3, 4, -1, pad, 8, 8, NAN_LIST, 5, 0, 3],           # the four-list round, then a list twice
                [-1, pad, -1, -1, pad, pad, -1, -1, -1, pad, -1, -1],   # nothing but padding
                [4, 4, 4, 5, 6, 7, 0, 0, 3, -1, 10, 11],
                [1, 2, 3, 4, 5, 6, 7, 8, -1, -1, -1, -1],
                [NAN_LIST, 0, 3, 1, 2, pad, -1, 11, 10, 6, 5, 4]]
    return np.array(rows, np.int32)


def probes_b():
    """int32 [7, 128] over partition B (130 lists of 0 .. 3 items): rows 0 / 1 probe 128 lists, row 2 only the lists of 0 or 1
    items between padding (fewer than 64 items in all), row 3 one list 128 times, the rest mix padding in."""
    rng = np.random.RandomState(77)
    rows = [np.arange(128), np.arange(129, 1, -1)]
    small = np.array([c for c in range(130) if (c * 7 + 3) % 4 < 2])
    rows.append(np.concatenate([small, np.full(128 - len(small), -1)]))
    rows.append(np.full(128, 2))
    for _ in range(3):
        r = rng.randint(-20, 150, size=128)
        rows.append(r)
    return np.array(rows, np.int32)


@functools.lru_cache(maxsize=None)
def case(dtype, d):
    """The tables of one (element type, width) pair with everything the variants need: wu / wi (the element type), ru / ri (the
    fp32 tables the reference scores), lists_a / lists_b, seen (a CSR over the users: user 3's swallows list 4 whole, user 7's is
    empty), mask (bool [I]) and (scale, offset) with one -inf offset."""
    rng = np.random.RandomState(1000 + d + (7 if dtype == "fp16" else 0))
    t = np.float32 if dtype == "fp32" else np.float16
    wu, wi = rng.randn(U, d).astype(t), rng.randn(I, d).astype(t)
    lists_a, lists_b = partition_a(rng), partition_b(rng)
    wi[lists_a[NAN_LIST]] = np.nan                                     # a list made of NaN rows only
    za, zb = lists_a[ZERO_LISTS[0]][0], lists_a[ZERO_LISTS[1]][0]      # +0 and -0 rows in two lists: their scores tie
    wi[za], wi[zb] = 0.0, -0.0
    seen = {u: rng.choice(I, size=rng.randint(0, 60), replace=False) for u in range(U)}
    seen[3] = np.concatenate([lists_a[4], lists_a[8][:9], lists_b[5]])
    seen[7] = []
    scale = (rng.rand(I) * 2 - 0.5).astype(np.float32)
    offset = rng.randn(I).astype(np.float32)
    offset[lists_a[NEG_INF_ITEM_LIST][3]] = -np.inf
    scale[za], offset[za], scale[zb], offset[zb] = 1.0, 0.0, -1.0, -0.0      # with terms: A = +0 and fmaf(+0, -1, -0) = -0, a tie
    c = dict(dtype=dtype, d=d, wu=wu, wi=wi, lists_a=lists_a, lists_b=lists_b, mask=rng.rand(I) < 0.7, terms=(scale, offset),
             seen=seen, zeros=(int(za), int(zb)))
    c["ru"], c["ri"] = (wu, wi) if dtype == "fp32" else (widen(wu), widen(wi))
    c["csr"] = K.F.seen_csr(U, I, seen)
    return c


def sub_b(c):
    """Case c cut down to partition B's catalogue (its first I_B items): (I_B, wi, ri, Seen CSR, mask, terms)."""
    n = sum(len(l) for l in c["lists_b"])
    seen = {u: [i for i in s if i < n] for u, s in c["seen"].items()}
    return n, c["wi"][:n], c["ri"][:n], K.F.seen_csr(U, n, seen), c["mask"][:n], (c["terms"][0][:n], c["terms"][1][:n])


def variant_args(variant, mask, terms):
    """(mask or None, (scale, offset) or None) of a variant."""
    return (mask if variant in ("filter", "both") else None), (terms if variant in ("terms", "both") else None)


def concat_lists(lists, probes):
    """The ragged candidate lists the defining identity names: per row the members of its valid probes, in probe order."""
    out = []
    for row in probes:
        parts = [lists[p] for p in row if 0 <= p < len(lists)]
        out.append(np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64))
    return out


def filter_words(mask):
    from sml_amd.retrieval import ItemFilter
    return ItemFilter.from_mask(np.asarray(mask, bool)).host()


def _p(a):
    return None if a is None else a.ctypes.data


def host_search(wu, wi, d, users, lists, probes, k, seen=None, mask=None, terms=None, junk=True):
    """(items int32 [n, k], scores float32 [n, k], n_elig int32 [n]) of sml_host_ivf_search, the outputs prefilled with junk."""
    from sml_amd import _lib
    lib = _lib.load()
    users = np.ascontiguousarray(users, np.int64)
    probes = np.ascontiguousarray(probes, np.int32)
    off, items_ = csr(lists)
    n = len(users)
    allow = None if mask is None else filter_words(mask)
    adj = None if terms is None else C.pad_adj(*terms)
    s_off, s_items = (None, None) if seen is None else (np.ascontiguousarray(seen[0], np.int64),
                                                        np.ascontiguousarray(np.concatenate([seen[1], [0]]), np.int32))
    items, scores, n_elig = np.full((n, k), 77, np.int32), np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32)
    _lib.check(lib.sml_host_ivf_search(_p(wu), _p(wi), wu.itemsize, d, wi.shape[0], _p(users), n, _p(off), _p(items_), len(lists),
                                       _p(probes), probes.shape[1], k, _p(s_off), _p(s_items), _p(allow), _p(adj), _p(items), _p(scores),
                                       _p(n_elig)), "sml_host_ivf_search")
    return items, scores, n_elig


def host_topk_items(wu, wi, d, users, k, seen=None, mask=None, terms=None):
    """(items, scores, n_elig) of sml_host_topk_items: the whole-catalogue definition on the host."""
    from sml_amd import _lib
    lib = _lib.load()
    users = np.ascontiguousarray(users, np.int64)
    n = len(users)
    allow = None if mask is None else filter_words(mask)
    adj = None if terms is None else C.pad_adj(*terms)
    s_off, s_items = (None, None) if seen is None else (np.ascontiguousarray(seen[0], np.int64),
                                                        np.ascontiguousarray(np.concatenate([seen[1], [0]]), np.int32))
    items, scores, n_elig = np.full((n, k), 77, np.int32), np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32)
    _lib.check(lib.sml_host_topk_items(_p(wu), _p(wi), wu.itemsize, d, wi.shape[0], _p(users), n, k, _p(s_off), _p(s_items), _p(allow),
                                       _p(adj), _p(items), _p(scores), _p(n_elig)), "sml_host_topk_items")
    return items, scores, n_elig


def host_centroids(wi, d, lists, cin, in_place=False):
    """sml_host_ivf_centroids: a new array, or cin itself rewritten (in_place)."""
    from sml_amd import _lib
    lib = _lib.load()
    off, items = csr(lists)
    cin = np.ascontiguousarray(cin)
    out = cin if in_place else np.full_like(cin, 7)
    _lib.check(lib.sml_host_ivf_centroids(_p(wi), wi.itemsize, d, wi.shape[0], _p(off), _p(items), len(lists), _p(cin), _p(out)),
               "sml_host_ivf_centroids")
    return out


def ref_centroids(wi, lists, cin):
    """The definition in numpy float64, one addition at a time in member order (not np.sum): acc += x; (T)(float32)(acc / len)."""
    out = np.array(cin, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, members in enumerate(lists):
            if len(members) == 0:
                continue
            acc = np.zeros(wi.shape[1], np.float64)
            for m in members:
                acc = acc + wi[m].astype(np.float64)
            out[c] = (acc / np.float64(len(members))).astype(np.float32).astype(wi.dtype)
    return out


def same_bytes(got, want, what=""):
    """items, scores (as int32 bit patterns) and n_elig, byte for byte."""
    for name, g, w in zip(("items", "scores", "n_elig"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name == "scores":
            g, w = g.astype(np.float32).view(np.int32), w.astype(np.float32).view(np.int32)
        else:
            g, w = g.astype(np.int64), w.astype(np.int64)
        assert g.shape == w.shape and (g == w).all(), (what, name, np.argwhere(g != w)[:5].tolist())
