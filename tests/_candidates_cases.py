"""Helpers shared by the per-user candidate-list tests (test_candidates_host.py, test_candidates_gpu.py): the CPU reference
of sml_topk_candidates and the seeded cases the GPU tests run and the host tests inspect.

The contract (include/sml_hip.h): row x of the call equals row 0 of the filtered top-K call for the single user users[x] with
the filter `allow AND bitmap(list x)`.  ref_topk_candidates is that sentence on the CPU: per user it builds
Seen' = Seen + (catalogue - list) + (catalogue - mask) and calls the exact references that the sibling suites already use
(_fp32_chain.ref_topk; with terms, _item_score_cases.ref_topk on the adjusted score row).  Tables: U = 300, I = 4,099."""
import numpy as np

import _fp32_chain as F
import _item_score_cases as C
from _half_cases import random_half_case, widen

LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300)        # around the 64-candidate round and the two-round step
KMAX = 128


def _valid(ids, n_item):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    return ids[(ids >= 0) & (ids < n_item)]


def _scores(wu, wi, u, adj):
    """float32 [I]: A(u, .) -- the chain, then one fma with the terms when adj = (scale, offset) is given."""
    S = F.chain(wu[u][None], wi)
    return S if adj is None else C.adjusted(S, adj[0], adj[1])


def ref_topk_candidates(wu, wi, users, lists, k, seen=None, mask=None, adj=None):
    """(items int64 [n, k], scores float32 [n, k], n_elig int64 [n]).  wu / wi: the fp32 tables the chain runs on (fp16 tables
    widened); lists: n int sequences; seen = (off, items) over all users or None; mask: bool [I] or None; adj = (scale,
    offset) float32 [I] or None."""
    wu, wi = np.asarray(wu, np.float32), np.asarray(wi, np.float32)
    I = wi.shape[0]
    n = len(users)
    items = np.full((n, k), -1, np.int64)
    scores = np.full((n, k), -np.inf, np.float32)
    n_elig = np.zeros(n, np.int64)
    for x, u in enumerate(np.asarray(users, np.int64)):
        valid = _valid(lists[x], I)
        excl = np.ones(I, bool)
        excl[valid] = False
        if mask is not None:
            excl |= ~np.asarray(mask, bool)
        if seen is not None:
            off, it = seen
            excl[np.asarray(it[off[u]:off[u + 1]], np.int64)] = True
        sp = (np.array([0, int(excl.sum())], np.int64), np.nonzero(excl)[0].astype(np.int32))
        if adj is None:
            items[x], scores[x] = (t[0] for t in F.ref_topk(wu[u:u + 1], wi, [0], k, sp))
            a = F.chain(wu[u], wi[valid]) if len(valid) else np.zeros(0, np.float32)
        else:
            A = _scores(wu, wi, u, adj)
            items[x], scores[x] = (t[0] for t in C.ref_topk(A[None], [0], k, sp, None))
            a = A[valid]
        n_elig[x] = int((~excl[valid] & ~np.isnan(a)).sum())
    return items, scores, n_elig


def ref_keep_repeats(wu, wi, users, lists, k, seen=None, mask=None, adj=None):
    """What a kernel that did NOT drop repeats would list: every eligible ENTRY in the top-K order, first k.  Exists so the
    host tests can show that the repeat cases tell the two apart."""
    wu, wi = np.asarray(wu, np.float32), np.asarray(wi, np.float32)
    I = wi.shape[0]
    items = np.full((len(users), k), -1, np.int64)
    for x, u in enumerate(np.asarray(users, np.int64)):
        valid = _valid(lists[x], I)
        ok = np.ones(len(valid), bool) if mask is None else np.asarray(mask, bool)[valid]
        if seen is not None:
            off, it = seen
            ok &= ~np.isin(valid, np.asarray(it[off[u]:off[u + 1]], np.int64))
        a = _scores(wu, wi, u, adj)[valid]
        ok &= ~np.isnan(a)
        ids, a = valid[ok], a[ok]
        o = ids[np.lexsort((ids, -a.astype(np.float64)))][:k]
        items[x, :len(o)] = o
    return items


def tables(dtype, d, seed=0):
    """The seeded random case of the sibling suites with `ru` / `ri`, the fp32 tables the references score."""
    c = F.random_case(d, seed) if dtype == "fp32" else random_half_case(d, seed)
    c["ru"], c["ri"] = (c["wu"], c["wi"]) if dtype == "fp32" else (widen(c["wu"]), widen(c["wi"]))
    c["dtype"], c["d"] = dtype, d
    return c


def draw_list(rng, c, u, length, seen_share=8):
    """`length` distinct item ids in random order; one in seen_share of them (where the user has that many) from Seen(u)."""
    I = c["wi"].shape[0]
    off, it = c["seen"]
    s = np.asarray(it[off[u]:off[u + 1]], np.int64)
    take = min(len(s), length // seen_share)
    own = rng.choice(s, size=take, replace=False) if take else np.zeros(0, np.int64)
    rest = rng.choice(np.setdiff1d(np.arange(I), own), size=length - take, replace=False)
    return rng.permutation(np.concatenate([own, rest]).astype(np.int64))


def boundary_case(dtype, d, seed=0):
    """27 lists of the lengths LENGTHS (three of each, shuffled), for random users (two of them repeat)."""
    c = tables(dtype, d, seed)
    rng = np.random.RandomState(100 + seed)
    lengths = rng.permutation(np.repeat(LENGTHS, 3))
    users = rng.choice(c["wu"].shape[0], size=len(lengths), replace=False)
    users[5], users[11] = users[2], users[2]
    c["users"] = users.astype(np.int64)
    c["lists"] = [draw_list(rng, c, u, int(m)) for u, m in zip(users, lengths)]
    return c


def mixed_case(dtype, d, seed=0, n=40, with_special=None):
    """n lists of random lengths up to 300 with repeats and padding inside: what the identity tests run.  with_special: item
    ids (e.g. the -inf / NaN items of a score case) that every third list also holds."""
    c = tables(dtype, d, seed)
    rng = np.random.RandomState(200 + seed)
    users = rng.choice(c["wu"].shape[0], size=n, replace=False).astype(np.int64)
    lists = []
    for x, u in enumerate(users):
        base = draw_list(rng, c, u, int(rng.randint(1, 301)))
        extra = [base[rng.randint(len(base), size=len(base) // 5)], np.full(3, -1, np.int64)]
        if with_special is not None and x % 3 == 0:
            extra.append(np.asarray(with_special, np.int64))
        lists.append(rng.permutation(np.concatenate([base] + extra)))
    lists[7] = np.zeros(0, np.int64)
    c["users"], c["lists"] = users, lists
    return c


def repeat_case(seed=0):
    """fp32, d = 32, with an all-NaN item row (item 11); lists built by hand around repeats and padding.  c["names"] tells
    which list is which; c["repeats"] marks the lists that hold an id twice."""
    c = tables("fp32", 32, seed)
    c["wi"][11] = np.nan
    rng = np.random.RandomState(300 + seed)
    wu, wi = c["wu"], c["wi"]
    I = wi.shape[0]
    off, it = c["seen"]
    names, users, lists = [], [], []

    def add(name, u, ids):
        names.append(name)
        users.append(int(u))
        lists.append(np.asarray(ids, np.int64))

    u = 3
    base = draw_list(rng, c, u, 100)
    add("every id doubled", u, np.repeat(base, 2))
    add("doubled, second copies last", u, np.concatenate([base, base]))
    # a repeat in a later round than its first occurrence: the best item of 300 again at entry 299 and the 20th at 200
    base = draw_list(rng, c, 5, 298)
    full = np.concatenate([base, [0, 0]])
    order, _, _ = ref_topk_candidates(wu, wi, [5], [base], 20, c["seen"])
    full[200], full[299] = order[0, 19], order[0, 0]
    add("best and K-th again in later rounds", 5, full)
    add("best item 64 times", 5, np.concatenate([np.full(64, order[0, 0]), base[:70]]))
    base = draw_list(rng, c, 9, 90)
    add("-1 inside and at the end", 9, np.concatenate([base[:40], [-1, -1, -1], base[40:], np.full(17, -1)]))
    add("ids past the catalogue", 9, np.concatenate([base[:30], [I, I + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, 2 ** 40, -2 ** 31, -2 ** 40], base[30:60]]))
    add("all padding", 9, np.concatenate([np.full(70, -1), [I, 2 ** 31 - 1, 2 ** 33]]))
    s = np.asarray(it[off[17]:off[18]], np.int64)
    assert len(s) >= 2
    add("all Seen", 17, np.concatenate([s, s[:5]]))
    add("NaN row among the candidates", 21, np.concatenate([draw_list(rng, c, 21, 30), [11, 11]]))
    add("only the NaN row", 21, [11])
    c["names"], c["users"], c["lists"] = names, np.asarray(users, np.int64), lists
    c["repeats"] = [len(np.unique(_valid(l, I))) < len(_valid(l, I)) for l in lists]
    return c


def tie_case(seed=0):
    """near_tie_case (fp32, d = 32): for 24 of the planted rows the list is every item whose row is the positive's up to the
    order of its values (the exact copies, the one-ulp copies, the dim-permuted copies), the positive itself and 40 random
    items -- fed in DESCENDING id order, so that the id tie-break has to reorder the bit-equal ones."""
    c = F.near_tie_case(32, seed)
    c["ru"], c["ri"], c["dtype"], c["d"] = c["wu"], c["wi"], "fp32", 32
    rng = np.random.RandomState(400 + seed)
    wi = c["wi"]
    I = wi.shape[0]
    ws = np.sort(wi.astype(np.float64), axis=1)
    users, lists, ties = [], [], 0
    for u, p in c["planted"][:24]:
        near = np.nonzero((ws != ws[p]).sum(1) <= 2)[0]
        assert len(near) >= 5, (u, p, len(near))
        ids = np.unique(np.concatenate([near, [p], rng.choice(I, size=40, replace=False)]))[::-1]
        users.append(int(u))
        lists.append(ids.astype(np.int64))
        s = F.chain(c["wu"][u], wi[np.asarray(near)])
        ties += len(s) - len(np.unique(s.view(np.int32)))
    c["users"], c["lists"], c["ties"] = np.asarray(users, np.int64), lists, ties
    return c


def ragged(lists, dtype=np.int32):
    """(cand_off int64 [n + 1], cand_items) of n lists."""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    flat = np.concatenate([np.asarray(l, np.int64) for l in lists]) if lists else np.zeros(0, np.int64)
    return off, flat.astype(dtype)


def dense(lists, dtype=np.int64, pad=-1):
    """[n, C] with C the longest list, short lists padded with `pad`."""
    C_ = max([len(l) for l in lists] + [1])
    m = np.full((len(lists), C_), pad, dtype)
    for x, l in enumerate(lists):
        m[x, :len(l)] = np.asarray(l, np.int64).astype(dtype)
    return m


def list_mask(ids, n_item):
    m = np.zeros(n_item, bool)
    m[_valid(ids, n_item)] = True
    return m
