"""Helpers shared by the adjusted-score tests (test_item_score_host.py, test_item_score_gpu.py): the exact reference of

    A(u, i) = fmaf(S(u, i), scale[i], offset[i])            (include/sml_hip.h, the sml_*_adjusted entry points)

on the fp32 chain of tests/_fp32_chain.py, small brute-force references over the full adjusted score matrix, the cosine scale
in numpy, and the seeded cases the GPU tests run and the host tests inspect.  Tables are small (300 x 4,099), so the whole
matrix is scored once per case and shared."""
import numpy as np

import _fp32_chain as F
from _half_cases import random_half_case, widen
from _user_rank_ref import ref_user_rank as _ref_user_rank

SEED = 5                                   # checked on the CPU by test_item_score_host.py: the terms change every answer


def adjusted(S, scale, offset, rounding="one"):
    """float32 A = fma32(S, scale, offset), rounded once.  rounding="two" (the product rounded to fp32, then the sum)
    exists only to show that the exact comparison tells the two apart."""
    if rounding == "one":
        return F.fma32(S, scale, offset)
    if rounding != "two":
        raise ValueError(rounding)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.asarray(S, np.float32) * np.asarray(scale, np.float32)).astype(np.float32)
        return (p + np.asarray(offset, np.float32)).astype(np.float32)


def cosine_scale(wi):
    """float32 [n_item]: n2 = chain(x, x); n2 > 0 ? 1 / sqrt(n2) : 0 -- np.sqrt and the float32 divide round correctly."""
    x = np.asarray(wi, dtype=np.float32)
    n2 = F.chain(x, x)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.float32(1.0) / np.sqrt(n2)
    return np.where(n2 > 0, s, np.float32(0.0)).astype(np.float32)


def pad_adj(scale, offset, pad_scale=1.0, pad_offset=0.0):
    """float32 [2, n_pad] from [n_item] arrays, the pad entries holding what is given."""
    n = len(scale)
    n_pad = (n + 31) // 32 * 32
    adj = np.empty((2, n_pad), np.float32)
    adj[0], adj[1] = pad_scale, pad_offset
    adj[0, :n], adj[1, :n] = scale, offset
    return adj


def _excluded(n_item, seen, u, mask):
    out = np.zeros(n_item, bool) if mask is None else ~np.asarray(mask, bool)
    if seen is not None:
        off, items = seen
        out[np.asarray(items[off[u]:off[u + 1]], np.int64)] = True
    return out


def ref_rank(A, rows, seen=None, mask=None):
    """int64 [n]: #{i != p, not in Seen(u), allowed : A(u, i) > A(u, p)}; A float32 [n_user, n_item] over ALL users."""
    out = np.zeros(len(rows), np.int64)
    for r, (u, p) in enumerate(np.asarray(rows)[:, :2]):
        ok = ~_excluded(A.shape[1], seen, u, mask)
        ok[p] = False
        with np.errstate(invalid="ignore"):
            out[r] = int((A[u][ok] > A[u, p]).sum())
    return out


def ref_topk(A, users, k, seen=None, mask=None):
    """(int64 items [n, k], float32 scores [n, k]): eligible = not in Seen, allowed, A not NaN; A descending then id
    ascending; (-1, -inf) padding."""
    items = np.full((len(users), k), -1, np.int64)
    scores = np.full((len(users), k), -np.inf, np.float32)
    for x, u in enumerate(users):
        a = A[u]
        ids = np.nonzero(~_excluded(A.shape[1], seen, u, mask) & ~np.isnan(a))[0]
        o = ids[np.lexsort((ids, -a[ids].astype(np.float64)))][:k]
        items[x, :len(o)] = o
        scores[x, :len(o)] = a[o]
    return items, scores


def ref_user_rank(A, users, pos_off, pos_items, seen=None, mask=None):
    """(above, pos) by the definitions of _user_rank_ref on the adjusted scores; a filter is Seen' (seen_prime)."""
    from _item_filter_cases import seen_prime
    users = np.asarray(users, np.int64)
    if mask is not None:
        seen = seen_prime(seen, mask, A.shape[0])
    return _ref_user_rank(None, np.empty((A.shape[1], 0)), users, pos_off, pos_items, seen, S=A[users])


def score_case(dtype, d, seed=SEED, base="random"):
    """random_case / random_half_case (U = 300, I = 4,099: 129 tiles, the last of 3 items; n = 256) -- or near_tie_case, fp32
    only -- with per-item terms: scale uniform in [0.25, 4], offset ~ randn (near_tie: offset +0, so that the planted
    near-ties of S stay near-ties of A; near_tie_offset: scale and a small non-zero offset shared by rows of the same
    content, so that they stay near-ties THROUGH the fma's rounding), and planted:

      ties      two free ids get the row AND the terms of a positive: A ties, broken by id;
      ulp       two more get the row and scale of a positive and its offset moved one ulp up / down;
      -inf      offset -inf on 12 items, NaN offset on 12, scale 0 on 12, NaN scale on 4 -- four of each (two of the last)
                are positives of rows, the rest random ids.
    S order and A order disagree throughout (random terms).  c["ru"], c["ri"]: the fp32 tables the references score."""
    if base in ("near_tie", "near_tie_offset"):
        assert dtype == "fp32"
        c = F.near_tie_case(d, seed)
    else:
        c = F.random_case(d, seed) if dtype == "fp32" else random_half_case(d, seed)
    rng = np.random.RandomState(1000 + seed)
    wi, rows = c["wi"], c["rows"]
    I = wi.shape[0]
    scale = rng.uniform(0.25, 4.0, I).astype(np.float32)
    offset = rng.randn(I).astype(np.float32) if base == "random" else np.zeros(I, np.float32)
    if base == "near_tie_offset":
        # near-ties of A that go through the fma's rounding: terms that depend on the row's CONTENT only (12 leading bits of
        # its L1 norm), so that near_tie_case's copies of a positive -- exact, one ulp off, dims permuted -- get the
        # positive's scale and a non-zero offset of the scores' own magnitude (the tables are scaled by 2^-70)
        m, _ = np.frexp(np.abs(wi.astype(np.float64)).sum(1))
        h = (np.floor(m * 4096) * 2654435761.0 % 2.0 ** 32) / 2.0 ** 32
        scale = (0.25 + 3.75 * h).astype(np.float32)
        offset = (((h * 7919.0) % 1.0 - 0.5) * 2.0 ** -68).astype(np.float32)
    taken = set(rows[:, 1].tolist())
    free = [i for i in rng.permutation(I) if i not in taken]
    for r in range(100, 124):                               # (rows past near_tie_case's planted 0..95)
        p = rows[r, 1]
        for q in range(2):
            i = free.pop()
            wi[i], scale[i], offset[i] = wi[p], scale[p], offset[p]
        for sgn in (1, -1):
            i = free.pop()
            wi[i], scale[i] = wi[p], scale[p]
            offset[i] = np.nextafter(offset[p], np.float32(sgn * np.inf))
    special = {}
    pos = list(dict.fromkeys(rows[130:200, 1].tolist()))
    for name, n_pos, n_free in (("neg_inf", 4, 8), ("nan_offset", 4, 8), ("zero_scale", 4, 8), ("nan_scale", 2, 2)):
        ids = np.array([pos.pop() for _ in range(n_pos)] + [free.pop() for _ in range(n_free)])
        special[name] = ids
    offset[special["neg_inf"]] = -np.inf
    offset[special["nan_offset"]] = np.nan
    scale[special["zero_scale"]] = 0.0
    scale[special["nan_scale"]] = np.nan
    c.update(scale=scale, offset=offset, special=special, dtype=dtype, d=d,
             ru=c["wu"] if dtype == "fp32" else widen(c["wu"]), ri=wi if dtype == "fp32" else widen(wi))
    return c


def case_scores(c):
    """float32 [U, I]: S of every user against every item (the kernels' chain), computed once per case."""
    if "S" not in c:
        c["S"] = F.score_chain(c["ru"], c["ri"])
    return c["S"]


def held_sets(c, n_users, seed=3):
    """(users, pos_off, pos_items): held-out sets of sizes 0, 1, 4, 30 in turn, plus the rows' positives of the user, some of
    its Seen items and, for every third user, the special items (so -inf, NaN and zero-scale items are held out)."""
    from _user_rank_ref import held_out_csr
    rng = np.random.RandomState(seed)
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    off, items = c["seen"]
    rows = c["rows"]
    extra = np.concatenate([v[:3] for v in c["special"].values()]) if "special" in c else ()
    lists = []
    for x, u in enumerate(rng.choice(U, size=n_users, replace=False)):
        it = set(rows[rows[:, 0] == u, 1].tolist())
        it.update(rng.choice(I, size=[0, 1, 4, 30][x % 4], replace=False).tolist())
        s = items[off[u]:off[u + 1]]
        if len(s) and x % 4 == 1:
            it.update(s[:3].tolist())
        if x % 3 == 2:
            it.update(int(i) for i in extra)
        lists.append((int(u), it))
    return held_out_csr(U, lists)
