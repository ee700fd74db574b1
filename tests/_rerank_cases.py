"""Greedy MMR re-ranking (include/sml_hip.h, "RE-RANKING"): the plain-numpy restatement ref_rerank and the seeded cases that
the host tests (tests/test_rerank_host.py) and the GPU tests (tests/test_rerank_gpu.py) share.

ref_rerank follows the header one named operation at a time: fma32 / chain of tests/_fp32_chain.py for the fused operations,
float32 numpy operations (each correctly rounded) for the single multiplies, adds, subtractions and divisions.  The pairwise
chain scores of a list's entries do not depend on lam, normalize, k or the metric, so they are computed once per (width,
element type) and shared (pairwise()); nothing else is cached, and no cached array is written again.
"""
import functools

import numpy as np

from _fp32_chain import chain, fma32

I = 4099                       # catalogue rows
C = 128                        # pool columns of the case
STRIDE = 131                   # pool_stride > pool_cols: the rows are read in place
LENGTHS = (1, 2, 63, 64, 65, 127, 128)
KS = (1, 20, 128)
WIDTHS = ((32, False), (64, False), (32, True), (64, True), (128, True))          # (d, fp16 table)
WIDTH_IDS = ["d%d-%s" % (d, "f16" if h else "f32") for d, h in WIDTHS]
# (lam, metric, normalize)
SETTINGS = ((0.7, "cosine", 1), (0.3, "dot", 0), (1.0, "cosine", 0), (0.0, "cosine", 1))
SETTING_IDS = ["lam%g-%s-%s" % (s[0], s[1], "norm" if s[2] else "raw") for s in SETTINGS]

# ids with planted rows
ID_ZERO = 7                                    # a zero row, norm 0
ID_ORIG, ID_COPIES = 100, (2000, 1500, 3000)   # exact copies of row 100 under other ids
ID_ULP = (200, 201, 202)                       # 201 / 202: row 200 with one coordinate one ulp up / down
ID_TINY = tuple(range(300, 340))               # subnormal-scale rows
LONG, SHORT = (28, 29, 30, 31), (32, 33, 34, 35)       # 128-entry lists, then short ones: the same wave under max_workgroups = 1


def _key(rel):
    """An integer key with the order of the non-NaN floats, -0 below +0 (the header's lo / hi)."""
    b = np.ascontiguousarray(rel, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def item_norms(wi32):
    """float32 [I]: 1 / ||row|| (0 for a zero row), an input of the call like any other: its own rounding is not under test."""
    n = np.sqrt((wi32.astype(np.float64) ** 2).sum(1))
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(n > 0, 1.0 / n, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(d, half):
    """dict: table (float32 or float16 [I, d]), table32 (the exact fp32 copy), nrm, pool_items int32 / pool_rel float32
    [n, STRIDE] (columns C.. are never read: they hold poison), n."""
    rng = np.random.RandomState(1900 + d + (7 if half else 0))
    dt = np.float16 if half else np.float32
    wi = rng.randn(I, d).astype(dt)
    wi[ID_ZERO] = 0
    for c in ID_COPIES:
        wi[c] = wi[ID_ORIG]
    for j, sgn in ((1, 1.0), (2, -1.0)):
        wi[ID_ULP[j]] = wi[ID_ULP[0]]
        q = rng.randint(d)
        wi[ID_ULP[j], q] = np.nextafter(wi[ID_ULP[0], q], dt(sgn * np.inf))
    scale = dt(2.0 ** -12) if half else dt(2.0 ** -70)          # fp16: subnormal halves; fp32: subnormal chain scores
    for i in ID_TINY:
        wi[i] = (wi[i] * scale).astype(dt)
    wi32 = wi.astype(np.float32)
    users = rng.randn(64, d).astype(np.float32)
    free = np.array([i for i in range(I) if i not in set((ID_ZERO, ID_ORIG) + ID_COPIES + ID_ULP + ID_TINY)])

    lists = []

    def sorted_pool(L, u):
        ids = rng.choice(free, size=L, replace=False)
        s = chain(users[u][None, :], wi32[ids])
        o = np.lexsort((ids, -s.astype(np.float64)))
        return ids[o], s[o]

    for j in range(14):                                        # pools as a top-K call returns them, (-1, -inf) behind
        lists.append(sorted_pool(LENGTHS[j % 7], j))
    for j in range(7):                                         # pools in random order, rel of any sign
        L = LENGTHS[j]
        lists.append((rng.choice(free, size=L, replace=False), rng.randn(L).astype(np.float32)))
    # 21: planted padding between live entries
    ids = rng.choice(free, size=40, replace=False).astype(np.int64)
    ids[[0, 5, 17, 39]] = (-1, I, 2 ** 31 - 1, -(2 ** 31))
    ids[[8, 9]] = (I + 64, -7)
    lists.append((ids, rng.randn(40).astype(np.float32)))
    # 22: repeated ids -- the first occurrence wins, unless its rel is NaN
    ids = rng.choice(free, size=70, replace=False)
    rel = rng.randn(70).astype(np.float32)
    ids[10], ids[33], ids[69] = ids[3], ids[3], ids[64]
    ids[40] = ids[20]
    rel[20] = np.nan                                           # position 40 is then the first occurrence with a number
    lists.append((ids, rel))
    # 23: NaN rel sprinkled, the first entry among them
    ids = rng.choice(free, size=65, replace=False)
    rel = rng.randn(65).astype(np.float32)
    rel[[0, 7, 63, 64]] = np.nan
    lists.append((ids, rel))
    # 24: exact copies of one row under other ids (equal sim, so value ties that the position breaks), equal rel among them
    ids = np.concatenate([rng.choice(free, size=20, replace=False), [ID_COPIES[0], ID_ORIG, ID_COPIES[1], ID_COPIES[2]]])
    rel = rng.randn(len(ids)).astype(np.float32)
    rel[20:24] = np.float32(0.25)
    lists.append((ids, rel))
    # 25: rows one ulp apart, equal rel
    ids = np.concatenate([[ID_ULP[1]], rng.choice(free, size=30, replace=False), [ID_ULP[2], ID_ULP[0]]])
    rel = rng.randn(len(ids)).astype(np.float32)
    rel[[0, -2, -1]] = np.float32(-0.5)
    lists.append((ids, rel))
    # 26: a zero row (norm 0) among others, as the most relevant entry
    ids = np.concatenate([rng.choice(free, size=9, replace=False), [ID_ZERO], rng.choice(free, size=9, replace=False)])
    rel = rng.randn(len(ids)).astype(np.float32)
    rel[9] = np.float32(5.0)
    lists.append((ids, rel))
    # 27: subnormal-scale rows only
    ids = np.array(ID_TINY)[rng.permutation(len(ID_TINY))]
    lists.append((ids, rng.randn(len(ids)).astype(np.float32)))
    for x in LONG:                                             # 28..31: full lists ...
        lists.append((rng.choice(free, size=128, replace=False), rng.randn(128).astype(np.float32)))
    for j, x in enumerate(SHORT):                              # 32..35: ... and short ones right behind them
        L = (2, 1, 3, 65)[j]
        lists.append((rng.choice(free, size=L, replace=False), rng.randn(L).astype(np.float32)))
    lists.append((np.array([-1, I, -5]), np.zeros(3, np.float32)))                       # 36: nothing eligible
    lists.append((rng.choice(free, size=30, replace=False), np.full(30, 1.5, np.float32)))   # 37: span == 0
    ids = rng.choice(free, size=12, replace=False)                                       # 38: signed zeros and infinities
    rel = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 0.0, -0.0, 2.0, -2.0, 0.5, -0.5], np.float32)
    lists.append((ids, rel))
    lists.append((rng.choice(free, size=6, replace=False), np.array([-0.0, 0.0, -0.0, 0.0, 3.0, 0.0], np.float32)))   # 39: lo is -0

    n = len(lists)
    pool_items = np.full((n, STRIDE), 5, np.int64)             # beyond the pools: a live id with a huge rel
    pool_rel = np.full((n, STRIDE), 1e30, np.float32)
    pool_items[:, :C] = -1
    pool_rel[:, :C] = -np.inf
    for x, (ids, rel) in enumerate(lists):
        pool_items[x, :len(ids)] = ids
        pool_rel[x, :len(ids)] = rel
    out = dict(d=d, half=half, table=wi, table32=wi32, nrm=item_norms(wi32), pool_items=pool_items.astype(np.int32), pool_rel=pool_rel,
               n=n, users=users)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pairwise(d, half):
    """float32 [n, C, C]: S[x, c, s] = the chain with entry s of list x on the user side and entry c on the item side
    (entries outside the catalogue read row 0; nothing uses those values)."""
    c = case(d, half)
    ids = c["pool_items"][:, :C].astype(np.int64)
    S = np.zeros((c["n"], C, C), np.float32)
    for x in range(c["n"]):
        L = int(np.nonzero(ids[x] != -1)[0].max(initial=-1)) + 1                   # behind it the row is (-1, -inf) padding
        rows = c["table32"][np.where((ids[x, :L] >= 0) & (ids[x, :L] < I), ids[x, :L], 0)]
        S[x, :L, :L] = chain(rows[None, :, :], rows[:, None, :])
    S.setflags(write=False)
    return S


def ref_rerank(table32, pool_items, pool_rel, pool_cols, nrm, lam, normalize, k, S=None, tie="first", norm_first="candidate",
               total_order="pick"):
    """(items int32 [n, k], pos int32 [n, k], value float32 [n, k], n_sel int32 [n], sim_sum float32 [n]) by the header's
    definition.  pool_items / pool_rel: [n, >= pool_cols], the first pool_cols columns are the pools.  S: the lists' pairwise
    chain scores [n, >= pool_cols, >= pool_cols] if the caller has them.  tie / norm_first / total_order are the definition's
    choices ("first", "candidate", "pick"); the other values ("last", "pick", "reverse") exist so the tests can show that the
    cases tell them apart."""
    n_item = table32.shape[0]
    n = pool_items.shape[0]
    lam = np.float32(lam)
    oml = np.float32(np.float32(1.0) - lam)
    items = np.full((n, k), -1, np.int32)
    pos = np.full((n, k), -1, np.int32)
    value = np.full((n, k), -np.inf, np.float32)
    n_sel = np.zeros(n, np.int32)
    sim_sum = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for x in range(n):
            ids = pool_items[x, :pool_cols].astype(np.int64)
            rel = pool_rel[x, :pool_cols].astype(np.float32)
            valid = (ids >= 0) & (ids < n_item) & ~np.isnan(rel)
            elig = valid.copy()
            for e in range(pool_cols):
                if elig[e] and (valid[:e] & (ids[:e] == ids[e])).any():
                    elig[e] = False
            m = int(elig.sum())
            if m == 0:
                continue
            if S is not None:
                Sx = S[x, :pool_cols, :pool_cols]
            else:
                rows = table32[np.where(valid, ids, 0)]
                Sx = chain(rows[None, :, :], rows[:, None, :])
            if nrm is None:
                sim = Sx
            else:
                nr = np.where(valid, nrm[np.where(valid, ids, 0)], np.float32(0)).astype(np.float32)
                if norm_first == "candidate":
                    sim = (Sx * nr[:, None]) * nr[None, :]
                else:
                    sim = (Sx * nr[None, :]) * nr[:, None]
            if normalize:
                key = _key(rel).astype(np.int64)
                hi = rel[int(np.argmax(np.where(elig, key, -1)))]
                lo = rel[int(np.argmin(np.where(elig, key, 1 << 40)))]
                span = np.float32(hi - lo)
                r = (rel - lo) / span if span > 0 else np.zeros(pool_cols, np.float32)
                r = r.astype(np.float32)
            else:
                r = rel
            pen = np.full(pool_cols, -np.inf, np.float32)
            acc = np.zeros(pool_cols, np.float32)
            live = elig.copy()
            picked_sums = []
            for t in range(min(k, m)):
                q = np.zeros(pool_cols, np.float32) if t == 0 else -(oml * pen)
                v = fma32(lam, r, q)
                idx = np.nonzero(live)[0]
                vv = v[idx]
                num = ~np.isnan(vv)
                cand = idx[num][vv[num] == vv[num].max()] if num.any() else idx
                s = int(cand[0] if tie == "first" else cand[-1])
                items[x, t], pos[x, t], value[x, t] = ids[s], s, v[s]
                picked_sums.append(acc[s])
                live[s] = False
                col = sim[:, s]
                pen = np.where(live & (col > pen), col, pen)
                acc = np.where(live, acc + col, acc)
            total = np.float32(0.0)
            for a in (picked_sums if total_order == "pick" else picked_sums[::-1]):
                total = np.float32(total + a)
            n_sel[x] = min(k, m)
            sim_sum[x] = total
    return items, pos, value, n_sel, sim_sum


@functools.lru_cache(maxsize=None)
def expected(d, half, setting, k, pool_cols=C):
    """ref_rerank on the case of (d, half) under SETTINGS[setting], computed once and shared (never written again)."""
    c = case(d, half)
    lam, metric, normalize = SETTINGS[setting]
    out = ref_rerank(c["table32"], c["pool_items"], c["pool_rel"], pool_cols, c["nrm"] if metric == "cosine" else None, lam, normalize, k,
                     S=pairwise(d, half))
    for a in out:
        a.setflags(write=False)
    return out


def same_bytes(got, want):
    """None, or the name of the first output whose bytes differ."""
    for name, g, w in zip(("items", "pos", "value", "n_sel", "sim_sum"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return name
    return None
