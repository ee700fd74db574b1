"""Training negatives ("training negatives", include/sml_hip.h) restated in plain Python / numpy, and the seeded cases.

Nothing here comes from the product: the generator, the candidate positions, the admissibility test, the pool and the
choice are written out from the definition, and the scores are tests/_fp32_chain.py's chain(..., "kernel").

walk_one    one element, one candidate at a time, Python integers: the definition read literally.
pools       the same for all elements at once (numpy over a first stretch of candidates, then element by element up to
            the cap): the first 64 admissible candidates of every element, from which every pool M <= 64 is a prefix.
walk        (negs, score, failed) of a case for one M, from the cached pools and scores.
The host test checks walk against walk_one on a sample of elements that includes every special user.
"""
import bisect
import functools

import numpy as np

from _fp32_chain import chain

K1, K2, GAMMA = 0xd1342543de82ef95, 0x632be59bd9b4e019, 0x9e3779b97f4a7c15
MASK = (1 << 64) - 1
CAP = 4096
MAXPOOL = 64
SEED = 2024
POOLS = (1, 2, 3, 8, 33, 64)


# ---- the definition, literally ----------------------------------------------------------------------------------------

def mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def stream(seed, e):
    return (seed ^ ((e * K1 + K2) & MASK)) & MASK


def draw(s0, c):
    return mix((s0 + (c + 1) * GAMMA) & MASK)


def position(z, pop, cdf):
    if cdf is None:
        return (z * pop) >> 64
    return bisect.bisect_right(cdf, float(z >> 11) * 2.0 ** -53)


def own_items(case, u):
    ptr, items = case["user_ptr"], case["user_items"]
    return set(items[ptr[u]:ptr[u + 1]].tolist()) if 0 <= u < len(ptr) - 1 else set()


def walk_one(case, users, e, M, seed=SEED):
    """(neg, score or None, failed 0/1, pool [(c, item), ...]) of element e."""
    u = int(users[e])
    own = own_items(case, u)
    item_all, pop = case["item_all"], len(case["item_all"])
    cdf = None if case["cdf"] is None else case["cdf"].tolist()
    s0 = stream(seed, e)
    pool, cand = [], int(item_all[0])
    for c in range(CAP):
        cand = int(item_all[position(draw(s0, c), pop, cdf)])
        if cand in own:
            continue
        pool.append((c, cand))
        if len(pool) == M:
            break
    score = lambda item: np.float32(chain(case["wu"][u], case["wi"][item], "kernel"))
    if not pool:
        return cand, (score(cand) if M > 1 else None), 1, pool
    if M == 1:
        return pool[0][1], None, 0, pool
    best = None
    for c, item in pool:
        s = score(item)
        if best is None:
            best = (s, item)
        elif np.isnan(best[0]) and not np.isnan(s):
            best = (s, item)
        elif not np.isnan(s) and s > best[0]:
            best = (s, item)
    return best[1], best[0], 0, pool


def draw_negative_walk(case, users, e, seed=SEED):
    """sml_sample_negatives' element: the splitmix64 state walked one step per try.  (neg, failed 0/1)"""
    u = int(users[e])
    own = own_items(case, u)
    item_all, pop = case["item_all"], len(case["item_all"])
    st, cand = stream(seed, e), int(item_all[0])
    for _ in range(CAP):
        st = (st + GAMMA) & MASK
        cand = int(item_all[(mix(st) * pop) >> 64])
        if cand not in own:
            return cand, 0
    return cand, 1


# ---- the same for every element at once -------------------------------------------------------------------------------

def _mix_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def _candidates(case, e, c, seed):
    """items drawn as candidates c (int array [k]) of elements e (int array [m]): int64 [m, k]"""
    with np.errstate(over="ignore"):
        s0 = np.uint64(seed) ^ (e.astype(np.uint64) * np.uint64(K1) + np.uint64(K2))
        z = _mix_np(s0[:, None] + (c.astype(np.uint64)[None, :] + np.uint64(1)) * np.uint64(GAMMA))
    pop = len(case["item_all"])
    if case["cdf"] is None:
        hi, lo = z >> np.uint64(32), z & np.uint64(0xffffffff)              # floor(z * pop / 2^64), pop < 2^31
        pos = (hi * np.uint64(pop) + ((lo * np.uint64(pop)) >> np.uint64(32))) >> np.uint64(32)
    else:
        pos = np.searchsorted(case["cdf"], (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, side="right")
    return case["item_all"][pos.astype(np.int64)]


def _own(case, u, cand):
    """bool [m, k]: cand[x, y] is one of u[x]'s items"""
    ptr, items = case["user_ptr"], case["user_items"]
    n_users, stride = len(ptr) - 1, int(max(items.max() if len(items) else 0, cand.max())) + 1
    codes = np.repeat(np.arange(n_users), np.diff(ptr)) * stride + items
    inside = (u >= 0) & (u < n_users)
    return np.isin(np.where(inside, u, 0)[:, None] * stride + cand, codes) & inside[:, None]


def pools(case, users, seed=SEED, first=96, keep=MAXPOOL):
    """(count int [n], c int [n, keep], item int64 [n, keep], last int64 [n]): the first `keep` admissible candidates of
    every element (unused slots: c = -1, item = 0) and candidate number 4095's item for the elements that found none."""
    users = np.asarray(users, dtype=np.int64)
    n = len(users)
    count = np.zeros(n, np.int64)
    pc = np.full((n, keep), -1, np.int64)
    pi = np.zeros((n, keep), np.int64)
    last = np.zeros(n, np.int64)

    def fill(rows, cs):
        cand = _candidates(case, rows, cs, seed)
        ok = ~_own(case, users[rows], cand)
        slot = np.cumsum(ok, axis=1) - 1
        take = ok & (slot < keep)
        x, y = np.nonzero(take)
        pc[rows[x], slot[x, y]] = cs[y]
        pi[rows[x], slot[x, y]] = cand[x, y]
        count[rows] = np.minimum(ok.sum(axis=1), keep)
        return cand

    every = np.arange(n)
    fill(every, np.arange(min(first, CAP)))
    short = every[count < keep]
    for s in range(0, len(short), 256):                                     # the rest walk up to the cap
        rows = short[s:s + 256]
        pc[rows], pi[rows] = -1, 0
        cand = fill(rows, np.arange(CAP))
        last[rows] = cand[:, CAP - 1]
    return count, pc, pi, last


def choose(count, pi, S, last, last_S, M):
    """(negs, score, failed) for pool M from the pools and their scores S float32 [n, keep] (None for M == 1)."""
    n = len(count)
    have = np.minimum(count, M)
    none = have == 0
    if M == 1:
        return np.where(none, last, pi[:, 0]), None, int(none.sum())
    inpool = np.arange(pi.shape[1])[None, :] < have[:, None]
    m = inpool & ~np.isnan(S)
    with np.errstate(invalid="ignore"):
        Sm = np.where(m, S, -np.inf)
        pick = np.argmax((Sm == Sm.max(axis=1, keepdims=True)) & m, axis=1)  # the first slot (smallest c) holding the greatest number
    pick = np.where(m.any(axis=1), pick, 0)                                 # all NaN: the smallest c
    rows = np.arange(n)
    negs = np.where(none, last, pi[rows, pick])
    score = np.where(none, last_S, S[rows, pick]).astype(np.float32)
    return negs, score, int(none.sum())


def scores(case, users, count, pi, last):
    """S float32 [n, keep] of the pooled candidates (NaN where there is none) and of candidate 4095 where the pool is empty"""
    users = np.asarray(users, dtype=np.int64)
    n, keep = pi.shape
    S = np.full((n, keep), np.nan, np.float32)
    x, y = np.nonzero(np.arange(keep)[None, :] < count[:, None])
    S[x, y] = chain(case["wu"][users[x]], case["wi"][pi[x, y]], "kernel")
    last_S = np.zeros(n, np.float32)
    z = np.nonzero(count == 0)[0]
    if len(z):
        last_S[z] = chain(case["wu"][users[z]], case["wi"][last[z]], "kernel")
    return S, last_S


# ---- the cases ----------------------------------------------------------------------------------------------------------

N_USERS, N_ROWS_U, N_ITEM, POP = 70, 72, 300, 257            # users of the CSR; rows of w_user; rows of w_item; len(item_all)
U_EMPTY, U_BUT3, U_BUT1, U_ALL, U_TINY, U_OUT = 0, 1, 2, 3, 4, 71       # U_OUT: inside w_user, outside the CSR -- an empty range
U_FAR = 10 ** 6                                              # outside everything: M == 1 only (no table is read)


def _tables(d, rng, item_all):
    wu = (rng.randn(N_ROWS_U, d) * 0.5).astype(np.float32)
    wi = (rng.randn(N_ITEM, d) * 0.5).astype(np.float32)
    ids = item_all[rng.permutation(len(item_all))]
    groups = ids[:36].reshape(6, 6)
    for g in groups:                                         # exact copies under several ids: ties, the earlier c must win
        wi[g[1:4]] = wi[g[0]]
        for k, sgn in ((4, 1), (5, -1)):                     # one ulp away
            y = wi[g[0]].copy()
            q = rng.randint(d)
            y[q] = np.nextafter(y[q], np.float32(sgn * np.inf))
            wi[g[k]] = y
    wi[ids[36], 3] = np.nan                                  # a NaN row
    wi[ids[37], d - 1] = np.nan
    tiny_items = ids[40:90]
    wi[tiny_items] *= np.float32(2.0 ** -70)                 # with the tiny users: subnormal scores
    tiny_users = np.array([U_TINY, 10, 11, 12, 13])
    wu[tiny_users] *= np.float32(2.0 ** -70)
    return wu, wi, dict(groups=groups, nan_items=ids[36:38], tiny_items=tiny_items, tiny_users=tiny_users)


def _csr(lists):
    ptr = np.zeros(N_USERS + 1, np.int64)
    items = []
    for u in range(N_USERS):
        it = np.unique(np.asarray(list(lists.get(u, ())), dtype=np.int64))
        ptr[u + 1] = ptr[u] + len(it)
        items.append(it)
    return ptr, np.concatenate(items).astype(np.int64)


def counts_cdf(item_all, items, alpha):
    """the three-line statement of popularity_cdf"""
    w = np.array([(items == i).sum() for i in item_all]).astype(np.float64) ** alpha
    cdf = np.cumsum(w) / np.cumsum(w)[-1]
    cdf[-1] = 1.0
    return cdf


def _build(name, d):
    rng = np.random.RandomState(1800 + d)
    item_all = np.sort(rng.permutation(N_ITEM)[:POP]).astype(np.int64)
    n = 4099 if name == "uniform" else 1031
    lists = {u: rng.permutation(N_ITEM)[:rng.randint(1, 41)] for u in range(4, N_USERS)}
    lists[U_BUT3] = item_all[3:]
    lists[U_BUT1] = np.delete(item_all, 100)
    lists[U_ALL] = item_all
    wu, wi, planted = _tables(d, rng, item_all)
    lists[U_TINY] = np.setdiff1d(item_all, planted["tiny_items"])      # a tiny user left with the tiny items: subnormal scores win
    cdf = None
    if name == "alpha075":
        col = item_all[np.minimum((rng.pareto(1.2, 20000) * 8).astype(np.int64), POP - 1)]      # skewed counts, some zero
        cdf = counts_cdf(item_all, col, 0.75)
    elif name == "flat":
        w = rng.rand(POP) * (rng.rand(POP) < 0.4)            # most entries have zero mass, the first and the last among them
        w[0], w[-1], w[5] = 0.0, 0.0, 1.0
        cdf = np.cumsum(w) / w.sum()
        cdf[-1] = 1.0
    elif name == "first":
        cdf = np.ones(POP, np.float64)
    elif name == "last":
        cdf = np.zeros(POP, np.float64)
        cdf[-1] = 1.0
    elif name == "pop1":
        item_all = item_all[7:8].copy()
        cdf = np.ones(1, np.float64)
        lists[U_BUT3], lists[U_BUT1] = [], []
        lists[U_ALL] = item_all
    if name in ("first", "last"):                            # the one item that is ever drawn: half of the plain users own it
        only = int(item_all[0] if name == "first" else item_all[-1])
        for u in range(4, N_USERS, 2):
            lists[u] = np.append(lists[u], only)
    ptr, items = _csr(lists)
    users = rng.randint(0, N_USERS, n).astype(np.int64)      # repeated users
    users[rng.permutation(n)[:40]] = U_OUT
    users[:4] = (U_EMPTY, U_BUT3, U_BUT1, U_ALL)
    users1 = users.copy()
    users1[users1 == U_OUT] = np.where(np.arange((users1 == U_OUT).sum()) % 2 == 0, U_FAR, U_OUT)
    return dict(name=name, d=d, n=n, item_all=item_all, user_ptr=ptr, user_items=items, cdf=cdf, wu=wu, wi=wi, users=users,
                users1=users1, planted=planted)


CASES = [("uniform", 32), ("uniform", 64), ("alpha075", 32), ("flat", 64), ("first", 32), ("last", 32), ("pop1", 32)]
CASE_IDS = ["%s-d%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def case(name, d):
    return _build(name, d)


def users_for(c, M):
    return c["users1"] if M == 1 else c["users"]


@functools.lru_cache(maxsize=None)
def _pooled(name, d, which, seed):
    c = case(name, d)
    users = c[which]
    count, pc, pi, last = pools(c, users, seed)
    S, last_S = scores(c, users, count, pi, last) if which == "users" else (None, None)
    return count, pc, pi, last, S, last_S


def walk(name, d, M, seed=SEED):
    """(negs int64 [n], score float32 [n] or None, failed) of case (name, d) with pool M: computed once, shared, read-only."""
    count, pc, pi, last, S, last_S = _pooled(name, d, "users1" if M == 1 else "users", seed)
    negs, score, failed = choose(count, pi, S, last, last_S, M)
    negs.setflags(write=False)
    if score is not None:
        score.setflags(write=False)
    return negs, score, failed


def pooled(name, d, M, seed=SEED):
    return _pooled(name, d, "users1" if M == 1 else "users", seed)
