"""Exact fp32 references for full-catalogue retrieval (sml_full_rank / sml_topk_items, include/sml_hip.h).

The kernels score (u, i) as ONE fmaf chain in a fixed order (retrieval.hip, score_chain / tile_scores):

    acc = 0;  for s in 0 .. D/2 - 1:  acc = fma(x[s], u[s], acc);  acc = fma(x[s + D/2], u[s + D/2], acc)

fma32 is a correctly rounded fp32 fused multiply-add in numpy: the product of two floats is exact in float64 (24 + 24
bits), the sum with the addend is taken in float64 with its exact error recovered by TwoSum, and the float64 result is
rounded to odd (a nonzero error on an even last bit steps it one ulp toward the error).  Since 53 >= 2 * 24 + 2, the
final cast to float32 then rounds correctly, subnormal results included.

ref_full_rank / ref_topk are exact under the header's rules at any catalogue size: float64 scores come first, and every
fp32 chain is bounded by |chain - s64| <= 2 gamma_d sum |x_i u_i| + d 2^-148 (the standard fma inner-product bound, with
the float64 error and underflow inside the slack); only items whose bound reaches the threshold or the K-th score are
emulated exactly.  order="kernel" is the kernels' chain; "sequential" (dims 0 .. D-1), "swapped" (dims D/2, 0, D/2 + 1,
1, ...) and "f64" (the float64 score rounded once) exist so the tests can show that an exact comparison tells them
apart.
"""
import numpy as np
import torch


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c), elementwise (numpy broadcasting); inf / NaN as IEEE 754 defines."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                              # exact
        s = p + c
        bc = s - p
        err = (p - (s - bc)) + (c - bc)        # TwoSum: s + err == p + c exactly
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    if np.any(fix):
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def chain(u, x, order="kernel"):
    """fp32 scores of row pairs: u, x float32 [..., D] (broadcast) -> float32 [...]."""
    u = np.asarray(u, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    D = u.shape[-1]
    if order == "f64":
        return np.einsum("...d,...d->...", u.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    if order == "kernel":
        dims = [q for s in range(D // 2) for q in (s, s + D // 2)]
    elif order == "sequential":
        dims = range(D)
    elif order == "swapped":                   # the kernel's pairs with the lane halves exchanged
        dims = [q for s in range(D // 2) for q in (s + D // 2, s)]
    else:
        raise ValueError(order)
    acc = np.zeros(np.broadcast_shapes(u.shape[:-1], x.shape[:-1]), dtype=np.float32)
    for q in dims:
        acc = fma32(x[..., q], u[..., q], acc)
    return acc


def score_chain(U, X, order="kernel"):
    """The full score matrix S[a, b] = chain(U[a], X[b]) (small tables only)."""
    U, X = np.asarray(U, dtype=np.float32), np.asarray(X, dtype=np.float32)
    return chain(U[:, None, :], X[None, :, :], order)


# ---- the float64 filter ---------------------------------------------------------------------------------------------

def _seen_pairs(seen, users):
    """(x, item) int64 arrays: the Seen items of users[x] for every x (seen = (off, items) CSR or None)."""
    if seen is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    off, items = (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in seen)
    lo, hi = off[users], off[users + 1]
    cnt = hi - lo
    xs = np.repeat(np.arange(len(users)), cnt)
    idx = np.repeat(lo - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())
    return xs.astype(np.int64), items[idx].astype(np.int64)


class _Scorer(object):
    """float64 scores and chain bounds of a set of user rows against item chunks, on `device`."""

    def __init__(self, wu, wi, users, device, chunk):
        self.wi = wi if torch.is_tensor(wi) else torch.from_numpy(np.ascontiguousarray(wi))
        wu_t = wu if torch.is_tensor(wu) else torch.from_numpy(np.ascontiguousarray(wu))
        self.dev = torch.device(device)
        ut = torch.as_tensor(users, dtype=torch.int64, device=wu_t.device)
        self.u32 = wu_t[ut].cpu().numpy()                 # float32 [n, D] for the exact chains
        self.u64 = torch.from_numpy(self.u32).to(self.dev, torch.float64)
        self.ua = self.u64.abs()
        self.n_item, self.D = self.wi.shape
        self.gamma = 2.0 * self.D * 2.0 ** -24 / (1 - self.D * 2.0 ** -24)
        self.slack = self.D * 2.0 ** -148
        self.chunk = chunk

    def chunks(self):
        for c0 in range(0, self.n_item, self.chunk):
            c1 = min(self.n_item, c0 + self.chunk)
            x = self.wi[c0:c1].to(self.dev, torch.float64)
            s = self.u64 @ x.T
            b = self.gamma * (self.ua @ x.abs().T) + self.slack
            bad = ~torch.isfinite(s) | ~torch.isfinite(b)
            lo = torch.where(bad, torch.full_like(s, -np.inf), s - b)
            hi = torch.where(bad, torch.full_like(s, np.inf), s + b)
            yield c0, c1, lo, hi

    def exact(self, xs, items, order):
        if len(xs) == 0:
            return np.zeros(0, np.float32)
        it = torch.as_tensor(items, dtype=torch.int64, device=self.wi.device)
        return chain(self.u32[xs], self.wi[it].cpu().numpy(), order)

    def mask(self, excl_x, excl_i, c0, c1, shape):
        """True where (x, c0 + j) is excluded."""
        m = torch.zeros(shape, dtype=torch.bool, device=self.dev)
        sel = (excl_i >= c0) & (excl_i < c1)
        if sel.any():
            m[torch.from_numpy(excl_x[sel]).to(self.dev), torch.from_numpy(excl_i[sel] - c0).to(self.dev)] = True
        return m


def ref_full_rank(wu, wi, rows, seen=None, order="kernel", device="cpu", chunk=1 << 16):
    """int64 [n]: #{i in [0, n_item): i != p, i not in Seen(u), S(u, i) > S(u, p)} under the fp32 chain `order`
    (strictly greater, NaN never above; a NaN positive ranks 0).  wu / wi: float32 numpy arrays or tensors (any device);
    rows int [n, >= 2]; seen = (seen_off, seen_items) or None."""
    rows = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows).astype(np.int64)
    users, pos = rows[:, 0], rows[:, 1]
    sc = _Scorer(wu, wi, users, device, chunk)
    n = len(users)
    thr = sc.exact(np.arange(n), pos, order)
    ex_x, ex_i = _seen_pairs(seen, users)
    ex_x, ex_i = np.concatenate([ex_x, np.arange(n)]), np.concatenate([ex_i, pos])     # p never counts against itself
    thr_t = torch.from_numpy(np.where(np.isnan(thr), np.inf, thr).astype(np.float64)).to(sc.dev)[:, None]
    rank = np.zeros(n, np.int64)
    for c0, c1, lo, hi in sc.chunks():
        ok = ~sc.mask(ex_x, ex_i, c0, c1, lo.shape)
        rank += ((lo > thr_t) & ok).sum(1).cpu().numpy()
        unsure = ok & ~(lo > thr_t) & ~(hi <= thr_t)
        ux, ui = (t.cpu().numpy() for t in torch.nonzero(unsure, as_tuple=True))
        ui = ui + c0
        np.add.at(rank, ux, sc.exact(ux, ui, order) > thr[ux])
    rank[np.isnan(thr)] = 0
    return rank


def ref_topk(wu, wi, users, k, seen=None, order="kernel", device="cpu", chunk=1 << 16):
    """(int64 items [n, k], float32 scores [n, k]): the k eligible items of each user (not in Seen, score not NaN),
    score descending then id ascending, padded with (-1, -inf)."""
    users = np.asarray(users.cpu() if torch.is_tensor(users) else users).astype(np.int64).reshape(-1)
    sc = _Scorer(wu, wi, users, device, chunk)
    n = len(users)
    ex_x, ex_i = _seen_pairs(seen, users)
    # pass 1: T[x] = the k-th largest lower bound among eligible items (every item whose upper bound is below it has
    # k eligible items strictly better than itself)
    best = torch.full((n, 0), -np.inf, dtype=torch.float64, device=sc.dev)
    for c0, c1, lo, hi in sc.chunks():
        lo = lo.masked_fill(sc.mask(ex_x, ex_i, c0, c1, lo.shape), -np.inf)
        both = torch.cat([best, lo], 1)
        best = torch.topk(both, min(k, both.shape[1]), dim=1).values
    T = best[:, -1:] if best.shape[1] == k else torch.full((n, 1), -np.inf, dtype=torch.float64, device=sc.dev)
    # pass 2: the candidates, scored exactly
    cx, ci = [], []
    for c0, c1, lo, hi in sc.chunks():
        cand = ~sc.mask(ex_x, ex_i, c0, c1, lo.shape) & ~(hi < T)
        x, i = (t.cpu().numpy() for t in torch.nonzero(cand, as_tuple=True))
        cx.append(x)
        ci.append(i + c0)
    cx, ci = np.concatenate(cx), np.concatenate(ci)
    cs = sc.exact(cx, ci, order)
    keep = ~np.isnan(cs)
    cx, ci, cs = cx[keep], ci[keep], cs[keep]
    o = np.lexsort((ci, -cs.astype(np.float64), cx))
    cx, ci, cs = cx[o], ci[o], cs[o]
    items = np.full((n, k), -1, np.int64)
    scores = np.full((n, k), -np.inf, np.float32)
    start = np.searchsorted(cx, np.arange(n + 1))
    for x in range(n):
        m = min(k, start[x + 1] - start[x])
        items[x, :m] = ci[start[x]:start[x] + m]
        scores[x, :m] = cs[start[x]:start[x] + m]
    return items, scores


# ---- the launch planner of retrieval.hip, mirrored (so tests can assert which geometry a shape reaches) -------------

RT = 32


def plan_slices(groups, n_item, target_blocks, max_mult):
    n_tiles = (n_item + RT - 1) // RT
    m = max(1, (target_blocks + 8 * groups - 1) // (8 * groups))
    m = min(m, max_mult)
    while m > 1 and n_tiles // (8 * m) < 16:
        m -= 1
    return 8 * m, (n_tiles + 8 * m - 1) // (8 * m)


def topk_waves(k):
    return min(4, 65536 // (2 * k * RT * 4))


def rank_plan(n, n_item):
    """(slices, slice_tiles, empty slices) of sml_full_rank."""
    s, st = plan_slices((n + RT * 4 - 1) // (RT * 4), n_item, 8192, 64)
    return s, st, _empty(s, st, n_item)


def topk_plan(n, k, n_item):
    """(waves per block, slices, slice_tiles, empty slices) of sml_topk_items."""
    w = topk_waves(k)
    s, st = plan_slices((n + RT * w - 1) // (RT * w), n_item, 2048, 4)
    return w, s, st, _empty(s, st, n_item)


def _empty(slices, slice_tiles, n_item):
    n_tiles = (n_item + RT - 1) // RT
    return sum(1 for q in range(slices) if q * slice_tiles >= n_tiles)


# ---- seeded cases the GPU tests run and the host tests inspect ------------------------------------------------------

def seen_csr(n_user, n_item, lists):
    """(seen_off int64, seen_items int32) from {user: iterable of items}."""
    off = np.zeros(n_user + 1, np.int64)
    items = []
    for u in range(n_user):
        it = np.unique(np.asarray(list(lists.get(u, ())), dtype=np.int64))
        off[u + 1] = off[u] + len(it)
        items.append(it)
    return off, np.concatenate(items).astype(np.int32) if items else np.zeros(0, np.int32)


def random_case(d, seed=0, U=300, I=4099, n=256):
    """randn tables, random rows (u, p) and users, up to 200 Seen items per user."""
    rng = np.random.RandomState(seed)
    wu = rng.randn(U, d).astype(np.float32)
    wi = rng.randn(I, d).astype(np.float32)
    rows = np.stack([rng.randint(0, U, size=n), rng.randint(0, I, size=n)], 1).astype(np.int64)
    users = rng.permutation(U)[:n]
    seen = {u: rng.choice(I, size=rng.randint(0, 200), replace=False) for u in range(U)}
    return dict(wu=wu, wi=wi, rows=rows, users=users, seen=seen_csr(U, I, seen), rng=rng)


def near_tie_case(d, seed=0, ks=(1, 20, 128)):
    """random_case with near-ties planted against the positives and against the k-th entries of the lists:

    - exact copies of p's item row under other ids (a tie: never counted, ordered by id in the lists);
    - copies with one coordinate moved by +-1 ulp;
    - copies with dims permuted among coordinates where the user's row holds equal values, so the exact score is the
      positive's and only the rounding of the chain tells them apart (those users' rows are built with repeated values);
    - copies of a user's k-th best item in other item slices (the merge breaks a non-dyadic tie by id across slices);
    - users whose scores are all fp32 subnormals (the item table is scaled by 2^-70, those user rows too).
    """
    c = random_case(d, seed)
    rng, wu, wi, rows, users = c["rng"], c["wu"], c["wi"], c["rows"], c["users"]
    U, I = wu.shape[0], wi.shape[0]
    wi *= np.float32(2.0 ** -70)
    tiny = rows[-16:, 0]
    wu[tiny] *= np.float32(2.0 ** -70)
    # rows 0..95: users with repeated values; their positives get planted copies
    planted = rows[:96]
    for u in np.unique(planted[:, 0]):
        if u in tiny:
            continue
        half = rng.randn(d // 2).astype(np.float32)
        wu[u] = np.concatenate([half, half])[rng.permutation(d)]
    taken = set(rows[:, 1].tolist())
    free = [i for i in rng.permutation(I) if i not in taken]
    for r, (u, p) in enumerate(planted):
        x = wi[p].copy()
        pairs = {}
        for q in range(d):
            pairs.setdefault(wu[u, q], []).append(q)
        swaps = [g for g in pairs.values() if len(g) == 2]
        for _ in range(2):                                     # exact copies
            wi[free.pop()] = x
        for sgn in (1, -1):                                    # one coordinate one ulp away
            y = x.copy()
            q = rng.randint(d)
            y[q] = np.nextafter(y[q], np.float32(sgn * np.inf))
            wi[free.pop()] = y
        for _ in range(4):                                     # same exact score, other rounding
            y = x.copy()
            for a, b in swaps:
                if rng.rand() < 0.5:
                    y[a], y[b] = y[b], y[a]
            wi[free.pop()] = y
    # the k-th best item of some list users, copied into other slices
    pick = users[:48]
    for j, u in enumerate(pick):
        k = ks[j % len(ks)]
        it, _ = ref_topk(wu, wi, [u], k, c["seen"])
        kth = it[0, -1]
        if kth < 0:
            continue
        for q in range(3):
            dst = free.pop()
            wi[dst] = wi[kth]
    c.update(tiny=tiny, planted=planted, pick=pick)
    return c
