"""Exact numpy references for per-user ranking of held-out sets (sml_user_rank / sml_user_metrics, include/sml_hip.h).

Scores are the kernels' fp32 chain (tests/_fp32_chain.py, score_chain), so `above` and `pos` are compared exactly.
ref_user_rank sorts each user's eligible items once in top-K order (score descending, then id ascending) and reads
`pos` as an index and `above` as a binary search; brute_user_rank counts item by item and exists to check it.
ref_user_metrics sums dcg / ap in float64 in ascending pos.
"""
import numpy as np

from _fp32_chain import score_chain


def _seen_of(seen, u):
    if seen is None:
        return np.zeros(0, np.int64)
    off, items = (np.asarray(t) for t in seen)
    return items[off[u]:off[u + 1]].astype(np.int64)


def user_scores(wu, wi, users, chunk=64):
    """float32 [n, n_item]: the kernels' S(users[x], i) for every item."""
    users = np.asarray(users, dtype=np.int64)
    out = np.empty((len(users), wi.shape[0]), np.float32)
    for c in range(0, len(users), chunk):
        out[c:c + chunk] = score_chain(wu[users[c:c + chunk]], wi)
    return out


def ref_user_rank(wu, wi, users, pos_off, pos_items, seen=None, S=None):
    """(above int64 [n_pos], pos int64 [n_pos]) under the header's rules."""
    users = np.asarray(users, dtype=np.int64)
    pos_off = np.asarray(pos_off, dtype=np.int64)
    pos_items = np.asarray(pos_items, dtype=np.int64)
    S = user_scores(wu, wi, users) if S is None else S
    n_item = wi.shape[0]
    above = np.zeros(len(pos_items), np.int64)
    pos = np.full(len(pos_items), -1, np.int64)
    for x, u in enumerate(users):
        lo, hi = pos_off[x], pos_off[x + 1]
        if lo == hi:
            continue
        s = S[x]
        elig = ~np.isnan(s)
        elig[_seen_of(seen, u)] = False
        ids = np.nonzero(elig)[0]
        order = ids[np.lexsort((ids, -s[ids].astype(np.float64)))]
        place = np.full(n_item, -1, np.int64)
        place[order] = np.arange(len(order))
        desc = -s[order].astype(np.float64)              # ascending
        p = pos_items[lo:hi]
        t = s[p].astype(np.float64)
        ab = np.searchsorted(desc, -t, side="left")       # #{eligible: S > t}
        above[lo:hi] = np.where(np.isnan(t), 0, ab)
        pos[lo:hi] = place[p]
    return above, pos


def brute_user_rank(wu, wi, users, pos_off, pos_items, seen=None, S=None):
    """The definitions of include/sml_hip.h, one (user, held-out item, item) triple at a time."""
    S = user_scores(wu, wi, users) if S is None else S
    above, pos = [], []
    for x, u in enumerate(users):
        excl = set(_seen_of(seen, u).tolist())
        s = S[x]
        elig = [i for i in range(wi.shape[0]) if i not in excl and not np.isnan(s[i])]
        for p in pos_items[pos_off[x]:pos_off[x + 1]]:
            above.append(sum(1 for i in elig if i != p and s[i] > s[p]))
            if p in excl or np.isnan(s[p]):
                pos.append(-1)
            else:
                pos.append(sum(1 for i in elig if s[i] > s[p] or (s[i] == s[p] and i < p)))
    return np.array(above, np.int64), np.array(pos, np.int64)


def ref_user_metrics(pos, pos_off, ks):
    """(hits int64 [n, n_k], dcg float64, ap float64, first int64 [n]) from pos.  hits counts every entry; dcg / ap take
    each non-negative pos value once (as the header states for a value repeated inside a range)."""
    pos = np.asarray(pos, dtype=np.int64)
    pos_off = np.asarray(pos_off, dtype=np.int64)
    n = len(pos_off) - 1
    hits = np.zeros((n, len(ks)), np.int64)
    dcg = np.zeros((n, len(ks)))
    ap = np.zeros((n, len(ks)))
    first = np.full(n, -1, np.int64)
    for x in range(n):
        p = np.sort(pos[pos_off[x]:pos_off[x + 1]])
        p = p[p >= 0]
        if len(p):
            first[x] = p[0]
        for q, K in enumerate(ks):
            hits[x, q] = int((p < K).sum())
            h = np.unique(p[p < K])
            dcg[x, q] = np.sum(1.0 / np.log2(h + 2.0))
            ap[x, q] = np.sum(np.arange(1, len(h) + 1) / (h + 1.0))
    return hits, dcg, ap, first


def held_out_csr(n_user, lists):
    """(users, pos_off, pos_items) for {user: items} in the given user order (a user may be listed twice through a
    list of (user, items) pairs instead of a dict)."""
    pairs = lists.items() if isinstance(lists, dict) else lists
    users, off, items = [], [0], []
    for u, it in pairs:
        it = np.unique(np.asarray(list(it), dtype=np.int64))
        users.append(u)
        items.append(it)
        off.append(off[-1] + len(it))
    return (np.array(users, np.int64), np.array(off, np.int64),
            np.concatenate(items).astype(np.int32) if items else np.zeros(0, np.int32))
