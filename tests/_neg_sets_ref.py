"""Test-set negatives (sml_neg_sets, sml_host_neg_sets, sml_amd.prepare): the definition restated in plain Python, the cases,
and the property checker.

The restatement shares no code with the product: Python integers carry the 64-bit arithmetic, sets hold H(g) and the
accepted candidates, and the stream is walked row by row.  tests/test_neg_sets_host.py compares the host entry with it byte
for byte; the GPU tests compare the kernel with it.

The stream is the concatenation of the periods; row g (a global position) is (u, i).  C(g) = the items of rows 0..g, H(g) =
the items of user u in rows 0..g (both include row g).  Periods >= start get negatives: the first neg_num accepted candidates
of the row's own counter-based stream, where a candidate in H(g) or equal to an earlier accept is rejected."""
import functools

import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9e3779b97f4a7c15
CAP = 262144


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _row_stream(seed, g):
    return (seed & M64) ^ ((g * 0xd1342543de82ef95 + 0x632be59bd9b4e019) & M64)


def ref_negatives(stream, start, neg_num, seed):
    """stream: a list of int arrays [n_p, >= 2].  Returns ([int64 [n_p, 2 + neg_num] for p >= start], [failed rows per such
    period], the largest number of candidates any served row looked at, the number of rows that failed for eligibility)."""
    order, in_cat, hist = [], set(), {}
    outs, fails, most, ineligible = [], [], 0, 0
    g = 0
    for p, rows in enumerate(stream):
        out = np.full((len(rows), 2 + neg_num), -1, dtype=np.int64)
        failed = 0
        for r in range(len(rows)):
            u, i = int(rows[r][0]), int(rows[r][1])
            if i not in in_cat:
                in_cat.add(i)
                order.append(i)
            h = hist.setdefault(u, set())
            h.add(i)
            if p >= start:
                out[r, 0], out[r, 1] = u, i
                n_cat = len(order)
                got = []
                if n_cat - len(h) >= neg_num:
                    s0, taken, c = _row_stream(seed, g), set(), 0
                    while c < CAP and len(got) < neg_num:
                        z = _mix((s0 + (c + 1) * GAMMA) & M64)
                        cand = order[(z * n_cat) >> 64]
                        c += 1
                        if cand in h or cand in taken:
                            continue
                        taken.add(cand)
                        got.append(cand)
                    most = max(most, c)
                else:
                    ineligible += 1
                out[r, 2:2 + len(got)] = got
                failed += len(got) < neg_num
            g += 1
        if p >= start:
            outs.append(out)
            fails.append(failed)
    return outs, fails, most, ineligible


def check_rows(stream, start, out):
    """The three properties of the reference's output: each row of out (one array [n_p, 2 + neg_num] per period >= start)
    repeats its (user, item), and its negatives are distinct, a subset of C(g) and disjoint from H(g)."""
    assert len(out) == len(stream) - start, (len(out), len(stream), start)
    in_cat, hist = set(), {}
    for p, rows in enumerate(stream):
        rows = np.asarray(rows)
        if p >= start:
            o = np.asarray(out[p - start])
            assert o.ndim == 2 and o.shape[0] == rows.shape[0], (p, o.shape, rows.shape)
            assert np.array_equal(o[:, :2], rows[:, :2]), p
        for r in range(len(rows)):
            u, i = int(rows[r][0]), int(rows[r][1])
            in_cat.add(i)
            h = hist.setdefault(u, set())
            h.add(i)
            if p >= start:
                negs = [int(x) for x in o[r, 2:]]
                assert len(set(negs)) == len(negs), ("repeated negative", p, r)
                assert set(negs) <= in_cat, ("negative outside C(g)", p, r)
                assert not (set(negs) & h), ("negative in H(g)", p, r)
    return True


def build_stream(seed, periods, rows, users, items0, growth):
    """`periods` arrays int64 [rows, 2] (period 0: items0 more rows in front, one per initial item, so the catalogue starts
    at items0).  Each later-arriving item (growth per period) first appears at a random row INSIDE its period; the other rows
    draw uniformly from the catalogue so far, so (u, i) pairs repeat.  The users of period p come from the first
    ceil(users * (p + 2) / (periods + 1)) ids: new users keep arriving."""
    rng = np.random.RandomState(seed)
    out, n_cat = [], items0
    for p in range(periods):
        pool = min(users, -(-users * (p + 2) // (periods + 1)))
        new_at = set(rng.choice(rows, size=min(growth, rows), replace=False).tolist())
        u = rng.randint(0, pool, rows)
        it = np.empty(rows, np.int64)
        for r in range(rows):
            if r in new_at:
                it[r] = n_cat
                n_cat += 1
            else:
                it[r] = rng.randint(0, n_cat)
        per = np.stack([u.astype(np.int64), it], 1)
        if p == 0:
            head = np.stack([rng.randint(0, pool, items0).astype(np.int64), rng.permutation(items0).astype(np.int64)], 1)
            per = np.concatenate([head, per])
        out.append(per)
    return out, users, n_cat


# name -> ((seed, periods, rows, users, items0, growth), neg_num, start)
CASES = {
    "k999": ((1, 4, 257, 40, 1200, 40), 999, 2),          # the file format's width; 16+ rounds of 64 per row
    "k1": ((2, 3, 65, 10, 50, 5), 1, 1),                  # one negative: the first round decides
    "k64": ((3, 3, 130, 10, 90, 5), 64, 1),               # exactly one round's width; rows that are served beside rows that fail
    "k65tight": ((4, 3, 130, 10, 80, 3), 65, 1),          # one past the round; nearly every row short of eligible items
    "k63": ((5, 3, 64, 7, 100, 0), 63, 1),                # one short of the round; a fixed catalogue
    # the launch's other shapes: 1,025 .. 2,048 negatives run two waves per workgroup, above that one (the hash set grows)
    "k1100": ((6, 2, 9, 5, 1500, 3), 1100, 1),
    "k4096": ((7, 2, 5, 3, 4300, 2), 4096, 1),            # the largest neg_num; ~15,000 candidates per row
}
SEED = 2000


@functools.lru_cache(maxsize=None)
def case(name):
    """(stream, n_user, n_item, neg_num, start, outs, fails, most candidates, ineligible rows): computed once, shared."""
    args, neg_num, start = CASES[name]
    stream, n_user, n_item = build_stream(*args)
    outs, fails, most, inel = ref_negatives(stream, start, neg_num, SEED)
    for o in outs:
        o.setflags(write=False)
    return stream, n_user, n_item, neg_num, start, outs, fails, most, inel


@functools.lru_cache(maxsize=None)
def exact_case():
    """One period-1 row with |C(g) \\ H(g)| == neg_num exactly: 12 items, user 0 holds 4 of them after its row, neg_num 8."""
    p0 = np.array([[1, k] for k in range(12)] + [[0, 0], [0, 5], [0, 7]], dtype=np.int64)
    p1 = np.array([[0, 9], [2, 3]], dtype=np.int64)
    stream, neg_num, start = [p0, p1], 8, 1
    outs, fails, most, inel = ref_negatives(stream, start, neg_num, SEED)
    return stream, 3, 12, neg_num, start, outs, fails


def timeline_arrays(stream, n_user, n_item):
    """(order int32, n_cat int32 [total], h_off int64 [n_user + 1], h_items int32, h_since int32) built with dicts and
    loops: what sml_amd.prepare.Timeline.host() must return."""
    order, in_cat, n_cat, first = [], set(), [], {}
    g = 0
    for rows in stream:
        for r in range(len(rows)):
            u, i = int(rows[r][0]), int(rows[r][1])
            if i not in in_cat:
                in_cat.add(i)
                order.append(i)
            n_cat.append(len(order))
            first.setdefault((u, i), g)
            g += 1
    keys = sorted(first)
    h_off = np.zeros(n_user + 1, np.int64)
    for u, _ in keys:
        h_off[u + 1] += 1
    h_off = np.cumsum(h_off).astype(np.int64)
    return (np.array(order, np.int32), np.array(n_cat, np.int32), h_off, np.array([k[1] for k in keys], np.int32),
            np.array([first[k] for k in keys], np.int32))
