"""Seeded cases of the graph propagation (sml_graph_propagate, include/sml_hip.h "PROPAGATION"), shared by test_graph_host.py and
test_graph_gpu.py, with a restatement of the definition to compare the host walk against.  Every comparison of rows made on them
is byte equality.

N = 48 output rows gather from a table of n_src() rows (4,096, or just enough for the split threshold's sizes).  The planted set
sizes are 0, 1, 7 / 8 / 9 (around the strand count), 255 / 256 / 257, 511 / 512 / 513, 2 * 256 + 3 (around the segment), 3,000,
and S * 256 - 1, S * 256, S * 256 + 1 for S = sml_graph_split_from(), clipped to n_src; the other rows are light (1 .. 40 members),
the common case.  Members and tables are random; a and b are random in [0.25, 1.25) or absent.

The restatement runs in numpy float32, vectorised over the dimension.  An fmaf is emulated in float64: the product of two floats
is exact there, the sum is rounded to odd (from the exact error of the float64 add), and the one rounding to float32 that follows
is then the correctly rounded fused result."""
import functools

import numpy as np

N = 48
SEG, STRANDS = 256, 8
PAIRS = tuple((t, d) for t in ("fp32", "fp16") for d in (32, 64, 128))
F32, F64 = np.float32, np.float64


def split_from():
    from sml_amd import _lib
    return int(_lib.load().sml_graph_split_from())


def n_src():
    return max(4096, split_from() * SEG)


def sizes():
    s, cap = split_from(), n_src()
    planted = [0, 1, 7, 8, 9, 255, 256, 257, 511, 512, 513, 2 * SEG + 3, 3000] + [min(cap, s * SEG + k) for k in (-1, 0, 1)]
    return tuple(planted) + tuple(1 + (7 * q + 3) % 40 for q in range(N - len(planted)))


def np_type(dtype):
    return np.float32 if dtype == "fp32" else np.float16


def csr(sets):
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=off[1:])
    items = np.concatenate([np.asarray(s, np.int64) for s in sets]).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return off, items


def transpose(sets, n_other):
    """The other side's sets of a list of ascending id lists, in numpy."""
    out = [[] for _ in range(n_other)]
    for u, s in enumerate(sets):
        for i in s:
            out[int(i)].append(u)
    return [np.asarray(s, np.int64) for s in out]


def degree_scale(sets):
    """deg^-1/2 in float64 rounded once to float32, 0 where the degree is 0."""
    deg = np.array([len(s) for s in sets], np.float64)
    return np.where(deg > 0, np.maximum(deg, 1.0) ** -0.5, 0.0).astype(np.float32)


ROWS = np.array([(17 * x + 5) % N for x in range(N)] + [3], np.int64)          # a permutation of 0 .. 47, then row 3 again
assert sorted(ROWS[:N].tolist()) == list(range(N))


@functools.lru_cache(maxsize=None)
def members():
    rng = np.random.RandomState(2400)
    return [np.sort(rng.choice(n_src(), size=s, replace=False)).astype(np.int64) for s in sizes()]


@functools.lru_cache(maxsize=None)
def case(dtype, d):
    """src [n_src, d] in the element type, the sets and their CSR, a [N] and b [n_src]."""
    rng = np.random.RandomState(2400 + d + (7 if dtype == "fp16" else 0))
    src = (rng.rand(n_src(), d) - 0.5).astype(np_type(dtype))
    a = (rng.rand(N) + 0.25).astype(np.float32)
    b = (rng.rand(n_src()) + 0.25).astype(np.float32)
    sets = members()
    return dict(dtype=dtype, d=d, src=src, sets=sets, csr=csr(sets), a=a, b=b)


# ---- the library's host walk ---------------------------------------------------------------------------------------------------
def _p(x):
    return None if x is None else x.ctypes.data


def host_propagate(src, d, sets_csr, rows=None, a=None, b=None, n=None):
    """float32 [n, d] of sml_host_graph_propagate; rows None: rows 0 .. n - 1 (n: every row of the set)."""
    from sml_amd import _lib
    src = np.ascontiguousarray(src)
    off, items = (None, None) if sets_csr is None else (np.ascontiguousarray(sets_csr[0], np.int64),
                                                        np.ascontiguousarray(np.concatenate([sets_csr[1], [0]]), np.int32))
    rows = None if rows is None else np.ascontiguousarray(rows, np.int64)
    n = (len(off) - 1 if n is None else n) if rows is None else len(rows)
    a = None if a is None else np.ascontiguousarray(a, np.float32)
    b = None if b is None else np.ascontiguousarray(b, np.float32)
    out = np.full((n, d), 7.0, np.float32)
    _lib.check(_lib.load().sml_host_graph_propagate(_p(src), src.itemsize, d, src.shape[0], _p(off), _p(items), _p(rows), n, _p(a), _p(b),
                                                    _p(out)), "sml_host_graph_propagate")
    return out


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def fmaf(b, v, acc):
    """float32(b * v + acc), rounded once, for finite float32 arrays (b may be a scalar)."""
    p = np.asarray(b, F32).astype(F64) * np.asarray(v, F32).astype(F64)           # exact: 24 + 24 bits
    c = np.asarray(acc, F32).astype(F64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                                                 # the add's exact error (two-sum)
    bits = s.view(np.int64).copy()
    inexact = err != 0
    toward = inexact & ((err > 0) != (s > 0))                                     # the true sum is smaller in magnitude than s
    bits = np.where(toward, bits - 1, bits)                                       # truncate ...
    bits = np.where(inexact, bits | 1, bits)                                      # ... and keep what was lost as a sticky last bit
    return bits.view(F64).astype(F32)


def ref_row(src, b, mem, ar):
    """out[x] of one row by the header's text: float32 [d]."""
    d = src.shape[1]
    tot = np.zeros(d, F32)
    for c0 in range(0, len(mem), SEG):
        acc = [np.zeros(d, F32) for _ in range(STRANDS)]
        for p in range(c0, min(c0 + SEG, len(mem))):
            m = mem[p]
            acc[p % STRANDS] = fmaf(F32(1.0) if b is None else b[m], src[m].astype(F32), acc[p % STRANDS])
        u = [acc[j] + acc[j + 4] for j in range(4)]
        v = [u[j] + u[j + 2] for j in range(2)]
        tot = tot + (v[0] + v[1])
    return (F32(1.0) if ar is None else F32(ar)) * tot


@functools.lru_cache(maxsize=None)
def ref_rows(dtype, d, scaled):
    """The restated rows of case(dtype, d), float32 [N, d]; scaled: with a and b, else both absent."""
    c = case(dtype, d)
    return np.stack([ref_row(c["src"], c["b"] if scaled else None, c["sets"][r], c["a"][r] if scaled else None) for r in range(N)])


@functools.lru_cache(maxsize=None)
def host_rows(dtype, d, scaled):
    """The host walk of case(dtype, d) over rows 0 .. N - 1: what the device tests compare against."""
    c = case(dtype, d)
    return host_propagate(c["src"], d, c["csr"], None, c["a"] if scaled else None, c["b"] if scaled else None)


def same_bytes(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got.view(np.uint8) != want.view(np.uint8)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:5].tolist())


# ---- a planted-cluster set for the model tests ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clusters(n_user=400, n_item=800, k=8, per_user=20):
    """k user clusters taking their own k item clusters: user u of cluster u % k holds per_user items of item cluster u % k."""
    rng = np.random.RandomState(2424)
    own = [np.arange(n_item)[np.arange(n_item) % k == c] for c in range(k)]
    return [np.sort(rng.choice(own[u % k], size=per_user, replace=False)).astype(np.int64) for u in range(n_user)]
