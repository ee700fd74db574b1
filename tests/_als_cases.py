"""Seeded cases of the fold-in (sml_gram / sml_als_solve, include/sml_hip.h "FOLD-IN"), shared by test_als_host.py and
test_als_gpu.py, with a restatement of the definition to compare the host walks against.  Every comparison of rows, Gram
matrices and status made on them is byte equality.

U = 40 rows are solved against a table of I = 420 rows, uniform in [-0.5, 0.5).  The set sizes are 0, 1, 2, 63 / 64 / 65 (around
the width), 200, 420 (the whole table) and 32 sizes in 1 .. 39 (the light rows that are the common case).  The Gram table has
2,500 rows, so n_rows can sit on, before and after the chunk boundary of 1,024.

The restatement runs the additions in numpy float64, one member at a time (an elementwise add rounds once, and the product of
two widened fp32 / fp16 values is exact in float64), and every fma through exact rationals, which round once."""
import functools
from fractions import Fraction

import numpy as np

U, I = 40, 420
PAIRS = (("fp32", 32), ("fp32", 64), ("fp16", 32), ("fp16", 64))
PARAMS = ((0.1, 0.1), (1e-3, 0.0), (1.0, 1.0))               # (reg, alpha0)
SIZES = (0, 1, 2, 63, 64, 65, 200, 420) + tuple(1 + (7 * q + 3) % 39 for q in range(32))
RESTATED_64 = (0, 1, 5, 7)                                   # the rows restated at d = 64: sizes 0, 1, 65 and 420
GRAM_ROWS = 2500
GRAM_N = (1, 1023, 1024, 1025, 2500)
CHUNK = 1024
assert len(SIZES) == U and [SIZES[r] for r in RESTATED_64] == [0, 1, 65, 420] and all(1 <= s <= 39 for s in SIZES[8:])


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


@functools.lru_cache(maxsize=None)
def case(dtype, d):
    """other [I, d] and the prior content of out [U, d] in the element type, the sets, their CSR, and the Gram table [2500, d]."""
    rng = np.random.RandomState(2200 + d + (7 if dtype == "fp16" else 0))
    t = np_type(dtype)
    other = (rng.rand(I, d) - 0.5).astype(t)
    out0 = (rng.rand(U, d) - 0.5).astype(t)
    sets = [np.sort(rng.choice(I, size=s, replace=False)).astype(np.int64) for s in SIZES]
    gram_tab = (rng.rand(GRAM_ROWS, d) - 0.5).astype(t)
    return dict(dtype=dtype, d=d, other=other, out0=out0, sets=sets, csr=csr(sets), gram_tab=gram_tab)


# ---- the library's host walks --------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data


def host_gram(w, d, n_rows=None):
    from sml_amd import _lib
    w = np.ascontiguousarray(w)
    g = np.full((d, d), 7.0, np.float64)
    _lib.check(_lib.load().sml_host_gram(_p(w), w.itemsize, d, w.shape[0] if n_rows is None else n_rows, _p(g)), "sml_host_gram")
    return g


def host_solve(other, d, gram, reg, alpha0, sets_csr, rows, out):
    """(a copy of `out` with the named rows solved, status int32 [n]) of sml_host_als_solve; rows None: every row of out."""
    from sml_amd import _lib
    other, out = np.ascontiguousarray(other), np.array(out, copy=True)
    off, items = (None, None) if sets_csr is None else (np.ascontiguousarray(sets_csr[0], np.int64),
                                                        np.ascontiguousarray(np.concatenate([sets_csr[1], [0]]), np.int32))
    rows = None if rows is None else np.ascontiguousarray(rows, np.int64)
    n = out.shape[0] if rows is None else len(rows)
    status = np.full(n, 77, np.int32)
    gram = None if gram is None else np.ascontiguousarray(gram, np.float64)
    _lib.check(_lib.load().sml_host_als_solve(_p(other), other.itemsize, d, other.shape[0], _p(gram), float(alpha0), float(reg), _p(off),
                                              _p(items), _p(rows), n, _p(out), out.shape[0], _p(status)), "sml_host_als_solve")
    return out, status


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once (finite arguments)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def ref_gram(w, n_rows):
    y = np.asarray(w[:n_rows], np.float64)
    d = y.shape[1]
    g = np.zeros((d, d), np.float64)
    for r0 in range(0, n_rows, CHUNK):
        part = np.zeros((d, d), np.float64)
        for i in range(r0, min(r0 + CHUNK, n_rows)):
            part = part + np.multiply.outer(y[i], y[i])            # exact products, one rounding per add
        g = g + part
    return g


def ref_row(other, gram, reg, alpha0, members):
    """(status, p as d Python floats or None) of one row, by the header's text."""
    d = other.shape[1]
    if len(members) == 0:
        return 1, [0.0] * d
    y = np.asarray(other, np.float64)
    A = np.array([[fma(alpha0, float(gram[a, b]), reg if a == b else 0.0) if b <= a else 0.0 for b in range(d)] for a in range(d)])
    rhs = np.zeros(d, np.float64)
    for m in members:
        A = A + np.multiply.outer(y[m], y[m])
        rhs = rhs + y[m]
    A, rhs = A.tolist(), rhs.tolist()
    L = [[0.0] * d for _ in range(d)]
    D = [0.0] * d
    for j in range(d):
        v = [L[j][k] * D[k] for k in range(j)]
        dj = A[j][j]
        for k in range(j):
            dj = fma(-L[j][k], v[k], dj)
        if not dj > 0:
            return 2, None
        D[j] = dj
        for i in range(j + 1, d):
            t = A[i][j]
            Li = L[i]
            for k in range(j):
                t = fma(-Li[k], v[k], t)
            Li[j] = t / dj
    z = [0.0] * d
    for j in range(d):
        t = rhs[j]
        for k in range(j):
            t = fma(-L[j][k], z[k], t)
        z[j] = t
    p = [0.0] * d
    for j in range(d - 1, -1, -1):
        t = z[j] / D[j]
        for k in range(j + 1, d):
            t = fma(-L[k][j], p[k], t)
        p[j] = t
    if not all(np.isfinite(p)):
        return 2, None
    return 0, p


@functools.lru_cache(maxsize=None)
def ref_rows(dtype, d, reg, alpha0):
    """{row: (status, the row in the element type)} of the restated rows of case(dtype, d): all of them at d = 32, RESTATED_64 at
    d = 64.  The Gram matrix is the host walk's (test_als_host.py holds it to ref_gram)."""
    c = case(dtype, d)
    g = host_gram(c["other"], d)
    out = {}
    for r in (range(U) if d == 32 else RESTATED_64):
        st, p = ref_row(c["other"], g, reg, alpha0, c["sets"][r])
        out[r] = (st, None if p is None else np.asarray(p, np.float64).astype(np.float32).astype(np_type(dtype)))
    return out


def same_bytes(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.view(np.uint8), want.view(np.uint8)
    assert (g == w).all(), (what, np.argwhere(got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(got.shape + (-1,)))[:5].tolist())
