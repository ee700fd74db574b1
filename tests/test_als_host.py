"""The fold-in, the parts that need no GPU: the C ABI surface, sml_host_gram and sml_host_als_solve -- the definitions of sml_gram
and sml_als_solve as single-threaded walks over host memory -- against a restatement of the header's text (byte equality), the
status codes, the rows a call may touch, the fp16 identity, every refusal of the host entry points, closeness to a float64
numpy solve, the objective's Gram identity and the monotone fall of the objective under alternating half-steps."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _als_cases as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sml_gram_scratch_bytes": 2, "sml_gram": 7, "sml_host_gram": 5, "sml_als_solve": 16, "sml_host_als_solve": 14}


def test_abi_surface():
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "als.hip" in build.SOURCES
    for name, n_args in NAMES.items():
        res_c = "int64_t " if name == "sml_gram_scratch_bytes" else "int "
        assert res_c + name + "(" in header and name in _lib.SIGNATURES and name in syms, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int64 if res_c == "int64_t " else ctypes.c_int) and len(args) == n_args, name
        decl = header[header.index(res_c + name + "("):]
        decl = decl[:decl.index(");")]
        params = [p.strip() for p in decl[decl.index("(") + 1:].split(",")]
        assert len(params) == n_args, (name, params)
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else \
                ctypes.c_double if p.startswith("double") else ctypes.c_int
            assert a is want, (name, p, a)
    for phrase in ("FOLD-IN", "#define SML_GRAM_CHUNK 1024", "SML_GRAM_CHUNK = 1024 rows, a constant of the definition",
                   "d = 128 needs a different register / LDS plan", "every fused step is an explicit\n * fma()",
                   "both triangles are written and are equal bit for bit", "if !(D[j] > 0) the row fails",
                   "the correctly rounded fp64 division", "the output row is left untouched",
                   "A row named\n * twice is written twice with the same bytes", "gram == NULL is accepted only with alpha0 == 0",
                   "no matrix instructions", "it never changes a byte"):
        assert phrase in header, phrase
    with open(os.path.join(REPO, "sml_amd", "csrc", "als.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "mfma" not in src.lower().replace("no matrix", "")


@pytest.mark.parametrize("dtype,d", A.PAIRS)
def test_host_gram_equals_the_restatement(dtype, d):
    c = A.case(dtype, d)
    for n_rows in A.GRAM_N:
        got = A.host_gram(c["gram_tab"], d, n_rows)
        A.same_bytes(got, A.ref_gram(c["gram_tab"], n_rows), (dtype, d, n_rows))
        A.same_bytes(got, np.ascontiguousarray(got.T), "both triangles")


def test_host_gram_propagates_nan_and_inf():
    w = A.case("fp32", 32)["gram_tab"][:1100].copy()
    w[1030, 3], w[5, 7] = np.nan, np.inf
    g = A.host_gram(w, 32)
    assert np.isnan(g[3]).all() and np.isnan(g[:, 3]).all() and np.isinf(g[7, 7]) and np.isfinite(g[0, 0])


@pytest.mark.parametrize("reg,alpha0", A.PARAMS)
@pytest.mark.parametrize("dtype,d", A.PAIRS)
def test_host_solve_equals_the_restatement(dtype, d, reg, alpha0):
    c = A.case(dtype, d)
    g = A.host_gram(c["other"], d)
    out, status = A.host_solve(c["other"], d, g, reg, alpha0, c["csr"], None, c["out0"])
    want = A.ref_rows(dtype, d, reg, alpha0)
    assert len(want) == (A.U if d == 32 else len(A.RESTATED_64))
    for r, (st, row) in want.items():
        assert status[r] == st == (1 if r == 0 else 0), (r, status[r], st)
        A.same_bytes(out[r], row, (dtype, d, reg, alpha0, r))
    assert (status[1:] == 0).all()
    if alpha0 == 0.0:                                  # gram == NULL reads as +0.0
        out2, status2 = A.host_solve(c["other"], d, None, reg, alpha0, c["csr"], None, c["out0"])
        A.same_bytes(out2, out)
        assert (status2 == status).all()


def test_status_codes():
    c = A.case("fp32", 32)
    other = c["other"].copy()
    other[10] = 0.0                                    # an all-zero member row
    other[11, 5] = np.nan
    other[12, 5] = np.inf
    sets = [[], [10], [3, 11], [12], [3, 4]]
    junk = np.full((5, 32), 7.0, np.float32)
    g = A.host_gram(c["other"], 32)
    out, status = A.host_solve(other, 32, g, 0.0, 0.0, A.csr(sets), None, junk)
    assert status[:4].tolist() == [1, 2, 2, 2]         # empty; an exactly zero pivot; NaN; Inf  (row 4: rank 2, left to rounding)
    assert (out[0].view(np.int32) == 0).all()          # +0.0, not -0.0
    A.same_bytes(out[1:4], junk[1:4], "failed rows are left untouched")
    out, status = A.host_solve(other, 32, g, 0.1, 0.1, A.csr(sets), None, junk)
    assert status.tolist() == [1, 0, 2, 2, 0]
    assert (out[1] == 0).all()                         # a zero member row: rhs = 0
    A.same_bytes(out[2:4], junk[2:4])
    nan_gram = g.copy()
    nan_gram[0, 0] = np.nan
    out, status = A.host_solve(other, 32, nan_gram, 0.1, 0.1, A.csr(sets), None, junk)
    assert status.tolist() == [1, 2, 2, 2, 2]
    out, status = A.host_solve(other, 32, g, 0.1, 0.1, None, None, junk)          # no set at all: every row is empty
    assert (status == 1).all() and (out.view(np.int32) == 0).all()


@pytest.mark.parametrize("dtype,d", (("fp32", 64), ("fp16", 32)))
def test_only_the_named_rows_are_written(dtype, d):
    c = A.case(dtype, d)
    g = A.host_gram(c["other"], d)
    full, st_full = A.host_solve(c["other"], d, g, 0.1, 0.1, c["csr"], None, c["out0"])
    rows = np.array([17, 3, 0, 39, 3, 6, 17], np.int64)              # permuted, with repeats
    out, status = A.host_solve(c["other"], d, g, 0.1, 0.1, c["csr"], rows, c["out0"])
    assert (status == st_full[rows]).all()
    want = c["out0"].copy()
    want[rows] = full[rows]
    A.same_bytes(out, want, "rows not named keep their bytes")
    out, status = A.host_solve(c["other"], d, g, 0.1, 0.1, c["csr"], np.zeros(0, np.int64), c["out0"])
    A.same_bytes(out, c["out0"])


@pytest.mark.parametrize("d", (32, 64))
def test_fp16_output_is_the_rounded_fp32_output(d):
    c = A.case("fp16", d)
    wide, out0 = c["other"].astype(np.float32), c["out0"].astype(np.float32)
    g = A.host_gram(c["other"], d)
    A.same_bytes(g, A.host_gram(wide, d), "the Gram matrix of the widened copy")
    for reg, alpha0 in A.PARAMS:
        h, st_h = A.host_solve(c["other"], d, g, reg, alpha0, c["csr"], None, c["out0"])
        f, st_f = A.host_solve(wide, d, g, reg, alpha0, c["csr"], None, out0)
        assert (st_h == st_f).all()
        A.same_bytes(h, f.astype(np.float16), (d, reg, alpha0))


def _refused(fn, *args):
    from sml_amd import _lib
    rc = fn(*args)
    assert rc != 0, args
    assert _lib.load().sml_last_error()


def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = A.case("fp32", 32)
    other, out = c["other"], c["out0"].copy()
    off, items = c["csr"]
    g = A.host_gram(other, 32)
    st = np.zeros(A.U, np.int32)
    p = A._p

    def solve(**kw):
        a = dict(other=p(other), eb=4, d=32, n_other=A.I, gram=p(g), alpha0=0.1, reg=0.1, off=p(off), items=p(items), rows=None, n=A.U,
                 out=p(out), n_out=A.U, status=p(st))
        a.update(kw)
        return lib.sml_host_als_solve(a["other"], a["eb"], a["d"], a["n_other"], a["gram"], a["alpha0"], a["reg"], a["off"], a["items"],
                                      a["rows"], a["n"], a["out"], a["n_out"], a["status"])

    assert solve() == 0
    for kw in (dict(d=128), dict(eb=2, d=128), dict(eb=8), dict(d=48), dict(reg=-1.0), dict(reg=float("nan")), dict(alpha0=-0.5),
               dict(alpha0=float("nan")), dict(n_other=0), dict(n_other=2 ** 31), dict(n_out=0), dict(n_out=2 ** 31), dict(n=-1),
               dict(off=None), dict(items=None), dict(gram=None), dict(out=p(other)), dict(out=p(g)), dict(out=p(off), n=1, n_out=1),
               dict(out=p(items)), dict(out=p(st)), dict(other=None), dict(out=None), dict(status=None), dict(status=p(other))):
        assert solve(**kw) != 0 and lib.sml_last_error(), kw
    assert solve(gram=None, alpha0=0.0) == 0
    assert solve(n=0, out=None, status=None) == 0                        # n == 0 does nothing
    gg = np.zeros((32, 32), np.float64)
    _refused(lib.sml_host_gram, p(other), 4, 128, A.I, p(gg))
    _refused(lib.sml_host_gram, p(other), 2, 128, A.I, p(gg))
    _refused(lib.sml_host_gram, p(other), 4, 32, 0, p(gg))
    _refused(lib.sml_host_gram, p(other), 4, 32, 2 ** 31, p(gg))
    _refused(lib.sml_host_gram, None, 4, 32, A.I, p(gg))
    _refused(lib.sml_host_gram, p(other), 4, 32, A.I, None)
    _refused(lib.sml_host_gram, p(other), 4, 32, A.I, p(other))


def _dense_system(other, g, reg, alpha0, members):
    y = other.astype(np.float64)[members]
    a = alpha0 * g + y.T @ y + reg * np.eye(other.shape[1])
    return a, y.sum(0)


@pytest.mark.parametrize("d", (32, 64))
def test_close_to_a_float64_solve(d):
    """max |out - (float32)ref| <= 2^-23 |ref|_inf per row: one fp32 rounding (2^-24 relative at the largest component) times a
    margin of 2 for the double rounding; the solve's own error, about cond * d * 2^-53, is far below that while cond <= 1e6,
    which is asserted on these inputs."""
    c = A.case("fp32", d)
    g = A.host_gram(c["other"], d)
    worst = 0.0
    for reg, alpha0 in A.PARAMS:
        out, status = A.host_solve(c["other"], d, g, reg, alpha0, c["csr"], None, c["out0"])
        for r in range(1, A.U):
            a, rhs = _dense_system(c["other"], g, reg, alpha0, c["sets"][r])
            cond = np.linalg.cond(a)
            worst = max(worst, cond)
            assert cond <= 1e6, (r, cond)
            ref = np.linalg.solve(a, rhs)
            err = np.abs(out[r].astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max()
            print("d=%d reg=%g alpha0=%g row %d: cond %.3g err %.3g bound %.3g" % (d, reg, alpha0, r, cond, err, 2.0 ** -23 * np.abs(ref).max()))
            assert status[r] == 0 and err <= 2.0 ** -23 * np.abs(ref).max(), (r, err)
    print("largest cond", worst)


def test_objective_identity():
    from sml_amd import als
    c = A.case("fp32", 32)
    p, q = c["out0"].astype(np.float64), c["other"].astype(np.float64)
    reg, alpha0 = 0.1, 0.1
    s = p @ q.T
    naive = alpha0 * (s ** 2).sum() + reg * ((p ** 2).sum() + (q ** 2).sum())
    for u, members in enumerate(c["sets"]):
        naive += ((1.0 - s[u, members]) ** 2).sum()
    got = als.objective(torch.from_numpy(c["out0"]), torch.from_numpy(c["other"]), c["csr"], reg, alpha0)
    assert abs(got - naive) <= 1e-9 * abs(naive), (got, naive)


def test_alternating_half_steps_lower_the_objective():
    """Eight half-steps through the host walks (fp32 tables, d = 32).  The float64 numpy iALS reference falls by at least 1e-3
    relative at each of them -- asserted first -- so the fp32 rounding of the rows cannot decide the sign."""
    from sml_amd import als
    c = A.case("fp32", 32)
    reg, alpha0 = 0.1, 0.1
    by_user, by_item = c["sets"], A.transpose(c["sets"], A.I)
    csr_u, csr_i = c["csr"], A.csr(by_item)

    def obj(p, q):
        return als.objective(torch.from_numpy(np.ascontiguousarray(p)), torch.from_numpy(np.ascontiguousarray(q)), csr_u, reg, alpha0)

    def half_ref(other, sets, n):
        g = other.T @ other
        out = np.zeros((n, 32))
        for r, members in enumerate(sets):
            if len(members):
                a, rhs = _dense_system(other, g, reg, alpha0, members)
                out[r] = np.linalg.solve(a, rhs)
        return out

    p, q = c["out0"].astype(np.float64), c["other"].astype(np.float64)
    ref = [obj(p, q)]
    for _ in range(4):
        p = half_ref(q, by_user, A.U)
        ref.append(obj(p, q))
        q = half_ref(p, by_item, A.I)
        ref.append(obj(p, q))
    falls = [(a - b) / a for a, b in zip(ref, ref[1:])]
    print("reference objective", ref, "relative falls", falls)
    assert len(falls) == 8 and min(falls) >= 1e-3, falls

    p, q = c["out0"].copy(), c["other"].copy()
    got = [obj(p, q)]
    for _ in range(4):
        p, st = A.host_solve(q, 32, A.host_gram(q, 32), reg, alpha0, csr_u, None, p)
        assert set(st.tolist()) <= {0, 1}
        got.append(obj(p, q))
        q, st = A.host_solve(p, 32, A.host_gram(p, 32), reg, alpha0, csr_i, None, q)
        assert set(st.tolist()) <= {0, 1}
        got.append(obj(p, q))
    print("host-walk objective", got)
    assert all(b < a for a, b in zip(got, got[1:])), got
