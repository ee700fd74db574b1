"""Graph propagation, the parts that need no GPU: the C ABI surface and sml_host_graph_propagate -- the definition of
sml_graph_propagate as a single-threaded walk over host memory -- against a restatement of the header's text (byte equality),
closeness to a float64 sum under a derived bound, the fp16 identity, special values, the rows a call writes and every refusal of
the host entry point."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _graph_cases as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sml_graph_split_from": 0, "sml_graph_scratch_bytes": 4, "sml_graph_propagate": 15, "sml_host_graph_propagate": 11}


def test_abi_surface():
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "graph.hip" in build.SOURCES
    for name, n_args in NAMES.items():
        res_c = "int64_t " if name == "sml_graph_scratch_bytes" else "int "
        assert res_c + name + "(" in header and name in _lib.SIGNATURES and name in syms, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int64 if res_c == "int64_t " else ctypes.c_int) and len(args) == n_args, name
        decl = header[header.index(res_c + name + "("):]
        decl = decl[:decl.index(");")]
        params = [p.strip() for p in decl[decl.index("(") + 1:].split(",") if p.strip() != "void"]
        assert len(params) == n_args, (name, params)
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
            assert a is want, (name, p, a)
    for phrase in ("PROPAGATION", "#define SML_PROP_SEG 256", "#define SML_PROP_STRANDS 8", "are constants of the definition",
                   "acc = fmaf(b[m_p], (float)src[m_p][s], acc)", "u_j = acc_j + acc_{j+4} for j = 0 .. 3",
                   "v_j = u_j + u_{j+2} for j = 0, 1", "seg_c = v_0 + v_1", "tot = +0.0f, then for c ascending: tot = tot + seg_c",
                   "out[x][s] = a[row] * tot, one fp32 rounding", "An empty set gives a[row] * +0.0f",
                   "every fused step is an explicit fmaf()", "no floating-point atomics and no matrix instructions",
                   "Neither ever changes a byte", "a refused call writes nothing"):
        assert phrase in header, phrase
    with open(os.path.join(REPO, "sml_amd", "csrc", "graph.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "mfma" not in src.lower() and "atomicAdd(float" not in src
    assert G.split_from() in (1, 2, 4, 8, 16)
    assert G.sizes()[:13] == (0, 1, 7, 8, 9, 255, 256, 257, 511, 512, 513, 515, 3000) and len(G.sizes()) == G.N


@pytest.mark.parametrize("scaled", (True, False))
@pytest.mark.parametrize("dtype,d", G.PAIRS)
def test_host_walk_equals_the_restatement(dtype, d, scaled):
    G.same_bytes(G.host_rows(dtype, d, scaled), G.ref_rows(dtype, d, scaled), (dtype, d, scaled))


def test_the_emulated_fmaf_rounds_once():
    """The restatement's fmaf against exact rational arithmetic, on operands chosen so that rounding the float64 sum first would
    land on a float32 tie."""
    from fractions import Fraction
    rng = np.random.RandomState(7)
    b = (rng.rand(4000) + 0.25).astype(np.float32)
    v = (rng.rand(4000) - 0.5).astype(np.float32)
    acc = ((rng.rand(4000) - 0.5) * 64).astype(np.float32)
    # a tie for the naive route: b * v = 2^24 - 2^-6 and acc = 2^48 + 2^25, whose float32 neighbours are 2^25 apart.  The float64
    # sum (spacing 2^-4) rounds to acc + 2^24, the float32 tie, which then goes to the even neighbour acc + 2^25; the fused result
    # is below the tie and stays at acc
    b[0], v[0], acc[0] = np.float32((2.0 ** 15 + 1) / 64), np.float32(2.0 ** 15 - 1), np.float32(2.0 ** 48 + 2.0 ** 25)
    assert np.float32(np.float64(b[0]) * np.float64(v[0]) + np.float64(acc[0])) == np.float32(2.0 ** 48 + 2.0 ** 26)
    got = G.fmaf(b, v, acc)
    for k in range(4000):
        exact = Fraction(float(b[k])) * Fraction(float(v[k])) + Fraction(float(acc[k]))
        lo = np.float32(float(exact))                                 # float(Fraction) rounds once to float64 ...
        want = None
        for cand in (lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))):
            if want is None or abs(Fraction(float(cand)) - exact) < abs(Fraction(float(want)) - exact):
                want = cand                                           # ... so take the nearest float32 of its neighbourhood exactly
        assert abs(Fraction(float(got[k])) - exact) <= abs(Fraction(float(want)) - exact), (k, got[k], want)
    assert got[0] == acc[0]


@pytest.mark.parametrize("dtype,d", (("fp32", 32), ("fp32", 128), ("fp16", 64)))
def test_close_to_float64(dtype, d):
    """|out - E| <= (40 + n_seg) * 2^-23 * |a| * sum |b * src| per element, E = a * sum b * src in float64.
    Derivation, with u = 2^-24 the unit roundoff: a member's term passes through at most 32 fmaf of its strand (256 / 8), 3 adds
    of the tree, n_seg adds of the segment sum and the final multiply, each of relative error at most u on a partial sum that is
    bounded in magnitude by sum |b * src| (1 + O(u)); so the first-order bound is (32 + 3 + n_seg + 1) u sum |b * src| |a|, and
    doubling it for the higher-order terms gives (72 + 2 n_seg) u <= (40 + n_seg) 2^-23."""
    c = G.case(dtype, d)
    got = G.host_rows(dtype, d, True).astype(np.float64)
    src, a, b = c["src"].astype(np.float64), c["a"].astype(np.float64), c["b"].astype(np.float64)
    worst = 0.0
    for r, mem in enumerate(c["sets"]):
        terms = b[mem, None] * src[mem]
        ref, mag = a[r] * terms.sum(0), abs(a[r]) * np.abs(terms).sum(0)
        n_seg = (len(mem) + G.SEG - 1) // G.SEG
        bound = (40 + n_seg) * 2.0 ** -23 * mag
        err = np.abs(got[r] - ref)
        if len(mem):
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (r, len(mem), float(err.max()), float(bound.min()))
    print("largest error in units of the bound: %.4f" % worst)


@pytest.mark.parametrize("d", (32, 64, 128))
def test_fp16_equals_the_widened_copy(d):
    c = G.case("fp16", d)
    wide = c["src"].astype(np.float32)
    for scaled in (True, False):
        G.same_bytes(G.host_rows("fp16", d, scaled),
                     G.host_propagate(wide, d, c["csr"], None, c["a"] if scaled else None, c["b"] if scaled else None), (d, scaled))


def test_special_values():
    c = G.case("fp32", 32)
    src = c["src"].copy()
    src[10, 3], src[11, 5], src[12, 5] = np.nan, np.inf, -np.inf
    sets = [[], [10, 20], [11, 20], [11, 12], [20, 21], []]
    a = np.array([-2.0, 1.0, 1.0, 1.0, 1.0, 0.5], np.float32)
    out = G.host_propagate(src, 32, G.csr(sets), None, a, None)
    assert (out[0].view(np.uint32) == 0x80000000).all()                # a * +0 with a < 0: -0.0, no special case
    assert (out[5].view(np.uint32) == 0).all()
    assert np.isnan(out[1, 3]) and np.isfinite(np.delete(out[1], 3)).all()
    assert out[2, 5] == np.inf and np.isnan(out[3, 5]) and np.isfinite(out[4]).all()
    b = np.ones(G.n_src(), np.float32)
    b[20] = np.nan
    out = G.host_propagate(src, 32, G.csr(sets), None, a, b)
    assert np.isnan(out[[1, 2, 4]]).all() and (out[0].view(np.uint32) == 0x80000000).all()
    out = G.host_propagate(src, 32, None, None, a, None, n=6)          # no set at all: every row is empty
    G.same_bytes(out, np.outer(a, np.zeros(32, np.float32)).astype(np.float32))
    assert G.host_propagate(src, 32, G.csr(sets), np.zeros(0, np.int64)).shape == (0, 32)


@pytest.mark.parametrize("dtype,d", (("fp32", 64), ("fp16", 32)))
def test_rows_name_the_output(dtype, d):
    c = G.case(dtype, d)
    full = G.host_rows(dtype, d, True)
    out = G.host_propagate(c["src"], d, c["csr"], G.ROWS, c["a"], c["b"])
    G.same_bytes(out, full[G.ROWS], "out[x] belongs to rows[x]")
    G.same_bytes(out[-1], out[G.ROWS[:-1].tolist().index(3)], "a row named twice is written twice with the same bytes")


def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = G.case("fp32", 32)
    src, a, b = c["src"], c["a"], c["b"]
    off, items = c["csr"]
    rows = G.ROWS
    out = np.full((G.N, 32), 7.0, np.float32)
    p = G._p

    def call(**kw):
        k = dict(src=p(src), eb=4, d=32, n_src=G.n_src(), off=p(off), items=p(items), rows=None, n=G.N, a=p(a), b=p(b), out=p(out))
        k.update(kw)
        return lib.sml_host_graph_propagate(k["src"], k["eb"], k["d"], k["n_src"], k["off"], k["items"], k["rows"], k["n"], k["a"], k["b"],
                                            k["out"])

    assert call() == 0
    G.same_bytes(out, G.host_rows("fp32", 32, True))
    out[:] = 7.0
    for kw in (dict(eb=8), dict(eb=1), dict(eb=0), dict(d=48), dict(d=16), dict(d=256), dict(n_src=0), dict(n_src=-1), dict(n_src=2 ** 31),
               dict(n=-1), dict(n=2 ** 31), dict(off=None), dict(items=None), dict(src=None), dict(out=None), dict(out=p(src)),
               dict(out=p(off)), dict(out=p(items)), dict(out=p(a)), dict(out=p(b)), dict(out=p(rows), rows=p(rows), n=len(rows))):
        assert call(**kw) != 0 and lib.sml_last_error(), kw
    assert (out == 7.0).all()                                            # a refused call writes nothing
    assert call(off=None, items=None) == 0 and (out == 0).all()          # both NULL: every set is empty
    assert call(n=0, out=None, src=None) == 0                            # n == 0 does nothing
    assert call(a=None, b=None) == 0
    G.same_bytes(out, G.host_rows("fp32", 32, False))
