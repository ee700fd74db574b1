"""Full-catalogue retrieval, the parts that need no GPU: the C ABI surface, the kernels' register report, the
Seen-items CSR builder, the CPU refusal of the model entry points, and the exact fp32 references (tests/_fp32_chain.py)
the GPU tests compare with: fma32 against rational arithmetic, the filtered references against brute force, and the
proof that the GPU tests' data separates the kernels' chain order from other orders."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import make_mf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sml_full_rank", "sml_topk_scratch_bytes", "sml_topk_items")


def test_abi_surface():
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert name in syms
    assert "retrieval.hip" in build.SOURCES


@functools.lru_cache(maxsize=None)
def _resources_report():
    """tools/kernel_resources.py over retrieval.hip, run once for the tests below."""
    return subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"),
                           os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")], capture_output=True, text=True)


def test_kernel_resources_report():
    r = _resources_report()
    assert r.returncode == 0, r.stdout + r.stderr
    for k in ("k_full_rank<32, float, false, false>", "k_full_rank<64, float, false, false>", "k_topk_slice<32, float, false, false>",
              "k_topk_slice<64, float, false, false>", "k_topk_merge"):
        assert k in r.stdout, r.stdout


def test_retrieval_kernel_instantiations_report():
    """Every table-reading kernel is one template k_x<D, T, F, A>: all 20 instantiations of each family exist, fp32 at
    d = 128 exists nowhere, and no kernel of the file spills or touches scratch (the tool's exit code)."""
    r = _resources_report()
    assert r.returncode == 0, r.stdout + r.stderr              # 1: a kernel spills or touches scratch
    names = {line.split("  ")[0] for line in r.stdout.splitlines()}
    for k in ("k_full_rank", "k_topk_slice", "k_ur_thresholds", "k_ur_count"):
        want = {"%s<%d, %s, %s, %s>" % (k, d, t, f, a) for t, ds in (("float", (32, 64)), ("half", (32, 64, 128))) for d in ds
                for f in ("false", "true") for a in ("false", "true")}
        assert len(want) == 20 and want <= names, (sorted(want - names), r.stdout)
        assert {n for n in names if n.startswith(k + "<")} == want, r.stdout      # nothing else: no fp32 at 128, no stray form
    assert "<128, float" not in r.stdout
    for k in ("k_filter_from_ids", "k_adjust_fill", "k_adjust_cosine<32, float>", "k_adjust_cosine<128, half>"):
        assert k in names, r.stdout


def _pairs(rng, m, U, I):
    return np.stack([rng.randint(0, U, size=m), rng.randint(0, I, size=m)], 1).astype(np.int64)


def test_seen_csr_sorted_unique():
    from sml_amd.retrieval import SeenItems
    rng = np.random.RandomState(0)
    U, I = 50, 300
    pairs = _pairs(rng, 2000, U, I)
    off, items = SeenItems(U, I).add(pairs).host()
    assert off.dtype == np.int64 and items.dtype == np.int32 and off.shape == (U + 1,)
    assert off[0] == 0 and off[-1] == items.shape[0] and (np.diff(off) >= 0).all()
    for u in range(U):
        r = items[off[u]:off[u + 1]]
        assert (np.diff(r) > 0).all()
        assert set(r.tolist()) == set(pairs[pairs[:, 0] == u, 1].tolist())


def test_seen_add_twice_equals_concatenation():
    from sml_amd.retrieval import SeenItems
    rng = np.random.RandomState(1)
    a, b = _pairs(rng, 700, 40, 90), _pairs(rng, 500, 40, 90)
    s1 = SeenItems(40, 90).add(a).add(b)
    s2 = SeenItems(40, 90).add(np.concatenate([a, b]))
    for x, y in zip(s1.host(), s2.host()):
        np.testing.assert_array_equal(x, y)


def test_seen_from_periods(tmp_path):
    from sml_amd import synth
    from sml_amd.retrieval import SeenItems
    info = synth.write_dataset(str(tmp_path), "tiny", 3, 400, 30, 70, neg=4, seed=7)
    seen = SeenItems.from_periods(str(tmp_path), "tiny", [0, 2])
    assert (seen.n_user, seen.n_item) == (int(info[1]), int(info[2]))
    want = set()
    for p in (0, 2):
        want |= {(int(u), int(i)) for u, i in np.load(str(tmp_path / "tiny" / "train" / ("%d.npy" % p)))}
    off, items = seen.host()
    got = {(u, int(i)) for u in range(seen.n_user) for i in items[off[u]:off[u + 1]]}
    assert got == want and len(seen) == len(want)


def test_seen_touches_no_rng(tmp_path):
    from sml_amd import synth
    from sml_amd.retrieval import SeenItems
    synth.write_dataset(str(tmp_path), "tiny", 2, 100, 10, 20, neg=2, seed=3)
    np.random.seed(5)
    torch.manual_seed(5)
    np_state, t_state = np.random.get_state(), torch.get_rng_state()
    seen = SeenItems.from_periods(str(tmp_path), "tiny", [0, 1])
    seen.add(np.array([[1, 2], [3, 4]]))
    seen.host()
    seen.device("cpu")
    assert np.random.get_state()[1].tobytes() == np_state[1].tobytes() and np.random.get_state()[2] == np_state[2]
    assert torch.equal(torch.get_rng_state(), t_state)


def test_seen_device_cache():
    from sml_amd.retrieval import SeenItems
    s = SeenItems(4, 8).add(np.array([[0, 1]]))
    a = s.device("cpu")
    assert s.device("cpu") is a
    s.add(np.array([[2, 3]]))
    b = s.device("cpu")
    assert b is not a and b[0].tolist() == [0, 1, 1, 2, 2] and b[1].tolist() == [1, 3]


def test_model_entry_points_refuse_cpu():
    mf = make_mf(5, 7, 32)
    with pytest.raises(RuntimeError):
        mf.recommend(torch.arange(3), topK=2)
    with pytest.raises(RuntimeError):
        mf.test_full(torch.zeros(2, 2, dtype=torch.int64), topK=2)


def test_retrieval_module_is_product_only():
    with open(os.path.join(REPO, "sml_amd", "retrieval.py")) as f:
        assert "oracle" not in f.read()


# ---- the exact fp32 references the GPU tests compare against (tests/_fp32_chain.py) ---------------------------------

def _round_f32(fr):
    """The float32 nearest to the Fraction fr, ties to even (IEEE round-to-nearest), overflowing to +-inf."""
    from fractions import Fraction
    lim = Fraction(2 ** 128) - Fraction(2 ** 103)        # halfway between FLT_MAX and 2^128: rounds to even = inf
    if fr >= lim:
        return np.float32(np.inf)
    if fr <= -lim:
        return np.float32(-np.inf)
    g = np.float32(float(fr))
    best = None
    for c in (np.nextafter(g, np.float32(-np.inf)), g, np.nextafter(g, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        key = (abs(Fraction(float(c)) - fr), int(np.array(c).view(np.int32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def _fma_fraction(a, b, c):
    from fractions import Fraction
    a, b, c = (np.float32(v) for v in (a, b, c))
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:                        # IEEE: +0 unless both the product and the addend are -0
        neg = c == 0 and np.signbit(c) and (a == 0 or b == 0) and np.signbit(a) != np.signbit(b)
        return np.float32(-0.0) if neg else np.float32(0.0)
    return _round_f32(v)


def _fma_cases():
    rng = np.random.RandomState(11)
    m = 4000

    def f(lo, hi):
        with np.errstate(over="ignore"):
            return (rng.randn(m) * 2.0 ** rng.randint(lo, hi, size=m)).astype(np.float32)

    cases = [(f(-30, 30), f(-30, 30), f(-60, 60))]                                    # random
    a, b = f(-20, 20), f(-20, 20)
    p = (a.astype(np.float64) * b).astype(np.float32)
    wiggle = (np.nextafter(-p, np.float32(np.inf)) - (-p)) * rng.randint(-3, 4, size=m)
    cases.append((a, b, (-p + wiggle).astype(np.float32)))                           # near-cancelling
    cases.append((f(-80, -70), f(-80, -70), f(-150, -140)))                         # subnormal results
    cases.append((f(60, 66), f(60, 66), f(120, 128)))                                # overflow
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0, 3.4e38], np.float32)
    g = np.array(np.meshgrid(sp, sp, sp)).reshape(3, -1)
    cases.append((g[0], g[1], g[2]))                                                  # inf / NaN / signed zeros
    return [tuple(np.asarray(x, np.float32) for x in c) for c in cases]


def test_fma32_matches_exact_rational_rounding():
    from _fp32_chain import fma32
    n_sub = n_inf = 0
    for a, b, c in _fma_cases():
        got = fma32(a, b, c)
        for q in range(len(a)):
            want = _fma_fraction(a[q], b[q], c[q])
            if np.isnan(want):
                assert np.isnan(got[q]), (a[q], b[q], c[q], got[q])
                continue
            assert np.array(got[q]).view(np.int32) == np.array(want).view(np.int32), (a[q], b[q], c[q], got[q], want)
            n_sub += bool(0 < abs(want) < np.finfo(np.float32).tiny)
            n_inf += bool(np.isinf(want))
    assert n_sub > 1000 and n_inf > 300           # the edge families really reached their edges


def test_chain_order_is_the_kernels():
    """chain(order='kernel') is fma over dims 0, D/2, 1, D/2 + 1, ...: the order of score_chain / tile_scores."""
    from _fp32_chain import chain, fma32
    rng = np.random.RandomState(12)
    u, x = rng.randn(50, 64).astype(np.float32), rng.randn(50, 64).astype(np.float32)
    acc = np.zeros(50, np.float32)
    for s in range(32):
        acc = fma32(x[:, s], u[:, s], acc)
        acc = fma32(x[:, s + 32], u[:, s + 32], acc)
    assert acc.tobytes() == chain(u, x).tobytes()
    with open(os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")) as f:
        src = f.read()
    assert "acc = fmaf(x[s], u[s], acc);\n        acc = fmaf(x[s + D / 2], u[s + D / 2], acc);" in src


@pytest.mark.parametrize("order", ["kernel", "sequential", "swapped", "f64"])
def test_filtered_references_equal_brute_force(order):
    """The float64 filter of ref_full_rank / ref_topk changes nothing: against the full emulated score matrix."""
    import _fp32_chain as F
    c = F.near_tie_case(32, seed=3)
    wu, wi, rows, users, (off, its) = c["wu"], c["wi"], c["rows"][:120], c["users"][:60], c["seen"]
    sets = [set(its[off[u]:off[u + 1]].tolist()) for u in range(wu.shape[0])]
    S = F.score_chain(wu[np.unique(np.concatenate([rows[:, 0], users]))], wi, order)
    idx = {u: q for q, u in enumerate(np.unique(np.concatenate([rows[:, 0], users])))}
    rank = F.ref_full_rank(wu, wi, rows, c["seen"], order=order)
    for r, (u, p) in enumerate(rows[:, :2]):
        s = S[idx[u]]
        m = s > s[p]
        m[p] = False
        m[list(sets[u])] = False
        assert rank[r] == int(m.sum()), r
    items, scores = F.ref_topk(wu, wi, users, 128, c["seen"], order=order)
    for x, u in enumerate(users):
        s = S[idx[u]]
        ok = ~np.isnan(s)
        ok[list(sets[u])] = False
        ids = np.nonzero(ok)[0]
        want = ids[np.lexsort((ids, -s[ids].astype(np.float64)))][:128]
        np.testing.assert_array_equal(items[x, :len(want)], want)
        assert scores[x, :len(want)].tobytes() == s[want].tobytes()


@pytest.mark.parametrize("d", [32, 64])
def test_exact_tests_have_teeth(d):
    """On the near-tie data the GPU tests use, a chain in another order (dims sequential, the lane halves swapped) or a
    once-rounded float64 score changes many ranks and list slots: an exact comparison would catch such a kernel, while
    the float64 brackets of the older tests cannot."""
    import _fp32_chain as F
    c = F.near_tie_case(d)
    ref = F.ref_full_rank(c["wu"], c["wi"], c["rows"], c["seen"])
    lists = F.ref_topk(c["wu"], c["wi"], c["users"], 128, c["seen"])
    planted = np.arange(len(c["planted"]))
    for order in ("sequential", "swapped", "f64"):
        alt = F.ref_full_rank(c["wu"], c["wi"], c["rows"], c["seen"], order=order)
        assert (alt[planted] != ref[planted]).sum() >= 40, order
        it, sc = F.ref_topk(c["wu"], c["wi"], c["users"], 128, c["seen"], order=order)
        assert (it != lists[0]).any(1).sum() >= 30, order
        assert (sc != lists[1]).sum() >= 5000, order
    # the subnormal users: a path that flushed their products to zero would rank every positive 0
    tiny_rows = np.arange(len(c["rows"]) - 16, len(c["rows"]))
    assert (ref[tiny_rows] > 0).sum() >= 12
    S = F.score_chain(c["wu"][c["tiny"]], c["wi"])
    assert (np.abs(S[S != 0]) < np.finfo(np.float32).tiny).all() and (S != 0).mean() > 0.99


def test_planner_mirror_reaches_the_named_geometry():
    """The GPU geometry tests are named for what retrieval.hip's planner does with their shapes; if the planner changes,
    this fails instead of that coverage vanishing."""
    import _fp32_chain as F
    with open(os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")) as f:
        src = f.read()
    for line in ("while (m > 1 && n_tiles / (8 * m) < 16) --m;", "return w > 4 ? 4 : w;",
                 "const int64_t groups = (n + RT * waves - 1) / (RT * waves);",
                 "return plan_grid(n, topk_waves(k), n_item, 2048, 4);", "return plan_grid(n, waves, n_item, 8192, 64);",
                 "const int per_wave = 2 * k * RT * 4;", "constexpr int kRankWaves = 4;"):
        assert line in src, line
    assert {F.topk_waves(k) for k in (1, 2, 63, 64, 65, 85, 86, 127, 128)} == {4, 3, 2}
    assert [F.topk_waves(k) for k in (64, 65, 85, 86)] == [4, 3, 3, 2]
    assert F.topk_plan(100, 20, 288)[1:] == (8, 2, 3)                  # 9 tiles, 8 slices, the last 3 empty
    w, s, st, empty = F.topk_plan(3, 20, 16411)
    assert (s, st, empty) == (32, 17, 1) and 16411 % 32 != 0          # 513 tiles, the last slice empty, last tile partial
    assert F.rank_plan(100, 262145) == (512, 17, 30)                  # the rank kernel's 512-slice maximum
    assert F.rank_plan(100, 1 << 24 | 1000)[0] == 512
