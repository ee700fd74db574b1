"""Full-catalogue retrieval on fp16 tables, the parts that need no GPU: the C ABI surface of the _f16 entry points, the
register report of the fp16 kernel instantiations, and the proof that the d = 128 GPU tests' data separates the kernels'
chain order from another order."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sml_full_rank_f16", "sml_topk_items_f16", "sml_user_rank_f16")


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
        # same argument list as the fp32 entry point: the tables are the only difference, and ctypes passes both as void*
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-4]]


@pytest.mark.parametrize("seed", [0])
def test_exact_tests_have_teeth_at_128(seed):
    """On the near-tie fp16 case the d = 128 GPU tests use, the chain in dim order 0 .. 127 instead of the kernels'
    0, 64, 1, 65, ... changes ranks and list entries: the exact comparison would catch a kernel that summed that way."""
    import _fp32_chain as F
    from _half_cases import half_near_tie_case, widen
    c = half_near_tie_case(128, seed=seed)
    wu, wi = widen(c["wu"]), widen(c["wi"])
    ref = F.ref_full_rank(wu, wi, c["rows"], c["seen"])
    alt = F.ref_full_rank(wu, wi, c["rows"], c["seen"], order="sequential")
    planted = np.arange(len(c["planted"]))
    assert (alt[planted] != ref[planted]).sum() >= 10
    it, sc = F.ref_topk(wu, wi, c["users"], 128, c["seen"])
    it2, sc2 = F.ref_topk(wu, wi, c["users"], 128, c["seen"], order="sequential")
    assert (it != it2).any(1).sum() >= 1
    assert (sc.view(np.int32) != sc2.view(np.int32)).sum() >= 1000


def test_half_cases_are_fp16_and_widen_exactly():
    from _half_cases import half_near_tie_case, plant_specials, random_half_case, widen
    c = random_half_case(32, seed=1, U=50, I=500, n=10)
    plant_specials(c, c["rng"])
    for w in (c["wu"], c["wi"]):
        assert w.dtype == np.float16
        w32 = widen(w)
        assert w32.dtype == np.float32
        ok = ~np.isnan(w)
        assert (w32[ok].astype(np.float16).view(np.uint16) == w[ok].view(np.uint16)).all() and np.isnan(w32[~ok]).all()
    assert half_near_tie_case(128, seed=0)["wi"].dtype == np.float16
