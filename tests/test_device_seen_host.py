"""Device interaction sets, the host side: the C ABI surface (header, ctypes signatures, exported symbols), the numpy
reference of tests/_device_seen_cases.py pinned against SeenItems.host(), the kernels' resources, and the wiring
(as_csr, the baseline's --full_eval flag).  No GPU involved."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from _device_seen_cases import build_cases, ref_contains, ref_set, union_cases
from conftest import REPO

NAMES = ("sml_iset_build_scratch_bytes", "sml_iset_build", "sml_iset_union_scratch_bytes", "sml_iset_union", "sml_iset_contains")


def test_abi_surface():
    from sml_amd import _lib
    header = " ".join(re.sub(r"^\s*\*", " ", line) for line in open(os.path.join(REPO, "include", "sml_hip.h")).read().splitlines())
    header = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "interaction sets" in header
    for phrase in ("off int64 [n_user + 1]", "items int32 [nnz], ascending and unique inside each user's range",
                   "room for m entries", "room for nnz_a + nnz_b", "every dependency is a launch boundary"):
        assert phrase in header, phrase
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m sml_amd.build)"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in exported.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name
    assert "interaction_set.hip" in __import__("sml_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("case", build_cases(), ids=lambda c: c[0])
def test_reference_equals_seen_items_build(case):
    from sml_amd.retrieval import SeenItems
    _, n_user, n_item, pairs = case
    off, items = SeenItems(n_user, n_item).add(pairs).host()
    r_off, r_items = ref_set([pairs], n_user, n_item)
    for a, b in ((off, r_off), (items, r_items)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("case", union_cases(), ids=lambda c: c[0])
def test_reference_equals_seen_items_union(case):
    from sml_amd.retrieval import SeenItems
    _, n_user, n_item, adds = case
    seen = SeenItems(n_user, n_item)
    for k, pairs in enumerate(adds):
        off, items = seen.add(pairs).host()
        r_off, r_items = ref_set(adds[:k + 1], n_user, n_item)
        for a, b in ((off, r_off), (items, r_items)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_reference_contains():
    pairs = np.array([[0, 1], [0, 3], [2, 0]])
    probe = np.array([[0, 1], [0, 2], [1, 1], [2, 0], [2, 3]])
    assert ref_contains(pairs, 4, probe).tolist() == [True, False, False, True, False]
    assert ref_contains(np.zeros((0, 2), np.int64), 4, probe).tolist() == [False] * 5


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", "interaction_set.hip"))
    names = [r["name"] for r in rows]
    assert names, "no kernel found"
    for k in ("k_rw_scatter", "k_is_tile_scan", "k_is_probe", "k_is_merge", "k_is_contains", "k_is_build_off"):
        assert any(k in n for n in names), k
    for r in rows:
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r


def test_as_csr_passes_a_device_seen_through():
    from sml_amd import retrieval

    class Stub(retrieval.DeviceSeen):
        def __init__(self):                      # (no engine: device() is all as_csr touches)
            pass

        def device(self, device=None):
            return ("off", "items", device)

    assert retrieval.as_csr(Stub(), "cuda:0") == ("off", "items", "cuda:0")
    assert retrieval.as_csr(None, "cuda:0") is None


def test_device_seen_surface():
    from sml_amd.retrieval import DeviceSeen
    for name in ("add", "device", "host", "contains", "from_periods", "from_seen", "__len__"):
        assert callable(getattr(DeviceSeen, name)), name
    from sml_amd.engine import HipEngine
    for name in ("iset_build", "iset_union", "iset_contains"):
        assert callable(getattr(HipEngine, name)), name


def test_baseline_flag():
    from sml_amd.baseline import SPMF, get_parse
    assert get_parse().parse_args([]).full_eval == 0
    assert get_parse().parse_args(["--full_eval", "1"]).full_eval == 1
    assert callable(SPMF.full_test)
