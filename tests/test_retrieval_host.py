"""Full-catalogue retrieval, the parts that need no GPU: the C ABI surface, the kernels' register report, the
Seen-items CSR builder, and the CPU refusal of the model entry points."""
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


def test_kernel_resources_report():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"),
                        os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in ("k_full_rank<32>", "k_full_rank<64>", "k_topk_slice<32>", "k_topk_slice<64>", "k_topk_merge"):
        assert k in r.stdout, r.stdout


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
