"""Per-user candidate lists (sml_topk_candidates), the parts that need no GPU: the C ABI surface, the forms
sml_amd.retrieval.as_candidates accepts, the proof that the lists of the GPU tests change the answers of the CPU reference,
and the register report of the five kernel instantiations."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _candidates_cases as K
import _fp32_chain as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface():
    import ctypes
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    name = "sml_topk_candidates"
    assert name + "(" in header and name in _lib.SIGNATURES and name in syms
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 23
    # the argument list of the header, type by type: pointers, the three 64-bit geometry words, the ints
    decl = header[header.index("int " + name + "("):]
    decl = decl[:decl.index(");")]
    params = [p.strip() for p in decl[decl.index("(") + 1:].split(",")]
    assert len(params) == 23
    for p, a in zip(params, args):
        want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
        assert a is want, (p, a)
    # the header states the identity, the padding rule, the repeat rule and the n_elig definition
    for phrase in ("Defining identity: row x equals, byte for byte in items and scores, row 0 of sml_topk_items_adjusted",
                   "(allow AND bitmap(list x))",
                   "Padding rule: an entry c outside [0, n_item) is padding and is skipped",
                   "never touch memory",
                   "Repeat rule: a repeated id appears once",
                   "the number of eligible entries of list x, repeats counted as they occur",
                   "n == 0 is a valid call that launches nothing"):
        assert phrase in header, phrase


def _same_lists(got, lists):
    assert got.n == len(lists)
    for a, b in zip(got.lists(), lists):
        np.testing.assert_array_equal(a, np.asarray(b, np.int64))


def test_as_candidates_forms_agree():
    from sml_amd.retrieval import CandidateRows, Candidates, as_candidates
    rng = np.random.RandomState(0)
    lists = [rng.randint(0, 4099, size=m).astype(np.int64) for m in (0, 1, 5, 64, 3, 0, 17)]
    n = len(lists)
    off, flat32 = K.ragged(lists, np.int32)
    padded = [np.concatenate([l, np.full(64 - len(l), -1)]) for l in lists]          # what a dense form holds per list
    for pair in ((off, flat32), (off, K.ragged(lists, np.int64)[1]), (torch.from_numpy(off), torch.from_numpy(flat32)),
                 (off.tolist(), flat32.tolist())):
        got = as_candidates(pair, n, "cpu")
        assert got.off is not None and got.off.dtype == torch.int64 and got.items.dtype in (torch.int32, torch.int64)
        _same_lists(got, lists)
    got = as_candidates([l.tolist() for l in lists], n, "cpu")                       # a list of sequences -> ragged int32
    assert got.items.dtype == torch.int32 and got.off.tolist() == off.tolist()
    _same_lists(got, lists)
    got = as_candidates([[1, 2 ** 31 + 3], []], None, "cpu")                         # ids past int32 keep 64 bits
    assert got.items.dtype == torch.int64 and got.n == 2
    for dt in (np.int32, np.int64):
        m = K.dense(lists, dt)
        for x in (m, torch.from_numpy(m)):
            got = as_candidates(x, n, "cpu")
            assert got.off is None and (got.stride, got.first, got.cols) == (64, 0, 64)
            assert got.items.dtype == (torch.int32 if dt == np.int32 else torch.int64)
            _same_lists(got, padded)
    t = torch.from_numpy(K.dense(lists, np.int64))
    assert as_candidates(t, n, "cpu").items.data_ptr() == t.data_ptr()               # already there: not copied
    assert as_candidates(got, n, "cpu") is got and isinstance(got, Candidates)
    # a test file's rows: user, then the candidates
    users = rng.randint(0, 300, size=n).astype(np.int64)
    rows = torch.from_numpy(np.concatenate([users[:, None], K.dense(lists, np.int64)], 1))
    cr = CandidateRows(rows, first_col=1)
    assert cr.geometry == (65, 1, 64) and cr.users.tolist() == users.tolist()
    assert cr.rows.data_ptr() == rows.data_ptr() and cr.users.data_ptr() == rows.data_ptr()
    got = as_candidates(cr, None, "cpu")
    assert got.items.data_ptr() == rows.data_ptr() and (got.stride, got.first, got.cols) == (65, 1, 64)
    assert got.users.tolist() == users.tolist() and got.n == n
    _same_lists(got, padded)
    assert CandidateRows(rows.numpy()).geometry == (65, 1, 64)

    class Rows(object):                                   # the surface of evaluation.DeviceRows that is used
        def __init__(self, rows):
            self.rows, self.waited = rows, 0

        def wait_ready(self):
            self.waited += 1

    dr = Rows(rows)
    got = as_candidates(dr, n, "cpu")
    assert dr.waited == 1 and got.items.data_ptr() == rows.data_ptr() and got.first == 1
    _same_lists(got, padded)


def test_as_candidates_refuses_bad_input():
    from sml_amd.retrieval import CandidateRows, as_candidates
    items = np.arange(10, dtype=np.int32)
    for bad_off in ([1, 5, 10], [0, 6, 5, 10], [0, 5, 11], [], np.zeros((2, 2), np.int64), [0.0, 10.0]):
        with pytest.raises(ValueError):
            as_candidates((bad_off, items), None, "cpu")
    with pytest.raises(ValueError):
        as_candidates(([0, 5, 10], items), 3, "cpu")                  # n + 1 offsets
    assert as_candidates(([0, 5, 10], items), 2, "cpu").n == 2
    assert as_candidates(([0, 5, 7], items), 2, "cpu").n == 2         # the last offset may stop short of the entries
    with pytest.raises(ValueError):
        as_candidates(np.arange(10), None, "cpu")                     # 1-D
    with pytest.raises(ValueError):
        as_candidates(np.zeros((3, 4), np.float32), None, "cpu")
    with pytest.raises(ValueError):
        as_candidates(torch.zeros(3, 4), None, "cpu")
    with pytest.raises(ValueError):
        as_candidates([[0.5, 1.0]], None, "cpu")
    with pytest.raises(ValueError):
        as_candidates(([0, 2], np.zeros((2, 1), np.int32)), None, "cpu")
    with pytest.raises(ValueError):
        as_candidates((1, 2, 3), None, "cpu")
    with pytest.raises(ValueError):
        as_candidates(np.zeros((3, 4), np.int64), 4, "cpu")           # three lists for four users
    with pytest.raises(ValueError):
        CandidateRows(np.zeros((3, 4), np.int32))                     # the rows are read in place: int64 only
    with pytest.raises(ValueError):
        CandidateRows(np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        CandidateRows(np.zeros((3, 4), np.int64), first_col=5)


def _restricted_differs(c, k, seen):
    """Per list: whether the reference's restricted list differs from the user's unrestricted one."""
    want, _, _ = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], k, seen)
    full, _ = F.ref_topk(c["ru"], c["ri"], c["users"], k, seen)
    return (want != full).any(1), want


def test_lists_have_teeth_on_the_cpu_reference():
    """Over the GPU cases' inputs the restricted list differs from the unrestricted one for EVERY user whose list is neither
    empty nor the whole catalogue (at most a few hundred candidates of 4,099 items at k = 20: asserted, not assumed), so a
    kernel that ignored the lists -- or a reference that did -- cannot pass."""
    I = 4099
    for c in (K.boundary_case("fp32", 32), K.mixed_case("fp32", 32), K.repeat_case(), K.tie_case()):
        differs, want = _restricted_differs(c, 20, c["seen"])
        sizes = [len(np.unique(K._valid(l, I))) for l in c["lists"]]
        assert max(sizes) <= 700
        for x, m in enumerate(sizes):
            assert m < I
            if m > 0:
                assert differs[x], (x, m)
            else:
                assert (want[x] == -1).all()
        for x, l in enumerate(c["lists"]):                          # the lists hold candidates only
            assert np.isin(want[x][want[x] >= 0], l).all()


def test_repeat_cases_tell_dropping_from_keeping():
    """Every case with repeats has at least one list whose result changes if repeats were kept."""
    c = K.repeat_case()
    assert sum(c["repeats"]) >= 5
    want, _, n_elig = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], 20, c["seen"])
    kept = K.ref_keep_repeats(c["ru"], c["ri"], c["users"], c["lists"], 20, c["seen"])
    changed = (want != kept).any(1)
    for name in ("every id doubled", "doubled, second copies last", "best and K-th again in later rounds", "best item 64 times"):
        x = c["names"].index(name)
        assert c["repeats"][x] and changed[x], name
    assert not changed[[x for x, r in enumerate(c["repeats"]) if not r]].any()
    # n_elig counts entries, so a doubled list counts twice what its distinct ids do
    x = c["names"].index("every id doubled")
    once = K.ref_topk_candidates(c["ru"], c["ri"], c["users"][x:x + 1], [np.unique(c["lists"][x])], 20, c["seen"])[2][0]
    assert once > 40 and n_elig[x] == 2 * once
    for name in ("all padding", "all Seen", "only the NaN row"):
        x = c["names"].index(name)
        assert n_elig[x] == 0 and (want[x] == -1).all(), name
    x = c["names"].index("NaN row among the candidates")
    assert 11 in c["lists"][x] and 11 not in want[x] and n_elig[x] > 0
    c = K.mixed_case("fp32", 32)
    want, _, _ = K.ref_topk_candidates(c["ru"], c["ri"], c["users"], c["lists"], 20, c["seen"])
    assert (want != K.ref_keep_repeats(c["ru"], c["ri"], c["users"], c["lists"], 20, c["seen"])).any(1).sum() >= 5
    # the tie case is fed in descending id order and holds bit-equal scores: the id tie-break reorders them
    c = K.tie_case()
    assert c["ties"] >= 24 and all((np.diff(l) < 0).all() for l in c["lists"])


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")) if "k_topk_cand" in r["name"]]
    names = sorted(r["name"] for r in rows)
    assert names == ["k_topk_cand<128, half>", "k_topk_cand<32, float>", "k_topk_cand<32, half>", "k_topk_cand<64, float>",
                     "k_topk_cand<64, half>"], names
    for r in rows:
        print("%-28s VGPR %3d AGPR %3d LDS %5d occupancy %d" % (r["name"], r.get("VGPRs", 0), r.get("AGPRs", 0),
                                                               r.get("LDS Size [bytes/block]", 0), r.get("Occupancy [waves/SIMD]", 0)))
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, r
