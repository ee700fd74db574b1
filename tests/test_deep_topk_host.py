"""Deep lists, the host side: sml_host_topk_items -- the definition of sml_topk_deep as a single-threaded walk over host memory --
against the exact reference of tests/_deep_topk_cases.py byte for byte (every case, both element types, k = 1, 128, 129, 500,
1,024), n_elig, the prefix identity, the C ABI surface, the refusals, the argument errors of the Python surface that need no
device, and the new kernels' resources.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _deep_topk_cases as D
from conftest import REPO

NAMES = ("sml_topk_deep_scratch_bytes", "sml_topk_deep", "sml_host_topk_items")
HOST_USERS = 33          # the walk is single-threaded: the host suite takes at most this many of a grid entry's users


def _p(a):
    return None if a is None else a.ctypes.data


def host_entry(c, users, k, variant="none", seen="case"):
    """(items int32 [n, k], scores float32 [n, k], n_elig int32 [n]) of sml_host_topk_items, the outputs prefilled with junk."""
    from sml_amd import _lib
    lib = _lib.load()
    users = np.ascontiguousarray(users, np.int64)
    n = len(users)
    off, seen_items = c["seen"] if seen == "case" else seen
    seen_items = np.ascontiguousarray(seen_items if len(seen_items) else np.zeros(1, np.int32))
    allow = D.words(c) if variant in ("filter", "both") else None
    adj = D.adj_table(c) if variant in ("terms", "both") else None
    items, scores, n_elig = np.full((n, k), 77, np.int32), np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32)
    _lib.check(lib.sml_host_topk_items(_p(c["wu"]), _p(c["wi"]), c["wu"].itemsize, c["d"], c["wi"].shape[0], _p(users), n, k, _p(off),
                                       _p(seen_items), _p(allow), _p(adj), _p(items), _p(scores), _p(n_elig)), "sml_host_topk_items")
    return items, scores, n_elig


def check_ref(got, want, what):
    items, scores, n_elig = want
    np.testing.assert_array_equal(got[0], items, err_msg=str(what))
    np.testing.assert_array_equal(got[1].view(np.int32), np.ascontiguousarray(scores).view(np.int32), err_msg=str(what))
    np.testing.assert_array_equal(got[2], n_elig, err_msg=str(what))


def test_abi_surface():
    from sml_amd import _lib
    text = open(os.path.join(REPO, "include", "sml_hip.h")).read()
    header = re.sub(r"\s+", " ", " ".join(re.sub(r"^\s*\*", " ", line) for line in text.splitlines()))
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "---- DEEP LISTS" in text and re.search(r"#define SML_TOPK_DEEP_MAX 1024\b", text)
    for phrase in ("1 <= k <= SML_TOPK_DEEP_MAX", "A descending, then item id ascending", "hold (-1, -inf)", "may be NULL",
                   "adj == NULL is accepted and means the bare score", "byte for byte", "is the first k' slots of row x of the k-call",
                   "Seen' = Seen U complement", "bit for bit", "whenever that is < k", "-0 and +0 tie and the id decides",
                   "fmaf(+0, -1, -0) is -0", "sends both zeros to one key", "keeps its own sign bit", "NaN never enters a list",
                   "-inf is eligible and orders last", "a value in [1, 256] forces the number of item slices", "empty slices included",
                   "n == 0 is a valid call that launches nothing", "No allocation, no copy to the host and no synchronise",
                   "there are no floating-point atomics", "k outside [1, 1024] or slices outside [0, 256]",
                   "a single-threaded walk over HOST memory"):
        assert phrase in header, phrase
    deep, host, size = (_lib.SIGNATURES[n][1] for n in ("sml_topk_deep", "sml_host_topk_items", "sml_topk_deep_scratch_bytes"))
    assert len(deep) == 18 and len(host) == 15 and len(size) == 5 and _lib.SIGNATURES["sml_topk_deep_scratch_bytes"][0] is ctypes.c_int64
    assert deep[3] is ctypes.c_int and deep[4] is ctypes.c_int64 and deep[7] is ctypes.c_int and deep[12] is ctypes.c_int
    assert host[2] is ctypes.c_int and host[3] is ctypes.c_int and host[4] is ctypes.c_int64 and host[7] is ctypes.c_int
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m sml_amd.build)"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in exported.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name
    src = open(os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")).read()
    assert "__host__ __device__ __forceinline__ float score_chain" in src, "the host walk and the kernels share the chain's text"
    deep_src = src[src.index("---- deep lists"):]
    assert not re.search(r"atomicAdd\([^;]*\bfloat\b", deep_src) and "atomicAdd(" in deep_src


@pytest.mark.parametrize("name,dtype,d,variant,n", D.GRID, ids=D.GRID_IDS)
def test_host_entry_equals_the_reference(name, dtype, d, variant, n):
    """Every grid entry at every k, n_elig included; the outputs come back fully overwritten (no junk survives)."""
    c = D.case(name, dtype, d)
    n = min(n, HOST_USERS)
    ref = D.reference(name, dtype, d, variant, n)
    users = c["users"][:n]
    for k in D.KS:
        got = host_entry(c, users, k, variant)
        check_ref(got, D.cut(ref, k), (name, dtype, d, variant, k))
        live = got[0] >= 0
        assert (live.sum(1) == np.minimum(got[2], k)).all() and (got[1][~live] == -np.inf).all() and (got[0][~live] == -1).all()


def test_prefix_identity():
    for name, dtype, d, variant in (("random", "fp32", 32, "none"), ("all_tie", "fp16", 128, "both"), ("near_tie", "fp32", 64, "filter")):
        c = D.case(name, dtype, d)
        users = c["users"][:HOST_USERS]
        deep = host_entry(c, users, 1024, variant)
        for k in (1, 20, 128, 129, 500, 1023):
            got = host_entry(c, users, k, variant)
            assert got[0].tobytes() == np.ascontiguousarray(deep[0][:, :k]).tobytes(), (name, k)
            assert got[1].tobytes() == np.ascontiguousarray(deep[1][:, :k]).tobytes(), (name, k)
            assert (got[2] == deep[2]).all()


def test_cases_have_teeth():
    """What the seeded cases hold, read off the references."""
    # padding and exactly-k users
    ref = D.reference("random", "fp32", 32, "none", 257)
    assert ref[2][0] == 50 and (ref[0][0, 50:] == -1).all() and (ref[0][0, :50] >= 0).all()
    for place, left in D.EXACT:
        assert ref[2][place] == left and (ref[0][place, :left] >= 0).all() and (ref[0][place, left:] == -1).all()
    assert ref[2][4:256].min() > 1024
    # all_tie: the first k eligible ids; with terms every third item scores -0 and still orders by id
    c = D.case("all_tie", "fp16", 128)
    it, sc, _ = D.reference("all_tie", "fp16", 128, "both", 97)
    assert (np.diff(it, axis=1) > 0).all() and (it[:, 0] > 0).any() and not (it == np.arange(1024)[None, :]).all(1).any()
    assert (sc == 0).all() and (np.signbit(sc) == (it % 3 == 0)).all() and np.signbit(sc).any() and not np.signbit(sc).all()
    assert c["mask"][it].all()
    # sorted: every top entry in the first tiles / in the last ones, the partial tile included
    assert D.reference("sorted_desc", "fp32", 64, "none", 33)[0].max() < 1024 + 200 + 1
    asc = D.reference("sorted_asc", "fp32", 32, "none", 97)[0]
    assert asc.min() >= D.I - 1024 - 200 - 1 and (asc[:, :3] >= D.I - 3 - 200).all() and (asc >= 32 * (D.I // 32)).any()
    # wide: both signs, +inf first, -inf last but eligible, NaN items in no list
    c = D.case("wide", "fp32", 32)
    it, sc, ne = D.reference("wide", "fp32", 32, "terms", 97)
    assert (sc[:, :500] > 0).any() and (sc[:, :1024][it >= 0] < 0).any() and (sc[20:, 0] == np.inf).all()
    gone = np.concatenate([c["planted"]["nan_rows"], c["planted"]["nan_offset"]])
    assert not np.isin(it, gone).any() and (ne <= D.I - len(gone)).all()
    small = D.reference("wide", "fp32", 64, "none", 33)
    assert not np.isin(small[0], c["planted"]["nan_rows"]).any()
    # long: more eligible items than a 16-bit bin holds
    assert D.reference("long", "fp32", 32, "none", 40)[2].min() > 65535
    # long_tie: every eligible item has the same key, so one bin of every pass counts them all -- beyond 16 bits
    it, sc, ne = D.reference("long_tie", "fp32", 32, "none", 8)
    assert ne.min() > 65535 and (sc == 0).all() and not np.signbit(sc).any() and (np.diff(it, axis=1) > 0).all() and it.max() < 1024 + 200 + 1
    # near_tie: lists whose k-th score repeats right behind the list (the planted copies), at the deep k values
    it, sc, _ = D.reference("near_tie", "fp32", 32, "none", 257)
    assert sum(int(sc[x, k - 1] == sc[x, k]) for x in range(48) for k in (129, 500) if it[x, k] >= 0) >= 8


def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = D.case("random", "fp32", 32)
    n, k = 8, 200
    wu, wi = c["wu"], c["wi"]
    users = np.ascontiguousarray(c["users"][:n])
    off, seen_items = c["seen"]
    allow, adj = D.words(c), D.adj_table(c)
    buf = np.zeros(2 * n * k + n + 16, np.int32)
    items, scores, n_elig = buf[:n * k], buf[n * k:2 * n * k].view(np.float32), buf[2 * n * k:2 * n * k + n]
    base = dict(wu=_p(wu), wi=_p(wi), eb=4, d=32, n_item=D.I, users=_p(users), n=n, k=k, off=_p(off), seen=_p(seen_items), allow=_p(allow),
                adj=_p(adj), items=_p(items), scores=_p(scores), n_elig=_p(n_elig))
    order = ("wu", "wi", "eb", "d", "n_item", "users", "n", "k", "off", "seen", "allow", "adj", "items", "scores", "n_elig")

    def call(**kw):
        a = dict(base, **kw)
        return lib.sml_host_topk_items(*[a[key] for key in order])
    assert call() == 0 and call(allow=None) == 0 and call(adj=None) == 0 and call(off=None, seen=None) == 0 and call(n_elig=None) == 0
    assert call(k=1) == 0 and call(k=1024, n=1) == 0
    assert call(n=0) == 0 and call(n=0, wu=None, wi=None, users=None, items=None, scores=None) == 0
    for bad, word in ((dict(k=0), "1 <= k <= 1024"), (dict(k=1025), "1 <= k <= 1024"), (dict(k=-1), "1 <= k <= 1024"),
                      (dict(off=None), "both or neither"), (dict(seen=None), "both or neither"),
                      (dict(d=128), "d must be"), (dict(d=16), "d must be"), (dict(eb=3), "elem_bytes"), (dict(eb=8), "elem_bytes"),
                      (dict(n_item=0), "n_item"), (dict(n_item=2 ** 31), "n_item"), (dict(n=-1), "n < 2^31"),
                      (dict(wu=None), "null"), (dict(wi=None), "null"), (dict(users=None), "null"), (dict(items=None), "null"),
                      (dict(scores=None), "null"),
                      (dict(scores=_p(items)), "outputs overlap"), (dict(n_elig=_p(scores) + 4 * (n * k - 1)), "outputs overlap"),
                      (dict(items=_p(users)), "overlaps an input"), (dict(scores=_p(adj) + 4), "overlaps an input"),
                      (dict(n_elig=_p(wi)), "overlaps an input"), (dict(items=_p(allow)), "overlaps an input")):
        assert call(**bad) != 0, bad
        assert word in lib.sml_last_error().decode(), (bad, lib.sml_last_error())
    half = D.case("random", "fp16", 128)
    assert call(wu=_p(half["wu"]), wi=_p(half["wi"]), eb=2, d=128) == 0
    # the size query and the device entry refuse before any launch (a null context is refused first of all)
    assert lib.sml_topk_deep_scratch_bytes(None, 8, 200, D.I, 0) < 0


def test_python_argument_errors_need_no_device():
    import torch
    from sml_amd import retrieval
    from sml_amd.mf import MFbasemode
    assert retrieval.DEEP_MAX == 1024 and 1 <= retrieval.DEEP_FROM <= 129
    assert retrieval.deep_args(1) == 1 and retrieval.deep_args(1024) == 1024 and retrieval.deep_args(np.int64(500)) == 500
    for bad in (0, 1025, -1, 2.0, 500.5, "20", None, True, float("nan")):
        with pytest.raises(ValueError):
            retrieval.deep_args(bad)
    model = MFbasemode(10, 50, 32)                               # on the CPU: a call that got past its arguments would raise RuntimeError
    users = torch.arange(4)
    with pytest.raises(ValueError, match="exceeds the pool"):
        model.recommend(users, topK=129, diversify=0.5)
    with pytest.raises(RuntimeError, match="HIP engine"):
        model.recommend(users, topK=500)
    with pytest.raises(RuntimeError, match="HIP engine"):
        model.similar_items(users, topK=300)


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", "retrieval.hip")) if "k_deep_" in r["name"]]
    names = sorted(r["name"] for r in rows)
    widths = ("32, float", "64, float", "32, half", "64, half", "128, half")
    want = ["k_deep_%s<%s, %s, %s>" % (fam, w, f, a) for fam in ("count", "collect") for w in widths for f in ("false", "true")
            for a in ("false", "true")] + ["k_deep_pick", "k_deep_sort"]
    assert names == sorted(want), names
    for r in rows:
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r
        assert r.get("LDS Size [bytes/block]", 0) <= 8192, r         # static LDS: the sort's 1,024 pairs (the histogram is dynamic)
