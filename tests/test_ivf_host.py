"""The clustered item index, the parts that need no GPU: the C ABI surface, sml_host_ivf_search -- the definition of
sml_ivf_search as a single-threaded walk over host memory -- against the reference of the per-user candidate lists on the
concatenated probed lists and against sml_host_topk_items under the filter `allow AND bitmap(probed lists)`, the nested-probe
property, sml_host_ivf_centroids against a sequential float64 restatement, every refusal, and the argument errors of the Python
surface that need no device.  All comparisons are byte equality."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _candidates_cases as K
import _ivf_cases as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sml_ivf_search": 22, "sml_host_ivf_search": 20, "sml_ivf_centroids": 10, "sml_host_ivf_centroids": 9}


def test_abi_surface():
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "ivf.hip" in build.SOURCES
    for name, n_args in NAMES.items():
        assert "int " + name + "(" in header and name in _lib.SIGNATURES and name in syms, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        decl = header[header.index("int " + name + "("):]
        decl = decl[:decl.index(");")]
        params = [p.strip() for p in decl[decl.index("(") + 1:].split(",")]
        assert len(params) == n_args, (name, params)
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
            assert a is want, (name, p, a)
    for phrase in ("CLUSTERED INDEX", "A probe\n * outside [0, n_list) is padding and forms no address", "a list probed twice is walked twice",
                   "Defining identity: row x equals, byte for byte in items, scores and n_elig, row x of sml_topk_candidates",
                   "probing every list once returns the bytes of sml_topk_items",
                   "An empty list copies centroids_in[c]", "there are no floating-point\n * atomics",
                   "an item whose every centroid score is NaN joins list 0"):
        assert phrase in header, phrase


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_host_search_equals_the_candidate_reference(dtype, d):
    """Row x = ref_topk_candidates on "members of probes[x, 0], then of probes[x, 1], ..." -- items, scores and n_elig."""
    c = V.case(dtype, d)
    for nprobe in V.NPROBES:
        probes = V.probes_a(nprobe)
        lists = V.concat_lists(c["lists_a"], probes)
        for variant in V.VARIANTS:
            mask, terms = V.variant_args(variant, c["mask"], c["terms"])
            for k in V.KS:
                want = K.ref_topk_candidates(c["ru"], c["ri"], V.USERS, lists, k, c["csr"], mask, terms)
                got = V.host_search(c["wu"], c["wi"], d, V.USERS, c["lists_a"], probes, k, c["csr"], mask, terms)
                V.same_bytes(got, want, (dtype, d, nprobe, variant, k))
    # no Seen at all
    probes = V.probes_a(3)
    want = K.ref_topk_candidates(c["ru"], c["ri"], V.USERS, V.concat_lists(c["lists_a"], probes), 20)
    V.same_bytes(V.host_search(c["wu"], c["wi"], d, V.USERS, c["lists_a"], probes, 20), want, (dtype, d, "no Seen"))


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_host_search_many_tiny_lists(dtype, d):
    """Partition B: 130 lists of 0 .. 3 items, 128 probes per user (two per lane), one user with fewer than 64 items in all."""
    c = V.case(dtype, d)
    n, wi, ri, seen, mask, terms = V.sub_b(c)
    probes = V.probes_b()
    lists = V.concat_lists(c["lists_b"], probes)
    assert 0 < len(lists[2]) < 64 and len(lists[0]) > 128
    for variant in ("none", "both"):
        m, t = V.variant_args(variant, mask, terms)
        for k in V.KS:
            want = K.ref_topk_candidates(c["ru"], ri, V.USERS, lists, k, seen, m, t)
            V.same_bytes(V.host_search(c["wu"], wi, d, V.USERS, c["lists_b"], probes, k, seen, m, t), want, (dtype, d, variant, k))


def test_cases_have_teeth():
    """The inputs exercise what they claim: a round of 64 over four lists, a swallowed list, an empty Seen, the NaN list, a
    repeat that n_elig counts twice, the +-0 tie and the -inf offset in a returned list."""
    c = V.case("fp32", 32)
    la = c["lists_a"]
    assert [len(l) for l in la] == list(V.SIZES_A) and sorted(np.concatenate(la).tolist()) == list(range(V.I))
    assert [len(la[p]) for p in (1, 2, 3, 4)] == [1, 1, 0, 70]
    off, it = c["csr"]
    assert np.isin(la[4], it[off[3]:off[4]]).all() and off[8] == off[7]
    assert np.isnan(c["wi"][la[V.NAN_LIST]]).all()
    probes = V.probes_a(3)
    got = V.host_search(c["wu"], c["wi"], 32, V.USERS, la, probes, 20, c["csr"])
    assert (got[0][3] == -1).all() and got[2][3] == 0                    # all padding
    once = V.host_search(c["wu"], c["wi"], 32, V.USERS[2:3], la, np.array([[8, -1, -1]], np.int32), 20, c["csr"])
    assert got[2][2] == 2 * once[2][0] > 0 and (got[0][2] == once[0][0]).all()      # list 8 twice: the same list, n_elig doubled
    nan_only = V.host_search(c["wu"], c["wi"], 32, V.USERS, la, V.probes_a(1), 20, c["csr"])
    assert nan_only[2][5] == 0 and (nan_only[0][5] == -1).all()
    gone = V.host_search(c["wu"], c["wi"], 32, V.USERS[:1], la, np.array([[4]], np.int32), 20, c["csr"])
    assert gone[2][0] == 0                                               # user 3's Seen swallows list 4
    # the zero rows tie at +0 / -0 under the terms and the lower id comes first, each keeping its sign bit
    za, zb = c["zeros"]
    pr = np.array([[V.ZERO_LISTS[0], V.ZERO_LISTS[1]]], np.int32)
    it_, sc_, _ = V.host_search(c["wu"], c["wi"], 32, np.array([7]), la, pr, 128, None, None, c["terms"])
    at = {int(i): q for q, i in enumerate(it_[0]) if i >= 0}
    assert za in at and zb in at and abs(at[za] - at[zb]) == 1 and (at[za] < at[zb]) == (za < zb)
    assert sc_[0, at[za]].view(np.int32) == 0 and sc_[0, at[zb]].view(np.int32) == np.int32(-2 ** 31)
    ninf = int(la[V.NEG_INF_ITEM_LIST][3])
    it_, sc_, ne = V.host_search(c["wu"], c["wi"], 32, np.array([7]), la, np.array([[V.NEG_INF_ITEM_LIST]], np.int32), 128, None, None, c["terms"])
    live = int((it_[0] >= 0).sum())
    assert it_[0, live - 1] == ninf and sc_[0, live - 1] == -np.inf and live == ne[0] == 127      # -inf is eligible and orders last


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_host_search_equals_filtered_topk_per_user(dtype, d):
    """Row x = sml_host_topk_items for users[x] alone under allow AND bitmap(union of the probed lists); probing every list once
    = sml_host_topk_items outright, n_elig included."""
    c = V.case(dtype, d)
    la = c["lists_a"]
    for nprobe, variant, k in ((1, "none", 20), (3, "both", 20), (12, "filter", 128), (12, "terms", 1), (3, "terms", 128)):
        probes = V.probes_a(nprobe)
        mask, terms = V.variant_args(variant, c["mask"], c["terms"])
        got = V.host_search(c["wu"], c["wi"], d, V.USERS, la, probes, k, c["csr"], mask, terms)
        for x, u in enumerate(V.USERS):
            m = K.list_mask(V.concat_lists(la, probes[x:x + 1])[0], V.I)
            if mask is not None:
                m &= mask
            want = V.host_topk_items(c["wu"], c["wi"], d, [u], k, c["csr"], m, terms)
            V.same_bytes((got[0][x:x + 1], got[1][x:x + 1]), want[:2], (dtype, d, nprobe, variant, k, x))
    every = np.tile(np.arange(12, dtype=np.int32), (len(V.USERS), 1))
    for variant in V.VARIANTS:
        mask, terms = V.variant_args(variant, c["mask"], c["terms"])
        for k in V.KS:
            V.same_bytes(V.host_search(c["wu"], c["wi"], d, V.USERS, la, every, k, c["csr"], mask, terms),
                         V.host_topk_items(c["wu"], c["wi"], d, V.USERS, k, c["csr"], mask, terms), (dtype, d, variant, k, "every list"))


def _better(s, i, ts, ti):
    i, ti = (2 ** 31 if v < 0 else int(v) for v in (i, ti))          # a padding slot is worse than every live one
    return s > ts or (s == ts and i < ti)


def test_nested_probes_never_lose():
    """probes[:, :m] a prefix of probes[:, :m']: no slot of the m'-list is worse, in the family's order, than the m-list's."""
    c = V.case("fp32", 64)
    probes = V.probes_a(12)
    moved = 0
    for variant in ("none", "both"):
        mask, terms = V.variant_args(variant, c["mask"], c["terms"])
        prev = None
        for m in (1, 2, 3, 7, 12):
            cur = V.host_search(c["wu"], c["wi"], 64, V.USERS, c["lists_a"], probes[:, :m], 20, c["csr"], mask, terms)
            if prev is not None:
                for x in range(len(V.USERS)):
                    for q in range(20):
                        assert not _better(prev[1][x, q], prev[0][x, q], cur[1][x, q], cur[0][x, q]), (variant, m, x, q)
                moved += int((prev[0] != cur[0]).any())
            prev = cur
    assert moved >= 4                                                    # (more probes did change the lists)


def _clean(c):
    wi = c["wi"].copy()
    wi[c["lists_a"][V.NAN_LIST]] = wi[:2]                              # finite rows: NaN payloads are no part of the definition
    return wi


@pytest.mark.parametrize("dtype,d", V.PAIRS)
def test_host_centroids(dtype, d):
    c = V.case(dtype, d)
    wi = _clean(c)
    rng = np.random.RandomState(5)
    for lists in (c["lists_a"], c["lists_b"]):
        tab = wi if lists is c["lists_a"] else wi[:sum(len(l) for l in lists)]
        cin = rng.randn(len(lists), d).astype(wi.dtype)
        want = V.ref_centroids(tab, lists, cin)
        got = V.host_centroids(tab, d, lists, cin)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (dtype, d, len(lists))
        empty = [q for q, l in enumerate(lists) if len(l) == 0]
        assert empty and (got[empty].view(np.uint8) == cin[empty].view(np.uint8)).all()          # an empty list keeps its input row
        assert (got[[q for q, l in enumerate(lists) if len(l)]] != 7).any()
        again = cin.copy()
        assert V.host_centroids(tab, d, lists, again, in_place=True) is again and again.tobytes() == want.tobytes()


def test_search_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = V.case("fp32", 32)
    off, items_ = V.csr(c["lists_a"])
    users = V.USERS.copy()
    probes = V.probes_a(3)
    s_off, s_items = np.ascontiguousarray(c["csr"][0]), np.ascontiguousarray(c["csr"][1])
    out_i, out_s, out_n = np.zeros((7, 20), np.int32), np.zeros((7, 20), np.float32), np.zeros(7, np.int32)
    base = dict(wu=c["wu"], wi=c["wi"], eb=4, d=32, n_item=V.I, users=users, n=7, off=off, items_=items_, n_list=12, probes=probes,
                nprobe=3, k=20, s_off=s_off, s_items=s_items, allow=None, adj=None, items=out_i, scores=out_s, n_elig=out_n)
    order = ("wu", "wi", "eb", "d", "n_item", "users", "n", "off", "items_", "n_list", "probes", "nprobe", "k", "s_off", "s_items", "allow",
             "adj", "items", "scores", "n_elig")

    def call(**kw):
        a = dict(base, **kw)
        return lib.sml_host_ivf_search(*[a[key].ctypes.data if isinstance(a[key], np.ndarray) else a[key] for key in order])

    assert call() == 0 and call(n_elig=None) == 0 and call(s_off=None, s_items=None) == 0 and call(nprobe=1) == 0
    assert call(n=0) == 0 and call(n=0, wu=None, wi=None, users=None, probes=None, items=None, scores=None) == 0
    for bad, word in ((dict(eb=3), "elem_bytes"), (dict(nprobe=0), "nprobe"), (dict(nprobe=129), "nprobe"), (dict(n_list=0), "n_list"),
                      (dict(n_list=-4), "n_list"), (dict(k=0), "1 <= k <= 128"), (dict(k=129), "1 <= k <= 128"), (dict(d=48), "d must be"),
                      (dict(d=128), "d must be"), (dict(n_item=0), "n_item"), (dict(n_item=2 ** 31), "n_item"), (dict(n=-1), "n >= 0"),
                      (dict(s_items=None), "both or neither"), (dict(s_off=None), "both or neither"),
                      (dict(wu=None), "null"), (dict(wi=None), "null"), (dict(users=None), "null"), (dict(off=None), "null"),
                      (dict(items_=None), "null"), (dict(probes=None), "null"), (dict(items=None), "null"), (dict(scores=None), "null"),
                      (dict(items=probes.view(np.int32)), "overlaps an input"), (dict(scores=out_i.view(np.float32)), "outputs overlap"),
                      (dict(n_elig=out_i.reshape(-1)), "outputs overlap")):
        assert call(**bad) != 0, bad
        assert word in lib.sml_last_error().decode(), (bad, lib.sml_last_error())


def test_centroid_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = V.case("fp16", 128)
    wi = _clean(c)
    off, items_ = V.csr(c["lists_a"])
    cin, cout = np.zeros((12, 128), np.float16), np.zeros((13, 128), np.float16)
    base = dict(wi=wi, eb=2, d=128, n_item=V.I, off=off, items_=items_, n_list=12, cin=cin, cout=cout)
    order = ("wi", "eb", "d", "n_item", "off", "items_", "n_list", "cin", "cout")

    def call(**kw):
        a = dict(base, **kw)
        return lib.sml_host_ivf_centroids(*[a[key].ctypes.data if isinstance(a[key], np.ndarray) else a[key] for key in order])

    assert call() == 0 and call(cout=cin) == 0
    for bad, word in ((dict(eb=8), "elem_bytes"), (dict(eb=4), "d must be"), (dict(d=16), "d must be"), (dict(n_item=0), "n_item"),
                      (dict(n_list=0), "n_list"), (dict(wi=None), "null"), (dict(off=None), "null"), (dict(items_=None), "null"),
                      (dict(cin=None), "null"), (dict(cout=None), "null"), (dict(cout=cout[1:], cin=cout), "overlap"),
                      (dict(cout=wi), "overlaps an input")):
        assert call(**bad) != 0, bad
        assert word in lib.sml_last_error().decode(), (bad, lib.sml_last_error())


def test_python_argument_errors_need_no_device():
    from sml_amd.mf import MFbasemode
    from sml_amd.retrieval import ItemIndex, default_n_list, index_args
    assert [default_n_list(n) for n in (1, 2, 3, 100, 123000, 1000000)] == [1, 1, 2, 10, 351, 1000]
    cen, off, items = torch.zeros(12, 32), torch.zeros(13, dtype=torch.int64), torch.zeros(V.I, dtype=torch.int32)
    idx = ItemIndex(cen, off, items)
    assert (idx.n_list, idx.n_item, idx.dtype, idx.metric) == (12, V.I, torch.float32, "cosine")
    assert idx.sizes().tolist() == [0] * 12 and sorted(idx.host()) == ["centroids", "list_items", "list_off"]
    for bad in (dict(metric="l2"), dict(centroids=cen.long()), dict(centroids=cen[0]), dict(list_off=off[:-1]), dict(list_off=off.int()),
                dict(list_items=items.long()), dict(list_items=items.reshape(2, -1))):
        with pytest.raises(ValueError):
            ItemIndex(**dict(dict(centroids=cen, list_off=off, list_items=items), **bad))
    assert index_args(idx, None, 20, V.I, torch.float32) == 8 and index_args(idx, 12, 128, V.I, torch.float32) == 12
    assert index_args(ItemIndex(cen[:3], off[:4], items), None, 20, V.I, torch.float32) == 3
    for bad in (dict(nprobe=0), dict(nprobe=129), dict(topK=129), dict(topK=0), dict(n_item=V.I + 1), dict(dtype=torch.float16),
                dict(candidates=[[1, 2]]), dict(index=(cen, off, items))):
        a = dict(dict(index=idx, nprobe=None, topK=20, n_item=V.I, dtype=torch.float32, candidates=None), **bad)
        with pytest.raises(ValueError):
            index_args(**a)
    with pytest.raises(ValueError):
        idx.probe(torch.zeros(4, 32), torch.arange(4), 0)
    with pytest.raises(ValueError):
        idx.refresh(torch.zeros(V.I, 64))
    tab = torch.zeros(V.I, 32)
    for bad in (dict(n_list=0), dict(n_list=V.I + 1), dict(iters=0), dict(metric="l2")):
        with pytest.raises(ValueError):
            ItemIndex.build(tab, **bad)
    # the model's surface refuses before it asks for a device
    model = MFbasemode(V.U, V.I, 32)
    for bad in (dict(candidates=[[1]] * 2), dict(topK=129), dict(nprobe=0)):
        with pytest.raises(ValueError):
            model.recommend(torch.arange(2), **dict(dict(index=idx), **bad))
    with pytest.raises(ValueError):
        MFbasemode(V.U, V.I + 1, 32).recommend(torch.arange(2), index=idx)
    with pytest.raises(ValueError):
        model.similar_items(torch.arange(2), index=idx, nprobe=200)


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    for src, fam, occ in (("retrieval.hip", "k_ivf_search", 2), ("ivf.hip", "k_ivf_centroids", 4)):
        rows = [r for r in kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", src)) if fam in r["name"]]
        assert sorted(r["name"] for r in rows) == [fam + t for t in ("<128, half>", "<32, float>", "<32, half>", "<64, float>", "<64, half>")]
        for r in rows:
            print("%-28s VGPR %3d LDS %5d occupancy %d" % (r["name"], r.get("VGPRs", 0), r.get("LDS Size [bytes/block]", 0),
                                                           r.get("Occupancy [waves/SIMD]", 0)))
            assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r
            assert r.get("Occupancy [waves/SIMD]", 0) >= occ, r
