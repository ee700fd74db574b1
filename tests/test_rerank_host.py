"""Greedy MMR re-ranking, the host side: the C ABI surface, the host entry sml_host_rerank_mmr against the plain-numpy
restatement of tests/_rerank_cases.py byte for byte (every case, setting and width, fp16 tables included), the restatement
against a float64 MMR where no rounding can matter, what the planted cases tell apart, the refusals, the argument errors of
the Python surface that need no device, and the kernels' resources.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _rerank_cases as R
from conftest import REPO

NAMES = ("sml_rerank_mmr", "sml_host_rerank_mmr")


def _p(a):
    return None if a is None else a.ctypes.data


def host_entry(table, d, pool_items, pool_rel, pool_cols, nrm, lam, normalize, k, n=None):
    """The five outputs of sml_host_rerank_mmr (prefilled with junk: every output is written)."""
    from sml_amd import _lib
    lib = _lib.load()
    table, pool_items, pool_rel = (np.ascontiguousarray(a) for a in (table, pool_items, pool_rel))
    nrm = None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float32)
    n = pool_items.shape[0] if n is None else n
    items, pos = np.full((n, k), 77, np.int32), np.full((n, k), 77, np.int32)
    value, n_sel, sim_sum = np.full((n, k), 7.0, np.float32), np.full(n, 77, np.int32), np.full(n, 7.0, np.float32)
    _lib.check(lib.sml_host_rerank_mmr(_p(table), table.itemsize, d, table.shape[0], _p(pool_items), _p(pool_rel), n, pool_cols,
                                       pool_items.shape[1], _p(nrm), lam, normalize, k, _p(items), _p(pos), _p(value), _p(n_sel), _p(sim_sum)),
               "sml_host_rerank_mmr")
    return items, pos, value, n_sel, sim_sum


def host_case(c, setting, k, pool_cols=R.C):
    lam, metric, normalize = R.SETTINGS[setting]
    return host_entry(c["table"], c["d"], c["pool_items"], c["pool_rel"], pool_cols, c["nrm"] if metric == "cosine" else None, lam, normalize, k)


def test_abi_surface():
    import ctypes
    from sml_amd import _lib
    text = open(os.path.join(REPO, "include", "sml_hip.h")).read()
    header = re.sub(r"\s+", " ", " ".join(re.sub(r"^\s*\*", " ", line) for line in text.splitlines()))
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "---- RE-RANKING" in text
    for phrase in ("the first occurrence wins", "no address is formed from it", "oml = 1.0f - lam, formed once in fp32",
                   "a correctly rounded fp32 division", "-0 orders below +0", "the candidate's norm first",
                   "q(e) = -(oml * pen(e)): one fp32 multiply, then an exact negation", "v(e) = fmaf(lam, r(e), q(e))",
                   "NaN last, then v descending, then pool position ascending", "a NaN sim never replaces pen", "in pick order",
                   "Unused slots hold (-1, -1, -inf)", "Every output is written", "is a single rounding",
                   "The bytes are the same for every launch geometry", "byte for byte", "bit for bit",
                   "n == 0 is a valid call that launches nothing"):
        assert phrase in header, phrase
    dev, host = _lib.SIGNATURES["sml_rerank_mmr"][1], _lib.SIGNATURES["sml_host_rerank_mmr"][1]
    assert len(dev) == 20 and len(host) == 18
    assert dev[10] is ctypes.c_float and host[10] is ctypes.c_float, "lam goes by value as a float"
    assert [a for a in dev if a is ctypes.c_float] == [ctypes.c_float] and dev[6] is ctypes.c_int64 and dev[8] is ctypes.c_int64
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m sml_amd.build)"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in exported.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name
    assert "rerank.hip" in __import__("sml_amd.build", fromlist=["SOURCES"]).SOURCES
    src = open(os.path.join(REPO, "sml_amd", "csrc", "rerank.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "__fdiv_rn" in src and not re.search(r"atomic\w*\(", src)


@pytest.mark.parametrize("width", R.WIDTHS, ids=R.WIDTH_IDS)
def test_host_entry_equals_the_restatement(width):
    c = R.case(*width)
    for s in range(len(R.SETTINGS)):
        for k in R.KS:
            assert R.same_bytes(host_case(c, s, k), R.expected(width[0], width[1], s, k)) is None, (R.SETTING_IDS[s], k)
    for cols in R.LENGTHS[:-1]:                                  # the call's own pool_cols: the columns behind it are not read
        assert R.same_bytes(host_case(c, 0, 20, cols), R.expected(width[0], width[1], 0, 20, cols)) is None, cols


def test_outputs_are_well_formed():
    c = R.case(32, False)
    for s in range(len(R.SETTINGS)):
        items, pos, value, n_sel, sim_sum = R.expected(32, False, s, 20)
        for x in range(c["n"]):
            m = int(n_sel[x])
            assert (items[x, m:] == -1).all() and (pos[x, m:] == -1).all() and (value[x, m:] == -np.inf).all()
            assert len(set(pos[x, :m].tolist())) == m and len(set(items[x, :m].tolist())) == m, "a pick is made once, an id once"
            assert (c["pool_items"][x, pos[x, :m]] == items[x, :m]).all()
            assert ((items[x, :m] >= 0) & (items[x, :m] < R.I)).all()
            assert not np.isnan(c["pool_rel"][x, pos[x, :m]]).any()
    n_sel = R.expected(32, False, 0, 128)[3]
    assert n_sel[36] == 0 and n_sel[21] == 34 and n_sel[22] == 66 and n_sel[23] == 61 and (n_sel[list(R.LONG)] == 128).all()
    assert 40 in R.expected(32, False, 0, 128)[1][22] and 20 not in R.expected(32, False, 0, 128)[1][22], "a NaN first occurrence does not win"


def test_lam_one_raw_returns_the_sorted_prefix_and_rels_bits():
    """lam == 1, normalize == 0: the picks are the pool by (rel descending, position ascending) and value is rel's bits; on the
    pools a top-K call returned (lists 0 .. 13) items is the pool's first k columns byte for byte."""
    for d, half in ((32, False), (64, True)):
        c = R.case(d, half)
        for k in R.KS:
            items, pos, value, n_sel, _ = host_case(c, 2, k)
            for x in range(14):
                m = int(n_sel[x])
                assert m == min(k, R.LENGTHS[x % 7])
                assert (pos[x, :m] == np.arange(m)).all()
                assert items[x].tobytes() == c["pool_items"][x, :k].tobytes()
                assert value[x].tobytes() == c["pool_rel"][x, :k].tobytes()
            for x in range(14, c["n"]):
                m = int(n_sel[x])
                rel = c["pool_rel"][x, pos[x, :m]]
                assert (np.diff(rel) <= 0).all() and (value[x, :m] == rel).all()
                same = np.nonzero(np.diff(rel) == 0)[0]
                assert (pos[x, same] < pos[x, same + 1]).all(), "equal rel: the lower position first"


def test_lam_zero_picks_the_first_eligible_entry_first():
    c = R.case(32, False)
    items, pos, value, n_sel, _ = host_case(c, 3, 20)
    for x in range(c["n"]):
        ids, rel = c["pool_items"][x, :R.C], c["pool_rel"][x, :R.C]
        first = [e for e in range(R.C) if 0 <= ids[e] < R.I and not np.isnan(rel[e])]
        assert (pos[x, 0] == first[0]) if first else (n_sel[x] == 0 and pos[x, 0] == -1), x


def _mmr64(rows, rel, lam, k):
    """Greedy cosine MMR with min-max relevance in float64: (positions picked, the smallest gap between a step's best and
    second-best value)."""
    rows = rows.astype(np.float64)
    unit = rows / np.sqrt((rows ** 2).sum(1))[:, None]
    sim = unit @ unit.T
    r = (rel.astype(np.float64) - rel.min()) / (rel.max() - rel.min())
    pen = np.full(len(rel), -np.inf)
    live = np.ones(len(rel), bool)
    picks, gap = [], np.inf
    for t in range(k):
        v = lam * r - ((1.0 - lam) * pen if t else 0.0)
        v[~live] = -np.inf
        o = np.argsort(-v, kind="stable")
        if live.sum() > 1:
            gap = min(gap, v[o[0]] - v[o[1]])
        picks.append(int(o[0]))
        live[o[0]] = False
        pen = np.maximum(pen, sim[:, o[0]])
    return picks, gap


def test_restatement_agrees_with_a_float64_mmr():
    """Two well-separated clusters, relevance favouring one: the float64 MMR's every choice is decided by a margin far above
    any fp32 rounding (asserted), and the restatement and the host entry make the same choices -- alternating clusters."""
    rng = np.random.RandomState(5)
    d, L, k = 32, 40, 12
    centre = np.zeros((2, d))
    centre[0, 0], centre[1, 1] = 1.0, 1.0
    cluster = np.arange(L) % 2
    table = (centre[cluster] + 0.15 * rng.randn(L, d)).astype(np.float32)
    rel = (np.where(cluster == 0, 1.0, 0.4) + 0.3 * rng.rand(L)).astype(np.float32)
    ids = np.arange(L, dtype=np.int32)[None, :]
    picks, gap = _mmr64(table, rel, 0.5, k)
    assert gap > 1e-4, gap
    got = R.ref_rerank(table, ids, rel[None, :], L, R.item_norms(table), 0.5, 1, k)
    assert got[1][0].tolist() == picks and got[3][0] == k
    assert len(set(cluster[picks[:2]])) == 2, "the second pick leaves the first one's cluster"
    assert (np.sort(rel)[::-1][:k] != rel[picks]).any(), "not the relevance order"
    pad = np.zeros((64 - L, d), np.float32)                      # (the entry wants nothing of the table but 16-byte alignment)
    tab = np.concatenate([table, pad])
    host = host_entry(tab, d, ids, rel[None, :], L, R.item_norms(tab), 0.5, 1, k)
    assert R.same_bytes(host, R.ref_rerank(tab, ids, rel[None, :], L, R.item_norms(tab), 0.5, 1, k)) is None
    assert host[1][0].tolist() == picks


def test_cases_have_teeth():
    """What the seeded cases tell apart, counted on the restatement (d = 32, fp32, k = 20)."""
    c = R.case(32, False)
    S = R.pairwise(32, False)
    base = R.expected(32, False, 0, 20)                          # lam 0.7, cosine, normalized
    args = (c["table32"], c["pool_items"], c["pool_rel"], R.C, c["nrm"])
    plain = R.ref_rerank(*args, 1.0, 1, 20, S=S)
    # diversification changes the list: of the 7 random pools (lists 14 .. 20, lengths 1, 2, 63, ..., 128) the two shortest
    # cannot differ (one entry; two entries of which the more relevant always goes first) and all 5 others do
    differ = [x for x in range(14, 21) if not np.array_equal(base[0][x], plain[0][x])]
    assert differ == [16, 17, 18, 19, 20]
    assert all(np.array_equal(np.sort(base[0][x]), np.sort(plain[0][x])) for x in (14, 15))
    assert all(not np.array_equal(base[0][x], plain[0][x]) for x in R.LONG)

    def changed(alt):
        return {name: [x for x in range(c["n"]) if np.ascontiguousarray(a[x]).tobytes() != np.ascontiguousarray(b[x]).tobytes()]
                for name, a, b in zip(("items", "pos", "value", "n_sel", "sim_sum"), alt, base)}
    tie = changed(R.ref_rerank(*args, 0.7, 1, 20, S=S, tie="last"))
    assert 24 in tie["items"] and 37 in tie["pos"], "the copies of one row and the equal-rel list need the position rule"
    norm = changed(R.ref_rerank(*args, 0.7, 1, 20, S=S, norm_first="pick"))
    assert len(norm["value"]) >= 5 and len(norm["sim_sum"]) >= 5 and not norm["n_sel"], "the order of the two norm multiplies shows"
    total = changed(R.ref_rerank(*args, 0.7, 1, 20, S=S, total_order="reverse"))
    assert len(total["sim_sum"]) >= 5 and not total["items"] and not total["value"], "the order of total's adds shows"
    # subnormal-scale rows: the chain scores are subnormal (fp32 table) and the similarities still differ
    assert (np.abs(S[27, :40, :40]) < 2.0 ** -126).all() and (S[27, :40, :40] != 0).any()
    # a zero row: its similarity to everything is 0 under the cosine (norm 0), so it is never penalised
    assert c["nrm"][R.ID_ZERO] == 0 and base[0][26, 0] == R.ID_ZERO
    # signed zeros: lo of list 39 is -0 and +0 - (-0) is +0
    assert np.signbit(c["pool_rel"][39, 0]) and R.expected(32, False, 0, 128)[3][39] == 6


def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = R.case(32, False)
    n, k = 8, 20
    tab, pi, pr, nrm = (np.ascontiguousarray(c[key]) for key in ("table", "pool_items", "pool_rel", "nrm"))
    buf = np.zeros(8 * n * k + 64, np.int32)                     # the outputs, side by side
    out = [buf[q * n * k:(q + 1) * n * k] for q in range(3)] + [buf[3 * n * k:3 * n * k + n], buf[3 * n * k + n:3 * n * k + 2 * n]]
    base = dict(w=_p(tab), eb=4, d=32, n_item=R.I, pi=_p(pi), pr=_p(pr), n=n, cols=R.C, stride=R.STRIDE, nrm=_p(nrm), lam=0.7, normalize=1, k=k,
                items=_p(out[0]), pos=_p(out[1]), value=_p(out[2]), n_sel=_p(out[3]), sim_sum=_p(out[4]))
    order = ("w", "eb", "d", "n_item", "pi", "pr", "n", "cols", "stride", "nrm", "lam", "normalize", "k", "items", "pos", "value", "n_sel", "sim_sum")

    def call(**kw):
        a = dict(base, **kw)
        return lib.sml_host_rerank_mmr(*[a[key] for key in order])
    assert call() == 0 and call(nrm=None) == 0 and call(lam=0.0) == 0 and call(lam=1.0) == 0 and call(normalize=0) == 0
    assert call(n=0) == 0 and call(n=0, w=None, pi=None, pr=None, items=None, pos=None, value=None, n_sel=None, sim_sum=None) == 0
    for bad, word in ((dict(d=128), "d must be"), (dict(d=16), "d must be"), (dict(eb=3), "elem_bytes"), (dict(eb=8), "elem_bytes"),
                      (dict(cols=0), "pool_cols"), (dict(cols=129, stride=129), "pool_cols"), (dict(stride=R.C - 1), "pool_stride"),
                      (dict(k=0), "k <= 128"), (dict(k=129), "k <= 128"), (dict(lam=-0.1), "lam"), (dict(lam=1.5), "lam"),
                      (dict(lam=float("nan")), "lam"), (dict(normalize=2), "normalize"), (dict(normalize=-1), "normalize"),
                      (dict(n=-1), "n < 2^31"), (dict(n_item=0), "n_item"), (dict(w=_p(tab) + 4), "16-byte aligned"),
                      (dict(w=None), "null"), (dict(pi=None), "null"), (dict(pr=None), "null"), (dict(items=None), "null"),
                      (dict(pos=None), "null"), (dict(value=None), "null"), (dict(n_sel=None), "null"), (dict(sim_sum=None), "null"),
                      (dict(pos=_p(out[0])), "outputs overlap"), (dict(value=_p(out[0]) + 4 * (n * k - 1)), "outputs overlap"),
                      (dict(sim_sum=_p(out[3])), "outputs overlap"), (dict(n_sel=_p(out[2]) + 4), "outputs overlap"),
                      (dict(items=_p(pi)), "overlaps an input"), (dict(value=_p(pr) + 4 * ((n - 1) * R.STRIDE + R.C - 1)), "overlaps an input"),
                      (dict(sim_sum=_p(nrm) + 4 * (R.I - 1)), "overlaps an input"), (dict(n_sel=_p(tab)), "overlaps an input")):
        assert call(**bad) != 0, bad
        assert word in lib.sml_last_error().decode(), (bad, lib.sml_last_error())
    # an fp16 table at d = 128 is a pair with kernels; value may start right behind the pools' last entry
    half = R.case(128, True)
    assert call(w=_p(np.ascontiguousarray(half["table"])), eb=2, d=128, nrm=None) == 0
    assert call(value=_p(pr) + 4 * ((n - 1) * R.STRIDE + R.C), n=1, k=1) == 0


def test_python_argument_errors_need_no_device():
    import torch
    from sml_amd import retrieval
    from sml_amd.mf import MFbasemode
    assert retrieval.rerank_args(20, 0.5) == (20, 0.5) and retrieval.rerank_args(128, 1, "dot", 128) == (128, 1.0)
    for bad in ((0, 0.5), (129, 0.5), (20, -0.01), (20, 1.01), (20, float("nan")), (20, 0.5, "euclid"), (20, 0.5, "cosine", 0),
                (20, 0.5, "cosine", 129)):
        with pytest.raises(ValueError):
            retrieval.rerank_args(*bad)
    assert retrieval.diversify_args(20, 0.7, None, "cosine") == 100 and retrieval.diversify_args(30, 0.7, None, "dot") == 128
    assert retrieval.diversify_args(20, 1.0, 20, "cosine") == 20
    model = MFbasemode(10, 50, 32)                               # on the CPU: a call that got past its arguments would raise RuntimeError
    users = torch.arange(4)
    with pytest.raises(ValueError, match="exceeds the pool"):
        model.recommend(users, topK=20, diversify=0.5, pool=10)
    with pytest.raises(ValueError, match="exceeds the pool"):
        model.recommend(users, topK=129, diversify=0.5)
    with pytest.raises(ValueError, match="must not exceed 128"):
        model.recommend(users, topK=20, diversify=0.5, pool=129)
    with pytest.raises(ValueError, match="lam"):
        model.recommend(users, topK=20, diversify=1.5)
    with pytest.raises(ValueError, match="metric"):
        model.recommend(users, topK=20, diversify=0.5, metric="euclid")
    with pytest.raises(RuntimeError, match="HIP engine"):
        model.recommend(users, topK=20, diversify=0.5)


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", "rerank.hip")) if "k_rerank_mmr" in r["name"]]
    names = sorted(r["name"] for r in rows)
    assert names == sorted("k_rerank_mmr<%s>" % a for a in ("32, float", "64, float", "32, half", "64, half", "128, half")), names
    for r in rows:
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r
        assert r.get("LDS Size [bytes/block]", 0) <= 4 * (128 * 4 + 256), r        # per wave: 128 ids and one row
