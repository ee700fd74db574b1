"""Training negatives, the host side: the C ABI surface, the host entry sml_host_sample_negatives_ex against the plain-Python
restatement of tests/_neg_sampler_cases.py byte for byte, the restatement against its own literal form, the prefix and
monotonicity properties, the two distributions, popularity_cdf, the refusals, the kernels' resources and the baseline's
control flow with an engine double.  No GPU."""
import contextlib
import io
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _neg_sampler_cases as C
from _fp32_chain import chain
from conftest import REPO

NAMES = ("sml_sample_negatives_ex", "sml_host_sample_negatives_ex")


def host_entry(users, item_all, user_ptr, user_items, M, seed=C.SEED, cdf=None, wu=None, wi=None, d=32, want_score=True):
    """(negs, score or None, failed) from sml_host_sample_negatives_ex."""
    from sml_amd import _lib
    lib = _lib.load()
    a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
    users, item_all, user_ptr, user_items = (a(x, np.int64) for x in (users, item_all, user_ptr, user_items))
    cdf, wu, wi = a(cdf, np.float64), a(wu, np.float32), a(wi, np.float32)
    p = lambda x: None if x is None else x.ctypes.data
    n = len(users)
    negs, failed = np.full(n, -7, np.int64), np.full(1, 99, np.int32)
    score = np.full(n, -7.0, np.float32) if want_score else None
    _lib.check(lib.sml_host_sample_negatives_ex(p(users), n, p(item_all), len(item_all), p(user_ptr), len(user_ptr) - 1, p(user_items), p(cdf),
                                                M, p(wu), p(wi), d, seed, p(negs), p(score), p(failed)), "sml_host_sample_negatives_ex")
    return negs, score, int(failed[0])


def host_case(c, M, seed=C.SEED, users=None):
    tables = dict(wu=c["wu"], wi=c["wi"]) if M > 1 else {}
    return host_entry(C.users_for(c, M) if users is None else users, c["item_all"], c["user_ptr"], c["user_items"], M, seed, c["cdf"],
                      d=c["d"], **tables)


def test_abi_surface():
    from sml_amd import _lib
    text = open(os.path.join(REPO, "include", "sml_hip.h")).read()
    header = re.sub(r"\s+", " ", " ".join(re.sub(r"^\s*\*", " ", line) for line in text.splitlines()))
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "training negatives" in header
    for phrase in ("first M admissible candidates in order of c", "restricted to c < 4096", "A NaN score loses to every non-NaN score",
                   "the smaller c wins", "cand_4095", "bisect right", "Entries of zero mass are never drawn", "any grid gives the same bytes",
                   "byte for byte", "prefix of the pool for M' > M"):
        assert phrase in header, phrase
    assert "left at -1" not in header, "the stale sentence of sml_sample_negatives"
    assert len(_lib.SIGNATURES["sml_sample_negatives_ex"][1]) == 19 and len(_lib.SIGNATURES["sml_host_sample_negatives_ex"][1]) == 16
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m sml_amd.build)"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in exported.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name
    assert "neg_sampler.hip" in __import__("sml_amd.build", fromlist=["SOURCES"]).SOURCES
    dev_h = open(os.path.join(REPO, "sml_amd", "csrc", "sml_dev.h")).read()
    for fn in ("uint64_t neg_draw", "int64_t neg_candidate_pos", "bool neg_is_own"):
        assert re.search(r"__host__ __device__ __forceinline__ %s\(" % re.escape(fn), dev_h), fn
    assert dev_h.count("0x9e3779b97f4a7c15") == 1, "the stream's constants exist once"


def _sample(c, M, k=24):
    users = C.users_for(c, M)
    special = [int(np.nonzero(users == u)[0][0]) for u in (C.U_EMPTY, C.U_BUT3, C.U_BUT1, C.U_ALL, C.U_OUT) if (users == u).any()]
    if M == 1:
        special.append(int(np.nonzero(users == C.U_FAR)[0][0]))
    rest = np.random.RandomState(M).permutation(c["n"])[:k].tolist()
    return users, sorted(set(special + rest + [c["n"] - 1]))


@pytest.mark.parametrize("case", [("uniform", 32), ("alpha075", 32), ("flat", 64), ("last", 32)], ids=lambda c: "%s-d%d" % c)
def test_restatement_agrees_with_its_literal_form(case):
    """The numpy walk over all elements equals the definition read one candidate at a time, on every special user and a
    sample of the others; pools are prefixes of one another."""
    c = C.case(*case)
    for M in (1, 3, 64):
        negs, score, failed = C.walk(case[0], case[1], M)
        users, sample = _sample(c, M)
        for e in sample:
            neg, s, f, pool = C.walk_one(c, users, e, M)
            assert int(negs[e]) == neg, (M, e)
            if M > 1:
                assert np.float32(score[e]).tobytes() == np.float32(s).tobytes(), (M, e)
            if M == 64:
                for m in (1, 2, 33):
                    assert C.walk_one(c, users, e, m)[3] == pool[:m]


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_host_entry_equals_the_restatement(case):
    c = C.case(*case)
    fails = set()
    for M in C.POOLS:
        want_negs, want_score, want_failed = C.walk(case[0], case[1], M)
        negs, score, failed = host_case(c, M)
        assert failed == want_failed, M
        assert negs.tobytes() == want_negs.tobytes(), M
        if M > 1:
            assert score.tobytes() == want_score.tobytes(), M
            fails.add(failed)
        else:
            assert (score == -7.0).all(), "score is written for M > 1 only"
        assert np.isin(negs, c["item_all"]).all()
    assert len(fails) == 1, "the failures do not depend on the pool"
    # another seed: other bytes, again the restatement's
    negs, score, failed = host_case(c, 8, seed=C.SEED + 1)
    other = C.walk(case[0], case[1], 8, seed=C.SEED + 1)
    assert (negs.tobytes(), score.tobytes(), failed) == (other[0].tobytes(), other[1].tobytes(), other[2])
    if case[0] not in ("first", "last", "pop1"):
        assert negs.tobytes() != C.walk(case[0], case[1], 8)[0].tobytes()
    # score not asked for
    again, none, _ = host_entry(c["users"], c["item_all"], c["user_ptr"], c["user_items"], 8, C.SEED, c["cdf"], c["wu"], c["wi"], c["d"],
                                want_score=False)
    assert none is None and again.tobytes() == C.walk(case[0], case[1], 8)[0].tobytes()


def test_cases_cover_what_they_claim():
    """What the seeded cases exercise, counted on the restatement (case uniform, d = 32, seed 2024)."""
    c = C.case("uniform", 32)
    users = c["users"]
    count, pc, pi, last, S, last_S = C.pooled("uniform", 32, 64)
    assert c["n"] == 4099 and len(c["item_all"]) == 257 and len(np.unique(users)) < c["n"] // 10
    assert c["item_all"][-1] - c["item_all"][0] + 1 > 257, "ids with gaps"
    but1, but3, own_all, empty = (np.nonzero(users == u)[0] for u in (C.U_BUT1, C.U_BUT3, C.U_ALL, C.U_EMPTY))
    assert ((count[but1] > 0) & (count[but1] < 64)).any(), "all but one: the cap arrives with a partial pool"
    assert (count[but1] > 1).any() and all(len(set(pi[e, :count[e]])) == 1 for e in but1), "the one item, again and again"
    assert (count[but3] >= 8).all() and (pc[but3, 7] >= 128).all(), "all but three: the pool of 8 fills over several rounds"
    assert all(len(set(pi[e, :8])) <= 3 for e in but3), "with repeats"
    assert (count[own_all] == 0).all() and len(own_all) > 1
    assert (count[empty] == 64).all() and (pc[empty, 63] == 63).all(), "no history: the first 64 candidates"
    # ties between different ids at the top of a pool, a NaN row inside a pool, subnormal chosen scores
    negs, score, failed = C.walk("uniform", 32, 64)
    top = (S == score[:, None]) & (np.arange(64)[None, :] < count[:, None])
    assert sum(len(set(pi[e, top[e]])) > 1 for e in range(c["n"])) > 20, "exact copies under several ids tie at the top"
    assert np.isin(pi, c["planted"]["nan_items"]).any() and np.isnan(S[np.arange(64)[None, :] < count[:, None]]).any()
    assert not np.isnan(score[count > 0]).any()
    tiny = (users == C.U_TINY) & (count > 0)
    assert tiny.sum() > 10 and (np.abs(score[tiny]) < np.float32(2.0 ** -126)).all() and (score[tiny] != 0).any(), "subnormal scores win"
    assert len(set(score[tiny].tolist())) >= 2
    assert failed == len(own_all)


def test_m1_without_cdf_is_draw_negatives_walk():
    c = C.case("uniform", 32)
    negs, _, failed = host_case(c, 1)
    users, sample = _sample(c, 1, k=300)
    for e in sample:
        neg, f = C.draw_negative_walk(c, users, e)
        assert int(negs[e]) == neg, e
    assert failed == int((users == C.U_ALL).sum())


@pytest.mark.parametrize("case", [("uniform", 64), ("alpha075", 32)], ids=lambda c: "%s-d%d" % c)
def test_prefix_property_and_score_monotonicity(case):
    """The pool for M is a prefix of the pool for M' > M (the restatement's pools are one list cut at M; the host entry
    agrees with it), so the chosen score never decreases as M grows, from the score of the M = 1 negative on."""
    c = C.case(*case)
    users = c["users"]
    first, _, _ = host_case(c, 1, users=users)
    prev = chain(c["wu"][users], c["wi"][first], "kernel")
    count, pc, pi, last, S, last_S = C.pooled(case[0], case[1], 64)
    assert (first[count > 0] == pi[count > 0, 0]).all()
    grew = 0
    for M in C.POOLS[1:]:
        negs, score, _ = host_case(c, M)
        worse = (~np.isnan(prev) & np.isnan(score)) | (prev > score)
        assert not worse.any(), M
        grew += int((score > prev).sum())
        prev = score
    assert grew > c["n"]


def _no_history():
    return np.zeros(2, np.int64), np.zeros(1, np.int64)          # one user, an empty range


def test_popularity_distribution_within_five_sigma():
    """200,000 draws over pop = 50 with the alpha = 0.75 cdf of skewed counts (seed 2024): every item's frequency within
    5 sigma, sigma = sqrt(p (1 - p) / n).  The restatement meets the bound on its own; the host entry is its bytes."""
    from sml_amd.sampling import popularity_cdf
    n, pop = 200000, 50
    rng = np.random.RandomState(50)
    item_all = np.sort(rng.permutation(500)[:pop]).astype(np.int64)
    col = item_all[np.minimum((rng.pareto(1.0, 5000) * 4).astype(np.int64), pop - 1)]
    col = col[~np.isin(col, item_all[[7, 30]])]
    cdf = popularity_cdf(item_all, col, 0.75)
    p = np.diff(np.concatenate([[0.0], cdf]))
    assert p.min() == 0.0 and p.max() > 20 * p[p > 0].min(), "skewed, with items nobody has"
    ptr, items = _no_history()
    users = np.zeros(n, np.int64)
    c = dict(item_all=item_all, user_ptr=ptr, user_items=items, cdf=cdf)
    count, pc, pi, last = C.pools(c, users, C.SEED, first=1, keep=1)
    for negs in (pi[:, 0], host_entry(users, item_all, ptr, items, 1, C.SEED, cdf)[0]):
        freq = np.array([(negs == i).sum() for i in item_all]) / n
        sigma = np.sqrt(p * (1 - p) / n)
        print("worst deviation in sigma:", np.nanmax(np.abs(freq - p)[p > 0] / sigma[p > 0]))
        assert (np.abs(freq - p) <= 5 * sigma).all()
    assert host_entry(users, item_all, ptr, items, 1, C.SEED, cdf)[0].tobytes() == pi[:, 0].tobytes()


def test_hardest_of_two_distribution_within_five_sigma():
    """M = 2, uniform draws, no Seen, scores strictly ordered by id: the item with the r-th lowest score is chosen with
    probability (2 r - 1) / pop^2; 200,000 draws over pop = 50 (seed 2024), every frequency within 5 sigma."""
    n, pop, d = 200000, 50, 32
    item_all = np.arange(pop, dtype=np.int64)
    wu = np.zeros((1, d), np.float32)
    wu[0, 0] = 1.0
    wi = np.zeros((pop, d), np.float32)
    wi[:, 0] = np.arange(1, pop + 1)
    ptr, items = _no_history()
    users = np.zeros(n, np.int64)
    c = dict(item_all=item_all, user_ptr=ptr, user_items=items, cdf=None, wu=wu, wi=wi)
    count, pc, pi, last = C.pools(c, users, C.SEED, first=2, keep=2)
    assert (count == 2).all()
    want = np.maximum(pi[:, 0], pi[:, 1])
    negs, score, failed = host_entry(users, item_all, ptr, items, 2, C.SEED, None, wu, wi, d)
    assert failed == 0 and negs.tobytes() == want.tobytes() and (score == (negs + 1).astype(np.float32)).all()
    r = np.arange(1, pop + 1)
    p = (2 * r - 1) / float(pop * pop)
    freq = np.bincount(negs, minlength=pop) / n
    sigma = np.sqrt(p * (1 - p) / n)
    print("worst deviation in sigma:", np.max(np.abs(freq - p) / sigma))
    assert abs(p.sum() - 1.0) < 1e-12 and (np.abs(freq - p) <= 5 * sigma).all()


def test_popularity_cdf_bytes_and_sampler_arguments():
    from sml_amd import sampling
    rng = np.random.RandomState(9)
    item_all = np.sort(rng.permutation(400)[:120]).astype(np.int64)
    col = rng.randint(0, 400, 5000)                              # ids outside item_all too; some of item_all never
    col = col[~np.isin(col, item_all[:5])]
    for alpha in (0.75, 1.0, 0.3):
        got = sampling.popularity_cdf(item_all, col, alpha)
        assert got.dtype == np.float64 and got.tobytes() == C.counts_cdf(item_all, col, alpha).tobytes()
        assert got[4] == 0.0 and got[-1] == 1.0 and sampling.check_cdf(got, 120) is not None
    assert sampling.popularity_cdf(item_all, col, 0) is None and sampling.popularity_cdf(item_all, col, 0.0) is None
    assert sampling.NegativeSampler().is_default and sampling.NegativeSampler().cdf(item_all, col) is None
    s = sampling.NegativeSampler(pool=4, alpha=0.75)
    assert not s.is_default and s.cdf(item_all, col).tobytes() == C.counts_cdf(item_all, col, 0.75).tobytes()
    assert sampling.NegativeSampler(1, 0.5).tables(None) == (None, None)
    with pytest.raises(ValueError, match="pass the model"):
        s.tables(None)
    with pytest.raises(ValueError, match="no item"):
        sampling.popularity_cdf(item_all, np.array([100000]), 0.5)
    for bad in (dict(pool=0), dict(pool=65), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(ValueError):
            sampling.NegativeSampler(**bad)
    good = np.array([0.0, 0.25, 0.25, 1.0])
    assert sampling.check_cdf(good, 4).tobytes() == good.tobytes()
    for bad, pop in ((good.astype(np.float32), 4), (good, 5), (np.array([0.0, 0.5, 0.4, 1.0]), 4), (np.array([0.0, 0.5, 0.999999]), 3),
                     (np.array([0.0, np.nan, 1.0]), 3), (np.array([-0.1, 1.0]), 2), (good.reshape(2, 2), 4), (np.zeros(0), 0),
                     (np.array([0.5, 1.0 + 2.0 ** -52]), 2)):
        with pytest.raises(ValueError, match="cdf"):
            sampling.check_cdf(bad, pop)
    with pytest.raises(ValueError, match="cdf"):
        sampling.device_cdf(np.array([0.5, 0.9]), "cpu")
    assert sampling.device_cdf(good, "cpu").tensor.dtype == torch.float64


def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    c = C.case("uniform", 32)
    users = np.ascontiguousarray(c["users"][:16])
    negs, score, failed = np.zeros(16, np.int64), np.zeros(16, np.float32), np.zeros(1, np.int32)
    base = dict(users=users.ctypes.data, n=16, item_all=c["item_all"].ctypes.data, pop=len(c["item_all"]), user_ptr=c["user_ptr"].ctypes.data,
                n_users=C.N_USERS, user_items=c["user_items"].ctypes.data, cdf=None, pool=2, wu=c["wu"].ctypes.data, wi=c["wi"].ctypes.data,
                d=32, seed=1, negs=negs.ctypes.data, score=score.ctypes.data, failed=failed.ctypes.data)
    order = ("users", "n", "item_all", "pop", "user_ptr", "n_users", "user_items", "cdf", "pool", "wu", "wi", "d", "seed", "negs", "score", "failed")

    def call(**kw):
        a = dict(base, **kw)
        return lib.sml_host_sample_negatives_ex(*[a[k] for k in order])
    assert call() == 0 and call(score=None) == 0 and call(pool=1, wu=None, wi=None, d=0) == 0 and call(n=0) == 0
    for kw in (dict(pool=0), dict(pool=65), dict(pool=-1), dict(wu=None), dict(wi=None), dict(d=48), dict(d=128), dict(users=None),
               dict(item_all=None), dict(user_ptr=None), dict(user_items=None), dict(negs=None), dict(failed=None), dict(pop=0), dict(pop=-3),
               dict(n=-1), dict(n_users=-1), dict(wu=c["wu"].ctypes.data + 4)):
        assert call(**kw) != 0, kw
        with pytest.raises(_lib.SmlError, match="sml_host_sample_negatives_ex"):
            _lib.check(call(**kw), "host walk")
    # the device entry refuses before it touches a device
    rc = lib.sml_sample_negatives_ex(None, *[base[k] for k in order[:13]], 0, base["negs"], base["score"], base["failed"], None)
    assert rc != 0
    with pytest.raises(_lib.SmlError, match=r"sml_sample_negatives_ex"):
        _lib.check(rc, "device entry")


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", "neg_sampler.hip"))
    names = [r["name"] for r in rows]
    for want in ("k_neg_one", "k_neg_pool<32>", "k_neg_pool<64>"):
        assert any(want in n for n in names), names
    for r in rows:
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r
        assert r.get("LDS Size [bytes/block]", 0) == 0, r


# ---- the baseline's control flow, with an engine double ---------------------------------------------------------------

class EngineDouble(object):
    """HipEngine's surface as far as SPMF._epoch and epoch_triples_device touch it, on the CPU; records every call."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = []

    def device_epoch(self, ui, n, seed, mat=None, row_stride=1, col=0):
        self.calls.append(("device_epoch", int(seed)))
        out = torch.zeros((int(n), 3), dtype=torch.int64)
        out[:, :2] = ui
        return out

    def sample_negatives(self, users, item_all, user_ptr, user_items, seed):
        self.calls.append(("sample_negatives", int(seed)))
        return item_all[torch.zeros_like(users)], torch.zeros(1, dtype=torch.int32)

    def sample_negatives_ex(self, users, item_all, user_ptr, user_items, seed, pool=1, cdf=None, w_user=None, w_item=None,
                            want_score=False, max_workgroups=0):
        self.calls.append(("sample_negatives_ex", int(seed), int(pool), cdf, w_user, w_item))
        return item_all[torch.zeros_like(users)], torch.zeros(1, dtype=torch.int32)

    def bare_adam_epoch(self, mf, tri, batch_size, lr, lu, li, bce=True):
        self.calls.append(("bare_adam_epoch", type(tri).__name__, tuple(tri.shape)))
        return np.array([0.5, 0.25], dtype=np.float32)

    def mf_flush(self, mf):
        self.calls.append(("mf_flush",))


def _baseline(eng, **over):
    from sml_amd.baseline import SPMF
    args = types.SimpleNamespace(lr=0.01, pool_size=0, neg_num=1, batch_size=64, l2_u=1e-5, l2_i=1e-5, epochs=2, pool_init_type=0)
    for k, v in over.items():
        setattr(args, k, v)
    rng = np.random.RandomState(4)
    train = np.stack([rng.randint(0, 30, 200), rng.randint(0, 40, 200)], 1).astype(np.int64)
    test = np.stack([rng.randint(0, 30, 20), rng.randint(0, 40, 20), rng.randint(0, 40, 20)], 1).astype(np.int64)
    data = types.SimpleNamespace(test_new_user=np.zeros(0, np.int64), test_new_item=np.zeros(0, np.int64),
                                 get_next=lambda stage_id, types="only_new": (train, test) if stage_id < 9 else (None, None))
    with contextlib.redirect_stdout(io.StringIO()):
        sp = SPMF(args, data, 30, 40, 32, device="cpu", engine=eng)
    sp.test = lambda rows, topk=(5, 10, 20): (np.zeros(3), np.zeros(3), 0.0, 0.0)
    return sp, train


def test_sampler_flags_need_the_device_route():
    from sml_amd.baseline import get_parse
    a = get_parse().parse_args([])
    assert (a.neg_pool, a.neg_pop_alpha, a.device_batches) == (1, 0.0, 0)
    a = get_parse().parse_args(["--neg_pool", "4", "--neg_pop_alpha", "0.75", "--device_batches", "1"])
    assert (a.neg_pool, a.neg_pop_alpha, a.device_batches) == (4, 0.75, 1)
    for over in (dict(neg_pool=4), dict(neg_pop_alpha=0.75), dict(neg_pool=4, device_batches=0), dict(neg_pop_alpha=0.5, device_batches=0)):
        with pytest.raises(ValueError, match="--device_batches 1"):
            _baseline(EngineDouble(), **over)
    with pytest.raises(ValueError, match="pool"):
        _baseline(EngineDouble(), neg_pool=65, device_batches=1)
    _baseline(EngineDouble(), neg_pool=1, neg_pop_alpha=0.0)      # the defaults, spelled out: the host route


@pytest.mark.parametrize("method", ["full", "fine"])
def test_full_and_fine_honour_device_batches(method):
    seed = lambda stage, epoch: (2002 * 1000003 + stage) * 1000003 + epoch
    kind = "not_only_new" if method == "full" else "only_new"
    # the host route: no device call, numpy's stream is consumed
    eng = EngineDouble()
    sp, train = _baseline(eng)
    np.random.seed(1)
    torch.manual_seed(1)
    before = np.random.get_state()[1].copy()
    with contextlib.redirect_stdout(io.StringIO()):
        assert sp.run_one_stage2(3, read_data_type=kind)
    assert [c[0] for c in eng.calls] == ["bare_adam_epoch", "mf_flush"] * 2 and eng.calls[0][1] == "ndarray"
    assert not np.array_equal(before, np.random.get_state()[1])
    # the device route, default sampler: device_epoch + sample_negatives keyed by (stage, epoch); no numpy or torch draw
    eng = EngineDouble()
    sp, train = _baseline(eng, device_batches=1)
    np.random.seed(1)
    torch.manual_seed(1)
    np_before, torch_before = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    with contextlib.redirect_stdout(io.StringIO()) as out:
        assert sp.run_one_stage2(3, read_data_type=kind)
    assert eng.calls == [("device_epoch", seed(3, 0)), ("sample_negatives", seed(3, 0) + 1), ("bare_adam_epoch", "Tensor", (200, 3)), ("mf_flush",),
                         ("device_epoch", seed(3, 1)), ("sample_negatives", seed(3, 1) + 1), ("bare_adam_epoch", "Tensor", (200, 3)), ("mf_flush",)]
    assert np.array_equal(np_before, np.random.get_state()[1]) and torch.equal(torch_before, torch.get_rng_state())
    assert out.getvalue().count("loss:0.3750") == 2
    # another sampler: sample_negatives_ex with the set's popularity cdf and the model's tables
    eng = EngineDouble()
    sp, train = _baseline(eng, device_batches=1, neg_pool=4, neg_pop_alpha=0.75)
    with contextlib.redirect_stdout(io.StringIO()):
        assert sp.run_one_stage2(4, read_data_type=kind)
    ex = [c for c in eng.calls if c[0] == "sample_negatives_ex"]
    assert [c[:3] for c in ex] == [("sample_negatives_ex", seed(4, 0) + 1, 4), ("sample_negatives_ex", seed(4, 1) + 1, 4)]
    assert not any(c[0] == "sample_negatives" for c in eng.calls)
    item_all = np.unique(train[:, 1])
    assert ex[0][3].tensor.numpy().tobytes() == C.counts_cdf(item_all, train[:, 1], 0.75).tobytes() and ex[1][3] is ex[0][3]
    assert ex[0][4] is sp.MFbase.user_laten.weight.data or ex[0][4].data_ptr() == sp.MFbase.user_laten.weight.data_ptr()
    assert ex[0][5].data_ptr() == sp.MFbase.item_laten.weight.data_ptr()
    # popularity alone: no tables are passed
    eng = EngineDouble()
    sp, train = _baseline(eng, device_batches=1, neg_pop_alpha=0.5)
    with contextlib.redirect_stdout(io.StringIO()):
        assert sp.run_one_stage2(4, read_data_type=kind)
    ex = [c for c in eng.calls if c[0] == "sample_negatives_ex"]
    assert len(ex) == 2 and ex[0][2] == 1 and ex[0][4] is None and ex[0][5] is None and ex[0][3] is not None


def test_epoch_triples_device_default_is_the_old_call():
    from sml_amd.datasets import offlineDataset_withsample
    from sml_amd.sampling import NegativeSampler
    rng = np.random.RandomState(2)
    rows = np.stack([rng.randint(0, 9, 50), rng.randint(0, 12, 50)], 1).astype(np.int64)
    with contextlib.redirect_stdout(io.StringIO()):
        train = offlineDataset_withsample(rows)
    eng = EngineDouble()
    train.epoch_triples_device(eng, 77)
    assert eng.calls == [("device_epoch", 77), ("sample_negatives", 78)]
    eng.calls = []
    train.epoch_triples_device(eng, 77, sampler=NegativeSampler())
    assert [c[:3] for c in eng.calls] == [("device_epoch", 77), ("sample_negatives_ex", 78, 1)] and eng.calls[1][3:] == (None, None, None)
    with pytest.raises(ValueError, match="pass the model"):
        train.epoch_triples_device(eng, 77, sampler=NegativeSampler(pool=2))
