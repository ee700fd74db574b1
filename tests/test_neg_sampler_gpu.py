"""Training negatives on the MI355X (sml_sample_negatives_ex through HipEngine.sample_negatives_ex, the datasets and the
baseline's command line).

The defining identity: the kernels' negatives, scores and failure counter equal the plain-Python restatement of the
definition (tests/_neg_sampler_cases.py, which shares no code with the product and is pinned on the CPU by
tests/test_neg_sampler_host.py) byte for byte, whatever the grid, for pools on both sides of every group width, with and
without a popularity cdf.  Every test runs under a watchdog of its own: a launch that does not come back ends the process
instead of letting the next test start on the same device; the command-line runs are child processes with a time limit."""
import contextlib
import faulthandler
import io
import os
import re

import numpy as np
import pytest
import torch

import _neg_sampler_cases as C
from _fp32_chain import chain
from conftest import REPO, make_mf, needs_gpu

pytestmark = needs_gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(150, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def engine(d=32):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_DEV = {}


def on_device(case):
    if case not in _DEV:
        c = C.case(*case)
        _DEV[case] = {k: gpu(c[k]) for k in ("item_all", "user_ptr", "user_items", "wu", "wi", "users", "users1")}
    return _DEV[case]


def device_walk(case, M, seed=C.SEED, max_workgroups=0, users=None):
    """(negs bytes, score bytes or None, failed) of the kernel on a case"""
    c, t = C.case(*case), on_device(case)
    users = t["users1" if M == 1 else "users"] if users is None else users
    tables = dict(w_user=t["wu"], w_item=t["wi"]) if M > 1 else {}
    negs, failed, score = engine(case[1]).sample_negatives_ex(users, t["item_all"], t["user_ptr"], t["user_items"], seed, pool=M, cdf=c["cdf"],
                                                              want_score=True, max_workgroups=max_workgroups, **tables)
    assert negs.dtype == torch.int64 and negs.shape == (c["n"],) and failed.dtype == torch.int32 and failed.shape == (1,)
    assert (score is None) == (M == 1) and (score is None or (score.dtype == torch.float32 and score.shape == (c["n"],)))
    return negs.cpu().numpy().tobytes(), None if score is None else score.cpu().numpy().tobytes(), int(failed)


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_identity_with_the_restatement(case):
    for M in C.POOLS:
        negs, score, failed = C.walk(case[0], case[1], M)
        want = (negs.tobytes(), None if score is None else score.tobytes(), failed)
        got = device_walk(case, M)
        assert got[2] == want[2], M
        assert got[0] == want[0], (M, np.argwhere(np.frombuffer(got[0], np.int64) != negs)[:4].tolist())
        assert got[1] == want[1], M
        # launch geometry: one workgroup, seven, the kernel's own choice -- and the same call again
        for mw in (1, 7, 0):
            assert device_walk(case, M, max_workgroups=mw) == got, (M, mw)
    # another seed: again the restatement's bytes; other bytes wherever more than one item can be drawn; the same elements
    # fail wherever failing is decided by the user's items alone (under a popularity cdf it also depends on the draws)
    negs, score, failed = C.walk(case[0], case[1], 8, seed=C.SEED + 1)
    other = device_walk(case, 8, seed=C.SEED + 1)
    assert other == (negs.tobytes(), score.tobytes(), failed)
    if case[0] not in ("first", "last", "pop1"):
        assert other[0] != device_walk(case, 8)[0]
    if case[0] != "alpha075":
        assert other[2] == device_walk(case, 8)[2]


@pytest.mark.parametrize("case", [("uniform", 32), ("uniform", 64)], ids=lambda c: "%s-d%d" % c)
def test_pool_one_without_cdf_is_sample_negatives(case):
    """pool=1, cdf=None: the bytes of the sampler the device batch supply has had all along, users outside the CSR included."""
    t = on_device(case)
    eng = engine(case[1])
    for seed in (C.SEED, 7):
        old, old_failed = eng.sample_negatives(t["users1"], t["item_all"], t["user_ptr"], t["user_items"], seed)
        for mw in (0, 3):
            new, new_failed = eng.sample_negatives_ex(t["users1"], t["item_all"], t["user_ptr"], t["user_items"], seed, max_workgroups=mw)
            assert new.cpu().numpy().tobytes() == old.cpu().numpy().tobytes() and int(new_failed) == int(old_failed) > 0
    # and the host entry
    from test_neg_sampler_host import host_case
    negs, _, failed = host_case(C.case(*case), 1)
    old, old_failed = eng.sample_negatives(t["users1"], t["item_all"], t["user_ptr"], t["user_items"], C.SEED)
    assert negs.tobytes() == old.cpu().numpy().tobytes() and failed == int(old_failed)


def test_device_equals_host_entry():
    from test_neg_sampler_host import host_case
    for case, M in ((("uniform", 64), 33), (("flat", 64), 3), (("alpha075", 32), 64)):
        negs, score, failed = host_case(C.case(*case), M)
        assert device_walk(case, M) == (negs.tobytes(), score.tobytes(), failed)


def _dataset():
    from sml_amd.datasets import offlineDataset_withsample
    rng = np.random.RandomState(18)
    rows = np.stack([rng.randint(0, 70, 4099), np.minimum((rng.pareto(1.1, 4099) * 20).astype(np.int64), 299)], 1).astype(np.int64)
    with contextlib.redirect_stdout(io.StringIO()):
        train = offlineDataset_withsample(rows)
    wu = (rng.randn(70, 32) * 0.4).astype(np.float32)
    wi = (rng.randn(300, 32) * 0.4).astype(np.float32)
    return train, make_mf(70, 300, 32, wu, wi, device=DEV), wu, wi


def test_epoch_triples_device_with_a_sampler():
    from sml_amd.sampling import NegativeSampler, popularity_cdf
    train, mf, wu, wi = _dataset()
    eng = engine(32)
    seed = 991
    plain = train.epoch_triples_device(eng, seed).cpu().numpy()
    same = train.epoch_triples_device(eng, seed, sampler=NegativeSampler()).cpu().numpy()
    assert plain.tobytes() == same.tobytes() and int(train._last_failed) == 0
    assert sorted(map(tuple, plain[:, :2].tolist())) == sorted(map(tuple, train._ui.tolist())), "a permutation of the rows"
    # pool = 8: the shuffle is the same, column 2 is the restatement run on column 0 with seed + 1
    tri = train.epoch_triples_device(eng, seed, sampler=NegativeSampler(pool=8), model=mf).cpu().numpy()
    assert tri[:, :2].tobytes() == plain[:, :2].tobytes()
    users = np.ascontiguousarray(tri[:, 0])
    c = dict(item_all=train.item_all.astype(np.int64), user_ptr=train._uptr, user_items=train._uitems, cdf=None, wu=wu, wi=wi)
    count, pc, pi, last = C.pools(c, users, seed + 1, keep=8)
    S, last_S = C.scores(c, users, count, pi, last)
    negs, score, failed = C.choose(count, pi, S, last, last_S, 8)
    assert failed == 0 and tri[:, 2].tobytes() == negs.tobytes()
    assert (pi[:, 0] == plain[:, 2]).all(), "the pool's first member is the uniform sampler's negative"
    # its score is never below the score of the pool = 1 negative
    t = lambda a: gpu(np.ascontiguousarray(a, dtype=np.int64))
    got, _, got_score = eng.sample_negatives_ex(t(users), t(train.item_all), t(train._uptr), t(train._uitems), seed + 1, pool=8,
                                                w_user=mf.user_laten.weight.data, w_item=mf.item_laten.weight.data, want_score=True)
    assert got.cpu().numpy().tobytes() == negs.tobytes() and got_score.cpu().numpy().tobytes() == score.tobytes()
    first = chain(wu[users], wi[plain[:, 2]], "kernel")
    assert (got_score.cpu().numpy() >= first).all() and (got_score.cpu().numpy() > first).sum() > len(users) // 2
    # popularity: the cdf of the set's own item column, the pool's tables not needed
    tri = train.epoch_triples_device(eng, seed, sampler=NegativeSampler(alpha=0.75)).cpu().numpy()
    c["cdf"] = popularity_cdf(train.item_all, train.item, 0.75)
    count, pc, pi, last = C.pools(c, users, seed + 1, keep=1)
    assert tri[:, 2].tobytes() == C.choose(count, pi, None, last, None, 1)[0].tobytes() and tri[:, 2].tobytes() != plain[:, 2].tobytes()
    with pytest.raises(ValueError, match="pass the model"):
        train.epoch_triples_device(eng, seed, sampler=NegativeSampler(pool=2))


def test_wrapper_refusals():
    """Indices outside the tables, and a cdf that is not one, are refused on the host before any launch."""
    from sml_amd._lib import SmlError
    c, t = C.case("uniform", 32), on_device(("uniform", 32))
    eng = engine(32)
    call = lambda users=t["users"], **kw: eng.sample_negatives_ex(users, t["item_all"], t["user_ptr"], t["user_items"], 1, **kw)
    tables = dict(w_user=t["wu"], w_item=t["wi"])
    for pool in (0, 65, -1):
        with pytest.raises(ValueError, match="pool must be in 1..64"):
            call(pool=pool, **tables)
    with pytest.raises(ValueError, match="w_user and w_item are needed"):
        call(pool=2)
    with pytest.raises(ValueError, match="outside the tables"):
        call(users=t["users1"], pool=2, **tables)                       # a user id of 10^6
    with pytest.raises(ValueError, match="outside the tables"):
        call(users=gpu(np.array([-1, 3])), pool=2, **tables)
    with pytest.raises(ValueError, match="outside the tables"):
        call(pool=2, w_user=t["wu"], w_item=t["wi"][:200].contiguous())  # item_all reaches past a 200-row table
    with pytest.raises(ValueError, match="expected a contiguous fp32"):
        call(pool=2, w_user=t["wu"].half(), w_item=t["wi"].half())
    good = np.linspace(0, 1, C.POP + 1)[1:]
    assert call(cdf=good)[0].shape == (c["n"],)
    for bad in (good[:-1], good.astype(np.float32), good * 0.5, good[::-1].copy(), np.where(np.arange(C.POP) == 5, np.nan, good)):
        with pytest.raises(ValueError, match="cdf"):
            call(cdf=bad)
    eng128 = engine(128)
    with pytest.raises(ValueError, match="width 32 or 64"):
        eng128.sample_negatives_ex(t["users"], t["item_all"], t["user_ptr"], t["user_items"], 1, pool=2,
                                   w_user=torch.zeros(72, 128, device=DEV), w_item=torch.zeros(300, 128, device=DEV))
    # the library's own refusal carries the entry point's name
    from sml_amd.engine import _ptr
    negs, failed = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = eng.lib.sml_sample_negatives_ex(eng._ctx, _ptr(t["users"]), 4, _ptr(t["item_all"]), C.POP, _ptr(t["user_ptr"]), C.N_USERS,
                                         _ptr(t["user_items"]), None, 2, None, _ptr(t["wi"]), 32, 1, 0, _ptr(negs), None, _ptr(failed), None)
    with pytest.raises(SmlError, match="sml_sample_negatives_ex"):
        from sml_amd._lib import check
        check(rc, "a NULL table")


def _lines(out):
    """the lines of a baseline run that training decides: losses and test metrics, the wall-clock figure taken out"""
    keep = [l for l in out.splitlines() if l.startswith(("epoch:", "before train test---", "        epoch test---", "FInal test---", "max result",
                                                         "average recall:", "weight average"))]
    return [re.sub(r"time:\d+\.\d+", "time:*", " ".join(l.split())) for l in keep]


def test_cli_spmf_device_mode_with_a_sampler(tmp_path):
    """SPMF's device mode: a non-default sampler redraws column 2 of the rank-weighted epoch; the run trains and differs."""
    from test_spmf_gpu import _cli
    losses = lambda out: [float(l.split("loss:")[1]) for l in out.splitlines() if l.startswith("epoch:")]
    plain = losses(_cli(tmp_path / "a", "--method", "spmf", "--device_batches", "1", "--lr", "0.002"))
    hard = losses(_cli(tmp_path / "b", "--method", "spmf", "--device_batches", "1", "--lr", "0.002", "--neg_pool", "8", "--neg_pop_alpha", "0.5"))
    assert len(plain) == len(hard) == 6 and np.isfinite(hard).all() and plain != hard
    assert hard[0] > plain[0], "the highest-scoring of eight negatives costs more than a uniform one"


def test_cli_fine_with_the_samplers(tmp_path):
    """`model.baseline --method fine` on the synthetic data set of the SPMF command-line test: the default flags print the
    lines recorded from the commit before the sampler existed (tests/golden/g18_fine_default_lines.txt); --device_batches 1
    trains on device-built epochs; --neg_pool 4 --neg_pop_alpha 0.75 prints finite losses, other than --neg_pool 1's."""
    from test_spmf_gpu import _cli
    default = _lines(_cli(tmp_path / "a", "--method", "fine"))
    want = [l.rstrip("\n") for l in open(os.path.join(REPO, "tests", "golden", "g18_fine_default_lines.txt")) if l.strip()]
    assert default == want
    one = _cli(tmp_path / "b", "--method", "fine", "--device_batches", "1", "--neg_pool", "1")
    four = _cli(tmp_path / "c", "--method", "fine", "--device_batches", "1", "--neg_pool", "4", "--neg_pop_alpha", "0.75")
    losses = lambda out: [float(l.split("loss:")[1]) for l in out.splitlines() if l.startswith("epoch:")]
    assert len(losses(one)) == len(losses(four)) == 6 and np.isfinite(losses(one)).all() and np.isfinite(losses(four)).all()
    assert losses(one) != losses(four) and losses(one)[0] != losses(four)[0]
    assert losses(one) != [float(l.split("loss:")[1]) for l in default if l.startswith("epoch:")], "the device route is another stream"
    assert "neg_pool=4" in four.split("parameters:")[1].splitlines()[0] and "neg_pop_alpha=0.75" in four.split("parameters:")[1].splitlines()[0]
