"""Test-set negatives on the MI355X (sml_neg_sets through HipEngine.neg_sets and sml_amd.prepare).

The defining identity: the kernel's rows and its failure counter equal the plain-Python restatement of the definition
(tests/_neg_sets_ref.py, which shares no code with the product and is pinned on the CPU by tests/test_neg_sets_host.py) byte
for byte, whatever the grid, for neg_num on both sides of the 64-lane round, catalogues that grow inside a period, repeated
(u, i) pairs, new users, and rows that are served beside rows that fail."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _neg_sets_ref as R
from conftest import REPO, make_mf, needs_gpu
from test_neg_sets_host import g17, host_entry

pytestmark = needs_gpu
DEV = "cuda:0"


def engine(d=32):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


_TL = {}


def timeline(name, stream, n_user, n_item):
    from sml_amd.prepare import Timeline
    if name not in _TL:
        _TL[name] = Timeline(stream, n_user, n_item, engine())
    return _TL[name]


def device_periods(tl, start, neg_num, seed=R.SEED, max_workgroups=0, rows=None):
    outs, fails = [], []
    for p in range(start, len(tl)):
        out, failed = engine().neg_sets(tl.rows[p] if rows is None else rows[p], tl.g0[p], tl, neg_num, seed, max_workgroups)
        assert out.dtype == torch.int64 and out.shape == (tl.rows[p].shape[0], 2 + neg_num) and failed.dtype == torch.int32
        outs.append(out.cpu().numpy())
        fails.append(int(failed))
    return outs, fails


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("name", list(R.CASES))
def test_identity_with_the_restatement(name):
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case(name)
    tl = timeline(name, stream, n_user, n_item)
    for g, w in zip(tl.host(), R.timeline_arrays(stream, n_user, n_item)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    got, got_fails = device_periods(tl, start, neg_num)
    same(got, outs, name)
    assert got_fails == fails
    # launch geometry: one workgroup, seven, the kernel's own choice -- and the same call again
    for mw in (1, 7, 0):
        again, again_fails = device_periods(tl, start, neg_num, max_workgroups=mw)
        same(again, got, "%s max_workgroups=%d" % (name, mw))
        assert again_fails == fails
    # another seed: other bytes (where anything is drawn), the same rows failing
    other, other_fails = device_periods(tl, start, neg_num, seed=R.SEED + 1)
    assert other_fails == fails and any(g.tobytes() != w.tobytes() for g, w in zip(other, got))
    # rows from a host array, and device rows that carry further columns
    host_rows = [np.ascontiguousarray(p) for p in stream]
    same(device_periods(tl, start, neg_num, rows=host_rows)[0], got, name + " host rows")
    wide = [torch.from_numpy(np.concatenate([p, np.full((len(p), 3), 5, np.int64)], 1)).to(DEV) for p in stream]
    same(device_periods(tl, start, neg_num, rows=wide)[0], got, name + " five columns")


def test_device_equals_host_entry():
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case("k999")
    got, got_fails = device_periods(timeline("k999", stream, n_user, n_item), start, neg_num)
    want, want_fails = host_entry(stream, n_user, n_item, neg_num, start)
    same(got, want, "device against sml_host_neg_sets")
    assert got_fails == want_fails == [0, 0]


def test_exact_eligibility():
    stream, n_user, n_item, neg_num, start, outs, fails = R.exact_case()
    tl = timeline("exact", stream, n_user, n_item)
    got, got_fails = device_periods(tl, start, neg_num)
    same(got, outs, "exact")
    assert got_fails == [0] and set(got[0][0, 2:].tolist()) == set(range(12)) - {0, 5, 7, 9}
    short, short_fails = device_periods(tl, start, neg_num + 1)              # one more than the row has: no draw, all -1
    assert short_fails == [1] and (short[0][0, 2:] == -1).all() and (short[0][1, 2:] >= 0).all()


def test_checker_on_device_output_for_the_reference_inputs():
    from sml_amd.prepare import Timeline, period_negatives
    stream, n_user, n_item, neg_num, start, test = g17()
    tl = Timeline(stream, n_user, n_item, engine())
    out = [period_negatives(tl, p, neg_num, seed=5).cpu().numpy() for p in range(start, len(stream))]
    assert all(o.shape == t.shape and o.dtype == np.int64 for o, t in zip(out, test))
    assert R.check_rows(stream, start, out)
    same(out, R.ref_negatives(stream, start, neg_num, 5)[0], "g17 inputs")


def test_refusals():
    from sml_amd._lib import SmlError, check
    from sml_amd.engine import _ptr
    from sml_amd.prepare import Timeline, period_negatives
    from sml_amd.retrieval import SeenItems
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case("k64")
    eng, tl = engine(), timeline("k64", stream, n_user, n_item)
    for bad in (0, 4097):
        with pytest.raises(SmlError, match="neg_num"):
            eng.neg_sets(tl.rows[start], tl.g0[start], tl, bad, 1)
        with pytest.raises(ValueError, match="neg_num"):
            period_negatives(tl, start, bad)
    with pytest.raises(ValueError, match="outside the timeline"):
        eng.neg_sets(tl.rows[start], tl.total - 1, tl, 5, 1)
    rows = torch.zeros((4, 6), device=DEV, dtype=torch.int64)                # an out that is the rows themselves
    failed = torch.zeros(1, device=DEV, dtype=torch.int32)
    with pytest.raises(SmlError, match="overlaps"):
        check(eng.lib.sml_neg_sets(eng._ctx, _ptr(rows), 4, 6, 0, _ptr(tl.n_cat_all), _ptr(tl.order), _ptr(tl.h_off), n_user,
                                   _ptr(tl.h_items), _ptr(tl.h_since), 4, 1, 0, _ptr(rows), _ptr(failed), eng._stream()), "sml_neg_sets")
    for bad in (np.array([[n_user, 0]]), np.array([[0, n_item]]), np.array([[-1, 0]]), np.array([[0, -1]])):
        with pytest.raises(ValueError) as host_err:
            SeenItems(n_user, n_item).add(bad)
        for x in (bad, torch.from_numpy(bad).to(DEV)):
            with pytest.raises(ValueError) as dev_err:
                Timeline([stream[0], x], n_user, n_item, eng)
            assert str(dev_err.value) == str(host_err.value)
    # a period with rows that cannot be served
    p = start
    with pytest.raises(ValueError, match=r"%d of the %d rows of period %d could not get 64 negatives" % (fails[0], len(stream[p]), p)):
        period_negatives(tl, p, neg_num, R.SEED)
    short = period_negatives(tl, p, neg_num, R.SEED, allow_short=True).cpu().numpy()
    assert short.tobytes() == outs[0].tobytes() and int(((short[:, 2:] == -1).all(1)).sum()) == fails[0]


def test_end_to_end(tmp_path):
    from sml_amd import prepare
    from sml_amd.datasets import testDataset
    from sml_amd.evaluation import DeviceRows, test_model
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case("k999")
    base = tmp_path / "toy"
    (base / "train").mkdir(parents=True)
    np.save(base / "information.npy", np.array([sum(len(p) for p in stream), n_user, n_item], dtype=np.int64))
    for p, rows in enumerate(stream):
        np.save(base / "train" / ("%d.npy" % p), rows)
    before = set(str(q.relative_to(tmp_path)) for q in tmp_path.rglob("*") if q.is_file())
    prepare.select_neg_forinteraction(str(tmp_path) + os.sep, "toy", [str(p) for p in range(len(stream))], leave_for_init_train=0.5,
                                      neg_num=neg_num, seed=R.SEED, engine=engine())
    after = set(str(q.relative_to(tmp_path)) for q in tmp_path.rglob("*") if q.is_file())
    assert sorted(after - before) == [os.path.join("toy", "test", "%d.npy" % i) for i in range(start, len(stream))] and before <= after
    files = [np.load(base / "test" / ("%d.npy" % i)) for i in range(start, len(stream))]
    same(files, outs, "test files")
    assert R.check_rows(stream, start, files)
    # the evaluation takes them as they are
    mf = make_mf(n_user, n_item, 32, device=DEV)
    hits, ndcg, idx = mf.test(torch.from_numpy(files[0]).to(DEV), topK=20)
    assert 0 <= hits <= len(files[0])
    assert len(testDataset(files[0])) == len(files[0]) and testDataset(files[0])[3].shape == (2 + neg_num,)
    recall, _ = test_model(mf, DeviceRows(files[0], DEV), topK=20)
    assert recall == pytest.approx(hits / len(files[0]))
    # the command line, in a process of its own
    for f in (base / "test").iterdir():
        f.unlink()
    run = subprocess.run([sys.executable, "-m", "sml_amd.prepare", "--data_path", str(tmp_path) + os.sep, "--data_name", "toy", "--periods",
                          str(len(stream)), "--leave", "0.5", "--neg_num", str(neg_num), "--seed", str(R.SEED)], cwd=REPO,
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    same([np.load(base / "test" / ("%d.npy" % i)) for i in range(start, len(stream))], outs, "test files of the command line")
