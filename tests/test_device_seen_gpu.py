"""Seen-item sets built and grown on the MI355X (sml_iset_* through HipEngine.iset_* and sml_amd.retrieval.DeviceSeen).

The defining identity: for any sequence of add calls DeviceSeen.host() equals SeenItems.host() after the same calls, byte
for byte -- checked against the numpy reference of tests/_device_seen_cases.py, which shares no code with SeenItems and is
pinned to it on the CPU (tests/test_device_seen_host.py)."""
import contextlib
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from _device_seen_cases import build_cases, random_pairs, ref_contains, ref_set, union_cases
from conftest import REPO, make_mf, needs_gpu

pytestmark = needs_gpu
DEV = "cuda:0"


def engine(d=32):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def same(got, want, what):
    for g, w, part in zip(got, want, ("off", "items")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, part)


@pytest.mark.parametrize("case", build_cases(), ids=lambda c: c[0])
def test_build_identity(case):
    from sml_amd.retrieval import DeviceSeen
    name, n_user, n_item, pairs = case
    want = ref_set([pairs], n_user, n_item)
    seen = DeviceSeen(n_user, n_item, engine())
    assert seen.add(pairs) is seen
    same(seen.host(), want, name)
    assert len(seen) == len(want[1])
    off, items = seen.device(DEV)
    assert off.dtype == torch.int64 and items.dtype == torch.int32 and off.shape[0] == n_user + 1
    assert items.shape[0] == max(len(want[1]), 1)                # one entry when empty: both arrays reach the kernels
    # rows already on the device (all their columns) give the same bytes
    same(DeviceSeen(n_user, n_item, engine()).add(torch.from_numpy(pairs).to(DEV)).host(), want, name + " (device rows)")


def test_engine_calls_take_host_arrays_and_device_tensors():
    rng = np.random.RandomState(5)
    eng = engine()
    a, b = random_pairs(rng, 90, 400, 5000), random_pairs(rng, 90, 400, 700)
    sa, sb = eng.iset_build(a, 90, 400), eng.iset_build(torch.from_numpy(b).to(DEV), 90, 400)
    same([t.cpu().numpy() for t in sa], ref_set([a], 90, 400), "a")
    same([t.cpu().numpy() for t in sb], ref_set([b], 90, 400), "b")
    want = ref_set([a, b], 90, 400)
    same([t.cpu().numpy() for t in eng.iset_union(sa, sb, 90)], want, "device union")
    same([t.cpu().numpy() for t in eng.iset_union(ref_set([a], 90, 400), ref_set([b], 90, 400), 90)], want, "host union")
    same([t.cpu().numpy() for t in sa], ref_set([a], 90, 400), "the inputs are left alone")
    # the width of the engine plays no part
    same([t.cpu().numpy() for t in engine(64).iset_union(sb, sa, 90)], want, "d = 64, sides swapped")
    from sml_amd._lib import SmlError, check
    from sml_amd.engine import _ptr
    scratch = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    room = torch.empty(len(sa[1]) + len(sb[1]), device=DEV, dtype=torch.int32)
    with pytest.raises(SmlError, match="overlaps"):               # an output that aliases an input is refused
        check(eng.lib.sml_iset_union(eng._ctx, 90, _ptr(sa[0]), _ptr(sa[1]), len(sa[1]), _ptr(sb[0]), _ptr(sb[1]), len(sb[1]),
                                     _ptr(scratch), _ptr(sa[0]), _ptr(room), eng._stream()), "sml_iset_union")


@pytest.mark.parametrize("case", union_cases(), ids=lambda c: c[0])
def test_union_identity(case):
    from sml_amd.retrieval import DeviceSeen
    name, n_user, n_item, adds = case
    runs = []
    for _ in range(2):                                           # each sequence twice: equal bytes
        seen = DeviceSeen(n_user, n_item, engine())
        for k, pairs in enumerate(adds):
            seen.add(pairs if k % 2 == 0 else torch.from_numpy(np.ascontiguousarray(pairs)).to(DEV))
            same(seen.host(), ref_set(adds[:k + 1], n_user, n_item), "%s after add %d" % (name, k))
        runs.append(seen.host())
    same(runs[0], runs[1], name + " run twice")


def test_from_seen_then_adds():
    from sml_amd.retrieval import DeviceSeen, SeenItems
    rng = np.random.RandomState(11)
    first, more = random_pairs(rng, 120, 900, 4000), [random_pairs(rng, 120, 900, 1500) for _ in range(2)]
    host = SeenItems(120, 900).add(first)
    seen = DeviceSeen.from_seen(host, engine())
    same(seen.host(), host.host(), "from_seen")
    for p in more:
        same(seen.add(p).host(), host.add(p).host(), "from_seen + add")
    empty = DeviceSeen.from_seen(SeenItems(120, 900), engine())
    assert len(empty) == 0
    same(empty.add(first).host(), ref_set([first], 120, 900), "from an empty SeenItems")


def test_refusals_match_seen_items():
    from sml_amd.retrieval import DeviceSeen, SeenItems
    seen = DeviceSeen(10, 20, engine()).add(np.array([[1, 2]]))
    for bad in (np.array([[10, 0]]), np.array([[0, 20]]), np.array([[-1, 0]]), np.array([[0, -1]]), np.array([[1, 2], [2 ** 32 + 1, 3]])):
        with pytest.raises(ValueError) as host_err:
            SeenItems(10, 20).add(bad)
        for x in (bad, torch.from_numpy(bad).to(DEV)):
            with pytest.raises(ValueError) as dev_err:
                seen.add(x)
            assert str(dev_err.value) == str(host_err.value)
            with pytest.raises(ValueError):
                seen.contains(x)
    with pytest.raises(ValueError) as host_err:
        SeenItems(10, 20).add(np.zeros((3, 1), np.int64))
    with pytest.raises(ValueError) as dev_err:
        seen.add(np.zeros((3, 1), np.int64))
    assert str(dev_err.value) == str(host_err.value)
    same(seen.host(), ref_set([np.array([[1, 2]])], 10, 20), "refused adds leave the set alone")


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 3000])
def test_contains(m):
    from sml_amd.retrieval import DeviceSeen
    rng = np.random.RandomState(100 + m)
    n_user, n_item = 60, 300
    pairs = random_pairs(rng, 50, n_item, 2500) + np.array([5, 0])       # users 0 .. 4 and 55 .. 59 have empty ranges
    seen = DeviceSeen(n_user, n_item, engine()).add(pairs)
    off, items = ref_set([pairs], n_user, n_item)
    u = np.nonzero(np.diff(off) > 1)[0][:8]
    ends = np.concatenate([np.stack([u, items[off[u]]], 1), np.stack([u, items[off[u + 1] - 1]], 1),      # first and last of a range
                           np.stack([u, items[off[u]] - 1], 1)[items[off[u]] > 0],                        # just below the first
                           np.array([[0, 0], [59, n_item - 1], [4, 7], [55, 7]])])                        # users with empty ranges
    probe = np.concatenate([ends, pairs[rng.randint(0, len(pairs), m)], random_pairs(rng, n_user, n_item, m)])[rng.permutation(len(ends) + 2 * m)[:m]]
    want = ref_contains(pairs, n_item, probe)
    wide = np.concatenate([probe, np.full((m, 3), 7)], 1)                 # further columns are ignored
    for x in (probe, torch.from_numpy(probe).to(DEV), wide, torch.from_numpy(wide).to(DEV)):
        got = seen.contains(x)
        assert got.dtype == torch.bool and got.shape == (m,)
        assert np.array_equal(got.cpu().numpy(), want)
    assert seen.contains(np.zeros((0, 2), np.int64)).shape == (0,)
    empty = DeviceSeen(n_user, n_item, engine())
    assert not empty.contains(probe).any()


def _retrieval_outputs(mf, seen, users, rows, test, extra):
    from sml_amd.retrieval import held_out
    out = list(mf.recommend(users, topK=20, exclude=seen, **extra))
    _, _, hit_rows = mf.test_full(rows, topK=10, exclude=seen, **extra)
    out.append(hit_rows)
    from sml_amd.mf import _engine_for
    from sml_amd.retrieval import as_csr, as_filter, as_score
    w = mf.user_laten.weight
    out.append(_engine_for(mf).full_rank(w.data, mf.item_laten.weight.data, rows, as_csr(seen, w.device),
                                         as_filter(extra.get("items"), mf.item_laten.weight.shape[0], w.device),
                                         as_score(extra.get("score"), mf)))
    res = mf.test_users(held_out(test, mf.user_laten.weight.shape[0], mf.item_laten.weight.shape[0]), topK=(20, 10, 5), exclude=seen, **extra)
    return out + [res[k] for k in ("above", "pos", "hits", "dcg", "ap", "first")]


@pytest.mark.parametrize("d,half", [(32, False), (128, True)])
def test_retrieval_with_device_seen_equals_seen_items(d, half):
    from sml_amd.evaluation import test_model_full, test_model_users
    from sml_amd.retrieval import DeviceSeen, ItemFilter, SeenItems
    U, I = 96, 4099
    rng = np.random.RandomState(77 + d)
    mf = make_mf(U, I, d, rng.randn(U, d).astype(np.float32) * 0.3, rng.randn(I, d).astype(np.float32) * 0.3, device=DEV)
    mf = mf.half() if half else mf
    adds = [random_pairs(rng, U, I, 3000), random_pairs(rng, U - 6, I, 2000)]
    host, dev = SeenItems(U, I), DeviceSeen(U, I, engine(d))
    for p in adds:
        host.add(p), dev.add(p)
    users = torch.from_numpy(rng.permutation(U)[:50]).to(DEV)
    rows = torch.from_numpy(random_pairs(rng, U, I, 300)).to(DEV)
    test = random_pairs(rng, U, I, 500)
    allow = ItemFilter(I).allow(rng.permutation(I)[:2500])
    for extra in ({}, {"items": allow}, {"score": "cosine"}):
        a, b = _retrieval_outputs(mf, host, users, rows, test, extra), _retrieval_outputs(mf, dev, users, rows, test, extra)
        assert len(a) == len(b) == 10
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y), extra
    assert test_model_full(mf, rows, seen=host, topK=10)[0] == test_model_full(mf, rows, seen=dev, topK=10)[0]
    assert test_model_users(mf, test, seen=host, topK=(5, 10, 20)) == test_model_users(mf, test, seen=dev, topK=(5, 10, 20))
    with pytest.raises(ValueError):
        dev.device("cpu")


def _tiny(tmp_path):
    from sml_amd import synth
    root = str(tmp_path)
    synth.write_dataset(root, "tiny", 4, 400, 70, 60, neg=30, seed=7)
    np.save(os.path.join(root, "tiny", "test_new_user.npy"), np.arange(0, 70, 9, dtype=np.int64))
    np.save(os.path.join(root, "tiny", "test_new_item.npy"), np.arange(0, 60, 7, dtype=np.int64))
    return root


def test_from_periods(tmp_path):
    from sml_amd.retrieval import DeviceSeen, SeenItems
    root = _tiny(tmp_path)
    for periods in ([0, 2], range(4), []):
        same(DeviceSeen.from_periods(root, "tiny", periods, engine()).host(), SeenItems.from_periods(root, "tiny", periods).host(), periods)
    got = DeviceSeen.from_periods(root, "tiny", [1], engine(), n_user=80, n_item=61)
    same(got.host(), SeenItems.from_periods(root, "tiny", [1], n_user=80, n_item=61).host(), "given sizes")


def _run_baseline(root, full_eval, method="fine"):
    from sml_amd.baseline import SPMF, StreamingData
    from sml_amd.engine import HipEngine
    args = types.SimpleNamespace(lr=0.01, pool_size=300, neg_num=1, batch_size=64, l2_u=1e-5, l2_i=1e-5, epochs=3, pool_init_type=0)
    if full_eval is not None:
        args.full_eval = full_eval
    torch.manual_seed(2000)
    torch.cuda.manual_seed(2001)
    np.random.seed(2002)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        # (a fresh engine: the process-wide one would carry the MF Adam state of an earlier run into this one)
        sp = SPMF(args, StreamingData(os.path.join(root, "tiny") + "/"), 70, 60, 32, device=DEV, engine=HipEngine(DEV, 32, 4096))
        if method == "spmf":
            sp.base_train_not_train(1)                           # as the program does before its first SPMF period
        sp.run(2, method=method)
    return sp, out.getvalue()


def _line(res, topk=(5, 10, 20)):
    buf = io.StringIO()
    print("full-catalogue test---", "recall(5,10,20):", np.array([res["recall"][k] for k in topk]),
          "ndcg (5,10,20):", np.array([res["ndcg"][k] for k in topk]), "users:", res["users"], file=buf)
    return buf.getvalue().rstrip("\n")


@pytest.mark.parametrize("method", ["fine", "spmf"])
def test_baseline_full_eval_in_process(tmp_path, method):
    from sml_amd.evaluation import test_model_users
    from sml_amd.retrieval import SeenItems
    root = _tiny(tmp_path)
    sp, log = _run_baseline(root, 1, method)
    full = [l for l in log.splitlines() if l.startswith("full-catalogue test---")]
    assert len(full) == 2 == sp.run_stage                        # stages 2 and 3 trained
    finals = [k for k, l in enumerate(log.splitlines()) if l.startswith("FInal test---")]
    assert [log.splitlines()[k + 1] for k in finals] == full     # right after the stage's final test line
    test3 = np.load(os.path.join(root, "tiny", "test", "3.npy"))
    want = test_model_users(sp.MFbase, test3, seen=SeenItems.from_periods(root, "tiny", range(3)), topK=(5, 10, 20))
    assert full[-1] == _line(want)
    assert want["users"] == len(np.unique(test3[:, 0]))
    same(sp._seen.host(), SeenItems.from_periods(root, "tiny", range(3)).host(), "the program's Seen")
    assert sp.full_test(3, test3) == want                        # the dict the line is made from
    # the sampled tests and the losses do not move with the flag (absent, as the fixtures' Namespaces have it, or 0)
    def trajectory(text):            # every sampled-test line and every epoch's loss (the epoch lines also carry wall time)
        lines = [l for l in text.splitlines() if not l.startswith("full-catalogue test---")]
        return [l for l in lines if "recall(5,10,20):" in l] + [l.split("loss:")[1] for l in lines if l.startswith("epoch:")]

    assert len(trajectory(log)) >= 2 * (3 + 3)
    for flag in (None, 0):
        _, plain = _run_baseline(root, flag, method)
        assert "full-catalogue" not in plain
        assert trajectory(plain) == trajectory(log)


def test_baseline_full_eval_cli(tmp_path):
    root = _tiny(tmp_path)
    cmd = [sys.executable, "-m", "model.baseline", "--data_path", root + "/", "--data_name", "tiny", "--pre_model", "",
           "--start_idx", "2", "--epochs", "3", "--batch_size", "64", "--laten_dim", "32", "--pool_size", "300",
           "--method", "fine", "--full_eval", "1"]
    r = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    assert "full_eval=1" in out.split("parameters:")[1].splitlines()[0]
    full = [l for l in out.splitlines() if l.startswith("full-catalogue test--- recall(5,10,20): [")]
    assert len(full) == 2 and all("ndcg (5,10,20): [" in l and "users: " in l for l in full), out[-3000:]
    assert "weight average recall@20:" in out
