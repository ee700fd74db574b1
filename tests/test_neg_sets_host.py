"""Test-set negatives, the host side: the C ABI surface, the property checker pinned to the reference's recorded output, the
host entry sml_host_neg_sets against the plain-Python restatement of tests/_neg_sets_ref.py byte for byte, the uniformity of
the definition, the kernel's resources, and the wiring (Timeline, select_neg_forinteraction, the command line).  No GPU."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _neg_sets_ref as R
from conftest import REPO, golden

NAMES = ("sml_neg_sets", "sml_host_neg_sets")


def host_entry(stream, n_user, n_item, neg_num, start, seed=R.SEED, extra_cols=0):
    """([out per period >= start], [failed per period]) from sml_host_neg_sets over the restatement's own timeline arrays."""
    from sml_amd import _lib
    lib = _lib.load()
    order, n_cat, h_off, h_items, h_since = R.timeline_arrays(stream, n_user, n_item)
    outs, fails, g0 = [], [], 0
    for p, rows in enumerate(stream):
        n = len(rows)
        if p >= start:
            rows = np.ascontiguousarray(np.concatenate([rows, np.full((n, extra_cols), 7, np.int64)], 1), dtype=np.int64)
            nc = np.ascontiguousarray(n_cat[g0:g0 + n])
            out, failed = np.empty((n, 2 + neg_num), np.int64), np.full(1, 99, np.int32)
            _lib.check(lib.sml_host_neg_sets(rows.ctypes.data, n, rows.shape[1], g0, nc.ctypes.data, order.ctypes.data, h_off.ctypes.data,
                                             n_user, h_items.ctypes.data, h_since.ctypes.data, neg_num, seed, out.ctypes.data,
                                             failed.ctypes.data), "sml_host_neg_sets")
            outs.append(out)
            fails.append(int(failed[0]))
        g0 += n
    return outs, fails


def g17():
    z = golden("g17_select_neg.npz")
    n_periods, rows, n_user, n_item, neg_num, start = (int(x) for x in z["hyper"])
    stream = [z["train.%d" % p].astype(np.int64) for p in range(n_periods)]
    test = [z["test.%d" % p].astype(np.int64) for p in range(start, n_periods)]
    return stream, n_user, n_item, neg_num, start, test


def test_abi_surface():
    from sml_amd import _lib
    header = " ".join(re.sub(r"^\s*\*", " ", line) for line in open(os.path.join(REPO, "include", "sml_hip.h")).read().splitlines())
    header = re.sub(r"\s+", " ", header)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "test-set negatives" in header
    for phrase in ("order[0 .. n_cat(g))", "h_since <= g", "first neg_num accepted candidates in acceptance order",
                   "262,144 candidates", "1 <= neg_num <= 4096", "any grid gives the same bytes", "zeroed by the call",
                   "No allocation, no copy to the host, no synchronise"):
        assert phrase in header, phrase
    assert len(_lib.SIGNATURES["sml_neg_sets"][1]) == 17 and len(_lib.SIGNATURES["sml_host_neg_sets"][1]) == 14
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m sml_amd.build)"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in exported.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name
    assert "neg_sets.hip" in __import__("sml_amd.build", fromlist=["SOURCES"]).SOURCES
    dev_h = open(os.path.join(REPO, "sml_amd", "csrc", "sml_dev.h")).read()
    assert re.search(r"__host__ __device__ __forceinline__ uint32_t neg_set_index\(", dev_h)
    assert dev_h.count("0x9e3779b97f4a7c15") == 1, "the stream's constants exist once"


def test_checker_passes_on_the_reference_output():
    stream, n_user, n_item, neg_num, start, test = g17()
    assert (len(stream), start, neg_num) == (6, 3, 30) and all(t.shape == (150, 32) for t in test)
    assert R.check_rows(stream, start, test)


def test_checker_refuses_what_the_reference_never_writes():
    stream, n_user, n_item, neg_num, start, test = g17()
    # row 0 of period 3, first negative: a repeat of its second negative, its own positive (in H(g)), an item nobody has seen
    for value in (int(test[0][0, 3]), int(test[0][0, 1]), 10 ** 6):
        bad = [t.copy() for t in test]
        bad[0][0, 2] = value
        with pytest.raises(AssertionError):
            R.check_rows(stream, start, bad)


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_entry_equals_the_restatement(name):
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case(name)
    got, got_fails = host_entry(stream, n_user, n_item, neg_num, start)
    assert got_fails == fails
    for g, w in zip(got, outs):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    assert sum(fails) == ineligible and most < R.CAP // 8           # every failure is eligibility; far inside the cap
    if sum(fails) == 0:
        assert R.check_rows(stream, start, outs)
    # rows with further columns, another seed
    wide, _ = host_entry(stream, n_user, n_item, neg_num, start, extra_cols=3)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(wide, outs))
    other, other_fails = host_entry(stream, n_user, n_item, neg_num, start, seed=R.SEED + 1)
    assert other_fails == fails
    if name != "k65tight":
        assert any(g.tobytes() != w.tobytes() for g, w in zip(other, outs))


def test_cases_cover_what_they_claim():
    """Counts of this builder under seed 2000 (rows with negatives / failing rows / most candidates one row looked at):
    k999 514 / 0 / 2,577; k1 130 / 0 / 4; k64 260 / 134 / 416; k65tight 260 / 160 / 541; k63 128 / 54 / 605."""
    want = {"k999": (514, 0), "k1": (130, 0), "k64": (260, 134), "k65tight": (260, 160), "k63": (128, 54)}
    for name, (n_rows, n_fail) in want.items():
        stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case(name)
        assert (sum(len(o) for o in outs), sum(fails)) == (n_rows, n_fail), name
        pairs = np.concatenate(stream)[:, :2]
        assert len(np.unique(pairs, axis=0)) < len(pairs), "repeated (u, i) pairs"
        first_user = {}
        for p, rows in enumerate(stream):
            for u in rows[:, 0]:
                first_user.setdefault(int(u), p)
        if name != "k63":
            assert max(first_user.values()) >= 1, "users that arrive after period 0"
            assert len(set(np.concatenate(stream[1:])[:, 1]) - set(stream[0][:, 1])) > 0, "the catalogue grows inside later periods"


def test_exact_eligibility():
    stream, n_user, n_item, neg_num, start, outs, fails = R.exact_case()
    assert fails == [0]
    assert set(outs[0][0, 2:].tolist()) == set(range(12)) - {0, 5, 7, 9} and len(outs[0][0, 2:]) == neg_num == 8
    got, got_fails = host_entry(stream, n_user, n_item, neg_num, start)
    assert got_fails == [0] and got[0].tobytes() == outs[0].tobytes()
    short, short_fails = host_entry(stream, n_user, n_item, neg_num + 1, start)      # one more than fits: decided before any draw
    assert short_fails == [1] and (short[0][0, 2:] == -1).all() and (short[0][1, 2:] >= 0).all()


def test_refusals():
    from sml_amd import _lib
    lib = _lib.load()
    stream, n_user, n_item, neg_num, start, outs, fails = R.exact_case()
    order, n_cat, h_off, h_items, h_since = R.timeline_arrays(stream, n_user, n_item)
    rows, g0 = np.ascontiguousarray(stream[1]), len(stream[0])
    nc = np.ascontiguousarray(n_cat[g0:])
    out, failed = np.empty((2, 2 + 4096), np.int64), np.zeros(1, np.int32)

    def call(n=2, n_cols=2, g=g0, k=neg_num, o=out):
        return lib.sml_host_neg_sets(rows.ctypes.data, n, n_cols, g, nc.ctypes.data, order.ctypes.data, h_off.ctypes.data, n_user,
                                     h_items.ctypes.data, h_since.ctypes.data, k, 1, o.ctypes.data, failed.ctypes.data)
    assert call() == 0
    for kw in (dict(k=0), dict(k=4097), dict(n_cols=1), dict(g=-1), dict(g=2 ** 31 - 2), dict(n=-1)):
        assert call(**kw) != 0, kw
    with pytest.raises(_lib.SmlError, match="overlaps"):
        _lib.check(call(o=rows), "sml_host_neg_sets")


def test_uniformity_of_the_restatement():
    """2 periods x 4,000 rows, 50 users, 200 items, neg_num 20: the chi-square of the per-item negative counts against
    sum over rows of neg_num / |C \\ H| stays below the 0.999 quantile of chi-square(199) (Wilson-Hilferty, about 267)."""
    rng = np.random.RandomState(5)
    stream = [np.stack([rng.randint(0, 50, 4000), rng.randint(0, 200, 4000)], 1).astype(np.int64) for _ in range(2)]
    stream[0][:200, 1] = rng.permutation(200)                     # the whole catalogue is there from the start
    outs, fails, most, ineligible = R.ref_negatives(stream, 1, 20, 5)
    assert fails == [0]
    hist = {}
    for u, i in stream[0]:
        hist.setdefault(int(u), set()).add(int(i))
    expect, count = np.zeros(200), np.bincount(outs[0][:, 2:].ravel(), minlength=200).astype(np.float64)
    for u, i in stream[1]:
        h = hist.setdefault(int(u), set())
        h.add(int(i))
        w = np.full(200, 20.0 / (200 - len(h)))
        w[list(h)] = 0.0
        expect += w
    chi2 = float((((count - expect) ** 2) / expect).sum())
    k, z = 199.0, 3.0902                                          # the 0.999 quantile of the standard normal
    bound = k * (1.0 - 2.0 / (9.0 * k) + z * math.sqrt(2.0 / (9.0 * k))) ** 3
    print("chi2 = %.1f, bound = %.1f" % (chi2, bound))
    assert 266.0 < bound < 268.0 and chi2 < bound


def test_kernel_resources():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is absent")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report(os.path.join(REPO, "sml_amd", "csrc", "neg_sets.hip"))
    assert any("k_neg_sets" in r["name"] for r in rows), rows
    for r in rows:
        assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, r


@pytest.mark.parametrize("name", ["k64", "k999"])
def test_timeline_and_period_negatives_on_the_host_route(name):
    from sml_amd.prepare import Timeline, TimelineArrays, period_negatives
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case(name)
    tl = Timeline(stream, n_user, n_item, "host")
    got = tl.host()
    assert isinstance(got, TimelineArrays) and len(tl) == len(stream) and tl.total == sum(len(p) for p in stream)
    for g, w in zip(got, R.timeline_arrays(stream, n_user, n_item)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    for j, p in enumerate(range(start, len(stream))):
        if fails[j]:
            with pytest.raises(ValueError, match=r"%d of the %d rows of period %d could not get %d negatives.*neg_num <= \d+ fits"
                               % (fails[j], len(stream[p]), p, neg_num)) as err:
                period_negatives(tl, p, neg_num, R.SEED)
            fits = int(re.search(r"neg_num <= (\d+)", str(err.value)).group(1))
            assert period_negatives(tl, p, fits, R.SEED).min() >= 0            # the named neg_num fits; one more does not
            with pytest.raises(ValueError):
                period_negatives(tl, p, fits + 1, R.SEED)
        out = period_negatives(tl, p, neg_num, R.SEED, allow_short=True)
        assert out.numpy().tobytes() == outs[j].tobytes()
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="neg_num"):
            period_negatives(tl, start, bad)
    with pytest.raises(ValueError, match=re.escape("pair out of range (n_user=%d, n_item=%d)" % (n_user, n_item - 1))):
        Timeline(stream, n_user, n_item - 1, "host")


def test_select_neg_forinteraction_on_the_host_route(tmp_path):
    import data.dataset2
    from sml_amd import datasets, prepare
    assert datasets.select_neg_forinteraction is prepare.select_neg_forinteraction is data.dataset2.select_neg_forinteraction
    stream, n_user, n_item, neg_num, start, outs, fails, most, ineligible = R.case("k1")
    base = tmp_path / "toy"
    (base / "train").mkdir(parents=True)
    np.save(base / "information.npy", np.array([sum(len(p) for p in stream), n_user, n_item], dtype=np.int64))
    names = ["a", "b", "c"]
    np.save(base / "train" / "a.npy", stream[0])
    np.save(base / "b.npy", stream[1])                             # the reference's own layout: beside information.npy
    np.save(base / "train" / "c.npy", stream[2])
    before = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*") if p.is_file())
    written = prepare.select_neg_forinteraction(str(tmp_path) + os.sep, "toy", names, leave_for_init_train=1 / 3, neg_num=neg_num,
                                                seed=R.SEED, engine="host")
    after = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*") if p.is_file())
    assert sorted(set(after) - set(before)) == [os.path.join("toy", "test", "%d.npy" % i) for i in (1, 2)] and set(before) <= set(after)
    assert [os.path.basename(w) for w in written] == ["1.npy", "2.npy"]
    for j, i in enumerate((1, 2)):
        t = np.load(base / "test" / ("%d.npy" % i))
        assert t.dtype == np.int64 and t.shape == (len(stream[i]), 2 + neg_num) and t.tobytes() == outs[j].tobytes()


def test_command_line_and_surface():
    from sml_amd import prepare
    from sml_amd.engine import HipEngine
    a = prepare.get_parse().parse_args(["--data_name", "yelp", "--periods", "40"])
    assert (a.data_path, a.periods, a.leave, a.neg_num, a.seed, a.host) == ("dataset/", 40, 0.7, 999, 2000, False)
    a = prepare.get_parse().parse_args(["--data_path", "d/", "--data_name", "n", "--periods", "3", "--leave", "0.5", "--neg_num", "7",
                                        "--seed", "1", "--host"])
    assert (a.data_path, a.data_name, a.leave, a.neg_num, a.seed, a.host) == ("d/", "n", 0.5, 7, 1, True)
    assert callable(HipEngine.neg_sets) and callable(prepare.Timeline.host) and callable(prepare.period_negatives)
    assert callable(prepare.main)
