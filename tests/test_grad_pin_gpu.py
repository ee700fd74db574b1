"""The TR and MF training steps' gradients, launch geometry by launch geometry, through the Adam moments they leave.
Run on the MI355X box:  python -m pytest tests/test_grad_pin_gpu.py -m gpu

The weights are frozen (TR: lr = 1e-12, weight decay 0; MF: a fresh engine, or lr = 1e-12 over two batches), so m and v are the
batches' gradients, linearly and squared, and tests/_grad_ref.py follows them in float64.  Per tensor, max-norm relative, the bound
is max(G2's tolerance, MARGIN x the fp32 oracle's own error) -- see _grad_ref.py; test_grad_pin_host.py shows that a dropped batch
row, a BCE mean over the wrong length, a tensor 1 % off and a dropped occurrence of a duplicated row all fail it.

Every case prints its figures before it asserts; with SML_GRAD_PIN_RATIOS=<path> the per-tensor ratios
err(HIP) / max(err(fp32 oracle), tolerance / 4) are written there as JSON (profiles/r14_grad_pin_ratios.json is such a run: the
margin is set from it)."""
import json
import os

import numpy as np
import pytest

import _grad_pin_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}


def engine(d, mb=1024):
    from sml_amd.engine import HipEngine
    return HipEngine(DEV, d, mb)


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    path = os.environ.get("SML_GRAD_PIN_RATIOS")
    if path and RATIOS:
        worst = max((r, case, q, k) for case, rep in RATIOS.items() for q, rr in rep.items() for k, r in rr.items() if r is not None)
        with open(path, "w") as f:
            json.dump(dict(ratio="err(HIP) / max(err(fp32 oracle), project tolerance / 4), all against float64; v: both halved",
                           margin=C.MARGIN, worst=dict(ratio=worst[0], case=worst[1], quantity=worst[2], tensor=worst[3]),
                           cases=RATIOS), f, indent=1, sort_keys=True)
        print("WORST ratio %.3f  %s %s %s" % worst)


def _report(case, rep):
    RATIOS[case] = C.ratios(rep)
    for q, rr in rep.items():
        for k, r in rr.items():
            print("%s %s %-32s err %.3e  fp32 %s  bound %.3e%s" % (case, q, k, r["err"], "%.3e" % r["yard"] if r["yard"] is not None else "-",
                                                                   r["bound"], "" if r["ok"] else "   <-- MISS"))


@pytest.mark.parametrize("case", C.TR_CASES, ids=C.case_id)
def test_tr_step_moments_and_kept_gradient_vs_float64(case, monkeypatch):
    """Two batches (the second at least 5 % shorter; the plan case: five, one of them empty) through the TR step as production
    runs it -- no flat gradient written -- and once more with keep_theta_grad: m and v of every theta tensor against float64,
    bit-identical between the two runs, and the kept buffer the LAST batch's (unclipped) gradient."""
    d, B, loss, special, env = case
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    x, ref = C.tr_case(d, B, loss, special)
    m, v, _ = C.run_tr(engine(d), x, DEV)
    m2, v2, g = C.run_tr(engine(d), x, DEV, keep_grad=True)
    rep = C.judge_tr(ref, m, v, C.MARGIN, grad=g)
    _report("tr-" + C.case_id(case), rep)
    for k in m:
        np.testing.assert_array_equal(m[k], m2[k], err_msg=k)
        np.testing.assert_array_equal(v[k], v2[k], err_msg=k)
    assert not C.all_failures(rep)


@pytest.mark.parametrize("case", C.MF_CASES, ids=C.case_id)
def test_mf_step_moments_vs_float64(case, monkeypatch, capfd):
    """One full batch, one ragged batch and two batches whose second misses rows of the first (their lazy moments decay when the
    flush replays the step they sat out), each on a fresh engine: the form the case names RAN (the SML_TRACE line), rows no batch
    touched hold m = v = 0 and the -1 stamp, touched rows are current and their moments agree with float64."""
    d, B, loss, beta, env, form = case
    monkeypatch.setenv("SML_TRACE", "1")
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    bad = {}
    for run in C.MF_RUNS:
        x, ref = C.mf_case(d, B, loss, beta, run)
        capfd.readouterr()
        eng = engine(d)
        m, v, s = C.run_mf(eng, x, run, DEV)
        step = eng.mf_step
        eng.close()
        lines = [l for l in capfd.readouterr().err.splitlines() if "mf_stage_epoch: form=" in l]
        assert len(lines) == 1 and ("form=%s " % form) in lines[0], lines
        assert step == ref.n_batches
        for tab in ("user", "item"):
            idle = ~ref.touched[tab]
            assert idle.any() and not m[tab][idle].any() and not v[tab][idle].any() and (s[tab][idle] == -1).all(), tab
            assert (s[tab][~idle] == step).all(), tab
        rep = C.judge_mf(ref, m, v, C.MARGIN)
        _report("mf-%s-%s" % (C.case_id(case[:5]), run), rep)
        bad.update({(run,) + k: f for k, f in C.all_failures(rep).items()})
    assert not bad


def test_mf_forward_product_switch_reaches_the_kernels(monkeypatch):
    """SML_MF_BX3 has no trace line of its own: the bf16x3 and the fp32 products of the MF forward give different bits."""
    x, _ = C.mf_case(32, 700, "bce", None, "full")
    got = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SML_MF_BX3", flag)
        eng = engine(32)
        got.append(C.run_mf(eng, x, "full", DEV)[0])
        eng.close()
    assert any((got[0][tab] != got[1][tab]).any() for tab in ("user", "item"))
