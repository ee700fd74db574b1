"""The gradient pin's host side (no GPU): the float64 reference of tests/_grad_ref.py agrees with what the reference program
recorded (G2), the fp32 oracle passes the GPU tests' criterion, and the criterion at the GPU tests' margin is SHARP -- a float64
reference with one defect planted in it fails it, by at least twice the bound on every tensor the defect reaches.  The last is what
keeps the margin honest: raise _grad_pin_cases.MARGIN far enough to hide a defect and these tests fail."""
import numpy as np
import pytest
import torch

import _grad_pin_cases as C
import _grad_ref as R
from conftest import golden, make_transfer, T
from oracle import sml_oracle as O
from test_oracle_golden import close

TR_KEYS = list(dict.fromkeys(c[:4] for c in C.TR_CASES))
MF_KEYS = list(dict.fromkeys(c[:4] for c in C.MF_CASES))


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("tag,bce,norm", [("bce", True, False), ("bpr", False, False), ("bprnorm", False, True)])
def test_float64_reference_agrees_with_the_recorded_reference_program(d, tag, bce, norm):
    """G2: the theta gradients and the gathered rows' gradients the reference program's autograd got, at the G2 tolerances."""
    z = golden("g2_run_mf_d%d.npz" % d)
    net = make_transfer(d, z)
    B = z["ul"].shape[0]
    last_u, hat_u = T(z["ul"]), T(z["uh"])
    last_i, hat_i = torch.cat([T(z["il"]), T(z["nl"])]), torch.cat([T(z["ih"]), T(z["nh"])])
    ar = torch.arange(B)
    tri = torch.stack([ar, ar, ar + B], 1)
    g = R.tr_gradients(net, last_u, last_i, hat_u, hat_i, [(tri, 1.0)], bce=bce, norm=norm)[0]
    for name in R.theta_names(net):
        ref = z["gtheta_%s.%s" % (tag, name)]
        if not np.any(ref):
            assert name == R.ZERO_TENSOR and not bce
            assert np.abs(g[name].numpy()).max() <= R.ZERO_ABS
            continue
        close(g[name].numpy(), ref, R.tol_of(name))
    gu, gi, gn, _ = R.mf_row_gradients(net, last_u, last_i, hat_u, hat_i, tri, bce=bce, norm=norm)
    for got, key in ((gu, "gu_"), (gi, "gi_"), (gn, "gn_")):
        close(got.numpy(), z[key + tag], R.TOL_ROWS)
    # ... and the scatter-add of the rows is the table gradient
    tu, ti = R.table_gradients(B, 2 * B, tri, gu, gi, gn)
    np.testing.assert_array_equal(tu.numpy(), gu.numpy())
    np.testing.assert_array_equal(ti.numpy(), torch.cat([gi, gn]).numpy())


def test_moment_constants_are_the_ones_fp32_applies():
    assert R.C1 == float(np.float32(1.0) - np.float32(0.9)) and abs(R.C1 - 0.1) < 1e-7
    assert abs(R.C2 - 0.001) / 0.001 > 1e-5           # (1.0f - 0.999f is NOT 0.001f: the library's constant, sml_dev.h adam_apply)
    g = [{"w": torch.tensor([2.0, -1.0], dtype=torch.float64)}, {"w": torch.tensor([0.0, 4.0], dtype=torch.float64)}]
    m, v = R.moments64(g)
    np.testing.assert_allclose(m["w"], [2 * R.C1 * (1 - R.C1), -R.C1 * (1 - R.C1) + 4 * R.C1], rtol=1e-14)
    np.testing.assert_allclose(v["w"], [4 * R.C2 * R.C2P, R.C2 * R.C2P + 16 * R.C2], rtol=1e-14)


def test_clipping_bites_with_a_different_factor_on_each_batch_and_equals_torchs():
    x, ref = C.tr_case(32, 256, "bce", "clip")
    assert 0.1 < ref.coef64[0] < 0.9 and 0.1 < ref.coef64[1] < 0.9 and abs(ref.coef64[0] - ref.coef64[1]) > 0.02
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in ref.g32_raw[0].values()]
    for p, g in zip(ps, ref.g32_raw[0].values()):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ps, C.CLIP_MAX_NORM, norm_type=2)
    for p, g in zip(ps, ref.g32[0].values()):
        np.testing.assert_allclose(p.grad.numpy(), g.numpy(), rtol=1e-6, atol=0)


@pytest.mark.parametrize("key", TR_KEYS, ids=C.case_id)
def test_fp32_oracle_passes_the_tr_criterion_at_margin_1(key):
    """The OracleEngine's own moments after the same frozen-weight epoch: the reference alone stays inside the test."""
    x, ref = C.tr_case(*key)
    m, v, _ = C.run_tr(O.OracleEngine(x.d), x)
    assert not C.all_failures(C.judge_tr(ref, m, v, 1.0))


@pytest.mark.parametrize("key", MF_KEYS, ids=C.case_id)
def test_fp32_oracle_passes_the_mf_criterion_at_margin_1(key):
    for run in C.MF_RUNS:
        x, ref = C.mf_case(*key, run)
        m, v, _ = C.run_mf(O.OracleEngine(x.d), x, run)
        for tab in ("user", "item"):
            assert not m[tab][~ref.touched[tab]].any() and not v[tab][~ref.touched[tab]].any()
        assert not C.all_failures(C.judge_mf(ref, m, v, 1.0)), run


def _must_fail(rep, affected, by=2.0, lenient=()):
    """The defect fails the case, and every affected tensor fails by at least `by` times its bound (tensors in `lenient`: beyond the
    bound).  A tensor is judged through its first moment, its second moment and, where kept, its raw gradient: it fails by the
    largest of their err / bound."""
    assert C.all_failures(rep)
    for k in affected:
        over = {q: rep[q][k]["err"] / rep[q][k]["bound"] for q in rep}
        print("%-32s %s" % (k, "  ".join("%s x%.1f" % (q, o) for q, o in over.items())))
        assert max(over.values()) >= (1.0 if k in lenient else by), (k, over)


@pytest.mark.parametrize("key", TR_KEYS, ids=C.case_id)
def test_tr_criterion_is_sharp_at_the_margin_of_the_gpu_tests(key):
    """Float64 gradients with one defect, judged as the GPU test judges the kernels (same bound, the fp32 oracle as yardstick):
    (a) the last batch's last triple contributes nothing; (b) the ragged batch's BCE mean is taken over `batch` rows instead of
    its own; (c) one theta tensor's gradient is 1 % too large -- each of the 16 in turn."""
    x, ref = C.tr_case(*key)
    d, B, loss, special = key
    live = [k for k in ref.names if k not in ref.zero]
    last = ref.n_batches - 1

    def judged(grads):
        m, v = R.moments64(R.clipped(grads, x.clip)[0])
        return C.judge_tr(ref, m, v, C.MARGIN, grad={k: g.numpy() for k, g in grads[last].items()})

    # (a) -- under BCE the item net's fc2.bias sums d_pos + d_neg terms that nearly cancel and one row in more than 600 moves it by
    # only a few project tolerances: there the defect must be beyond the bound, not twice beyond it
    net = x.make_net()
    drop = R.tr_gradients(net, x.last_user, x.last_item, x.hat_user, x.hat_item, x.batches, bce=x.bce, drop_last_of=last)
    _must_fail(judged(drop), live, lenient=(R.ZERO_TENSOR,) if (loss == "bce" and B > 600) else ())
    # (b)
    if loss == "bce" and special is None:
        short = x.batches[last][0].shape[0] / float(B)
        wrong = [dict(g) for g in ref.g64_raw]
        wrong[last] = {k: g * short for k, g in wrong[last].items()}
        _must_fail(judged(wrong), live)
    # (c)
    for k in live:
        wrong = [dict(g) for g in ref.g64_raw]
        for g in wrong:
            g[k] = g[k] * 1.01
        rep = judged(wrong)
        _must_fail(rep, [k])
        if not x.clip:            # (a clipped gradient's norm moves with the scaled tensor, and every tensor with the norm)
            assert all(kk == k for _, kk in C.all_failures(rep))


@pytest.mark.parametrize("key", MF_KEYS, ids=C.case_id)
def test_mf_criterion_is_sharp_at_the_margin_of_the_gpu_tests(key):
    """One occurrence of the user with B/2 occurrences left out of its row's sum (and, with the adaptive term, of the user's count:
    that term is B/2 times larger than one occurrence's share, which alone would be invisible beside it): the user table fails, the
    item table does not."""
    for run in ("full", "ragged"):
        x, ref = C.mf_case(*key, run)
        tri, batches = x.triples(run)
        rows = R.mf_row_gradients(x.net, x.last_user, x.last_item, x.w_user, x.w_item, tri, 1.0, x.bce, x.norm, C.L2, x.adaptive_beta)
        assert tri[x.hot_user_occurrence, 0] == 5 and int((tri[:, 0] == 5).sum()) >= len(tri) // 2
        if x.adaptive_beta:
            less = torch.cat([tri[:x.hot_user_occurrence], tri[x.hot_user_occurrence + 1:]])
            rows = rows[:3] + (R.mf_row_gradients(x.net, x.last_user, x.last_item, x.w_user, x.w_item, less, 1.0, x.bce, x.norm, C.L2,
                                                  x.adaptive_beta)[3],)
        gu, gi = R.table_gradients(C.N_USER, C.N_ITEM, tri, *rows, skip_user_occurrence=x.hot_user_occurrence)
        m, v = R.moments64([{"user": gu, "item": gi}])
        rep = C.judge_mf(ref, m, v, C.MARGIN)
        _must_fail(rep, ["user"])
        assert all(k == "user" for _, k in C.all_failures(rep))
