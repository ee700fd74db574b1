"""The transfer-forward pin without a GPU: the float64 reference against the fixtures recorded from the real model, the cases' own
sanity, and a restatement of the bf16x3 product that shows what the per-row bound of test_fwd_f64_gpu.py can see.

The emulation (tests/_fwd_f64_cases.py: Bx3Forward) runs k_transfer_fwd_bx3's arithmetic on the CPU -- three round-to-nearest-even
bf16 planes per operand, the six named products, float64 sums -- over all 8224 rows of the four d = 32 cases, both nets.  Measured
(err / e_ref, worst row; the figures the tests print):

  six exact products                               0.22 .. 0.36   (at or below e_ref: required)
  third weight plane zeroed in ONE fc1 k-step      0.2 .. 6.2 over (case, net, k-step); per k-step, the best case sees 2.9 .. 6.2
  the same in ONE fc2 k-step                       0.8 .. 3.4;  per k-step, the best case sees 2.1 .. 3.4
  a2 b2 dropped in both products                   6.6 .. 13.3

A fault of the kernel is the same fault in every case, and the suite fails when one case fails: a fault counts as seen when SOME case
puts it above M_bx3 x e_ref.  At the measured M_bx3 = 1.5 every one of the 5 + 16 single-k-step faults and the dropped a2 b2 is
seen; no single (case, net) sees them all (fc1's k-steps are the five conv channels, and a channel can be nearly idle in one net).
The same outputs pass what the suite held the kernel to before -- whole-tensor max-norm, 1e-4 against the float32 oracle and 3e-6
against the fp32-product sibling (here: the unfaulted emulation): single k-step, at most 2.8e-6 against either; a2 b2 dropped,
5.7e-6 against the oracle and 5.8e-6 against the sibling, which the 3e-6 bound would have caught."""
import json
import os

import numpy as np
import pytest
import torch

import _fwd_f64_cases as C
from conftest import golden, make_transfer, T, REPO
from oracle import sml_oracle as O

RTOL, ATOL = 2e-5, 2e-6          # what test_oracle_golden.py holds the oracle to on the same fixtures
D32 = [c for c in C.CASES if c[0] == 32]


def f64(net):
    return {k: v.detach().double() for k, v in net.items()}


# ----------------------------------------------------------------------------- the reference is the real model's forward
@pytest.mark.parametrize("name,unit_user", [("g1_transfer_forward_d32.npz", False), ("g1_transfer_forward_d64.npz", False),
                                            ("g11_convtransfer_d32.npz", True)])
def test_float64_reference_reproduces_the_recorded_forwards(name, unit_user):
    z = golden(name)
    theta = O.split_theta(z, "theta.")
    assert (O.net_kernel(theta["user"]) == 2) == unit_user
    x_t, x_hat = T(z["x_t"]).double(), T(z["x_hat"]).double()
    for which, key in (("user", "y_user"), ("item", "y_item")):
        y = O.transfer_forward(f64(theta[which]), x_t, x_hat, unit_norm=unit_user and which == "user")
        assert y.dtype == torch.float64
        np.testing.assert_allclose(y.numpy(), z[key], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("variant", ["", "_conv"])
def test_float64_reference_reproduces_the_recorded_updata(variant):
    z = golden("g5_updata%s.npz" % variant)
    net = make_transfer(z["Wlast_user"].shape[1], z)
    theta = O.OracleEngine.theta_of(net)
    k2 = O.net_kernel(theta["user"]) == 2
    assert k2 == (variant == "_conv")
    for which, key in (("user", "user"), ("item", "item")):
        y = O.transfer_forward(f64(theta[which]), T(z["Wlast_" + key]).double(), T(z["What_" + key]).double(),
                               unit_norm=k2 and which == "user")
        np.testing.assert_allclose(y.numpy(), z["Wnew_" + key], rtol=RTOL, atol=ATOL)


# ----------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("cs", C.CASES, ids=C.case_id)
def test_case_sanity(cs):
    c = C.case(*cs)
    d = cs[0]
    assert c.x_t.shape == (C.ROWS, d) and c.x_t.dtype == torch.float32 and c.ref["user"].dtype == np.float64
    print("%s e_ref %.3e" % (C.case_id(cs), c.e_ref))
    assert 1e-7 <= c.e_ref <= 2e-6, c.e_ref
    planted_nan = np.zeros(C.ROWS, dtype=bool)
    planted_nan[list(C.PLANTED["t0"] + C.PLANTED["tm"])] = True
    smallest = np.inf
    for which in C.NETS:
        nan = C.nan_rows_of(c.ref[which])
        assert np.array_equal(nan, planted_nan if cs[1] == "com" else np.zeros(C.ROWS, dtype=bool)), which
        assert np.array_equal(nan, c.nan_rows()) and np.array_equal(np.isnan(c.ref[which]).all(1), nan)
        assert np.isfinite(c.ref[which][~nan]).all()
        assert np.array_equal(C.nan_rows_of(c.f32[which]), nan)
        smallest = min(smallest, float(np.abs(c.ref[which][~nan]).max(1).min()))
    print("%s smallest max|ref(row)| %.4f" % (C.case_id(cs), smallest))
    assert smallest >= 0.05                                      # no denominator floor in err(row): none is needed
    # planted rows: present, signed as named, in more than one 16-row and 32-row tile, and inside what the small row counts read
    assert not c.x_t[list(C.PLANTED["t0"])].any() and not torch.signbit(c.x_t[list(C.PLANTED["t0"])]).any()
    assert not c.x_hat[list(C.PLANTED["h0"])].any() and not torch.signbit(c.x_hat[list(C.PLANTED["h0"])]).any()
    assert torch.signbit(c.x_t[list(C.PLANTED["tm"])]).all() and torch.signbit(c.x_hat[list(C.PLANTED["hm"])]).all()
    rows = sorted(r for v in C.PLANTED.values() for r in v)
    assert len({r // 16 for r in rows}) >= 4 and len({r // 32 for r in rows}) >= 4 and min(rows) < 15 and rows[0] != 0
    assert any(8192 <= r for r in rows) and C.ROWS - 1 in rows
    # every 16-row tile mixes magnitudes: at least a decade between its largest and smallest row
    live = np.ones(C.ROWS, dtype=bool)
    live[[r for r in C.PLANTED["t0"] + C.PLANTED["tm"]]] = False
    amp = c.x_t.abs().max(1).values.numpy()
    for t0 in range(0, C.ROWS, 16):
        a = amp[t0:t0 + 16][live[t0:t0 + 16]]
        assert a.max() / a.min() >= 10.0, t0
    assert amp[live].max() / amp[live].min() > 1e3
    # both weight sets are what they say
    w = c.theta["user"]["fc1.weight"]
    want = 4.0 / np.sqrt(5 * d) if cs[2] == "trained" else 1.0 / np.sqrt(3 * 5 * d)     # (init: uniform(+-1/sqrt(fan_in)))
    assert abs(float(w.std()) / want - 1.0) < 0.05
    assert O.net_kernel(c.theta["user"]) == (2 if cs[1] == "conv" else 3)


def test_rows_are_independent_so_a_prefix_is_a_case():
    c = C.case(32, "com", "trained")
    for n in (1, 17, 100):
        y = O.transfer_forward(f64(c.theta["item"]), c.x_t[:n].double(), c.x_hat[:n].double()).numpy()
        assert C.worst_row(y, c.ref["item"][:n]) < 1e-13


def test_the_criterion_is_per_row():
    """A small row entirely wrong beside a large one: the whole-tensor norm passes it, err(row) does not."""
    ref = np.array([[100.0, -50.0], [1e-2, 2e-2], [np.nan, np.nan]])
    got = ref.copy()
    got[1] = [2e-2, 1e-2]
    assert np.abs(got[:2] - ref[:2]).max() / np.abs(ref[:2]).max() < 1.1e-4
    e = C.row_errors(got, ref)
    assert e[0] == 0.0 and e[1] == 0.5 and np.isnan(e[2]) and C.worst_row(got, ref) == 0.5
    got[0, 1] = np.inf
    assert C.worst_row(got, ref) == np.inf


# ----------------------------------------------------------------------------- the margins come from the recorded run
def test_margin_rule_and_the_recorded_ratios():
    assert C.margin_from(0.3) == 1.5 and C.margin_from(1.0) == 1.5 and C.margin_from(1.01) == 2.0 and C.margin_from(1.34) == 2.5
    with open(os.path.join(REPO, "profiles", "r21_fwd_f64_ratios.json")) as f:
        rec = json.load(f)
    assert set(rec["worst"]) == set(C.M)
    for fam, m in C.M.items():
        worst = max(r for key, r in rec["cases"].items() if key.endswith("|" + fam))
        assert abs(worst - rec["worst"][fam]["ratio"]) < 1e-12
        assert m == C.margin_from(worst), (fam, m, worst)


# ----------------------------------------------------------------------------- what the bound can see
@pytest.fixture(scope="module")
def emulation():
    """err / e_ref of the six-product forward and of every planted fault, per (case, net): computed once."""
    out = {}
    for cs in D32:
        c = C.case(*cs)
        for which in C.NETS:
            ref, f32 = c.ref[which], c.f32[which]
            fwd = C.Bx3Forward(c, which, C.ROWS)
            six = fwd.run()
            rec = dict(six=C.worst_row(six, ref) / c.e_ref, fc1=[], fc2=[], old=[])
            for layer, steps in (("fc1", 5), ("fc2", 16)):
                for ks in range(steps):
                    y = fwd.run(**{layer: dict(zero_b3=(32 * ks, 32 * ks + 32))})
                    rec[layer].append(C.worst_row(y, ref) / c.e_ref)
                    rec["old"].append(C.old_criteria(y, six, f32))
            y = fwd.run(fc1=dict(drop=((1, 1),)), fc2=dict(drop=((1, 1),)))
            rec["a2b2"] = C.worst_row(y, ref) / c.e_ref
            rec["a2b2_old"] = C.old_criteria(y, six, f32)
            assert np.array_equal(C.nan_rows_of(six), c.nan_rows()) and np.array_equal(C.nan_rows_of(y), c.nan_rows())
            out[(cs, which)] = rec
            print("%s %s six %.3f  fc1 %s  fc2 %s  a2b2 %.1f" % (C.case_id(cs), which, rec["six"], " ".join("%.1f" % r for r in rec["fc1"]),
                                                              " ".join("%.1f" % r for r in rec["fc2"]), rec["a2b2"]))
    return out


def test_bf16x3_split_is_exact_to_three_planes():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * torch.logspace(-6, 3, 4096)
    p = C.split3(x)
    for q in p:
        assert torch.equal(q, q.bfloat16().float())
    rem = (x.double() - p[0].double() - p[1].double() - p[2].double()).abs()
    assert float((rem / x.double().abs()).max()) < 2.0 ** -24


def test_six_bf16_products_err_at_or_below_the_float32_forward(emulation):
    for key, rec in emulation.items():
        assert rec["six"] <= 1.0, (key, rec["six"])


def test_bound_sees_a_lost_third_plane_k_step_and_a_dropped_product(emulation):
    m = C.M["bx3"]
    unseen = []
    for layer, steps in (("fc1", 5), ("fc2", 16)):
        for ks in range(steps):
            best = max(rec[layer][ks] for rec in emulation.values())
            print("%s k-step %2d: best case %.2f x e_ref (bound %.1f)" % (layer, ks, best, m))
            if not best > m:
                unseen.append((layer, ks, best))
    best = max(rec["a2b2"] for rec in emulation.values())
    print("a2 b2 dropped: best case %.2f x e_ref, every case at least %.2f" % (best, min(rec["a2b2"] for rec in emulation.values())))
    assert min(rec["a2b2"] for rec in emulation.values()) > m
    assert not unseen, unseen


def test_the_earlier_criteria_pass_the_same_faults(emulation):
    """Whole-tensor max-norm against the six-product sibling (3e-6) and the float32 oracle (1e-4): every single-k-step fault passes
    both; the dropped a2 b2 passes the oracle bound."""
    sib = max(o[0] for rec in emulation.values() for o in rec["old"])
    orc = max(o[1] for rec in emulation.values() for o in rec["old"])
    a22 = max(rec["a2b2_old"][1] for rec in emulation.values())
    print("single k-step faults: sibling max-norm %.2e (< 3e-6), oracle max-norm %.2e (< 1e-4); a2 b2 dropped: oracle %.2e, sibling %.2e"
          % (sib, orc, a22, max(rec["a2b2_old"][0] for rec in emulation.values())))
    assert sib < 3e-6 and orc < 1e-4 and a22 < 1e-4
