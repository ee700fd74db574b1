"""The bare-step pin without a GPU: the float64 reference against oracle.sml_oracle.bare_step, the cases' census and layout, the
sensitivity condition, and a simulated engine with planted faults that shows what the criterion of test_bare_f64_gpu.py can see.

Per case (tests/_bare_f64_cases.py):
  * census -- the multiset of run lengths of every batch, per table, equals the plan (a planted 129 cannot silently become 130);
    the batches' row ranges are disjoint; planted rows sit at both ends of every range (row 0 and the last row of both tables
    among them); every i == j triple is a planned one and its user is a filler row;
  * sensitivity -- for EVERY occurrence of every planted run, removing it from the reference (or counting it twice) moves the row by
    at least 4 * (store(r) + M * e_ref * scale(r)), with the committed M;
  * mutation -- the float64 step with one fault, stored in the table's type, under the GPU module's criterion: one occurrence of
    every planted run dropped / doubled, the last occurrence of a 512-chunk of every hot run skipped, every unique row never
    updated.  Each fault must fail the case, and every planted row it hits must be among the failing rows.  The unfaulted simulated
    engine passes with e(r) = 0 wherever the float64 result rounds once.
The figures are printed before they are asserted on."""
import collections

import numpy as np
import pytest
import torch

import _bare_f64_cases as C
from oracle import sml_oracle as O

IDS = [s.id for s in C.ALL_CASES]


# ----------------------------------------------------------------------------- the reference is the oracle's step
@pytest.mark.parametrize("bce", [True, False])
@pytest.mark.parametrize("half", [False, True])
def test_float64_reference_agrees_with_the_oracle_in_float64(bce, half):
    """O.bare_step on .double() tensors: agreement at float64 rounding -- tables, loss; scale(r) against a direct sum."""
    rng = np.random.RandomState(5 + 2 * bce + half)
    U, I, d, B = 60, 40, 32, 300
    wu = torch.from_numpy((rng.standard_normal((U, d)) * 0.3).astype(np.float32))
    wi = torch.from_numpy((rng.standard_normal((I, d)) * 0.3).astype(np.float32))
    if half:
        wu, wi = wu.half(), wi.half()
    tri = np.stack([rng.randint(0, U - 5, B), rng.randint(0, I - 5, B), rng.randint(0, I - 5, B)], 1)
    tri[:40, 0] = 3
    tri[7, 2] = tri[7, 1]
    lr, lam_u, lam_i = 0.05, 1e-2, 2e-2
    nu, ni, loss, su, si = C.bare_step_f64(wu.double().numpy(), wi.double().numpy(), tri, lr, lam_u, lam_i, bce)
    ou, oi = wu.double().clone(), wi.double().clone()
    t = torch.from_numpy(tri)
    want = O.bare_step(ou, oi, t[:, 0], t[:, 1], t[:, 2], lr, lam_u, lam_i, bce=bce)
    assert abs(loss - want) <= 1e-13 * abs(want)
    err = max(np.abs(nu - ou.numpy()).max(), np.abs(ni - oi.numpy()).max())
    print("float64 reference vs O.bare_step(double): max abs difference %.3e, loss %.15g vs %.15g" % (err, loss, want))
    assert err <= 1e-15
    # untouched rows are the input's, touched rows moved, scale is zero exactly on the untouched rows
    assert C.untouched_identical(nu, wu.double().numpy(), np.unique(tri[:, 0])) and not su[U - 5:].any() and (su[np.unique(tri[:, 0])] > 0).all()
    assert C.untouched_identical(ni, wi.double().numpy(), np.unique(tri[:, 1:])) and not si[I - 5:].any()
    # scale(r) by hand for the planted user: lr * max_k sum_t |g_t[k]|
    _, gx, _, _ = C.bare_grads_f64(wu.double().numpy(), wi.double().numpy(), tri, lam_u, lam_i, bce)
    assert abs(su[3] - lr * np.abs(gx[tri[:, 0] == 3]).sum(0).max()) <= 1e-15
    # float32 autograd gradient (the Adam half's yardstick) against the float64 sums
    g32u, g32i = C.oracle_grad32(wu.float(), wi.float(), tri, lam_u, lam_i, bce)
    _, Gu, Gi, Au, Ai = C.summed_grads_f64(wu.double().numpy(), wi.double().numpy(), tri, lam_u, lam_i, bce)
    assert np.abs(g32u.double().numpy() - Gu).max() <= 2e-6 * Au.max() and np.abs(g32i.double().numpy() - Gi).max() <= 2e-6 * Ai.max()


def test_half_ulp():
    for half, dt in ((False, np.float32), (True, np.float16)):
        x = np.array([1.0, 1.5, 0.3, 0.25, 0.2499, 1e-3, 3.0, 0.0], dtype=np.float64)
        want = [float(np.spacing(dt(abs(v)))) / 2 for v in x]
        assert np.array_equal(C.half_ulp(x, half), np.array(want)), (half, C.half_ulp(x, half), want)
    assert C.half_ulp(0.3, True) == 2.0 ** -13 and C.half_ulp(-0.3, False) == 2.0 ** -26


def test_the_criterion_is_per_row_and_forgives_the_storage_rounding_only():
    ref = np.array([[10.0, -5.0], [0.25, 0.125]])
    store, scale, rows = C.half_ulp(ref, True).max(1), np.array([1.0, 1e-2]), np.arange(2)
    got = ref.astype(np.float16).astype(np.float64)
    assert not C.row_e(got, ref, store, scale, rows).any()
    got[1, 1] += 4 * store[1]                                    # four half-ulps of the small row: nothing beside the large one
    e = C.row_e(got, ref, store, scale, rows)
    assert e[0] == 0.0 and abs(e[1] - 3 * store[1] / 1e-2) < 1e-12
    got[0, 0] = np.nan
    assert C.row_e(got, ref, store, scale, rows)[0] == np.inf


# ----------------------------------------------------------------------------- the margins come from the recorded run
def test_margin_rule_and_the_recorded_ratios():
    assert C.margin_from(0.3) == 1.5 and C.margin_from(1.01) == 2.0
    rec = C.recorded_ratios()
    assert set(rec["worst"]) == set(C.M)
    for fam, m in C.M.items():
        worst = max(r for key, r in rec["cases"].items() if key.endswith("|" + fam))
        assert abs(worst - rec["worst"][fam]["ratio"]) < 1e-12
        assert m == C.margin_from(worst), (fam, m, worst)
    # every case and launch form of the GPU module is in the record
    keys = set(rec["cases"])
    for s in C.ALL_CASES:
        forms = ("adam",) if s.adam else ("inline", "prepared")
        assert all("%s|%s|%s" % (s.id, f, s.family) in keys for f in forms), s.id


# ----------------------------------------------------------------------------- census, layout, sensitivity, mutations
def _check_layout(c):
    s = c.spec
    u0 = i0 = 0
    seen_u, seen_i = set(), set()
    for bt in c.batches:
        got_u, got_i = C.census(bt.tri)
        want_u, want_i = bt.expected_census()
        assert got_u == want_u, (s.id, bt.index, sorted((got_u - want_u).items()), sorted((want_u - got_u).items()))
        assert got_i == want_i, (s.id, bt.index, sorted((got_i - want_i).items()), sorted((want_i - got_i).items()))
        assert max(bt.filler_u) <= 3 and max(bt.filler_i) <= 3
        for L in bt.plan_u:
            assert got_u[L] >= 1
        # the planted rows hold exactly their planned lengths
        for r, L in zip(bt.planted_u.tolist(), bt.plan_u):
            assert int((bt.tri[:, 0] == r).sum()) == L, (s.id, bt.index, r, L)
        for r, L in zip(bt.planted_i.tolist(), bt.plan_i):
            n_pos, n_neg = int((bt.tri[:, 1] == r).sum()), int((bt.tri[:, 2] == r).sum())
            assert n_pos + n_neg == L, (s.id, bt.index, r, L)
            kind = bt.kinds[r]
            assert (kind != "pos" or n_neg == 0) and (kind != "neg" or n_pos == 0) and (kind != "mixed" or L < 2 or (n_pos and n_neg))
            assert kind != "deep" or (n_pos == bt.size and n_neg == C.DEEP_NEG)
        # disjoint, contiguous ranges; planted rows at both ends of each
        ru, ri = np.unique(bt.tri[:, 0]), np.unique(bt.tri[:, 1:])
        assert ru.min() >= u0 and ru.max() < u0 + bt.n_user_rows and ri.min() >= i0 and ri.max() < i0 + bt.n_item_rows
        assert not (seen_u & set(ru.tolist())) and not (seen_i & set(ri.tolist()))
        seen_u |= set(ru.tolist())
        seen_i |= set(ri.tolist())
        assert len(ru) == bt.n_user_rows - C.SLACK and len(ri) == bt.n_item_rows - C.SLACK
        if len(bt.plan_u) >= 4:
            assert {u0, u0 + 1, u0 + bt.n_user_rows - 1, u0 + bt.n_user_rows - 2} <= set(bt.planted_u.tolist())
        if len(bt.plan_i) >= 4:
            assert {i0, i0 + 1, i0 + bt.n_item_rows - 1, i0 + bt.n_item_rows - 2} <= set(bt.planted_i.tolist())
        elif bt.plan_i:
            assert i0 in bt.planted_i
        # i == j: the planned triples only, on the planned item, under filler users
        eq = bt.tri[:, 1] == bt.tri[:, 2]
        assert int(eq.sum()) == bt.eq_count and (bt.eq_count == 0 or (bt.tri[eq, 1] == bt.eq_item).all())
        assert not np.isin(bt.tri[eq, 0], bt.planted_u).any()
        u0, i0 = u0 + bt.n_user_rows, i0 + bt.n_item_rows
    assert (u0, i0) == (c.U, c.I) and c.U <= 24576 and c.I <= 24576
    assert len(c.batches) == len(s.batches) and c.tri.shape == (sum(b[0] for b in s.batches), 3)
    if not s.adam:
        assert len(c.batches) == 3 and c.batches[0].size == c.batches[1].size == s.B and c.batches[2].size < s.B
        assert (0 in c.batches[0].planted_u or not c.batches[0].plan_u) and 0 in c.batches[0].planted_i
        assert c.U - 1 in c.batches[2].planted_u and c.I - 1 in c.batches[2].planted_i
        assert all(bt.decorrelated for bt in c.batches)
    if s.plan in ("classes", "adam_u", "adam_i"):
        kinds = collections.Counter(k for bt in c.batches for k in bt.kinds.values())
        assert kinds["pos"] and kinds["neg"] and kinds["mixed"] and all(bt.eq_count == 1 for bt in c.batches)
    if s.plan == "capped":
        assert max(max(bt.plan_u) for bt in c.batches) == C.SML_HOT and min(bt.size for bt in c.batches) >= C.HOT_MIN_BATCH
    if s.plan == "many_hot":
        assert sum(L > C.SML_HOT for L in c.batches[0].plan_u + c.batches[0].plan_i) == 260
    if s.plan == "classes":
        assert c.batches[2].size < C.HOT_MIN_BATCH and s.hot_capable


def _check_sensitivity(c):
    """Every occurrence of every planted run against 4 * (store + M * e_ref * scale).  Returns the weakest ratio."""
    weakest, n_occ = np.inf, 0
    for bt in c.batches:
        cu, ci = c.contributions(bt)
        for table, contrib in (("user", cu), ("item", ci)):
            for row, slots in c.occurrences(bt)[table].items():
                ratio = contrib[slots] / c.need(table, row)
                n_occ += len(slots)
                if ratio.min() < weakest:
                    weakest = float(ratio.min())
                assert ratio.min() >= 1.0, "%s batch %d %s row %d (run of %d): an occurrence moves the row by %.3e, needed %.3e" % (
                    c.spec.id, bt.index, table, row, len(slots), contrib[slots].min(), c.need(table, row))
    return weakest, n_occ


def _faults(c):
    """{fault: (weights_of, {"user": rows hit, "item": rows hit})} -- the rows hit are planted rows."""
    rng = np.random.RandomState(11)
    occ = {bt.index: c.occurrences(bt) for bt in c.batches}
    out = {}

    def per_run(pick, value, applies=lambda bt, slots: True):
        hit = {"user": [], "item": []}
        w = {}
        for bt in c.batches:
            wx, wyz = np.ones(bt.size), np.ones(2 * bt.size)
            for table, arr in (("user", wx), ("item", wyz)):
                for row, slots in occ[bt.index][table].items():
                    if applies(bt, slots):
                        arr[slots[pick(slots)]] = value
                        hit[table].append(row)
            w[bt.index] = (wx, wyz[:bt.size], wyz[bt.size:])
        return (lambda bt: w[bt.index]), {k: np.array(v, dtype=np.int64) for k, v in hit.items()}

    out["dropped"] = per_run(lambda s: rng.randint(len(s)), 0.0)
    out["doubled"] = per_run(lambda s: rng.randint(len(s)), 2.0)
    if c.spec.hot_capable:
        hot = lambda bt, slots: len(slots) > C.SML_HOT
        if any(len(s) > C.SML_HOT for o in occ.values() for t in o.values() for s in t.values()):
            out["chunk-end"] = per_run(lambda s: min(len(s), C.SML_HOT_CHUNK) - 1, 0.0, hot)
        if any(len(s) > C.SML_HOT_CHUNK for o in occ.values() for t in o.values() for s in t.values()):
            out["last-chunk-end"] = per_run(lambda s: len(s) - 1, 0.0, hot)
    # a unique row never updated: every run of length 1, filler rows too; the planted ones must be seen
    w, hit = {}, {"user": [], "item": []}
    for bt in c.batches:
        ru, inv_u, cnt_u = np.unique(bt.tri[:, 0], return_inverse=True, return_counts=True)
        ij = np.concatenate([bt.tri[:, 1], bt.tri[:, 2]])
        ri, inv_i, cnt_i = np.unique(ij, return_inverse=True, return_counts=True)
        wx, wyz = (cnt_u[inv_u] > 1).astype(np.float64), (cnt_i[inv_i] > 1).astype(np.float64)
        w[bt.index] = (wx, wyz[:bt.size], wyz[bt.size:])
        hit["user"] += [r for r in ru[cnt_u == 1].tolist() if r in set(bt.planted_u.tolist())]
        hit["item"] += [r for r in ri[cnt_i == 1].tolist() if r in set(bt.planted_i.tolist())]
    out["unique-never-updated"] = ((lambda bt: w[bt.index]), {k: np.array(v, dtype=np.int64) for k, v in hit.items()})
    return out


@pytest.mark.parametrize("cid", IDS)
def test_case_census_sensitivity_and_planted_faults(cid):
    c = C.case(cid)
    s = c.spec
    _check_layout(c)
    print("%s U %d I %d e_ref %.3e M %.1f lr %g lam %g %g" % (s.id, c.U, c.I, c.e_ref, C.M[s.family], s.lr, s.lam_u, s.lam_i))
    # a float32 step whose sums run in sequence: at most half an ulp of the absolute sum per addition (the long runs of identical
    # addends -- a hot user under a hot item -- do round one way: 1.4e-5 at 3001 occurrences)
    longest = max(max(bt.plan_u + bt.plan_i) for bt in c.batches)
    assert 0.0 < c.e_ref <= (longest + 8) * 2.0 ** -24, c.e_ref
    assert np.isfinite(c.ref_u).all() and np.isfinite(c.ref_i).all() and (c.scale_u[c.touched_u] > 0).all() and (c.scale_i[c.touched_i] > 0).all()
    weakest, n_occ = _check_sensitivity(c)
    print("%s sensitivity: %d planted occurrences, weakest moves its row by %.1f x what is needed" % (s.id, n_occ, weakest))
    # the simulated engine without a fault: float64 rounded once
    su, si = c.simulate()
    e, table, row = c.worst(su, si)
    print("%s simulated engine: worst e %.3e (%s row %d), bound %.3e" % (s.id, e, table, row, c.bound()))
    assert e == 0.0 and not any(len(v) for v in c.failing_rows(su, si).values())
    w0u, w0i = (np.zeros((c.U, s.d)), np.zeros((c.I, s.d))) if s.adam else (c.wu.double().numpy(), c.wi.double().numpy())
    assert C.untouched_identical(su, w0u, c.touched_u) and C.untouched_identical(si, w0i, c.touched_i)
    for fault, (weights_of, hit) in _faults(c).items():
        gu, gi = c.simulate(weights_of)
        bad = c.failing_rows(gu, gi)
        n_hit = len(hit["user"]) + len(hit["item"])
        print("%s fault %-20s hits %3d planted rows, %5d rows fail" % (s.id, fault, n_hit, len(bad["user"]) + len(bad["item"])))
        assert len(bad["user"]) + len(bad["item"]) > 0, (s.id, fault)
        for k in ("user", "item"):
            missed = np.setdiff1d(hit[k], bad[k])
            assert not len(missed), (s.id, fault, k, missed[:8])
        if fault != "unique-never-updated":
            assert n_hit > 0 and len(bad["user"]) == len(hit["user"]) and len(bad["item"]) == len(hit["item"]), (s.id, fault)

