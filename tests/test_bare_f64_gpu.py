"""The bare embed+loss step -- SGD (sml_embed_loss_sgd_epoch: k_bare_grad -> k_run_update<D,T,0,HOTB> -> k_hot_apply) and Adam
(sml_embed_loss_adam_epoch: k_bare_grad<LAZY> -> k_run_update<D,float,1,false>) -- against the float64 reference, row by row.
Run on the MI355X box:  python -m pytest tests/test_bare_f64_gpu.py -m gpu

Cases, reference and criterion: tests/_bare_f64_cases.py (what they can see: tests/test_bare_f64_host.py).  Which code a row's update
takes is decided by its run length in the batch, the batch size of the epoch and the launch form:

  inline     bare_epoch builds the lists itself; their read-back has not landed when the run kernel is launched, so with a batch size
             >= 4096 the hot-capable kernel (HOTB = true) and k_hot_apply run whatever the run lengths are;
  prepared   bare_prepare, a device synchronise (so that sml_embed_loss_sgd_epoch finds the lists' event complete: `known`), then
             bare_epoch(prepared=...): plain arguments, an exact grid, and the light-tailed kernel (HOTB = false, no k_hot_apply)
             when no run of the epoch exceeds 128.

Per SGD case, both forms:
  1. every touched row of both tables has e(r) <= M[family] x e_ref(case);
  2. every row no batch touches is bit-identical (test_hip_parity._untouched_identical);
  3. the per-batch losses agree with the float64 losses at rtol 1e-4, fp16 tables included (the reference reads the same values);
  4. the two forms give the same bits, tables and losses;
  5. the timing classes count one k_bare_grad and one k_seg_update_sgd per batch, and k_hot_rows (k_hot_apply) per batch exactly
     when the form and the case say so -- for the capped cases the two forms ARE the two kernels that must round alike.
Per Adam case (a fresh optimiser state, one batch): m / C1 of every touched row against the float64 gradient sum under the same
figure (family "adam"), m = v = 0 exactly on every other row, the loss at rtol 1e-4.

Every figure is printed before it is asserted on; with SML_BARE_F64_RATIOS=<path> the worst e / e_ref per (case, form) and family is
written there as JSON.  profiles/r23_bare_f64_ratios.json is such a run; test_bare_f64_host.py re-derives M from it."""
import json
import os

import numpy as np
import pytest
import torch

import _bare_f64_cases as C
from conftest import make_mf
from test_hip_parity import _untouched_identical

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}
LOSS_RTOL = 1e-4


def engine(d, mb):
    from sml_amd.engine import HipEngine
    return HipEngine(DEV, d, mb)


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    path = os.environ.get("SML_BARE_F64_RATIOS")
    if path and RATIOS:
        worst = {}
        for key, r in RATIOS.items():
            fam = key.rsplit("|", 1)[1]
            if fam not in worst or r > worst[fam]["ratio"]:
                worst[fam] = dict(ratio=r, case=key)
        with open(path, "w") as f:
            json.dump(dict(ratio="worst touched row's e(HIP) / e_ref(case) over both tables; e(r) = max(0, max_k |got - ref| - store(r)) / "
                                 "scale(r) against float64, e_ref: the same for the float32 oracle (fp16 tables: rounded once)",
                           margin=C.M, worst=worst, cases=RATIOS), f, indent=1, sort_keys=True)
        print("WORST ratios %s" % worst)


def judge(c, got_u, got_i, tag, misses):
    """Assertion 1: prints the worst row's figure, records e / e_ref, notes a miss."""
    e, table, row = c.worst(got_u, got_i)
    bad = c.failing_rows(got_u, got_i)
    n_bad = len(bad["user"]) + len(bad["item"])
    print("%s: worst %s row %d e %.3e  e_ref %.3e  ratio %.3f  bound %.3e  rows over %d%s"
          % (tag, table, row, e, c.e_ref, e / c.e_ref, c.bound(), n_bad, "" if not n_bad else "   <-- MISS %s %s" % (bad["user"][:6], bad["item"][:6])))
    key = "%s|%s" % (tag, c.spec.family)
    RATIOS[key] = max(RATIOS.get(key, 0.0), e / c.e_ref)
    if n_bad or not e <= c.bound():
        misses.append((tag, table, row, e, c.bound(), n_bad))


def run_sgd(eng, c, form):
    """One epoch over the case's three batches; returns (user table, item table, losses, {timing class: launches})."""
    s = c.spec
    gu, gi = c.wu.to(DEV).clone(), c.wi.to(DEV).clone()
    tri = torch.from_numpy(c.tri).to(DEV)
    torch.cuda.synchronize()
    eng.profile(True)
    if form == "prepared":
        prep = eng.bare_prepare(tri, s.B, c.U, c.I)
        torch.cuda.synchronize()                          # the lists' read-back has landed: the epoch knows its longest run
        losses = eng.bare_epoch(gu, gi, tri, s.B, s.lr, s.lam_u, s.lam_i, bce=s.bce, prepared=prep)
    else:
        losses = eng.bare_epoch(gu, gi, tri, s.B, s.lr, s.lam_u, s.lam_i, bce=s.bce)
    torch.cuda.synchronize()
    prof = {k: v[0] for k, v in eng.profile_read("main").items()}
    eng.profile(False)
    return gu, gi, losses.cpu(), prof


@pytest.mark.parametrize("cid", [s.id for s in C.SGD_CASES])
def test_sgd_step_vs_float64_inline_and_prepared(cid):
    c = C.case(cid)
    s = c.spec
    nb = len(c.batches)
    longest = max(max(bt.plan_u + bt.plan_i) for bt in c.batches)
    eng = engine(s.d, s.B)
    misses, out = [], {}
    wu0, wi0 = c.wu.to(DEV), c.wi.to(DEV)
    for form in ("inline", "prepared"):
        gu, gi, losses, prof = run_sgd(eng, c, form)
        out[form] = (gu, gi, losses)
        tag = "%s|%s" % (s.id, form)
        print("%s: launches %s" % (tag, {k: prof.get(k, 0) for k in ("k_bare_grad", "k_seg_update_sgd", "k_hot_rows")}))
        judge(c, gu.cpu().double().numpy(), gi.cpu().double().numpy(), tag, misses)
        assert _untouched_identical(gu, wu0, c.touched_u) and _untouched_identical(gi, wi0, c.touched_i), tag
        rel = np.abs(losses.double().numpy() - c.loss64) / np.abs(c.loss64)
        print("%s: losses %s  float64 %s  worst relative difference %.3e" % (tag, losses.numpy(), c.loss64, rel.max()))
        assert rel.max() <= LOSS_RTOL, (tag, rel)
        assert prof.get("k_bare_grad", 0) == nb and prof.get("k_seg_update_sgd", 0) == nb, (tag, prof)
        if form == "prepared":
            # the epoch knows its longest run: the hot kernels run exactly when one exceeds SML_HOT in a hot-capable epoch
            assert prof.get("k_hot_rows", 0) == (nb if s.hot_capable and longest > C.SML_HOT else 0), (tag, prof)
        else:
            # (lists in flight: hot rows are assumed -- unless the read-back won the race, which changes no bit)
            assert prof.get("k_hot_rows", 0) in ((0, nb) if s.hot_capable else (0,)), (tag, prof)
    eng.close()
    (au, ai, al), (bu, bi, bl) = out["inline"], out["prepared"]
    assert torch.equal(au, bu) and torch.equal(ai, bi) and torch.equal(al, bl), "%s: the two launch forms differ" % s.id
    assert not torch.equal(au, wu0) and not torch.equal(ai, wi0)
    assert not misses, misses


@pytest.mark.parametrize("cid", [s.id for s in C.ADAM_CASES])
def test_adam_first_moments_vs_float64(cid):
    c = C.case(cid)
    s = c.spec
    eng = engine(s.d, s.B)                                 # a fresh engine: a fresh optimiser state
    mf = make_mf(c.U, c.I, s.d, c.wu.numpy(), c.wi.numpy(), device=DEV)
    losses = eng.bare_adam_epoch(mf, torch.from_numpy(c.tri).to(DEV), s.B, 0.01, s.lam_u, s.lam_i, bce=s.bce).cpu()
    torch.cuda.synchronize()
    st = {k: eng.mf_state[k].cpu() for k in ("m_u", "m_i", "v_u", "v_i")}
    eng.close()
    misses = []
    judge(c, st["m_u"].double().numpy() / C.C1, st["m_i"].double().numpy() / C.C1, "%s|adam" % s.id, misses)
    for k, touched in (("m_u", c.touched_u), ("v_u", c.touched_u), ("m_i", c.touched_i), ("v_i", c.touched_i)):
        assert _untouched_identical(st[k], torch.zeros_like(st[k]), touched), k
        assert bool((st[k][torch.from_numpy(touched)] != 0).any(1).all()), k
    rel = np.abs(losses.double().numpy() - c.loss64) / np.abs(c.loss64)
    print("%s: loss %s  float64 %s  relative difference %.3e" % (s.id, losses.numpy(), c.loss64, rel.max()))
    assert rel.max() <= LOSS_RTOL, rel
    assert not misses, misses
