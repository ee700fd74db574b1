"""The cases of the gradient pin (test_grad_pin_host.py, test_grad_pin_gpu.py): inputs, float64 references (built once per case and
shared by every launch form of it), and the runs of an engine -- HipEngine on the GPU, OracleEngine on the host -- over them.
TEST INFRASTRUCTURE ONLY.

The batch sizes sit on the edges of the launch-geometry policy (capi.hip fwd_split / bwd_split over ceil(B/16) + ceil(2B/16) row
tiles): 336 | 337 is the last 4-way / first 2-way hidden split of the forward, 680 | 681 the last 2-way split with the
coordinate-split backward / first one-workgroup-per-tile forward and backward, 400 the middle of the 2-way range."""
import functools

import numpy as np
import torch

import _grad_ref as R
from conftest import make_transfer, quiet

# What the HIP step may exceed the fp32 oracle's own error by ("Gradient pin"): set from
# profiles/r14_grad_pin_ratios.json by the rule  margin = 4 if the worst recorded ratio <= 2 else twice the worst ratio.
MARGIN = 4.0
N_USER, N_ITEM, TABLE_SCALE = 300, 200, 0.3
LR_FROZEN = 1e-12

TR_SHAPES = [(32, 17), (32, 336), (32, 337), (32, 400), (32, 680), (32, 681), (32, 768),
             (64, 100), (64, 400), (64, 681), (128, 17), (128, 400), (128, 699)]
TR_BPR_SHAPES = [(32, 17), (32, 400), (32, 768), (64, 100), (64, 400), (64, 681), (128, 17), (128, 400), (128, 699)]
# (d, B, loss, special, env): special is None, "conv" (the ConvTransfer nets), "plan" or "clip"
TR_CASES = [(d, B, "bce", None, {}) for d, B in TR_SHAPES] + [(d, B, "bpr", None, {}) for d, B in TR_BPR_SHAPES] + [
    (32, 336, "bce", None, {"SML_TR_DEFER": "0"}),
    (32, 768, "bce", None, {"SML_TR_A2_RECOMPUTE": "0"}),
    (32, 256, "bpr", "conv", {}),
    (32, 256, "bce", "plan", {}),
    (32, 256, "bce", "clip", {}),
]
PLAN_SIZES, PLAN_SCALES = [256, 93, 0, 201, 40], [1.0, 0.4, 0.0, 0.85, 0.15625]
CLIP_MAX_NORM = 0.004


def case_id(c):
    """d32-B400-bce[-special][-ENV=value ...]: widths and batch sizes first, dictionaries as their items, None left out."""
    parts = ["d%d" % c[0], "B%d" % c[1]]
    for x in c[2:]:
        if isinstance(x, dict):
            parts += ["%s=%s" % kv for kv in sorted(x.items())]
        elif x is not None:
            parts.append(str(x))
    return "-".join(parts)


def short_batch(B):
    """The second batch: shorter than the first by at least 5 %."""
    return B - 37 if B >= 100 else B - B // 4


class TRInputs(object):
    def __init__(self, d, B, loss, special):
        torch.manual_seed(7 * d + B)                                  # (the seeds of test_tr_stage_every_backward_geometry_vs_oracle)
        self.d, self.B, self.bce = d, B, loss == "bce"
        wu, wi = torch.randn(N_USER, d) * TABLE_SCALE, torch.randn(N_ITEM, d) * TABLE_SCALE
        self.last_user, self.last_item, self.hat_user, self.hat_item = wu * 0.9, wi * 0.9, wu, wi
        sizes = PLAN_SIZES if special == "plan" else [B, short_batch(B)]
        scales = PLAN_SCALES if special == "plan" else [1.0, 1.0]
        n = sum(sizes)
        self.tri = torch.stack([torch.randint(0, N_USER, (n,)), torch.randint(0, N_ITEM, (n,)), torch.randint(0, N_ITEM, (n,))], 1)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.batches = [(self.tri[off[b]:off[b + 1]], scales[b]) for b in range(len(sizes))]
        self.plan = dict(batch_off=off, loss_scale=np.array(scales, dtype=np.float32)) if special == "plan" else None
        self.clip = CLIP_MAX_NORM if special == "clip" else None
        self.conv = special == "conv"
        self.state = None
        self.state = {k: v.clone() for k, v in self.make_net().state_dict().items()}

    def make_net(self, device="cpu"):
        if self.conv:
            from sml_amd.conv_transfer import ConvTransfer
            with quiet():
                net = ConvTransfer(self.d, self.d)
        else:
            net = make_transfer(self.d)
        if self.state is not None:
            net.load_state_dict(self.state)
        return net.to(device)

    def tables(self, device):
        return [t.to(device) for t in (self.last_user, self.last_item, self.hat_user, self.hat_item)]


@functools.lru_cache(maxsize=None)
def tr_case(d, B, loss, special):
    """(inputs, reference) of a TR case: the launch forms of one case share them, and nothing writes to them."""
    x = TRInputs(d, B, loss, special)
    ref = R.TRReference(x.make_net(), x.last_user, x.last_item, x.hat_user, x.hat_item, x.batches, bce=x.bce, clip_max_norm=x.clip)
    return x, ref


def run_tr(eng, x, device="cpu", keep_grad=False):
    """One TR epoch at frozen weights; returns (m, v, flat gradient buffer or None) by parameter name, as float64 arrays."""
    net = x.make_net(device)
    if keep_grad:
        eng.keep_theta_grad = True
    eng.tr_stage_epoch(net, *x.tables(device), x.tri, x.B, LR_FROZEN, 0.0, bce=x.bce, plan=x.plan, clip_max_norm=x.clip)
    if isinstance(eng.tr_state, list):                                 # the oracle: one AdamState per parameter
        m = {k: s.m.numpy().astype(np.float64) for (k, _), s in zip(net.named_parameters(), eng.tr_state)}
        v = {k: s.v.numpy().astype(np.float64) for (k, _), s in zip(net.named_parameters(), eng.tr_state)}
        return m, v, None
    names = {id(p): k for k, p in net.named_parameters()}
    out = []
    for flat in eng.tr_state[:3] if keep_grad else eng.tr_state[:2]:
        flat = flat.cpu().numpy()
        t = {}
        for p, off, cnt in eng.theta_views(net):
            if p.dim() == 4 and p.shape[2] == 2 and p.shape[0] == 10:
                # ConvTransfer's (2,1) conv1 kernel sits in the first two columns of the [10][3] block; the third stays zero
                block = flat[off:off + 30].reshape(10, 3)
                assert not block[:, 2].any()
                t[names[id(p)]] = block[:, :2].reshape(tuple(p.shape)).astype(np.float64)
            else:
                t[names[id(p)]] = flat[off:off + cnt].reshape(tuple(p.shape)).astype(np.float64)
        out.append(t)
    return out[0], out[1], (out[2] if keep_grad else None)


def judge_tr(ref, m, v, margin, grad=None):
    """The criterion over the moments of a TR epoch (and the kept flat buffer: the LAST batch's unclipped gradient).  Returns
    {"m" | "v" | "g": {tensor: report}}."""
    wm, wv = R.moment_weights(ref.n_batches)
    rep = {"m": R.judge(m, ref.m64, ref.m32, margin, zero=ref.zero, zero_abs=R.ZERO_ABS * wm)}
    yard_m = {k: r["yard"] for k, r in rep["m"].items() if r["yard"] is not None}
    rep["v"] = R.judge(v, ref.v64, yard_m, margin, factor=2.0, zero=ref.zero, zero_abs=R.ZERO_ABS ** 2 * wv)
    if grad is not None:
        rep["g"] = R.judge(grad, ref.grad64(-1), ref.grad32(-1), margin, zero=ref.zero)
    return rep


def all_failures(rep):
    return {(q, k): f for q, r in rep.items() for k, f in R.failures(r).items()}


def ratios(rep):
    return {q: {k: (None if r["ratio"] is None else round(r["ratio"], 4)) for k, r in rr.items()} for q, rr in rep.items()}


# ---------------------------------------------------------------------------------------------------------------- MF step
L2 = 1e-6
FORM_DISTINCT, FORM_FUSED, FORM_RUN = "distinct-rows", "per-occurrence+fused-update", "per-occurrence+run-update"
# (d, B, loss, adaptive_beta, env, the form the trace line must name)
MF_CASES = [
    (32, 48, "bce", None, {}, FORM_RUN),
    (32, 400, "bce", None, {}, FORM_RUN),
    (32, 400, "bprnorm", None, {}, FORM_RUN),
    (32, 700, "bce", None, {}, FORM_DISTINCT),
    (32, 700, "bce", None, {"SML_MF_BX3": "0"}, FORM_DISTINCT),
    (32, 700, "bce", None, {"SML_MF_DISTINCT": "0"}, FORM_FUSED),
    (32, 700, "bce", None, {"SML_MF_FUSED_UPDATE": "0"}, FORM_RUN),
    (32, 700, "bpr", None, {}, FORM_DISTINCT),
    (32, 700, "bprnorm", None, {"SML_MF_DISTINCT": "0"}, FORM_FUSED),
    (32, 700, "bce", 0.1, {}, FORM_RUN),
    (32, 1024, "bce", None, {}, FORM_DISTINCT),
    (32, 1024, "bce", None, {"SML_MF_DISTINCT": "0", "SML_MF_BX3": "0"}, FORM_FUSED),
    (32, 1024, "bpr", None, {"SML_MF_FUSED_UPDATE": "0", "SML_MF_BX3": "1"}, FORM_RUN),
    (64, 100, "bce", None, {}, FORM_RUN),
    (64, 100, "bpr", None, {}, FORM_RUN),
    (64, 1024, "bce", None, {"SML_MF_DISTINCT": "1", "SML_MF_FUSED_UPDATE": "1"}, FORM_DISTINCT),
    (64, 1024, "bce", None, {"SML_MF_DISTINCT": "0"}, FORM_FUSED),
    (64, 1024, "bprnorm", None, {"SML_MF_FUSED_UPDATE": "0"}, FORM_RUN),
    (128, 17, "bce", None, {}, FORM_RUN),
    (128, 17, "bprnorm", None, {}, FORM_RUN),
    (128, 700, "bce", None, {}, FORM_RUN),
    (128, 700, "bpr", None, {}, FORM_RUN),
]
MF_RUNS = ("full", "ragged", "two")       # one full batch; one ragged batch; two batches, the second missing rows of the first


class MFInputs(object):
    def __init__(self, d, B, loss, adaptive_beta):
        torch.manual_seed(11 * d + B)
        self.d, self.B = d, B
        self.bce, self.norm = loss == "bce", loss == "bprnorm"
        self.adaptive_beta = adaptive_beta
        wu, wi = torch.randn(N_USER, d) * TABLE_SCALE, torch.randn(N_ITEM, d) * TABLE_SCALE
        self.w_user, self.w_item, self.last_user, self.last_item = wu, wi, wu * 0.9, wi * 0.9
        # rows 0..19 of both tables are kept out of the random draws: planted rows and the two-batch run use them
        u, i, j = torch.randint(20, N_USER, (B,)), torch.randint(20, N_ITEM, (B,)), torch.randint(20, N_ITEM, (B,))
        u[::2] = 5                                                     # one user with B/2 occurrences
        i[1::7] = 3; j[2::7] = 3                                       # an item that is a positive and a negative of the batch
        j[0] = i[0]                                                    # pos == neg in one triple
        self.tri = torch.stack([u, i, j], 1)
        self.hot_user_occurrence = 2                                   # (an even position: one of user 5's)
        self.net = make_transfer(d)
        self.state = {k: v.clone() for k, v in self.net.state_dict().items()}

    def make_net(self, device="cpu"):
        net = make_transfer(self.d)
        net.load_state_dict(self.state)
        return net.to(device)

    def triples(self, run):
        """(all triples of the run, [(batch, scale)])."""
        B = self.B
        if run == "full":
            return self.tri, [(self.tri, 1.0)]
        if run == "ragged":
            t = self.tri[:short_batch(B)]
            return t, [(t, 1.0)]
        # two batches: the second one is the first with its users and items moved onto rows 0..19 wherever the row index is odd,
        # so about half of the first batch's rows sit the second step out and rows 0..19 arrive fresh
        t2 = self.tri.clone()
        for c in range(3):
            odd = t2[:, c] % 2 == 1
            t2[odd, c] = t2[odd, c] % 20
        return torch.cat([self.tri, t2]), [(self.tri, 1.0), (t2, 1.0)]


@functools.lru_cache(maxsize=None)
def mf_case(d, B, loss, adaptive_beta, run):
    x = mf_inputs(d, B, loss, adaptive_beta)
    _, batches = x.triples(run)
    ref = R.MFReference(x.net, x.last_user, x.last_item, x.w_user, x.w_item, batches, bce=x.bce, norm=x.norm, l2=L2,
                        adaptive_beta=adaptive_beta)
    return x, ref


@functools.lru_cache(maxsize=None)
def mf_inputs(d, B, loss, adaptive_beta):
    return MFInputs(d, B, loss, adaptive_beta)


def run_mf(eng, x, run, device="cpu"):
    """The MF stage over the run's batches on a FRESH engine, then the flush: (m, v, s) by table as float64 / int arrays."""
    from conftest import make_mf
    tri, batches = x.triples(run)
    mf = make_mf(N_USER, N_ITEM, x.d, x.w_user.numpy(), x.w_item.numpy(), device=device)
    net = x.make_net(device)
    lr = LR_FROZEN if len(batches) > 1 else 0.01          # one batch from zero moments: m = c1 g whatever the lr is
    eng.mf_stage_epoch(mf, net, x.last_user.to(device), x.last_item.to(device), tri, x.B, lr, L2, norm=x.norm, bce=x.bce,
                       adaptive_beta=x.adaptive_beta)
    eng.mf_flush(mf)
    st = eng.mf_state
    if isinstance(st, tuple):                                          # the oracle: dense AdamStates, no step stamps
        m = {"user": st[0].m.numpy().astype(np.float64), "item": st[1].m.numpy().astype(np.float64)}
        v = {"user": st[0].v.numpy().astype(np.float64), "item": st[1].v.numpy().astype(np.float64)}
        return m, v, None
    g = lambda k: st[k].cpu().numpy()
    return ({"user": g("m_u").astype(np.float64), "item": g("m_i").astype(np.float64)},
            {"user": g("v_u").astype(np.float64), "item": g("v_i").astype(np.float64)}, {"user": g("s_u"), "item": g("s_i")})


def judge_mf(ref, m, v, margin):
    """The criterion over the touched rows of each table; untouched rows must hold m = v = 0 exactly (asserted by the caller)."""
    sel = lambda t: {k: np.asarray(t[k])[ref.touched[k]] for k in ("user", "item")}
    rep = {"m": R.judge(sel(m), sel(ref.m64), sel(ref.m32), margin, tol=R.TOL_ROWS)}
    yard_m = {k: r["yard"] for k, r in rep["m"].items()}
    rep["v"] = R.judge(sel(v), sel(ref.v64), yard_m, margin, tol=R.TOL_ROWS, factor=2.0)
    return rep
