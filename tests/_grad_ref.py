"""Float64 reference for the gradients of the TR and MF training steps, and the criterion that holds Adam moments (or raw
gradients) against it.  TEST INFRASTRUCTURE ONLY, CPU only.

Why moments: Adam-updated weights (adam_close) divide the gradient by sqrt(v), so they neither see a gradient's size nor,
after two steps at lr = 1e-3, a contribution of a percent that went missing.  With the weights frozen (lr = 1e-12, weight decay 0, or
a fresh engine) the first and second moments ARE the gradients, linearly and squared:

    m <- m + c1 (g - m)        v <- c2' v + c2 g^2

so float64 can follow them.  The net is not transcribed a second time: oracle/sml_oracle.py's run_mf / transfer_forward do not
depend on the dtype, so the reference is torch.autograd over them with theta and the tables cast to float64, and the yardstick is
the same call in float32.

The criterion is per tensor (one of theta's 16, or the touched rows of one table), max-norm relative:

    err(x) = max|x - ref64| / max|ref64|        bound = max(project tolerance of the kind, margin * err(fp32 oracle))

The project tolerances are G2's (test_g2_run_mf_backward_...): 5e-5 for weights and rows, 3e-4 for biases; they were set at G2's
small batch, and at ~700 rows the fp32 oracle itself is off from float64 by more than that -- hence the measured yardstick.  v's
bound is twice m's.  Under the BPR kinds d loss / d(item fc2.bias) is exactly zero: that tensor has no scale to be relative to, it is
held to G2's absolute 1e-5 times the weight the moment gives it.
"""
import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
from oracle import sml_oracle as O

# the decay constants as fp32 arithmetic applies them (sml_dev.h adam_apply: 1.0f - SML_BETA1, SML_BETA2, 1.0f - SML_BETA2)
C1 = float(np.float32(1.0) - np.float32(0.9))
C2P = float(np.float32(0.999))
C2 = float(np.float32(1.0) - np.float32(0.999))
TOL_WEIGHT, TOL_BIAS, TOL_ROWS = 5e-5, 3e-4, 5e-5
ZERO_ABS = 1e-5                 # a gradient that is exactly zero in the reference (G2's bound)
ZERO_TENSOR = "item_transfer.fc2.bias"


def tol_of(name):
    return TOL_BIAS if name.endswith("bias") else TOL_WEIGHT


def theta_names(net):
    return [k for k, _ in net.named_parameters()]


def _theta(net, dtype):
    """{'user': {...}, 'item': {...}} of fresh leaves in `dtype`, and the same leaves by parameter name."""
    by_name = {k: p.detach().to(dtype).clone().requires_grad_(True) for k, p in net.named_parameters()}
    theta = {w: {k: by_name["%s_transfer.%s" % (w, k)] for k in O.NET_KEYS} for w in ("user", "item")}
    return theta, by_name


def is_bpr(net, bce):
    """The loss the step takes is a BPR kind: asked for, or the ConvTransfer nets (their run_MF has no other)."""
    return (not bce) or int(net.user_transfer.conv1.weight.shape[2]) == 2


def clip_coef(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_'s factor, min(1, max_norm / (||g||_2 + 1e-6)), in the gradients' own dtype."""
    total = torch.sqrt(sum((g * g).sum() for g in grads.values()))
    return torch.clamp(max_norm / (total + 1e-6), max=1.0)


def tr_gradients(net, last_user, last_item, hat_user, hat_item, batches, bce=True, dtype=torch.float64, drop_last_of=None, norm=False):
    """d loss / d theta of every batch in `batches` [(triples [n,3], loss scale)], at the FIXED weights of `net`: a list of
    {parameter name: tensor}.  An empty batch has a zero gradient.  drop_last_of = b: batch b's last triple contributes nothing
    while the batch keeps its length (what a kernel that skips a row computes: the BCE mean's divisor stays) -- a planted defect.
    norm: the BPR-norm kind (the TR stage never takes it; G2 records it)."""
    theta, by_name = _theta(net, dtype)
    tabs = [t.detach().to(dtype) for t in (last_user, hat_user, last_item, hat_item)]
    names = list(by_name)

    def grad_of(t, scale):
        if t.shape[0] == 0:
            return {k: torch.zeros_like(by_name[k]) for k in names}
        u, i, j = t[:, 0], t[:, 1], t[:, 2]
        loss = scale * O.run_mf(theta, tabs[0][u], tabs[1][u], tabs[2][i], tabs[3][i], tabs[2][j], tabs[3][j], norm=norm, bce=bce)
        gs = torch.autograd.grad(loss, [by_name[k] for k in names], allow_unused=True)
        return {k: (g if g is not None else torch.zeros_like(by_name[k])) for k, g in zip(names, gs)}

    out = []
    for b, (t, scale) in enumerate(batches):
        g = grad_of(t, scale)
        if drop_last_of == b:
            # the loss is a mean (BCE) or a sum (BPR) of per-triple terms: the last triple's share is the one-row batch's
            # gradient, divided by the batch length under BCE
            share = scale / t.shape[0] if not is_bpr(net, bce) else scale
            last = grad_of(t[-1:], share)
            g = {k: g[k] - last[k] for k in names}
        out.append(g)
    return out


def clipped(grads, max_norm):
    """The per-batch gradients after clip_grad_norm_ (each batch has its own factor), and the factors."""
    if not max_norm:
        return grads, [1.0] * len(grads)
    coefs = [clip_coef(g, max_norm) if any(bool(x.any()) for x in g.values()) else torch.ones(()) for g in grads]
    return [{k: x * c for k, x in g.items()} for g, c in zip(grads, coefs)], [float(c) for c in coefs]


def moments64(grads):
    """Adam's moments after the batches' gradients, from m = v = 0, in float64 with the fp32 decay constants."""
    m = {k: np.zeros(tuple(g.shape)) for k, g in grads[0].items()}
    v = {k: np.zeros(tuple(g.shape)) for k, g in grads[0].items()}
    for g in grads:
        for k in m:
            x = g[k].detach().double().numpy()
            m[k] = m[k] + C1 * (x - m[k])
            v[k] = C2P * v[k] + C2 * x * x
    return m, v


def moments32(grads):
    """The same moments as the fp32 oracle forms them (O.adam_dense_step on fp32 gradients; the weights it steps are thrown away)."""
    m = {k: torch.zeros_like(g, dtype=torch.float32) for k, g in grads[0].items()}
    v = {k: torch.zeros_like(g, dtype=torch.float32) for k, g in grads[0].items()}
    for s, g in enumerate(grads):
        for k in m:
            O.adam_dense_step(torch.zeros_like(m[k]), g[k].detach().float(), m[k], v[k], s + 1, 0.0)
    return {k: x.numpy().astype(np.float64) for k, x in m.items()}, {k: x.numpy().astype(np.float64) for k, x in v.items()}


def moment_weights(n_batches):
    """What a constant gradient g (g^2) leaves in m (v) after n batches: the scale of the absolute bound of a zero tensor."""
    wm = wv = 0.0
    for _ in range(n_batches):
        wm = wm + C1 * (1.0 - wm)
        wv = C2P * wv + C2
    return wm, wv


class TRReference(object):
    """Everything the tests hold a TR epoch against: per batch the float64 gradient of every theta tensor (raw: g64_raw; after
    clipping: g64), the moments they give (m64, v64), and the same in fp32 (g32_raw, g32, m32, v32) -- the yardstick."""

    def __init__(self, net, last_user, last_item, hat_user, hat_item, batches, bce=True, clip_max_norm=None, drop_last_of=None):
        self.names = theta_names(net)
        self.n_batches = len(batches)
        self.zero = {ZERO_TENSOR} if is_bpr(net, bce) else set()
        args = (net, last_user, last_item, hat_user, hat_item, batches)
        self.g64_raw = tr_gradients(*args, bce=bce, dtype=torch.float64, drop_last_of=drop_last_of)
        self.g32_raw = tr_gradients(*args, bce=bce, dtype=torch.float32)
        self.g64, self.coef64 = clipped(self.g64_raw, clip_max_norm)
        self.g32, self.coef32 = clipped(self.g32_raw, clip_max_norm)
        self.m64, self.v64 = moments64(self.g64)
        self.m32, self.v32 = moments32(self.g32)

    def grad64(self, b, raw=True):
        return {k: x.detach().numpy() for k, x in (self.g64_raw if raw else self.g64)[b].items()}

    def grad32(self, b, raw=True):
        return {k: x.detach().numpy().astype(np.float64) for k, x in (self.g32_raw if raw else self.g32)[b].items()}


def mf_row_gradients(net, last_user, last_item, w_user, w_item, tri, scale=1.0, bce=True, norm=False, l2=0.0, adaptive_beta=None,
                     dtype=torch.float64):
    """The MF stage's loss of one batch (mf_batch_loss of the oracle: run_MF over the six gathered row blocks + the l2 term, and
    the --need_adaptive term over the batch's unique users) differentiated with respect to the GATHERED rows: per-occurrence
    gradients (gu, gi, gn: [n,d] each), and the unique users with the adaptive term's gradient rows (or None).  The table gradient
    is their scatter-add (table_gradients)."""
    theta = {w: {k: p.detach().to(dtype) for k, p in t.items()} for w, t in O.OracleEngine.theta_of(net).items()}
    lu, li, wu, wi = [t.detach().to(dtype) for t in (last_user, last_item, w_user, w_item)]
    u, i, j = tri[:, 0], tri[:, 1], tri[:, 2]
    uh, ih, nh = [x.clone().requires_grad_(True) for x in (wu[u], wi[i], wi[j])]
    loss = scale * O.run_mf(theta, lu[u], uh, li[i], ih, li[j], nh, norm=norm, bce=bce)
    loss = loss + l2 * 0.5 * torch.sum(uh ** 2 + ih ** 2 + nh ** 2)
    gu, gi, gn = torch.autograd.grad(loss, [uh, ih, nh])
    extra = None
    if adaptive_beta:
        count = torch.bincount(u)
        uu = torch.unique(u)
        ul = wu[uu].clone().requires_grad_(True)
        norm_user = (ul.detach() ** 2).sum(dim=-1).sqrt()
        term = torch.mul(adaptive_beta * count[uu] / norm_user, (ul ** 2).sum(dim=-1)).sum()
        extra = (uu, torch.autograd.grad(term, [ul])[0])
    return gu, gi, gn, extra


def table_gradients(n_user, n_item, tri, gu, gi, gn, extra=None, skip_user_occurrence=None):
    """Dense table gradients from per-occurrence ones.  skip_user_occurrence = k: the k-th triple's user row contributes nothing
    (one occurrence of a duplicated row left out) -- a planted defect."""
    g_user = torch.zeros(n_user, gu.shape[1], dtype=gu.dtype)
    g_item = torch.zeros(n_item, gi.shape[1], dtype=gi.dtype)
    keep = torch.ones(tri.shape[0], dtype=torch.bool)
    if skip_user_occurrence is not None:
        keep[skip_user_occurrence] = False
    g_user.index_add_(0, tri[keep, 0], gu[keep])
    g_item.index_add_(0, tri[:, 1], gi)
    g_item.index_add_(0, tri[:, 2], gn)
    if extra is not None:
        g_user.index_add_(0, extra[0], extra[1])
    return g_user, g_item


class MFReference(object):
    """The MF stage's table gradients of each batch at FIXED tables, the dense-Adam moments they give (a row that sits a batch out
    decays: m <- (1 - c1) m, v <- c2' v) and the rows each table has touched, in float64 and in fp32."""

    def __init__(self, net, last_user, last_item, w_user, w_item, batches, bce=True, norm=False, l2=0.0, adaptive_beta=None,
                 skip_user_occurrence=None):
        U, I = w_user.shape[0], w_item.shape[0]
        self.n_batches = len(batches)
        self.g = {}
        for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
            gs = []
            for tri, scale in batches:
                rows = mf_row_gradients(net, last_user, last_item, w_user, w_item, tri, scale, bce, norm, l2, adaptive_beta, dtype)
                skip = skip_user_occurrence if tag == "64" else None
                gu, gi = table_gradients(U, I, tri, *rows, skip_user_occurrence=skip)
                gs.append({"user": gu, "item": gi})
            self.g[tag] = gs
        self.m64, self.v64 = moments64(self.g["64"])
        self.m32, self.v32 = moments32(self.g["32"])
        tu = np.zeros(U, dtype=bool); ti = np.zeros(I, dtype=bool)
        for tri, _ in batches:
            tu[tri[:, 0].numpy()] = True
            ti[tri[:, 1].numpy()] = True
            ti[tri[:, 2].numpy()] = True
        self.touched = {"user": tu, "item": ti}


def err(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-300))


def judge(got, ref, yard, margin, tol=tol_of, factor=1.0, zero=(), zero_abs=ZERO_ABS):
    """The criterion, tensor by tensor: {name: dict(err, yard, bound, ratio, ok)}.  `got`, `ref` (float64) and `yard` (the fp32
    oracle's) map names to arrays; `yard` may instead map names to ready-made errors (v's bound is twice m's: pass m's yardstick
    and factor = 2).  ratio = err / max(err(fp32 oracle), tolerance / 4) is what the margin is set from.  Tensors in `zero` are
    exactly zero in the reference and held to `zero_abs` absolutely."""
    out = {}
    for k in ref:
        if k in zero:
            assert not np.any(ref[k]), k
            e = float(np.abs(np.asarray(got[k], dtype=np.float64)).max())
            out[k] = dict(err=e, yard=None, bound=zero_abs, ratio=None, ok=e <= zero_abs)
            continue
        y = yard[k] if np.isscalar(yard[k]) else err(yard[k], ref[k])
        t = tol(k) if callable(tol) else tol
        e = err(got[k], ref[k])
        bound = factor * max(t, margin * y)
        out[k] = dict(err=e, yard=y, bound=bound, ratio=e / (factor * max(y, t / 4.0)), ok=e <= bound)
    return out


def failures(report):
    return {k: (r["err"], r["bound"]) for k, r in report.items() if not r["ok"]}
