"""The cases of the transfer-forward pin (test_fwd_f64_host.py, test_fwd_f64_gpu.py): seeded inputs built on the CPU, the float64
reference of every case (built once and shared, never written to) and the per-row criterion.  TEST INFRASTRUCTURE ONLY.

Reference: oracle.sml_oracle.transfer_forward on .double() copies of the float32 rows and float32 weights -- ConvTransfer_com.forward
(conv1 kernel (3,1), the x_com row) and ConvTransfer.forward (conv1 kernel (2,1), the user net's output divided by its norm).
test_fwd_f64_host.py anchors it to the fixtures recorded from the real model.

Criterion, per row:  err(row) = max|got - ref| / max|ref(row)|;  a case's error is its worst row.  Never the whole-tensor norm: the
rows span three and a half orders of magnitude, and a small row may not hide beside a large one.

e_ref(case): the same figure for the oracle's float32 CPU forward over all ROWS rows of both nets.  Every bound of the two test
modules is a multiple of it.

A case is (d, type, weights): type "com" | "conv", weights "init" (the module's own initialisation) | "trained" (every tensor,
biases included, randn * 4 / sqrt(fan_in): the sigmoid-GELUs leave their linear range).  Both nets (user, item) of a case are run.
Rows: x_t and x_hat are randn times one per-row scale, log-uniform over [1e-3, 3] and shuffled, so that every 16- and 32-row tile
mixes magnitudes; PLANTED rows sit in different tiles at the head (what the small row counts see) and around row 8192 (what the
ragged tails of the 32-row form see).  A call on n rows uses the first n: rows are independent."""
import functools
import math

import numpy as np
import torch

from conftest import quiet
from oracle import sml_oracle as O

ROWS = 8224
GUARD_ROWS = 64
WIDTHS = (32, 64, 128)
CASES = [(d, typ, w) for d in WIDTHS for typ in ("com", "conv") for w in ("init", "trained")]
NETS = ("user", "item")
SCALE_LO, SCALE_HI = 1e-3, 3.0

# row counts: the 16-row form, its ragged tail, the last count before the switch | the 32-row form with tails of 1, 16, 17 rows, none
N_SMALL = (1, 15, 16, 17, 8192)
N_LARGE = (8193, 8208, 8209, 8224)

# planted rows: kind -> rows.  "t0": x_t = +0 (NaN row in ConvTransfer_com: x_com = 0 / 0, as the reference; finite in ConvTransfer),
# "h0": x_hat = +0, "tm": x_t = -0.0 (a zero-norm row as well), "hm": x_hat = -0.0
PLANTED = {"t0": (3, 8191, 8223), "h0": (13, 8192), "tm": (16, 8208), "hm": (40, 8200)}

# What a kernel may exceed e_ref by, per family.  The rule: 1.5 x the family's worst measured err / e_ref, rounded up to the next 0.5,
# never below 1.5.  Measured on an MI355X (profiles/r21_fwd_f64_ratios.json):
#   fp32 -- the fp32-product kernels (k_transfer_fwd<D,MT,NS,HSEQ>, k_side_transfer_fwd<D>): 0.72 .. 0.93 at d = 32, 0.95 .. 1.10 at
#           d = 64, 1.11 .. 1.65 at d = 128 (fc1 there is one chain of 160 dependent fp32 matrix products per accumulator)  -> 2.5
#   bx3  -- k_transfer_fwd_bx3<32,SIDE>: 0.68 .. 0.84                                                                          -> 1.5
M = {"fp32": 2.5, "bx3": 1.5}


def margin_from(worst_ratio):
    """The rule that turns a family's worst measured err / e_ref into its M."""
    return max(1.5, math.ceil(1.5 * worst_ratio / 0.5 - 1e-9) * 0.5)


def case_id(c):
    return "d%d-%s-%s" % c


class Case(object):
    def __init__(self, d, typ, weights):
        from sml_amd.conv_transfer import ConvTransfer, ConvTransfer_com
        self.d, self.typ, self.weights = d, typ, weights
        self.k2 = typ == "conv"
        seed = 1000 * d + 10 * (typ == "conv") + (weights == "trained")
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng():
            torch.manual_seed(seed)
            with quiet():
                self.module = (ConvTransfer if self.k2 else ConvTransfer_com)(d, d)
        if weights == "trained":
            with torch.no_grad():
                for net in (self.module.user_transfer, self.module.item_transfer):
                    for layer in (net.conv1, net.conv2, net.fc1, net.fc2):
                        s = 4.0 / math.sqrt(int(np.prod(layer.weight.shape[1:])))      # fan_in
                        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * s)
                        layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * s)
        for p in self.module.parameters():
            p.requires_grad_(False)
        # one scale per row: a log-uniform ladder, shuffled
        ladder = torch.exp(torch.linspace(math.log(SCALE_LO), math.log(SCALE_HI), ROWS, dtype=torch.float64)).float()
        scale = ladder[torch.randperm(ROWS, generator=g)].unsqueeze(1)
        self.x_t = torch.randn(ROWS, d, generator=g) * scale
        self.x_hat = torch.randn(ROWS, d, generator=g) * scale
        for r in PLANTED["t0"]:
            self.x_t[r] = 0.0
        for r in PLANTED["h0"]:
            self.x_hat[r] = 0.0
        for r in PLANTED["tm"]:
            self.x_t[r] = -0.0
        for r in PLANTED["hm"]:
            self.x_hat[r] = -0.0
        assert torch.signbit(self.x_t[PLANTED["tm"][0]]).all() and torch.signbit(self.x_hat[PLANTED["hm"][0]]).all()
        self.theta = {w: {k: v.detach().clone() for k, v in t.items()} for w, t in O.OracleEngine.theta_of(self.module).items()}
        self.ref, self.f32 = {}, {}
        for w in NETS:
            un = self.k2 and w == "user"
            self.ref[w] = O.transfer_forward({k: v.double() for k, v in self.theta[w].items()}, self.x_t.double(), self.x_hat.double(),
                                             unit_norm=un).numpy()
            self.f32[w] = O.transfer_forward(self.theta[w], self.x_t, self.x_hat, unit_norm=un).numpy()
            self.ref[w].setflags(write=False)
            self.f32[w].setflags(write=False)
        self.e_ref = max(worst_row(self.f32[w], self.ref[w]) for w in NETS)

    def nan_rows(self, n=ROWS):
        """The rows of the first n that the reference makes NaN: the zero-norm x_t rows, under ConvTransfer_com only."""
        rows = np.zeros(n, dtype=bool)
        if not self.k2:
            for r in PLANTED["t0"] + PLANTED["tm"]:
                if r < n:
                    rows[r] = True
        return rows


@functools.lru_cache(maxsize=None)
def case(d, typ, weights):
    return Case(d, typ, weights)


def row_errors(got, ref):
    """err per row against the float64 reference `ref`; rows whose reference is NaN are left out (nan), a non-finite value in any
    other row makes that row's error inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ref_nan = np.isnan(ref).any(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - ref).max(1) / np.abs(ref).max(1)
    e[~np.isfinite(got).all(1)] = np.inf
    e[ref_nan] = np.nan
    return e


def worst_row(got, ref):
    e = row_errors(got, ref)
    e = e[~np.isnan(e)]
    return float(e.max()) if e.size else 0.0


def nan_rows_of(a):
    return np.isnan(np.asarray(a)).any(1)


def check_rows(c, which, got, n, family, tag, ratios=None):
    """Assertions 1 and 2 of a call on the first n rows: the NaN rows are the reference's, nothing else is non-finite, and the worst
    row is within M[family] x e_ref.  Prints the figure before it asserts; records err / e_ref in `ratios` under `tag`."""
    got = np.asarray(got)
    ref = c.ref[which][:n]
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    want_nan = nan_rows_of(ref)
    assert np.array_equal(want_nan, c.nan_rows(n)), tag
    assert np.array_equal(np.isnan(got).all(1), want_nan) and np.array_equal(nan_rows_of(got), want_nan), \
        "%s: NaN rows %s, the reference's %s" % (tag, np.flatnonzero(nan_rows_of(got))[:8], np.flatnonzero(want_nan)[:8])
    assert np.isfinite(got[~want_nan]).all(), tag
    e = row_errors(got, ref)
    err = float(np.nanmax(e)) if (~want_nan).any() else 0.0
    at = int(np.nanargmax(e)) if (~want_nan).any() else -1
    assert err == worst_row(got, ref)
    bound = M[family] * c.e_ref
    print("%s n=%d %s: worst row %d err %.3e  e_ref %.3e  ratio %.3f  bound %.3e%s"
          % (tag, n, which, at, err, c.e_ref, err / c.e_ref, bound, "" if err <= bound else "   <-- MISS"))
    if ratios is not None:
        key = "%s|%s" % (tag, family)
        ratios[key] = max(ratios.get(key, 0.0), err / c.e_ref)
    return err, bound


# ------------------------------------------------------------------------------------------------------------------------------
# The bf16x3 product of k_transfer_fwd_bx3, restated: every fp32 operand split round-to-nearest-even into three bf16 planes, the six
# products a1 b1 + a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1 (each exact in float64), summed in float64.  `drop` removes plane pairs
# (a, b) by their 0-based planes; `zero_b3` = (k0, k1) zeroes the weight's third plane over reduction columns k0 .. k1 - 1 (one
# k-step of 32 in the tests).
SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))


def split3(x):
    x = x.float()
    p1 = x.bfloat16().float()
    r1 = x - p1
    p2 = r1.bfloat16().float()
    p3 = (r1 - p2).bfloat16().float()
    return [p1, p2, p3]


class Bx3Product(object):
    """a [n, K] x w [N, K]^T on the six bf16 products, float64 sums.  The six-term sum is formed once; a fault is that sum less the
    terms the fault loses (the same float64 additions in another order: differences far below the float32 rounding that follows)."""

    def __init__(self, a, w):
        self.ap, self.wp = [p.double() for p in split3(a)], [p.double() for p in split3(w)]
        self.six = sum(self.ap[pa] @ self.wp[pb].t() for pa, pb in SIX)

    def __call__(self, drop=(), zero_b3=None):
        out = self.six
        for pa, pb in drop:
            assert (pa, pb) in SIX
            out = out - self.ap[pa] @ self.wp[pb].t()
        if zero_b3 is not None:
            assert (0, 2) not in drop
            k0, k1 = zero_b3
            out = out - self.ap[0][:, k0:k1] @ self.wp[2][:, k0:k1].t()
        return out.float()                                            # rounded to float32 once


class Bx3Forward(object):
    """The forward of net `which` over the first n rows as the bf16x3 kernel computes it: the conv prologue, biases and GELUs in
    float32, fc1 and fc2 on Bx3Product.  run(fc1=..., fc2=...): keyword dictionaries for the products -- the planted faults."""

    def __init__(self, c, which, n):
        net, x_t, x_hat = c.theta[which], c.x_t[:n], c.x_hat[:n]
        if c.k2:
            X = torch.stack([x_t, x_hat], dim=1)
        else:
            X = torch.stack([x_t, x_hat, x_t * x_hat / (x_t ** 2).sum(-1).sqrt().unsqueeze(-1)], dim=1)
        N, H, d = X.shape
        h1 = O.gelu(torch.einsum("ch,nhw->ncw", net["conv1.weight"].reshape(O.C1, H), X) + net["conv1.bias"][None, :, None])
        h2 = torch.einsum("oc,ncw->now", net["conv2.weight"].reshape(O.C2, O.C1), h1) + net["conv2.bias"][None, :, None]
        self.net, self.unit = net, c.k2 and which == "user"
        self.p1 = Bx3Product(O.gelu(h2.reshape(N, O.C2 * d)), net["fc1.weight"])
        self.p2 = None                                                # fc2 over the unfaulted fc1, formed on first use

    def run(self, fc1=None, fc2=None):
        a2 = lambda: O.gelu(self.p1(**(fc1 or {})) + self.net["fc1.bias"])
        if fc1:
            p2 = Bx3Product(a2(), self.net["fc2.weight"])
        else:
            p2 = self.p2 = self.p2 if self.p2 is not None else Bx3Product(a2(), self.net["fc2.weight"])
        y = p2(**(fc2 or {})) + self.net["fc2.bias"]
        if self.unit:
            y = y / (y ** 2).sum(-1).sqrt().unsqueeze(-1)
        return y.numpy()


def old_criteria(got, sibling, oracle32):
    """What the suite held the bf16x3 kernel to before this pin (test_table_sized_forward_on_bf16_products_equals_the_fp32_products):
    whole-tensor max-norm difference from its fp32 sibling (< 3e-6) and from the oracle's float32 forward (1e-4), finite rows only."""
    ok = ~nan_rows_of(oracle32)
    sib = np.abs(got[ok] - sibling[ok]).max() / np.abs(sibling[ok]).max()
    orc = np.abs(got[ok] - oracle32[ok]).max() / np.abs(oracle32[ok]).max()
    return float(sib), float(orc)
