"""The cases of the bare-step pin (test_bare_f64_host.py, test_bare_f64_gpu.py): seeded triples with PLANTED run lengths, the float64
reference of one synchronous minibatch step, and the per-row criterion.  TEST INFRASTRUCTURE ONLY.

The step under test: sml_embed_loss_sgd_epoch (k_bare_grad -> k_run_update<.., 0, HOTB> -> k_hot_apply) and, over the same run
records, sml_embed_loss_adam_epoch (k_bare_grad<LAZY> -> k_run_update<.., 1, false>).  What decides the code a row's update takes is
the row's RUN LENGTH in its batch (sml_amd/csrc/mf_kernels.hip): 1 -- applied in place by k_bare_grad (SGD); <= LONG (4 SGD, 8 Adam)
-- the record's own lane group, from the slots inlined in the record (Adam: slots 4 .. 7 from the value list); longer -- the whole
wavefront in LD * G strides and an xor tree; > SML_HOT = 128 in an epoch whose batch size is >= 4096 -- chunk reducers of
SML_HOT_CHUNK = 512 occurrences (16 * GB occurrences a trip) and k_hot_apply (8 * G chunk partials a trip).  So every case PLANTS rows
with chosen run lengths and the host module takes a census of them.

Reference: bare_step_f64 -- numpy float64 on the table values exactly as stored (fp16 -> float64 is exact); loss and gradient of
oracle.sml_oracle.bare_step (pair loss: BCE a mean over the batch, BPR a sum; plus lam / 2 * sum over occurrences).

Criterion, per touched row r (never per tensor):
    store(r) = the largest half-ulp, in the table's type, of ref_new[r, :]
    scale(r) = lr * max_k sum_t |g_t[k]|       (the absolute sum of the row's per-occurrence gradient contributions, L2 term included)
    e(r)     = max(0, max_k |got - ref_new| - store(r)) / scale(r)
    e_ref    = the worst e(r) of the float32 oracle (O.bare_step, on one thread: see one_thread) on the same case; fp16 tables: its
               result rounded once to fp16
    pass     <=> every touched row has e(r) <= M[family] * e_ref(case)
Adam moments: after step 1 from a fresh state m = (1 - beta1) * g, so m / C1 is the row's summed gradient; ref = the float64 sum,
store = half-ulp of m scaled back by 1 / C1, scale without the lr, e_ref from the float32 autograd gradient.

Epoch layout (SGD): three batches -- two full, one ragged -- over DISJOINT row ranges of both tables, so every row is stepped by
exactly one batch and the one-step reference from the initial tables is exact for it, while the per-batch slicing of the lists
(batch_index, off_*, cnt_*) is still exercised.  Since the ranges are disjoint, "row 0 and the last row in every batch" is read as:
the first and last rows of the batch's own range are planted, and their neighbours (planted rows fill the range from both ends
inwards) -- row 0 and the last row of either table are therefore planted, and so are the rows on both sides of every range border.
Items are planted as positive only, negative only or mixed (cycling with the plan and the batch); one mixed item per batch has one
i == j triple.  In an i == j triple the user's gradient is only (dsp + dsn) * w_i + lam * w_u -- nearly nothing -- so the users of
such triples are always filler rows (the sensitivity condition speaks of planted occurrences).  Filler: rows with run lengths 1, 2
and 3 (about half, a quarter and a quarter of the filler occurrences), drawn without replacement from the middle of the range;
SLACK rows of every range are named by no triple.

Coherent sums.  Shuffled independently, a user of 3001 occurrences and an item of 3001 would share 3001 * 3001 / 8192 = 1100
triples, each adding the SAME gradient row to both: the row then moves by a thousand times one occurrence, and neither an fp16 table
(11 bits) nor the float32 oracle's sequential sum (identical addends round one way: e_ref = 1.4e-5 instead of 1e-6) resolves one
occurrence of it.  So (a) in a batch, no run longer than DECORRELATE = 256 of a user shares a triple with such a run of an item
(users swapped after the shuffle; needs the long runs of both tables to fit the batch side by side), and (b) where they do not fit
-- the classes plan has 7359 user occurrences in a batch of 8192 -- the plan is split: the first full batch plants every length
for users and the lengths up to 130 for items, the second the reverse.  Every length is still planted for a user and for an item
in every epoch, the lengths up to 130 twice.  The Adam cases are one batch of 2048 each, with 1800 long occurrences per table: they
come in pairs, adam_u (every length for users, up to 65 for items) and adam_i (the reverse).

Step sizes.  The criterion can see ONE lost occurrence only if that occurrence moves the row by more than the storage rounding:
    fp32 tables: randn * 0.3 * sqrt(32 / d) (the scores of d = 32 at every width: at 0.3 and d = 128 one triple in a few thousand
    is ranked so well that its coefficient sigmoid(-x) all but vanishes, and with it that occurrence), BPR lr = 0.01;   fp16 tables: randn * 0.1 (scores in the sigmoid's linear range: every pair coefficient
    is about 0.5), BPR lr = 0.05 -- one occurrence moves a row by about lr * 0.5 * 0.2 = 5e-3, forty fp16 half-ulps at |w| ~ 0.25.
    BCE is a mean: lr = lr_BPR * B and lam = lam_BPR / B make its step the size of the BPR step (the pair term stays the larger part
    of every occurrence: lam_u = 0.02, lam_i = 0.04 against coefficients of 0.5).
test_bare_f64_host.py checks that this is enough for every planted occurrence (the sensitivity condition)."""
import collections
import contextlib
import functools
import json
import os

import numpy as np
import torch

from _fwd_f64_cases import margin_from          # noqa: F401  (the one rule that turns a worst measured ratio into a margin)
from _grad_ref import C1
from conftest import REPO
from oracle import sml_oracle as O

LONG_SGD, LONG_ADAM, SML_HOT, SML_HOT_CHUNK, HOT_MIN_BATCH = 4, 8, 128, 512, 4096      # sml_kernels.h / mf_kernels.hip / capi.hip
SLACK = 37                                   # rows of every batch's range (both tables) that no triple names
LAM_U, LAM_I = 0.002, 0.004
DECORRELATE = 256                            # runs longer than this: a long user never meets a long item in a triple
DEEP_NEG = 200
RATIOS_FILE = os.path.join(REPO, "profiles", "r23_bare_f64_ratios.json")

# What a kernel may exceed e_ref by, per family: margin_from(the family's worst measured e / e_ref on an MI355X,
# profiles/r23_bare_f64_ratios.json) -- 1.5 x the worst, rounded up to the next 0.5, never below 1.5.
#   fp32 -- k_bare_grad / k_run_update<D,float,0,*> / k_hot_apply<D,float>: 0.04 .. 1.16 (the kernels' own e(r) is 0.9e-7 .. 1.6e-7
#           in every case; e_ref runs from 1.0e-7 to 3.8e-6, the oracle's sequential sum over 8392 occurrences)             -> 2.0
#   fp16 -- the same kernels on __half tables: 0.87 .. 1.00; in eleven of twelve cases exactly 1.00 -- the worst row is a value the
#           float32 result rounds to the far side of an fp16 midpoint, and the kernel's float32 result rounds the same way   -> 1.5
#   adam -- k_bare_grad<LAZY> / k_run_update<D,float,1,false>, m / C1: 0.02 .. 1.09 (own e(r) 1.7e-7 .. 5.4e-7)              -> 2.0
M = {"fp32": 2.0, "fp16": 1.5, "adam": 2.0}

# run-length plans (for a user and for an item each)
CLASSES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128, 129, 130, 511, 512, 513, 1024, 1025, 3001)
CAPPED = tuple(L for L in CLASSES if L <= SML_HOT)
SHORT = tuple(L for L in CLASSES if L <= SML_HOT + 2)
RAGGED, RAGGED_CAPPED = (129, 600), (100, 128)
NO_HOT = (129, 700, 1500)
ADAM = (1, 4, 5, 8, 9, 16, 17, 64, 65, 300, 1500)
MANY_HOT_U = tuple(129 + k % 12 for k in range(100))
MANY_HOT_I = tuple(129 + (k + 5) % 12 for k in range(160))


class Spec(object):
    """name, width, table type, loss, batch size, [(batch length, user plan, item plan, deep)], optimiser."""

    def __init__(self, plan, d, half, bce, B, batches, adam=False):
        self.plan, self.d, self.half, self.bce, self.B, self.batches, self.adam = plan, d, half, bce, B, batches, adam
        self.family = "adam" if adam else ("fp16" if half else "fp32")
        self.id = "%s-d%d-%s-%s" % (plan, d, "f16" if half else "f32", "bce" if bce else "bpr")
        self.scale = 0.1 if half else 0.3 * (32.0 / d) ** 0.5
        k = float(B) if bce else 1.0
        self.lr = (0.05 if half else 0.01) * k
        self.lam_u, self.lam_i = LAM_U / k, LAM_I / k
        self.hot_capable = (not adam) and B >= HOT_MIN_BATCH

    def __repr__(self):
        return self.id


def _epoch(B, plan_u, plan_i, ragged_len, ragged_plan, deep=False):
    return [(B, plan_u, plan_i, deep), (B, plan_u, plan_i, deep), (ragged_len, ragged_plan, ragged_plan, False)]


TYPES = [(d, half) for d in (32, 64, 128) for half in (False, True)]
# every class boundary, both table types, both losses; the ragged third batch is shorter than 4096 inside a hot-capable epoch
# (the first full batch plants the whole plan for users beside the items up to 130, the second the whole plan for items beside the
# users up to 130: see "Coherent sums" in the module's text)
CLASSES_CASES = [Spec("classes", d, half, bce, 8192, [(8192, CLASSES, SHORT, False), (8192, SHORT, CLASSES, False), (3001, RAGGED, RAGGED, False)])
                 for d, half in TYPES for bce in (True, False)]
# nothing longer than 128 on batches >= 4096: the prepared form runs the light-tailed kernel, the inline form the hot-capable one
CAPPED_CASES = [Spec("capped", d, half, (d == 64) != half, 8192, _epoch(8192, CAPPED, CAPPED, 4100, RAGGED_CAPPED)) for d, half in TYPES]
# B = 2048: hot_cap = 0, the wavefront loop takes runs however long they are.  (A batch of 2048 has 2048 user occurrences, fewer than
# 129 + 700 + 1500: the user of 1500 is in the first full batch, the three item runs in the second, 700 for both in the ragged one.)
NO_HOT_CASES = [Spec("no_hot_path", d, half, d == 64, 2048,
                     [(2048, (129, 1500), (129,), False), (2048, (129,), NO_HOT, False), (1501, (129, 700), (129, 700), False)])
                for d, half in ((32, True), (64, False), (128, True))]
# 260 hot runs in one batch: per = (nh + 255) / 256 = 2 in the chunk prefix, and the binary search over pre[] has 261 entries
MANY_HOT_CASES = [Spec("many_hot", 32, False, bce, 16384, _epoch(16384, MANY_HOT_U, MANY_HOT_I, 5000, RAGGED)) for bce in (True, False)]
# One item is the positive of every triple and the negative of DEEP_NEG more: 8392 occurrences = 17 chunks.  k_hot_apply's lane
# groups take 8 * G chunk partials a trip; G = 64 / (D / VEC) is 2 at d = 128 fp32 (8 at d = 32 fp32, 16 at d = 32 fp16), so 17
# chunks reach the SECOND trip of that loop at d = 128 fp32 -- the only geometry that can at this batch size (3 * B / 512 = 48
# chunks at most).  d = 32 fp16 for contrast: one trip, 16 lane groups.
DEEP_HOT_CASES = [Spec("deep_hot", d, half, False, 8192, _epoch(8192, (), (), 3001, RAGGED, deep=True)) for d, half in ((128, False), (32, True))]
SGD_CASES = CLASSES_CASES + CAPPED_CASES + NO_HOT_CASES + MANY_HOT_CASES + DEEP_HOT_CASES
# the Adam half: one batch from a fresh optimiser state, LONG = 8 (slots 4 .. 7 of the short-run path come from the value list)
# (one batch of 2048 cannot hold the runs of 300 and 1500 of both tables apart -- "Coherent sums" above -- so a case plants the whole
# plan in one table and the lengths up to 65 in the other: adam_u, adam_i)
ADAM_SHORT = tuple(L for L in ADAM if L <= 65)
ADAM_CASES = [Spec("adam_" + t, d, False, bce, 2048, [(2048, ADAM if t == "u" else ADAM_SHORT, ADAM if t == "i" else ADAM_SHORT, False)], adam=True)
              for d in (32, 64, 128) for t in "ui" for bce in (True, False)]
ALL_CASES = SGD_CASES + ADAM_CASES
BY_ID = {s.id: s for s in ALL_CASES}


# ------------------------------------------------------------------------------------------------------------------ triples
def filler_lengths(n_occ):
    """Run lengths of the filler rows over n_occ occurrences: threes (half of the occurrences), twos and ones (a quarter each)."""
    assert n_occ >= 0, n_occ
    n3, n2 = n_occ // 6, n_occ // 8
    return np.array([3] * n3 + [2] * n2 + [1] * (n_occ - 3 * n3 - 2 * n2), dtype=np.int64)


def _planted_ids(n_planted, r0, n_rows):
    """Planted rows fill the range [r0, r0 + n_rows) from both ends inwards: first, last, second, last but one, ..."""
    return np.array([r0 + k // 2 if k % 2 == 0 else r0 + n_rows - 1 - k // 2 for k in range(n_planted)], dtype=np.int64)


def _place(rng, plan, n_occ, r0):
    """(planted ids, filler ids, filler lengths, rows of the range) for one table of one batch."""
    fl = filler_lengths(n_occ - int(sum(plan)))
    n_rows = len(plan) + len(fl) + SLACK
    ids = _planted_ids(len(plan), r0, n_rows)
    front, back = (len(plan) + 1) // 2, len(plan) // 2
    middle = np.arange(r0 + front, r0 + n_rows - back)
    return ids, rng.permutation(middle)[:len(fl)], fl, n_rows


class Batch(object):
    """One batch's triples and what was planted in them."""

    def __init__(self, rng, index, size, plan_u, plan_i, deep, u0, i0):
        self.index, self.size, self.u0, self.i0 = index, size, u0, i0
        if deep:
            plan_i = (size + DEEP_NEG,)
        self.plan_u, self.plan_i = tuple(plan_u), tuple(plan_i)
        # users
        pu, fu, flu, self.n_user_rows = _place(rng, plan_u, size, u0)
        u = rng.permutation(np.concatenate([np.repeat(pu, plan_u).astype(np.int64), np.repeat(fu, flu)]))
        # items: a positive column and a negative column
        pi, fi, fli, self.n_item_rows = _place(rng, plan_i, 2 * size, i0)
        kinds = ["deep"] if deep else [("pos", "neg", "mixed")[(k + index) % 3] for k in range(len(plan_i))]
        n_pos = [L - DEEP_NEG if kd == "deep" else L if kd == "pos" else 0 if kd == "neg" else (L + 1) // 2 for L, kd in zip(plan_i, kinds)]
        pos_planted = np.repeat(pi, n_pos).astype(np.int64)
        neg_planted = np.repeat(pi, [L - p for L, p in zip(plan_i, n_pos)]).astype(np.int64)
        fill = rng.permutation(np.repeat(fi, fli))
        k = size - len(pos_planted)
        assert 0 <= k <= len(fill) and len(fill) - k == size - len(neg_planted)
        i = rng.permutation(np.concatenate([pos_planted, fill[:k]]))
        j = rng.permutation(np.concatenate([neg_planted, fill[k:]]))
        self.kinds = dict(zip(pi.tolist(), kinds))
        # the i == j triples: every one of the deep item's negatives; else ONE triple of the first mixed item with both kinds
        locked = np.zeros(size, dtype=bool)
        self.eq_item, self.eq_count = None, 0
        if deep:
            self.eq_item, self.eq_count = int(pi[0]), DEEP_NEG
            locked = j == pi[0]
        else:
            mixed = [int(r) for r, L, kd in zip(pi, plan_i, kinds) if kd == "mixed" and L >= 2]
            if mixed:
                e = self.eq_item = mixed[0]
                self.eq_count = 1
                t, s = int(np.flatnonzero(i == e)[0]), int(np.flatnonzero(j == e)[0])
                j[s], j[t] = j[t], j[s]
                locked[t] = True
        # no other triple has i == j: swap such a negative with one of another triple
        for t in np.flatnonzero((i == j) & ~locked):
            ok = np.flatnonzero(~locked & (j != i[t]) & (i != j[t]))
            s = int(ok[rng.randint(len(ok))])
            j[s], j[t] = j[t], j[s]
        # a long user never meets a long item: such a triple's user changes places with the user of a triple that has neither
        long_u = np.isin(u, pu[np.array(plan_u, dtype=np.int64) > DECORRELATE]) if len(plan_u) else np.zeros(size, dtype=bool)
        long_rows = pi[np.array(plan_i, dtype=np.int64) > DECORRELATE] if len(plan_i) and not deep else pi[:0]
        long_i = np.isin(i, long_rows) | np.isin(j, long_rows)
        free = rng.permutation(np.flatnonzero(~long_u & ~long_i & ~locked))
        clash = np.flatnonzero(long_u & long_i)
        if len(clash) <= len(free):
            s = free[:len(clash)]
            u[clash], u[s] = u[s], u[clash]
        self.decorrelated = len(clash) <= len(free)
        # the users of i == j triples are filler rows
        is_planted_u = np.isin(u, pu)
        for t in np.flatnonzero(locked & is_planted_u):
            ok = np.flatnonzero(~locked & ~is_planted_u)
            s = int(ok[rng.randint(len(ok))])
            u[s], u[t] = u[t], u[s]
            is_planted_u[s], is_planted_u[t] = True, False
        assert int(((i == j) & ~locked).sum()) == 0 and int((i == j).sum()) == self.eq_count
        self.tri = np.stack([u, i, j], 1)
        self.planted_u, self.planted_i = pu, pi
        self.filler_u, self.filler_i = collections.Counter(flu.tolist()), collections.Counter(fli.tolist())

    def expected_census(self):
        return (collections.Counter(self.plan_u) + self.filler_u, collections.Counter(self.plan_i) + self.filler_i)


def census(tri):
    """The multisets of run lengths of one batch: per user, and per item over both item columns."""
    cu = np.unique(tri[:, 0], return_counts=True)[1]
    ci = np.unique(tri[:, 1:].reshape(-1), return_counts=True)[1]
    return collections.Counter(cu.tolist()), collections.Counter(ci.tolist())


# ------------------------------------------------------------------------------------------------------------------ reference
def half_ulp(x, half):
    """Half a unit in the last place of |x| in float16 / float32 (subnormal spacing below the smallest normal)."""
    p, emin = (11, -14) if half else (24, -126)
    ax = np.abs(np.asarray(x, dtype=np.float64))
    e = np.maximum(np.where(ax > 0, np.frexp(ax)[1] - 1, emin), emin)
    return np.ldexp(1.0, e - p + 1) * 0.5


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def bare_grads_f64(wu, wi, tri, lam_u, lam_i, bce):
    """(loss, gx, gy, gz): the loss of oracle.sml_oracle.bare_step in float64 and every occurrence's gradient row -- gx[t] to the
    user of triple t, gy[t] to its positive, gz[t] to its negative, each with its own L2 term."""
    u, i, j = tri[:, 0], tri[:, 1], tri[:, 2]
    ue, ie, ne = wu[u], wi[i], wi[j]
    sp, sn = (ue * ie).sum(1), (ue * ne).sum(1)
    if bce:
        n = float(len(u))
        gp, gn = _sigmoid(sp), _sigmoid(sn)
        ap, an = gp + 1e-15, (1.0 - gn) + 1e-15
        pair = -np.mean(np.log(ap)) - np.mean(np.log(an))
        dsp, dsn = -(gp * (1.0 - gp) / ap) / n, (gn * (1.0 - gn) / an) / n
    else:
        x = sp - sn
        pair = np.sum(np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x))))
        dsp = -_sigmoid(-x)
        dsn = -dsp
    loss = pair + 0.5 * lam_u * np.sum(ue ** 2) + 0.5 * lam_i * (np.sum(ie ** 2) + np.sum(ne ** 2))
    gx = dsp[:, None] * ie + dsn[:, None] * ne + lam_u * ue
    gy = dsp[:, None] * ue + lam_i * ie
    gz = dsn[:, None] * ue + lam_i * ne
    return float(loss), gx, gy, gz


def _scatter(rows, idx, src):
    out = torch.zeros(rows, src.shape[1], dtype=torch.float64)
    out.index_add_(0, torch.from_numpy(np.ascontiguousarray(idx)), torch.from_numpy(np.ascontiguousarray(src)))
    return out.numpy()


def summed_grads_f64(wu, wi, tri, lam_u, lam_i, bce, weights=None):
    """(loss, G_user, G_item, A_user, A_item): the rows' summed gradients and the sums of their absolute contributions.
    weights = (wx, wy, wz): a multiplier per occurrence (the planted faults of the host module: 0 drops it, 2 counts it twice)."""
    loss, gx, gy, gz = bare_grads_f64(wu, wi, tri, lam_u, lam_i, bce)
    if weights is not None:
        gx, gy, gz = gx * weights[0][:, None], gy * weights[1][:, None], gz * weights[2][:, None]
    ij, gyz = np.concatenate([tri[:, 1], tri[:, 2]]), np.concatenate([gy, gz])
    return (loss, _scatter(wu.shape[0], tri[:, 0], gx), _scatter(wi.shape[0], ij, gyz),
            _scatter(wu.shape[0], tri[:, 0], np.abs(gx)), _scatter(wi.shape[0], ij, np.abs(gyz)))


def bare_step_f64(wu, wi, tri_b, lr, lam_u, lam_i, bce, weights=None):
    """One synchronous minibatch SGD step in float64 on float64 copies of the tables as stored.  Returns (new user table, new item
    table, loss, scale_user, scale_item): scale(r) = lr * max_k sum_t |g_t[k]| for every row the batch touches, 0 elsewhere."""
    wu, wi = np.asarray(wu, dtype=np.float64), np.asarray(wi, dtype=np.float64)
    loss, Gu, Gi, Au, Ai = summed_grads_f64(wu, wi, tri_b, lam_u, lam_i, bce, weights)
    return wu - lr * Gu, wi - lr * Gi, loss, lr * Au.max(1), lr * Ai.max(1)


@contextlib.contextmanager
def one_thread():
    """The float32 oracle on ONE thread.  On several, torch's CPU backward of an indexed read adds a row's occurrences in whatever
    order its threads arrive: e_ref then differs from run to run (seen: 1.75e-7 and 4.11e-7 for one case on one machine), and a
    bound that is a multiple of it would flicker.  One thread adds them in sequence, the same on every run."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def oracle_grad32(wu, wi, tri, lam_u, lam_i, bce):
    """The float32 oracle's gradient of the same loss (autograd over O.pair_loss, as O.bare_step and OracleEngine.bare_adam_epoch)."""
    Wu, Wi = wu.clone().requires_grad_(True), wi.clone().requires_grad_(True)
    t = torch.from_numpy(tri)
    ue, ie, ne = Wu[t[:, 0]], Wi[t[:, 1]], Wi[t[:, 2]]
    loss = O.pair_loss((ue * ie).sum(-1), (ue * ne).sum(-1), bce)
    loss = loss + lam_u * 0.5 * torch.sum(ue ** 2) + lam_i * 0.5 * (torch.sum(ie ** 2) + torch.sum(ne ** 2))
    loss.backward()
    return Wu.grad.detach(), Wi.grad.detach()


def row_e(got, ref, store, scale, rows):
    """e(r) over `rows`; a non-finite value makes its row's figure inf."""
    got = np.asarray(got, dtype=np.float64)[rows]
    with np.errstate(invalid="ignore"):
        e = np.maximum(0.0, np.abs(got - ref[rows]).max(1) - store[rows]) / scale[rows]
    e[~np.isfinite(got).all(1)] = np.inf
    return e


def untouched_identical(after, before, touched):
    """numpy twin of test_hip_parity._untouched_identical (bit patterns: the arrays hold what the table's type stores)."""
    mask = np.ones(after.shape[0], dtype=bool)
    mask[touched] = False
    return bool(np.array_equal(after[mask], before[mask]))


class Case(object):
    """A case's triples, tables, float64 reference and float32 yardstick.  Built once, shared, never written to."""

    def __init__(self, spec):
        self.spec = s = spec
        rng = np.random.RandomState(zlib_seed(s.id))
        self.batches, u0, i0 = [], 0, 0
        for b, (size, plan_u, plan_i, deep) in enumerate(s.batches):
            bt = Batch(rng, b, size, plan_u, plan_i, deep, u0, i0)
            self.batches.append(bt)
            u0, i0 = u0 + bt.n_user_rows, i0 + bt.n_item_rows
        self.U, self.I = u0, i0
        self.tri = np.ascontiguousarray(np.concatenate([bt.tri for bt in self.batches]))
        assert all(bt.size == s.B for bt in self.batches[:-1]) and self.batches[-1].size <= s.B
        dt = torch.float16 if s.half else torch.float32
        self.wu = torch.from_numpy((rng.standard_normal((self.U, s.d)) * s.scale).astype(np.float32)).to(dt)
        self.wi = torch.from_numpy((rng.standard_normal((self.I, s.d)) * s.scale).astype(np.float32)).to(dt)
        w0u, w0i = self.wu.double().numpy(), self.wi.double().numpy()
        self.touched_u = np.unique(self.tri[:, 0])
        self.touched_i = np.unique(self.tri[:, 1:])
        # the float64 reference: every batch from the initial tables (its rows are nobody else's)
        unit = 1.0 if s.adam else s.lr
        ref_u, ref_i = (np.zeros_like(w0u), np.zeros_like(w0i)) if s.adam else (w0u.copy(), w0i.copy())
        self.scale_u, self.scale_i, self.loss64 = np.zeros(self.U), np.zeros(self.I), []
        for bt in self.batches:
            loss, Gu, Gi, Au, Ai = summed_grads_f64(w0u, w0i, bt.tri, s.lam_u, s.lam_i, s.bce)
            ru, ri = np.unique(bt.tri[:, 0]), np.unique(bt.tri[:, 1:])
            ref_u[ru] = Gu[ru] if s.adam else w0u[ru] - s.lr * Gu[ru]
            ref_i[ri] = Gi[ri] if s.adam else w0i[ri] - s.lr * Gi[ri]
            self.scale_u[ru], self.scale_i[ri] = unit * Au[ru].max(1), unit * Ai[ri].max(1)
            self.loss64.append(loss)
        self.ref_u, self.ref_i, self.loss64 = ref_u, ref_i, np.array(self.loss64)
        # storage rounding of what the engine writes, and the float32 oracle's figure under its own
        if s.adam:
            self.store_u, self.store_i = (half_ulp(C1 * r, False).max(1) / C1 for r in (ref_u, ref_i))
            with one_thread():
                g32u, g32i = oracle_grad32(self.wu, self.wi, self.tri, s.lam_u, s.lam_i, s.bce)
            self.f32_u, self.f32_i = g32u.double().numpy(), g32i.double().numpy()
            yard_u, yard_i = half_ulp(ref_u, False).max(1), half_ulp(ref_i, False).max(1)
        else:
            self.store_u, self.store_i = half_ulp(ref_u, s.half).max(1), half_ulp(ref_i, s.half).max(1)
            ou, oi = self.wu.float().clone(), self.wi.float().clone()
            with one_thread():
                for bt in self.batches:
                    t = torch.from_numpy(bt.tri)
                    O.bare_step(ou, oi, t[:, 0], t[:, 1], t[:, 2], s.lr, s.lam_u, s.lam_i, bce=s.bce)
            self.f32_u, self.f32_i = ou.to(dt).double().numpy(), oi.to(dt).double().numpy()
            yard_u, yard_i = self.store_u, self.store_i
        self.e_ref = float(max(row_e(self.f32_u, ref_u, yard_u, self.scale_u, self.touched_u).max(),
                               row_e(self.f32_i, ref_i, yard_i, self.scale_i, self.touched_i).max()))
        for a in (self.tri, ref_u, ref_i, self.scale_u, self.scale_i, self.store_u, self.store_i, self.f32_u, self.f32_i, self.loss64):
            a.setflags(write=False)

    # -- the criterion
    def figures(self, got_u, got_i):
        """e(r) of the touched rows of both tables: {"user": (rows, e), "item": (rows, e)}."""
        return {"user": (self.touched_u, row_e(got_u, self.ref_u, self.store_u, self.scale_u, self.touched_u)),
                "item": (self.touched_i, row_e(got_i, self.ref_i, self.store_i, self.scale_i, self.touched_i))}

    def bound(self):
        return M[self.spec.family] * self.e_ref

    def failing_rows(self, got_u, got_i):
        """{"user": rows, "item": rows} whose e(r) exceeds M x e_ref."""
        return {k: rows[~(e <= self.bound())] for k, (rows, e) in self.figures(got_u, got_i).items()}

    def worst(self, got_u, got_i):
        """(worst e(r), table, row)."""
        best = (-1.0, None, -1)
        for k, (rows, e) in self.figures(got_u, got_i).items():
            at = int(np.argmax(e))
            if e[at] > best[0]:
                best = (float(e[at]), k, int(rows[at]))
        return best

    # -- planted occurrences
    def occurrences(self, bt):
        """For batch bt: {"user": {row: [slot]}, "item": {row: [slot]}} of its planted rows, slots in the order the run lists hold
        them (ascending; a user's slot is its triple t, a positive's t, a negative's size + t)."""
        out = {"user": {}, "item": {}}
        for r in bt.planted_u.tolist():
            out["user"][r] = np.flatnonzero(bt.tri[:, 0] == r)
        ij = np.concatenate([bt.tri[:, 1], bt.tri[:, 2]])
        for r in bt.planted_i.tolist():
            out["item"][r] = np.flatnonzero(ij == r)
        return out

    def contributions(self, bt):
        """unit * max_k |g_t[k]| of every occurrence of batch bt: (users [size], items [2 * size], by slot)."""
        s = self.spec
        _, gx, gy, gz = bare_grads_f64(self.wu.double().numpy(), self.wi.double().numpy(), bt.tri, s.lam_u, s.lam_i, s.bce)
        unit = 1.0 if s.adam else s.lr
        return unit * np.abs(gx).max(1), unit * np.concatenate([np.abs(gy).max(1), np.abs(gz).max(1)])

    def need(self, table, row):
        """What ONE occurrence must move `row` by for the criterion to see its loss: 4 * (store(r) + M * e_ref * scale(r))."""
        store, scale = (self.store_u, self.scale_u) if table == "user" else (self.store_i, self.scale_i)
        return 4.0 * (store[row] + self.bound() * scale[row])

    # -- a simulated engine: the float64 step with occurrence weights, stored in the table's type
    def simulate(self, weights_of=None):
        """weights_of(bt) -> (wx, wy, wz) or None.  Returns (user table, item table) as float64 arrays of what the type stores (Adam:
        the float32 moment m = C1 * g scaled back by 1 / C1)."""
        s = self.spec
        w0u, w0i = self.wu.double().numpy(), self.wi.double().numpy()
        out_u, out_i = (np.zeros_like(w0u), np.zeros_like(w0i)) if s.adam else (w0u.copy(), w0i.copy())
        for bt in self.batches:
            w = weights_of(bt) if weights_of is not None else None
            _, Gu, Gi, _, _ = summed_grads_f64(w0u, w0i, bt.tri, s.lam_u, s.lam_i, s.bce, w)
            ru, ri = np.unique(bt.tri[:, 0]), np.unique(bt.tri[:, 1:])
            out_u[ru] = Gu[ru] if s.adam else w0u[ru] - s.lr * Gu[ru]
            out_i[ri] = Gi[ri] if s.adam else w0i[ri] - s.lr * Gi[ri]
        if s.adam:
            return ((C1 * out_u).astype(np.float32).astype(np.float64) / C1, (C1 * out_i).astype(np.float32).astype(np.float64) / C1)
        st = np.float16 if s.half else np.float32
        return out_u.astype(st).astype(np.float64), out_i.astype(st).astype(np.float64)


def zlib_seed(text):
    import zlib
    return zlib.crc32(text.encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=2)
def case(case_id):
    return Case(BY_ID[case_id])


def recorded_ratios():
    with open(RATIOS_FILE) as f:
        return json.load(f)
