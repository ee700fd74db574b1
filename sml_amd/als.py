"""Closed-form fold-in and the iALS baseline on the HIP engine (include/sml_hip.h, FOLD-IN).

A user (or item) the last training run did not see gets the row that solves its regularised least-squares problem against the
other side's fixed table, from its interaction set:

    p_u = (alpha0 Y^T Y + sum_{i in S(u)} y_i y_i^T + reg I)^-1 sum_{i in S(u)} y_i

fold_in does that for any rows of a table (HipEngine.gram + HipEngine.als_solve: one wavefront builds and factors one d x d
system); transpose_sets gives the item -> users sets so that the same call folds in items; fit alternates the two half-steps,
which is the iALS baseline, and objective is the loss both half-steps minimise.  d = 32 / 64, fp32 or fp16 tables.

The defaults reg = 0.1 and alpha0 = 0.1 are conventions of the iALS literature, not values tuned for this project's data."""
import collections

import torch

FoldIn = collections.namedtuple("FoldIn", "solved empty failed status")
FoldIn.__doc__ = """What a fold-in did: the number of rows solved and written, of rows with an empty set (written as zero), of rows
that could not be solved (left untouched), and the device int32 status per row (0 / 1 / 2 in that order)."""

WIDTHS = (32, 64)


def _engine(engine, tab):
    if engine is not None:
        return engine
    from .engine import get_engine
    if tab.shape[-1] not in WIDTHS:
        raise ValueError("fold-in exists at d = 32 / 64 only (d = 128 is out of scope), got d = %d" % tab.shape[-1])
    return get_engine(tab.device, tab.shape[-1])


def fold_in(out_tab, other_tab, sets, rows=None, reg=0.1, alpha0=0.1, gram=None, engine=None, strict=True):
    """Solve the rows `rows` (int ids; None: every row) of out_tab IN PLACE against other_tab held fixed, from their ranges of
    sets = (off, items) (anything sml_amd.retrieval.as_csr takes).  gram: HipEngine.gram(other_tab) when the caller has it
    already (it is computed here otherwise, unless alpha0 == 0).  Returns a FoldIn; one read-back (the three counts).
    strict: raise ValueError when any row could not be solved -- such rows keep their old bytes.  reg and alpha0 default to
    conventions, not tuned values."""
    from .retrieval import as_csr
    eng = _engine(engine, out_tab)
    if gram is None and float(alpha0) != 0.0:
        gram = eng.gram(other_tab)
    status = eng.als_solve(other_tab, gram, as_csr(sets, out_tab.device), out_tab, rows, reg=reg, alpha0=alpha0)
    solved, empty, failed = torch.bincount(status.long(), minlength=3).tolist()[:3] if status.numel() else (0, 0, 0)
    if strict and failed:
        raise ValueError("fold_in: %d of %d rows could not be solved (a pivot was not positive or the solution is not finite); "
                         "they are left untouched" % (failed, status.numel()))
    return FoldIn(solved, empty, failed, status)


def transpose_sets(sets, n_user, n_item, engine):
    """The item -> users CSR (off int64 [n_item + 1], users int32) of sets = the user -> items CSR over n_user users: the pairs
    are expanded on the device, their columns swapped and the set rebuilt (HipEngine.iset_build); no new kernel."""
    from .retrieval import as_csr
    off, items = as_csr(sets, engine.device)
    off = engine._dev(off, torch.int64)[:int(n_user) + 1]
    users = torch.repeat_interleave(torch.arange(int(n_user), device=engine.device), off[1:] - off[:-1])
    items = engine._dev(items, torch.int64)[:users.shape[0]]
    return engine.iset_build(torch.stack([items, users], 1), int(n_item), int(n_user))


def objective(user_tab, item_tab, sets, reg, alpha0):
    """sum_u [sum_{i in S(u)} (1 - p_u.q_i)^2 + alpha0 sum_{all i} (p_u.q_i)^2] + reg (|P|^2 + |Q|^2) as a Python float, in
    float64 torch on the tables' device.  The all-pairs term goes through the Gram identity sum_{u,i} (p_u.q_i)^2 =
    <P^T P, Q^T Q>, so nothing of size n_user x n_item is formed."""
    p, q = user_tab.detach().double(), item_tab.detach().double()
    off, items = (torch.as_tensor(t).to(p.device) for t in sets)
    off = off.long()[:p.shape[0] + 1]
    users = torch.repeat_interleave(torch.arange(p.shape[0], device=p.device), off[1:] - off[:-1])
    s = (p[users] * q[items.long()[:users.shape[0]]]).sum(1)
    seen = ((1.0 - s) ** 2).sum()
    every = ((p.t() @ p) * (q.t() @ q)).sum()
    return float(seen + float(alpha0) * every + float(reg) * ((p * p).sum() + (q * q).sum()))


def fit(model, sets, sweeps=4, reg=0.1, alpha0=0.1, engine=None):
    """iALS on a model's tables (an MFbasemode on the device; d = 32 / 64): `sweeps` times a user half-step then an item
    half-step, every row solved from sets (user -> items, anything as_csr takes).  Returns the objective after every half-step
    (2 * sweeps floats); each half-step minimises it over its own side exactly, so the sequence does not rise beyond the
    rounding of the table's element type.  reg and alpha0 default to conventions, not tuned values."""
    from .retrieval import as_csr
    wu, wi = model.user_laten.weight.data, model.item_laten.weight.data
    eng = _engine(engine, wu)
    by_user = as_csr(sets, wu.device)
    by_item = transpose_sets(by_user, wu.shape[0], wi.shape[0], eng)
    out = []
    with torch.no_grad():
        for _ in range(int(sweeps)):
            fold_in(wu, wi, by_user, reg=reg, alpha0=alpha0, engine=eng)
            out.append(objective(wu, wi, by_user, reg, alpha0))
            fold_in(wi, wu, by_item, reg=reg, alpha0=alpha0, engine=eng)
            out.append(objective(wu, wi, by_user, reg, alpha0))
    return out
