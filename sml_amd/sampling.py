"""Training negatives of the device batch supply: which sampler an epoch uses ("training negatives", include/sml_hip.h).

`NegativeSampler(pool=1, alpha=0.0)` names one: candidates drawn with p(i) proportional to count(i) ** alpha over the
set's items (alpha = 0: uniform, today's draws), and of the first `pool` admissible candidates the one the current model
scores highest (pool = 1: the first, today's negative).  The default sampler is the uniform one, byte for byte.

The popularity cdf is numpy on the host: the host defines its bytes, and at most one entry per item is uploaded.
"""
import numpy as np


class DeviceCdf(object):
    """A validated cdf on a device: `tensor` float64 [pop]."""

    def __init__(self, tensor):
        self.tensor = tensor


def check_cdf(cdf, pop=None):
    """The cdf as a contiguous float64 numpy array, or ValueError: float64, one dimension (of length pop when given), no
    NaN, nondecreasing, first entry >= 0, last entry exactly 1.0."""
    a = np.asarray(cdf)
    if a.dtype != np.float64 or a.ndim != 1 or a.shape[0] == 0:
        raise ValueError("cdf: a float64 vector with one entry per item of item_all, got %s %s" % (a.dtype, a.shape))
    if pop is not None and a.shape[0] != int(pop):
        raise ValueError("cdf: %d entries for %d items" % (a.shape[0], int(pop)))
    if np.isnan(a).any() or a[0] < 0.0 or (np.diff(a) < 0.0).any():
        raise ValueError("cdf: must be nondecreasing from >= 0, without NaN")
    if a[-1] != 1.0:
        raise ValueError("cdf: the last entry must be exactly 1.0, got %r" % float(a[-1]))
    return np.ascontiguousarray(a)


def device_cdf(cdf, device, pop=None):
    """check_cdf, then the upload: a DeviceCdf for HipEngine.sample_negatives_ex (which then skips the validation)."""
    import torch
    return DeviceCdf(torch.from_numpy(check_cdf(cdf, pop)).to(device))


def popularity_cdf(item_all, items, alpha):
    """float64 [len(item_all)]: the cdf of p(i) proportional to count(i) ** alpha, count(i) = how often id item_all[i]
    occurs among `items`: cumsum of the weights, divided by its last entry, the last entry then set to 1.0.  alpha == 0
    returns None -- no cdf, not a flat one, so the uniform draws stay the bytes they are."""
    if float(alpha) == 0.0:
        return None
    item_all, items = np.asarray(item_all), np.asarray(items)
    w = _counts(item_all.reshape(-1), items.reshape(-1)).astype(np.float64) ** float(alpha)
    cdf = np.cumsum(w)
    if not cdf[-1] > 0.0:
        raise ValueError("popularity_cdf: no item of item_all occurs among the items")
    cdf = cdf / cdf[-1]
    cdf[-1] = 1.0
    return cdf


def _counts(item_all, items):
    order = np.argsort(item_all, kind="stable")
    sorted_all = item_all[order]
    pos = np.searchsorted(sorted_all, items)
    pos[pos == sorted_all.shape[0]] = 0
    hit = sorted_all[pos] == items
    counts = np.zeros(item_all.shape[0], dtype=np.int64)
    np.add.at(counts, order[pos[hit]], 1)
    return counts


class NegativeSampler(object):
    """pool: 1..64 candidates to choose the highest-scoring one from; alpha >= 0: the popularity exponent."""

    def __init__(self, pool=1, alpha=0.0):
        pool, alpha = int(pool), float(alpha)
        if pool < 1 or pool > 64:
            raise ValueError("NegativeSampler: pool must be in 1..64, got %d" % pool)
        if not alpha >= 0.0 or alpha == float("inf"):
            raise ValueError("NegativeSampler: alpha must be a finite number >= 0, got %r" % alpha)
        self.pool, self.alpha = pool, alpha

    @property
    def is_default(self):
        return self.pool == 1 and self.alpha == 0.0

    def cdf(self, item_all, items):
        return popularity_cdf(item_all, items, self.alpha)

    def tables(self, model):
        """(w_user, w_item) of an MFbasemode for pool > 1, else (None, None)."""
        if self.pool == 1:
            return None, None
        if model is None:
            raise ValueError("NegativeSampler(pool=%d) scores its candidates: pass the model (an MFbasemode)" % self.pool)
        return model.user_laten.weight.data, model.item_laten.weight.data

    def __repr__(self):
        return "NegativeSampler(pool=%d, alpha=%g)" % (self.pool, self.alpha)
