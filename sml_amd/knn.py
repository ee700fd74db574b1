"""The neighbourhood model (ItemKNN) on the HIP engine (include/sml_hip.h, NEIGHBOURS).

ItemNeighbours.build counts, for every item, how often each other item was taken by the same users, turns the counts into
similarities (cosine, asymmetric cosine or the bare count; with users that do not count equally: the random-walk similarities
P3alpha and RP3beta, or any of the three under a per-user weight) and keeps the k best: "people who took X also took Y", exact the
moment an item's first interactions exist, with no training run and no embedding table.  ItemNeighbours.recommend scores a
history -- a session, a basket, a user who arrived after the last period -- by adding the similarities of its members'
neighbours; the history needs no row anywhere, and the model works at any embedding width because it reads no table.

Both halves are one device operation each (HipEngine.cooc_topk or cooc_topk_weighted, HipEngine.knn_topk): integer atomics only, so the lists are the
same bytes for every launch geometry.  engine="host" routes both through the single-threaded host walks of the library
(sml_host_cooc_topk / sml_host_knn_topk) on CPU tensors: the same definitions, no GPU."""
import ctypes
import math

import numpy as np
import torch

METRICS = ("cosine", "asymmetric", "count")
WALK_METRICS = ("rp3beta", "p3alpha")                  # the random-walk similarities: weighted by construction


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class HostWalks(object):
    """cooc_topk / cooc_topk_weighted / knn_topk / transpose with HipEngine's signatures, through the library's host walks on CPU tensors."""
    device = torch.device("cpu")

    def __init__(self):
        from . import _lib
        self.lib = _lib.load()

    @staticmethod
    def _np(t, dtype):
        return None if t is None else np.ascontiguousarray(np.asarray(t.cpu() if torch.is_tensor(t) else t), dtype=dtype)

    def _csr(self, s):
        if s is None:
            return None, None
        off, items = self._np(s[0], np.int64), self._np(s[1], np.int32)
        return off, items if items.size else np.zeros(1, np.int32)

    def _allow(self, allow, n_item):
        if allow is None:
            return None
        from .retrieval import as_filter
        return self._np(as_filter(allow, n_item, "cpu"), np.int32)

    def knn_lds_limit(self):
        return int(self.lib.sml_knn_lds_limit())

    def transpose(self, sets, n_user, n_item):
        off, items = self._csr(sets)
        off = off[:int(n_user) + 1]
        items = items[:int(off[-1])]
        users = np.repeat(np.arange(int(n_user), dtype=np.int32), np.diff(off))
        order = np.argsort(items, kind="stable")
        t_off = np.zeros(int(n_item) + 1, np.int64)
        np.cumsum(np.bincount(items, minlength=int(n_item)), out=t_off[1:])
        return torch.from_numpy(t_off), torch.from_numpy(users[order])

    def cooc_topk(self, by_item, by_user, k, rows=None, norm=None, shrink=0.0, min_co=1, allow=None, max_workgroups=0, path=0):
        from ._lib import check
        i_off, i_users = self._csr(by_item)
        u_off, u_items = self._csr(by_user)
        n_item, n_user = len(i_off) - 1, len(u_off) - 1
        na, nb = (None, None) if norm is None else norm if isinstance(norm, (tuple, list)) else (norm, norm)
        na, nb = self._np(na, np.float64), self._np(nb, np.float64)
        rows = None if rows is None else self._np(rows, np.int64).reshape(-1)
        n, k = n_item if rows is None else len(rows), int(k)
        allow = self._allow(allow, n_item)
        items, sims, n_elig = np.empty((n, max(k, 0)), np.int32), np.empty((n, max(k, 0)), np.float32), np.empty(n, np.int32)
        check(self.lib.sml_host_cooc_topk(_p(i_off), _p(i_users), _p(u_off), _p(u_items), n_user, n_item, _p(rows), n, _p(na), _p(nb),
                                          float(shrink), int(min_co), _p(allow), k, _p(items), _p(sims), _p(n_elig)),
              "sml_host_cooc_topk")
        return torch.from_numpy(items).long(), torch.from_numpy(sims), torch.from_numpy(n_elig)

    def cooc_topk_weighted(self, by_item, by_user, k, user_w, frac_bits=30, rows=None, norm=None, shrink=0.0, allow=None,
                           max_workgroups=0, path=0):
        from ._lib import check
        i_off, i_users = self._csr(by_item)
        u_off, u_items = self._csr(by_user)
        n_item, n_user = len(i_off) - 1, len(u_off) - 1
        if not torch.is_tensor(user_w) or user_w.dtype != torch.float32 or user_w.device != self.device or not user_w.is_contiguous() \
                or tuple(user_w.shape) != (n_user,):
            raise ValueError("cooc_topk_weighted: user_w is a contiguous float32 [%d] tensor on %s" % (n_user, self.device))
        w = self._np(user_w, np.float32)
        na, nb = (None, None) if norm is None else norm if isinstance(norm, (tuple, list)) else (norm, norm)
        na, nb = self._np(na, np.float64), self._np(nb, np.float64)
        rows = None if rows is None else self._np(rows, np.int64).reshape(-1)
        n, k = n_item if rows is None else len(rows), int(k)
        allow = self._allow(allow, n_item)
        items, sims, n_elig = np.empty((n, max(k, 0)), np.int32), np.empty((n, max(k, 0)), np.float32), np.empty(n, np.int32)
        check(self.lib.sml_host_cooc_topk_weighted(_p(i_off), _p(i_users), _p(u_off), _p(u_items), n_user, n_item, _p(rows), n, _p(w),
                                                   int(frac_bits), _p(na), _p(nb), float(shrink), _p(allow), k, _p(items), _p(sims),
                                                   _p(n_elig)), "sml_host_cooc_topk_weighted")
        return torch.from_numpy(items).long(), torch.from_numpy(sims), torch.from_numpy(n_elig)

    def knn_topk(self, nbr_items, nbr_sims, n_item, history, k, users=None, frac_bits=30, seen=None, allow=None, max_workgroups=0,
                 path=0):
        from ._lib import check
        nbr_items, nbr_sims = self._np(nbr_items, np.int32), self._np(nbr_sims, np.float32)
        h_off, h_items = self._csr(history)
        s_off, s_items = self._csr(seen)
        users = None if users is None else self._np(users, np.int64).reshape(-1)
        n, k, n_item = len(h_off) - 1 if users is None else len(users), int(k), int(n_item)
        allow = self._allow(allow, n_item)
        items, scores, n_elig = np.empty((n, max(k, 0)), np.int32), np.empty((n, max(k, 0)), np.float32), np.empty(n, np.int32)
        check(self.lib.sml_host_knn_topk(_p(nbr_items), _p(nbr_sims), nbr_items.shape[0], nbr_items.shape[1], n_item, _p(h_off),
                                         _p(h_items), _p(users), n, int(frac_bits), _p(s_off), _p(s_items), _p(allow), k, _p(items),
                                         _p(scores), _p(n_elig)), "sml_host_knn_topk")
        return torch.from_numpy(items).long(), torch.from_numpy(scores), torch.from_numpy(n_elig)


def _csr(x, eng):
    """history / exclude -> a (off, items) pair the engine takes (None stays None)."""
    from .retrieval import DeviceSeen, SeenItems, as_csr
    if x is None:
        return None
    if isinstance(eng, HostWalks):
        return tuple(torch.as_tensor(t) for t in (x.host() if isinstance(x, (SeenItems, DeviceSeen)) else x))
    return as_csr(x, eng.device)


def frac_bits_for(max_abs):
    """The largest F in [0, 32] with max_abs * 2^F <= 2^32, so that no slot of a table whose largest |sim| is max_abs is dropped
    by the fixed point of sml_knn_topk (a table with sims above 2^32 gets F = 0 and loses those slots)."""
    if not (max_abs > 0.0) or math.isinf(max_abs):
        return 32
    m, e = math.frexp(max_abs)                                      # max_abs = m * 2^e, 0.5 <= m < 1
    return max(0, min(32, 32 - e + (1 if m == 0.5 else 0)))


def _top_finite(t):
    """The largest finite |value| of a tensor as a Python float (one read-back); 0.0 if it has none."""
    t = t[torch.isfinite(t)]
    return float(t.abs().max()) if t.numel() else 0.0


class ItemNeighbours(object):
    """Each item's k nearest items and their similarities: items int64 [n_item, k] (-1 pads), sims float32 [n_item, k] (-inf
    pads), n_nbr int32 [n_item] (the live slots of each row), the metric and the fixed point (frac_bits) recommend adds the
    sims in: 30 for cosine and asymmetric, whose sims lie in [0, 1]; 0 for count, whose sims are integers; for the weighted
    forms, frac_bits_for(the largest finite |sim|)."""

    def __init__(self, items, sims, n_nbr, metric, frac_bits, engine):
        self.items, self.sims, self.n_nbr = items, sims, n_nbr
        self.metric, self.frac_bits, self.engine = metric, int(frac_bits), engine
        self._narrow = items.to(torch.int32).contiguous()

    @property
    def n_item(self):
        return int(self.items.shape[0])

    @property
    def k(self):
        return int(self.items.shape[1])

    @classmethod
    def build(cls, history, n_user, n_item, k=64, metric="cosine", alpha=None, shrink=0.0, min_co=1, among=None, engine=None, beta=0.6,
              user_weight=None):
        """From a user -> items set: history is anything sml_amd.retrieval.as_csr takes (a SeenItems, a DeviceSeen, a (off, items)
        CSR) over n_user users and n_item items.  The transpose comes from als.transpose_sets and deg[i] is the number of users of
        item i.  metric: "cosine" -- count / (deg[i]^1/2 deg[j]^1/2 + shrink); "asymmetric" -- count / (deg[i]^alpha
        deg[j]^(1 - alpha) + shrink), alpha = 0.5 unless given; "count" -- the bare co-occurrence count.  The norm tables are made
        in float64 torch on the engine's device; the call itself holds no square root.  min_co: the smallest count that makes a
        neighbour; among: an ItemFilter on the neighbours; engine: a HipEngine (any width), "host" for the library's host walks,
        or None for the device's shared engine.

        The weighted forms (include/sml_hip.h, WEIGHTED NEIGHBOURS OF ITEMS; engine.cooc_topk_weighted), in which a common user u
        adds a weight w[u] where the forms above add 1:
        metric "rp3beta" -- sum of deg_u^-alpha over the common users / (deg[i]^alpha deg[j]^beta + shrink), the two-step random
        walk i -> u -> j with its popularity penalty; "p3alpha" -- rp3beta with beta = 0.  alpha = 1.0 (unless given) and
        beta = 0.6 are the literature's conventions, not values tuned here.  w = deg_u^-alpha is made in float64 torch and cast to
        float32; a user with no item gets 0.
        user_weight: a float [n_user] tensor for "cosine" / "asymmetric" / "count" -- inverse user frequency, Adamic-Adar, any
        per-user trust or recency weight; the norm tables stay the metric's.
        The weights are added in fixed point with frac_bits_for(largest finite weight) fractional bits, and the container's
        frac_bits for recommend is frac_bits_for(largest finite |sim|): one read-back each.  min_co other than 1 with a weighted
        form is a ValueError: a weighted sum has no count to compare it with."""
        if metric not in METRICS + WALK_METRICS:
            raise ValueError("metric is one of %s, got %r" % (", ".join(METRICS + WALK_METRICS), metric))
        walk = metric in WALK_METRICS
        if walk and user_weight is not None:
            raise ValueError("metric %r makes its own user weights; user_weight goes with %s" % (metric, ", ".join(METRICS)))
        weighted = walk or user_weight is not None
        if weighted and int(min_co) != 1:
            raise ValueError("min_co = %d with a weighted form: a weighted sum has no count to compare it with" % int(min_co))
        alpha = (1.0 if walk else 0.5) if alpha is None else float(alpha)
        if engine is None:
            from .engine import get_engine
            engine = get_engine(torch.device("cuda", torch.cuda.current_device()), 32)
        elif isinstance(engine, str) and engine == "host":
            engine = HostWalks()
        n_user, n_item = int(n_user), int(n_item)
        by_user = _csr(history, engine)
        if isinstance(engine, HostWalks):
            by_item = engine.transpose(by_user, n_user, n_item)
        else:
            from .als import transpose_sets
            by_user = tuple(engine._dev(t, dt) for t, dt in zip(by_user, (torch.int64, torch.int32)))
            by_item = transpose_sets(by_user, n_user, n_item, engine)
        by_user = (by_user[0][:n_user + 1], by_user[1])
        norm = None
        if metric != "count":
            deg = (by_item[0][1:] - by_item[0][:-1]).to(torch.float64)
            if walk:
                norm = (deg.pow(alpha).contiguous(), deg.pow(0.0 if metric == "p3alpha" else float(beta)).contiguous())
            else:
                norm = deg.sqrt() if metric == "cosine" else (deg.pow(alpha).contiguous(), deg.pow(1.0 - alpha).contiguous())
        if not weighted:
            items, sims, n_elig = engine.cooc_topk(by_item, by_user, k, norm=norm, shrink=shrink, min_co=min_co, allow=among)
            return cls(items, sims, n_elig.clamp(max=int(k)), metric, 0 if metric == "count" else 30, engine)
        if walk:
            deg_u = (by_user[0][1:] - by_user[0][:-1]).to(torch.float64)
            w = torch.where(deg_u > 0, deg_u.clamp(min=1.0).pow(-alpha), torch.zeros_like(deg_u)).to(torch.float32)
        else:
            w = torch.as_tensor(user_weight)
            if not w.is_floating_point() or tuple(w.shape) != (n_user,):
                raise ValueError("user_weight is a float [%d] tensor, got %s %s" % (n_user, w.dtype, tuple(w.shape)))
            w = w.to(device=engine.device, dtype=torch.float32)
        w = w.contiguous()
        items, sims, n_elig = engine.cooc_topk_weighted(by_item, by_user, k, w, frac_bits=frac_bits_for(_top_finite(w)), norm=norm,
                                                        shrink=shrink, allow=among)
        return cls(items, sims, n_elig.clamp(max=int(k)), metric, frac_bits_for(_top_finite(sims[items >= 0])), engine)

    @classmethod
    def from_model(cls, model, k, metric="cosine"):
        """The same container filled by MFbasemode.similar_items (embedding neighbours; no new kernel).  frac_bits is chosen from
        one read-back of max |sim| so that no slot exceeds the fixed point's range (frac_bits_for)."""
        from .mf import _engine_for
        w = model.item_laten.weight.data
        items, sims = model.similar_items(torch.arange(w.shape[0], device=w.device), int(k), metric=metric)
        live = items >= 0
        finite = sims[live & torch.isfinite(sims)]
        top = float(finite.abs().max()) if finite.numel() else 0.0
        return cls(items, sims, live.sum(1).to(torch.int32), "model:" + metric, frac_bits_for(top), _engine_for(model))

    def recommend(self, history, users=None, topK=20, exclude=None, items=None):
        """(items int64 [n, topK], scores float32 [n, topK]) as MFbasemode.recommend returns them: for each named row of
        `history` (a SeenItems, a DeviceSeen or a (off, items) CSR; users=None: every row) the topK items by the sum of the
        similarities its members' neighbour lists give them, score descending then id ascending, (-1, -inf) in missing slots.
        exclude: the items to leave out per user, as recommend takes it (a common call is exclude=history); items: an item
        filter.  History members are not excluded unless exclude says so."""
        eng = self.engine
        it, sc, _ = eng.knn_topk(self._narrow, self.sims, self.n_item, _csr(history, eng), int(topK), users=users,
                                 frac_bits=self.frac_bits, seen=_csr(exclude, eng), allow=items)
        return it, sc

    def similar_items(self, items, topK=20):
        """(int64 [n, topK], float32 [n, topK]): the stored rows' first topK slots."""
        if not 1 <= int(topK) <= self.k:
            raise ValueError("1 <= topK <= %d (the lists' length), got %d" % (self.k, int(topK)))
        q = torch.as_tensor(items).to(self.items.device).long().reshape(-1)
        return self.items[q, :int(topK)], self.sims[q, :int(topK)]
