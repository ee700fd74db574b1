"""MF base model: the module surface of the reference's model/MF.py on the HIP engine.

Same class names, constructor signature, attribute names (misspellings included:
user_bais, item_bais, user_laten, item_laten) and creation order as the reference
(model/MF.py:18-27) -- the order fixes state_dict keys and the RNG draw sequence of
the initialisers, and the class path `model.MF.MFbasemode` is the on-disk contract
of the --pre_model checkpoint (a whole pickled module, model/transfer.py:322-325).

forward / test run on libsml_hip.so (no autograd through them: SML trains the
tables through HipEngine.mf_stage_epoch, not through this module's graph).
"""
import torch
import torch.nn as nn

from .engine import get_engine


def _engine_for(module):
    w = module.user_laten.weight
    if w.device.type != "cuda":
        raise RuntimeError("%s runs on the HIP engine only: move it to a GPU (.cuda()); there is no CPU path"
                           % type(module).__name__)
    eng = getattr(module, "_sml_engine", None)
    return eng if eng is not None else get_engine(w.device, module.hidden_dim)


def _topk(eng, topK):
    """The engine call that makes lists of topK items, returning (items, scores): topk_items up to its 128, the deep lists
    (HipEngine.topk_deep, up to 1,024) beyond; anything else is topk_items' to refuse."""
    if 128 < topK <= 1024:
        return lambda *a, **kw: eng.topk_deep(*a, **kw)[:2]
    return eng.topk_items


class MFbasemode(nn.Module):
    def __init__(self, num_user=0, num_item=0, laten_factor=10):
        super(MFbasemode, self).__init__()
        # creation order matters (reference model/MF.py:21-24)
        self.user_bais = nn.Embedding(num_user, 1)
        self.item_bais = nn.Embedding(num_item, 1)
        self.user_laten = nn.Embedding(num_user, laten_factor)
        self.item_laten = nn.Embedding(num_item, laten_factor)
        self.user_num = num_user
        self.item_num = num_item
        self.hidden_dim = laten_factor

    def reset_parameters(self):
        # same order as the reference (model/MF.py:28-32)
        for emb in (self.user_bais, self.user_laten, self.item_bais, self.item_laten):
            emb.reset_parameters()

    def forward(self, user, item, norm=False):
        """(user rows, item rows, dot products [/ ||u|| if norm]).  model/MF.py:34-43."""
        eng = _engine_for(self)
        return eng.mf_forward(self.user_laten.weight.data, self.item_laten.weight.data, user, item, norm)

    def _ranks(self, inputs_data):
        eng = _engine_for(self)
        return eng, eng.eval_ranks(self.user_laten.weight.data, self.item_laten.weight.data, inputs_data)

    def test(self, inputs_data, topK=20):
        """inputs_data [n, 2+neg]: user, positive, negatives.  Returns (hits, ndcg_sum,
        indices of the rows that hit).  model/MF.py:45-80.  The positive's rank is the
        count of candidates scoring strictly above it, which is the position torch.topk
        gives it when scores are tie-free."""
        eng, ranks = self._ranks(inputs_data)
        hits, ndcg = eng.eval_metrics(ranks, topK)
        hit_rows = (ranks < topK).nonzero()[:, 0]
        batch_ndcg = torch.tensor(ndcg) if hits > 0 else 0
        return hits * 1.0, batch_ndcg, hit_rows

    def test2(self, inputs_data, topK=20):
        """model/MF.py:82-106: (hit rows, rank, hits, ndcg_sum); `rank` here is the
        positive's rank per row (the reference returns the top-k index matrix: test_lists
        returns those lists)."""
        eng, ranks = self._ranks(inputs_data)
        hits, ndcg = eng.eval_metrics(ranks, topK)
        hit_rows = (ranks < topK).nonzero()[:, 0]
        return hit_rows, ranks, hits * 1.0, (torch.tensor(ndcg) if hits > 0 else 0)

    def recommend(self, users, topK=20, exclude=None, items=None, score=None, candidates=None, diversify=None, pool=None,
                  metric="cosine", index=None, nprobe=None):
        """(items int64 [n, topK], scores float32 [n, topK]): each user's topK items over the whole catalogue by the score
        test() uses (no bias terms), score descending then item id ascending, leaving out `exclude` (a
        sml_amd.retrieval.SeenItems or a (seen_off, seen_items) CSR); missing slots are (-1, -inf).  1 <= topK <= 1024: above
        128 the lists come from HipEngine.topk_deep (the same definition, selected by radix); candidates= and diversify= keep
        their limit of 128.  items: restrict the
        lists to a subset of the catalogue (a sml_amd.retrieval.ItemFilter, a bool mask [item_num] or int32 filter words).
        score: rank by A(u, i) = fmaf(S(u, i), scale[i], offset[i]) instead (sml_amd.retrieval.as_score): "bias" adds
        item_bais, "cosine" divides by the item row's norm, an ItemScore gives any per-item terms; None / "dot" is the bare
        dot product.  The returned scores are A.  candidates: the same call restricted PER USER -- each user's own list of
        item ids (anything sml_amd.retrieval.as_candidates takes: a matrix [n, C] padded with -1, a (cand_off, cand_items)
        pair, a list of sequences, a CandidateRows); the lists hold the distinct eligible candidates only, and no catalogue
        walk is made (HipEngine.topk_candidates).  users may be None when candidates is a CandidateRows.
        diversify: None -- nothing changes -- or lam in [0, 1]: "the same list, but not topK of the same thing".  The call
        then takes each user's top `pool` items (default min(128, 5 * topK); exclude, items, score and candidates apply as
        above) and re-ranks them greedily by lam * r - (1 - lam) * max similarity to the items already picked (r: the score,
        min-max scaled per list; similarity by `metric`, "cosine" or "dot" of the item rows; HipEngine.rerank_mmr).  The
        returned scores are the model's scores of the picked items, gathered from the pool.  diversify=1 returns the plain
        list; sml_amd.evaluation.intra_list_similarity says how alike a list's items are.
        index: None -- the call as above, the same bytes -- or a sml_amd.retrieval.ItemIndex over this model's item table: each
        user then scores only the members of its nprobe nearest lists (default min(8, n_list); at most 128) instead of the
        catalogue (HipEngine.ivf_search).  What is returned is exact for the items that were scored; what may be missing is an
        item of a list that was not probed (sml_amd.evaluation.index_recall measures it; nprobe = n_list returns the exact
        lists).  topK <= 128; exclude, items and score apply as above, diversify takes its pool from the indexed call, and
        candidates= together with index= is a ValueError, as is an index over another catalogue size or element type."""
        from .retrieval import as_csr, as_filter, as_score
        if index is not None:
            from .retrieval import index_args
            # (with diversify the indexed call makes the pool, whose size diversify_args checks)
            nprobe = index_args(index, nprobe, topK if diversify is None else 1, self.item_laten.weight.shape[0],
                                self.item_laten.weight.dtype, candidates)
        if diversify is not None:
            from .retrieval import diversify_args
            pool = diversify_args(topK, diversify, pool, metric)
            it, sc = self.recommend(users, pool, exclude=exclude, items=items, score=score, candidates=candidates, index=index,
                                    nprobe=nprobe)
            picked, at, _, _, _ = _engine_for(self).rerank_mmr(self.item_laten.weight.data, it, sc, topK, diversify, metric=metric)
            return picked, torch.where(at >= 0, sc.gather(1, at.clamp(min=0).long()), sc.new_full((), float("-inf")))
        eng = _engine_for(self)
        w = self.user_laten.weight
        if candidates is not None:
            it, sc, _ = eng.topk_candidates(w.data, self.item_laten.weight.data, users, candidates, topK, as_csr(exclude, w.device),
                                            as_filter(items, self.item_laten.weight.shape[0], w.device), as_score(score, self))
            return it, sc
        if index is not None:
            it, sc, _ = eng.ivf_search(w.data, self.item_laten.weight.data, users, index, index.probe(w.data, users, nprobe), topK,
                                       as_csr(exclude, w.device), as_filter(items, self.item_laten.weight.shape[0], w.device),
                                       as_score(score, self))
            return it, sc
        return _topk(eng, int(topK))(w.data, self.item_laten.weight.data, users, topK, as_csr(exclude, w.device),
                                     as_filter(items, self.item_laten.weight.shape[0], w.device), as_score(score, self))

    def test_lists(self, inputs_data, topK=20, exclude=None, score=None):
        """inputs_data [n, 2 + neg] as test() takes it (user, positive, negatives; an array, a tensor or a DeviceRows) ->
        (items int64 [n, topK], scores float32 [n, topK]): the top-K matrix of each row's 1 + neg candidates, as item ids
        -- what the reference's test2 returns as indices (model/MF.py:82-106).  The order is the retrieval family's, not
        torch.topk's: the score is the fmaf chain of include/sml_hip.h (score_chain; with score=, the adjusted score of
        recommend), descending, ties broken by the smaller item id; an id a row repeats is listed once, (-1, -inf) fills a
        short list.  It is not claimed equal to eval_ranks' arithmetic, which sums the same products in another order.
        The rows are read where they lie (sml_amd.retrieval.CandidateRows): no copy of the candidate matrix is made."""
        from .retrieval import CandidateRows
        if not isinstance(inputs_data, CandidateRows):
            if not hasattr(inputs_data, "wait_ready"):                       # (a DeviceRows goes in as it is)
                inputs_data = torch.as_tensor(inputs_data).long()            # (int64 already: the same tensor)
            inputs_data = CandidateRows(inputs_data, 1)
        return self.recommend(None, topK, exclude=exclude, score=score, candidates=inputs_data)

    def similar_items(self, items, topK=20, metric="cosine", among=None, exclude_self=True, index=None, nprobe=None):
        """(int64 [n, topK], float32 [n, topK]): for each query item its topK most similar items of the catalogue, the item
        table serving as both tables (score descending, then id ascending; missing slots (-1, -inf)).  metric="dot": the
        bare dot product <x_q, x_i>.  metric="cosine": the order is the kernel's A(q, i) = <x_q, x_i> / ||x_i|| (the query's
        norm cannot reorder its own list); the returned score is A * (1 / ||x_q||), one more fp32 rounding done in torch, so
        it is the cosine up to three roundings, not a correctly rounded one.  among: an item filter (as recommend's items=)
        on the returned items; exclude_self: leave the query out of its own list.  Every cosine call rebuilds the norm table
        of the whole catalogue from the current weights (one pass over the item table, never stale): batch small query sets
        into one call rather than paying it per query.  index / nprobe: as in recommend -- the query item probes the index's
        lists with its own row and only their members are scored (topK <= 128)."""
        from .retrieval import as_filter, self_seen
        if index is not None:
            from .retrieval import index_args
            nprobe = index_args(index, nprobe, topK, self.item_laten.weight.shape[0], self.item_laten.weight.dtype)
        eng = _engine_for(self)
        w = self.item_laten.weight.data
        q = torch.as_tensor(items).to(w.device).long().reshape(-1)
        seen = self_seen(w.shape[0], w.device) if exclude_self else None
        allow = as_filter(among, w.shape[0], w.device)
        topk = _topk(eng, int(topK))
        if index is not None:
            probes = index.probe(w, q, nprobe)

            def topk(wu, wi, users, k, seen_, allow_, adjust=None):
                return eng.ivf_search(wu, wi, users, index, probes, k, seen_, allow_, adjust)[:2]
        if metric == "dot":
            return topk(w, w, q, topK, seen, allow)
        if metric != "cosine":
            raise ValueError('metric is "cosine" or "dot", got %r' % (metric,))
        adj = eng.item_adjust_cosine(w)
        it, sc = topk(w, w, q, topK, seen, allow, adjust=adj)
        return it, torch.where(it >= 0, sc * adj[0, q].unsqueeze(1), sc)

    def test_full(self, inputs_data, topK=20, exclude=None, items=None, score=None):
        """test() with the positive ranked against the WHOLE catalogue: inputs_data [n, >= 2] (user, positive, ... --
        further columns are ignored), rank = #{items != positive, not excluded, scoring strictly above it}.
        Returns (hits, ndcg_sum, indices of the rows that hit).  items (as in recommend): the positive is ranked among
        the allowed items only; a positive outside the subset still gets its rank among them.  score (as in recommend):
        rank by the adjusted score."""
        from .retrieval import as_csr, as_filter, as_score
        eng = _engine_for(self)
        w = self.user_laten.weight
        ranks = eng.full_rank(w.data, self.item_laten.weight.data, inputs_data, as_csr(exclude, w.device),
                              as_filter(items, self.item_laten.weight.shape[0], w.device), as_score(score, self))
        hits, ndcg = eng.eval_metrics(ranks, topK)
        hit_rows = (ranks < topK).nonzero()[:, 0]
        batch_ndcg = torch.tensor(ndcg) if hits > 0 else 0
        return hits * 1.0, batch_ndcg, hit_rows

    def test_users(self, held_out, topK=(20, 10, 5), exclude=None, items=None, score=None):
        """Every user's whole held-out set ranked against the WHOLE catalogue at once (HipEngine.user_ranks), by the score
        test() uses.  held_out: a sml_amd.retrieval.SeenItems (retrieval.held_out) or a (off, items) CSR over all users;
        exclude as in recommend().  Returns a dict: users, pos_off, pos_items (the users with at least one held-out item
        and their items, sml_amd.retrieval.nonempty_users), ks, and the engine's above / pos / hits / dcg / ap / first.
        items (as in recommend): only the allowed items are ranked; a held-out item outside the subset has pos -1.
        score (as in recommend): rank by the adjusted score."""
        from .retrieval import as_csr, as_filter, as_score, nonempty_users
        eng = _engine_for(self)
        w = self.user_laten.weight
        users, pos_off, pos_items = nonempty_users(held_out)
        ks = tuple(int(k) for k in (topK if hasattr(topK, "__len__") else (topK,)))
        out = eng.user_ranks(w.data, self.item_laten.weight.data, users, pos_off, pos_items, as_csr(exclude, w.device), ks,
                             as_filter(items, self.item_laten.weight.shape[0], w.device), as_score(score, self))
        out.update(users=users, pos_off=pos_off, pos_items=pos_items, ks=ks)
        return out

    def _fold_in_check(self):
        from . import als
        if isinstance(self, MF2):
            raise ValueError("fold-in solves the bare dot-product model: MF2's biased score has no closed-form row here")
        if self.hidden_dim not in als.WIDTHS:
            raise ValueError("fold-in exists at laten_factor 32 / 64 only (128 is out of scope), got %d" % self.hidden_dim)

    def _fold_in(self, out_emb, other_emb, sets, rows, reg, alpha0):
        from . import als
        with torch.no_grad():
            return als.fold_in(out_emb.weight.data, other_emb.weight.data, sets, rows, reg=reg, alpha0=alpha0, engine=_engine_for(self))

    def fold_in_users(self, history, users=None, reg=0.1, alpha0=0.1):
        """Give users the closed-form row of the iALS half-step against the current item table (sml_amd.als.fold_in;
        include/sml_hip.h, FOLD-IN): user_laten's rows are rewritten in place, nothing else changes.  history: the users'
        interaction sets -- a sml_amd.retrieval.SeenItems, a DeviceSeen or a (off, items) CSR over all users.  users: the ids to
        solve (None: every user with a non-empty history, sml_amd.retrieval.nonempty_users).  Works on fp32 and .half()
        models at laten_factor 32 / 64; 128, or MF2's biased score, is a ValueError.  reg and alpha0 default to conventions,
        not tuned values.  Returns a sml_amd.als.FoldIn (solved / empty / failed counts and the status per row)."""
        from .retrieval import as_csr, nonempty_users
        self._fold_in_check()
        if users is None:
            users = nonempty_users(history)[0]
        return self._fold_in(self.user_laten, self.item_laten, as_csr(history, self.user_laten.weight.device), users, reg, alpha0)

    def fold_in_items(self, history, items=None, reg=0.1, alpha0=0.1):
        """fold_in_users with the roles swapped: items get their closed-form row against the current user table, from the
        users that interacted with them.  history is the same user -> items set; it is transposed on the device
        (sml_amd.als.transpose_sets).  items: the ids to solve (None: every item with at least one user)."""
        from . import als
        from .retrieval import as_csr, nonempty_users
        self._fold_in_check()
        by_item = als.transpose_sets(as_csr(history, self.user_laten.weight.device), self.user_num, self.item_num, _engine_for(self))
        if items is None:
            items = nonempty_users(by_item)[0]
        return self._fold_in(self.item_laten, self.user_laten, by_item, items, reg, alpha0)

    def set_parameters(self, user_weight, item_weight):
        # last column is the bias (model/MF.py:108-112)
        self.user_laten.weight.data.copy_(user_weight[:, 0:-1])
        self.user_bais.weight.data.copy_(user_weight[:, -1].unsqueeze(-1))
        self.item_laten.weight.data.copy_(item_weight[:, 0:-1])
        self.item_bais.weight.data.copy_(item_weight[:, -1].unsqueeze(-1))


class _MF2Train(torch.autograd.Function):
    """MF2.forward's training branch (reference model/MF.py:129-147) as ONE differentiable op: the row gathers and the two
    dot products run on the HIP engine (k_mf_forward), the bias terms, -sum(logsigmoid) and the reference's "l2" (row NORMS,
    the negatives' as one Frobenius norm) are a handful of elementwise device ops, and backward scatters the hand-derived
    gradient rows into dense table gradients -- what autograd hands nn.Embedding(sparse=False)."""

    @staticmethod
    def forward(ctx, module, user, item, neg, wu, wi, bu, bi):
        eng = _engine_for(module)
        dev = wu.device
        user, item, neg = (x.to(dev).long() for x in (user, item, neg))
        ue, ie, sp = eng.mf_forward(wu.detach(), wi.detach(), user, item)
        _, ne, sn = eng.mf_forward(wu.detach(), wi.detach(), user, neg)
        ub, ib, nb = bu.detach()[user, 0], bi.detach()[item, 0], bi.detach()[neg, 0]
        score = (ub + ib + sp) - (ub + nb + sn)             # result_pos - result_neg, formed as the reference forms it
        bpr = -torch.sum(torch.nn.functional.logsigmoid(score))
        nu, ni, nn_ = ue.norm(dim=-1), ie.norm(dim=-1), ne.norm()
        l2 = nu.sum() + ni.sum() + nn_.sum()
        ctx.save_for_backward(user, item, neg, ue, ie, ne, score, nu, ni, nn_)
        ctx.shapes = (wu.shape, wi.shape, bu.shape, bi.shape)
        return bpr, l2

    @staticmethod
    def backward(ctx, g_bpr, g_l2):
        user, item, neg, ue, ie, ne, score, nu, ni, nn_ = ctx.saved_tensors
        ds = (-g_bpr * torch.sigmoid(-score)).unsqueeze(-1)               # d bpr / d score
        du = ds * (ie - ne) + g_l2 * ue / nu.unsqueeze(-1)
        di = ds * ue + g_l2 * ie / ni.unsqueeze(-1)
        dn = -ds * ue + g_l2 * ne / nn_
        su, si, sbu, sbi = ctx.shapes
        gwu = torch.zeros(su, device=ue.device, dtype=ue.dtype).index_add_(0, user, du)
        gwi = torch.zeros(si, device=ue.device, dtype=ue.dtype).index_add_(0, item, di).index_add_(0, neg, dn)
        gbu = torch.zeros(sbu, device=ue.device, dtype=ue.dtype)          # the user bias cancels in result_pos - result_neg
        gbi = torch.zeros(sbi, device=ue.device, dtype=ue.dtype).index_add_(0, item, ds).index_add_(0, neg, -ds)
        return None, None, None, None, gwu, gwi, gbu, gbi


class MF2(MFbasemode):
    """model/MF.py:118-156.  Test branch: the dot product plus both biases.  Training branch (`neg_item` given): the
    reference's (bpr_loss, l2loss) pair, differentiable w.r.t. the four embedding tables (`_MF2Train`).  Nothing in the
    reference calls this class; the bare BPR step at table scale is HipEngine.bare_epoch(bce=False).

    Retrieval: recommend / test_full / test_users rank by the bare dot product unless told otherwise, as they do for
    MFbasemode.  score="bias" is the order of this class's own test-branch score: the user bias is constant per user and
    cannot reorder a user's list, the item bias can.  The scores returned then are fmaf(dot, 1, item bias) -- they leave out
    the user bias and are rounded once, so they are not bit-equal to forward's three-term sum."""

    def forward(self, user, item, neg_item=None):
        if neg_item is not None:
            return _MF2Train.apply(self, user, item, neg_item, self.user_laten.weight, self.item_laten.weight,
                                   self.user_bais.weight, self.item_bais.weight)
        ue, ie, s = MFbasemode.forward(self, user, item)
        user = user.to(s.device).long()
        item = item.to(s.device).long()
        s = s + self.user_bais.weight.data[user, 0] + self.item_bais.weight.data[item, 0]
        return ue, ie, s


# checkpoints written by this build name the reference's module path, and vice versa
MFbasemode.__module__ = "model.MF"
MF2.__module__ = "model.MF"
