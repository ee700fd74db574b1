"""recall@K / ndcg@K over (user, positive, negatives) rows -- reference
evalution/evaluation2.py:8-26 on the HIP rank kernel."""
import numpy as np
import torch

from .datasets import loader_base_seed_draw


class DeviceRows(object):
    """A whole test set resident on the GPU, standing in for the reference's
    DataLoader(testDataset(rows), batch_size=1024): one kernel launch ranks every row.
    Iterating it makes the one global-RNG draw a DataLoader iteration makes, so a run's
    random stream stays aligned with the reference's."""

    def __init__(self, rows, device, stream=None):
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(np.ascontiguousarray(rows))
        self.ready = None
        if stream is None:
            self.rows = rows.to(device=device, dtype=torch.int64).contiguous()
        else:
            # upload on a stream of its own (a copy on the default stream would first wait for every queued kernel);
            # the first consumer orders itself behind `ready` (wait_ready)
            with torch.cuda.stream(stream):
                self.rows = rows.to(device=device, dtype=torch.int64).contiguous()
                self.ready = torch.cuda.Event()
                self.ready.record(stream)

    def wait_ready(self):
        """Order the current stream behind the upload (once)."""
        if self.ready is not None:
            torch.cuda.current_stream(self.rows.device).wait_event(self.ready)
            self.ready = None

    def __len__(self):
        return 1

    def __iter__(self):
        loader_base_seed_draw()
        yield self.rows


def test_model(model, test_set, old_user=None, old_item=None, topK=10, need_pbar=False):
    """-> (recall@topK, ndcg@topK) = (hits, sum 1/log2(rank+2)) / number of rows."""
    model.eval()
    device = model.user_laten.weight.device
    num_test = 0
    hits = 0.0
    ndcg = 0.0
    for datas in test_set:
        datas = torch.as_tensor(datas).long().to(device)
        batch_hit, batch_ndcg, _ = model.test(datas, topK=topK)
        hits += batch_hit
        ndcg += float(batch_ndcg)
        num_test += datas.shape[0]
    return hits / num_test, torch.tensor(np.float32(ndcg / num_test))


def test_model_full(model, test_set, seen=None, topK=10, items=None, score=None):
    """(recall@topK, ndcg@topK) as test_model returns them, with every positive ranked against the whole catalogue
    (MFbasemode.test_full), leaving out `seen` (a sml_amd.retrieval.SeenItems or a (seen_off, seen_items) CSR).
    test_set: a DeviceRows, an array / tensor [n, >= 2], or an iterable of such batches.  Unlike test_model this
    makes no DataLoader-emulating RNG draw: the run's random streams stay where they were.  items: rank inside a subset
    of the catalogue (a sml_amd.retrieval.ItemFilter, a bool mask or filter words, as MFbasemode.recommend takes).  score:
    rank by an adjusted score ("bias", "cosine", an ItemScore ..., as MFbasemode.recommend takes); None is the bare dot."""
    model.eval()
    device = model.user_laten.weight.device
    if isinstance(test_set, DeviceRows):
        test_set.wait_ready()
        batches = [test_set.rows]
    elif isinstance(test_set, (np.ndarray, torch.Tensor)):
        batches = [test_set]
    else:
        batches = test_set
    num_test = 0
    hits = 0.0
    ndcg = 0.0
    extra = dict(([("items", items)] if items is not None else []) + ([("score", score)] if score is not None else []))
    for datas in batches:
        datas = torch.as_tensor(datas).long().to(device)
        batch_hit, batch_ndcg, _ = model.test_full(datas, topK=topK, exclude=seen, **extra)
        hits += batch_hit
        ndcg += float(batch_ndcg)
        num_test += datas.shape[0]
    return hits / num_test, torch.tensor(np.float32(ndcg / num_test))


def idcg(n):
    """sum_{r < n} 1 / log2(r + 2) in float64, elementwise over an int array (the reference's IDCG, evalution_function.py)."""
    n = np.asarray(n, dtype=np.int64)
    c = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(int(n.max(initial=0))) + 2.0))])
    return c[n]


def user_metrics(out, old_user=None, old_item=None):
    """Means over users of the per-user metrics of MFbasemode.test_users' result `out`, at each K of out["ks"]:

      recall = hits / m;  precision = hits / K;  ndcg = dcg / IDCG(min(K, m));  ndcg_ref = dcg / IDCG(m) (the reference's
      get_NDCG);  map = ap / min(K, m) (get_MAP);  mrr = 1 / (first + 1) when first < K, else 0 (get_MRR)

    with m = |T(u)| > 0.  With old_user and old_item (id collections), `hit_shares` gives test_model_pre's split of the
    hits at each K (reference evalution/evaluation2.py): shares of (old user, old item), (old user, new item),
    (new user, old item), (new user, new item); all 0 when nothing hits."""
    host = lambda t: np.asarray(t.cpu() if torch.is_tensor(t) else t)     # noqa: E731
    pos_off = host(out["pos_off"]).astype(np.int64)
    m = np.diff(pos_off).astype(np.float64)
    hits, dcg, ap = (host(out[k]).astype(np.float64).reshape(m.shape[0], -1) for k in ("hits", "dcg", "ap"))
    first = host(out["first"]).reshape(-1)
    res = {"users": int(m.shape[0])}
    for name in ("recall", "precision", "ndcg", "ndcg_ref", "map", "mrr"):
        res[name] = {}
    if old_user is not None and old_item is not None:
        res["hit_shares"] = {}
        pos = host(out["pos"])
        u_of = np.repeat(np.asarray(out["users"], dtype=np.int64), np.diff(pos_off))
        ou = np.isin(u_of, np.asarray(list(old_user) if isinstance(old_user, (set, frozenset)) else old_user))
        oi = np.isin(np.asarray(out["pos_items"], dtype=np.int64),
                     np.asarray(list(old_item) if isinstance(old_item, (set, frozenset)) else old_item))
    for q, K in enumerate(out["ks"]):
        mk = np.minimum(m, K)
        with np.errstate(invalid="ignore", divide="ignore"):
            vals = {"recall": hits[:, q] / m, "precision": hits[:, q] / K, "ndcg": dcg[:, q] / idcg(mk),
                    "ndcg_ref": dcg[:, q] / idcg(m), "map": ap[:, q] / mk,
                    "mrr": np.where((first >= 0) & (first < K), 1.0 / (first + 1.0), 0.0)}
        for name in ("recall", "precision", "ndcg", "ndcg_ref", "map", "mrr"):
            res[name][K] = float(np.mean(vals[name])) if m.shape[0] else 0.0
        if "hit_shares" in res:
            h = (pos >= 0) & (pos < K)
            c = [int((h & ou & oi).sum()), int((h & ou & ~oi).sum()), int((h & ~ou & oi).sum()), int((h & ~ou & ~oi).sum())]
            tot = sum(c)
            res["hit_shares"][K] = tuple(x / tot if tot else 0.0 for x in c)
    return res


def test_model_users(model, test_pairs, seen=None, topK=(20, 10, 5), old_user=None, old_item=None, items=None, score=None):
    """All-ranking evaluation of a test period: every user's whole held-out set T(u) (the distinct (user, item) pairs of
    test_pairs [n, >= 2]; further columns are ignored) placed in the user's ranked list over the entire catalogue minus
    `seen` (MFbasemode.test_users), then Recall / Precision / NDCG / MAP / MRR @K averaged over the users with m > 0
    (user_metrics).  Makes no RNG draw.  items: rank inside a subset of the catalogue (as test_model_full); held-out items
    outside it never hit.  score: rank by an adjusted score (as test_model_full)."""
    from .retrieval import held_out
    model.eval()
    sets = held_out(test_pairs, model.user_num, model.item_num)
    extra = dict(([("items", items)] if items is not None else []) + ([("score", score)] if score is not None else []))
    out = model.test_users(sets, topK=topK, exclude=seen, **extra)
    return user_metrics(out, old_user, old_item)


def recall_curve(model, held_out, ks, exclude=None, items=None, score=None):
    """[recall@K for K in ks]: the mean over the users with a non-empty held-out set T(u) (retrieval.nonempty_users) of
    |first K of the user's list AND T(u)| / |T(u)|, the lists being MFbasemode.recommend(users, max(ks)) -- one call, up to
    K = 1,024 (HipEngine.topk_deep above 128).  held_out: a sml_amd.retrieval.SeenItems (retrieval.held_out) or a (off, items)
    CSR over all users; exclude, items and score as recommend takes them.  At any K the value is the recall
    test_model_users reports at that K: a held-out item hits when its place in the list is below K, and an item that is
    excluded or filtered out is in no list."""
    from .retrieval import deep_args, nonempty_users
    ks = [deep_args(k) for k in ks]
    if not ks:
        return []
    users, pos_off, pos_items = nonempty_users(held_out)
    if len(users) == 0:
        return [0.0 for _ in ks]
    model.eval()
    n_item = int(model.item_laten.weight.shape[0])
    extra = dict(([("items", items)] if items is not None else []) + ([("score", score)] if score is not None else []))
    lists = model.recommend(torch.from_numpy(users), max(ks), exclude=exclude, **extra)[0].cpu().numpy()
    m = np.diff(pos_off)
    row = np.arange(len(users), dtype=np.int64)
    held = np.repeat(row, m) * n_item + pos_items.astype(np.int64)             # ascending: users ascend, items ascend inside a user
    keys = row[:, None] * n_item + lists
    at = np.minimum(np.searchsorted(held, keys), len(held) - 1)
    hit = (lists >= 0) & (held[at] == keys)
    hits = np.concatenate([np.zeros((len(users), 1), np.int64), np.cumsum(hit, axis=1)], axis=1)
    return [float(np.mean(hits[:, k].astype(np.float64) / m.astype(np.float64))) for k in ks]


def recall_of_lists(lists, users, held_out, ks):
    """[recall@K for K in ks] of lists that are given rather than made: lists int [n, >= max(ks)] (a tensor or an array; -1 pads
    a short list) belongs row by row to `users` [n]; the value is the mean, over the rows whose user has a non-empty held-out set
    T(u), of |first K of the row AND T(u)| / |T(u)| -- the list half of recall_curve, for any source of lists (a neighbourhood
    model has no tables for recall_curve to call).  held_out: a sml_amd.retrieval.SeenItems (retrieval.held_out) or a (off,
    items) CSR over all users.  With users = retrieval.nonempty_users(held_out)[0] and lists = model.recommend(users, max(ks),
    exclude=e)[0] the result equals recall_curve(model, held_out, ks, exclude=e)."""
    from .retrieval import DeviceSeen, SeenItems
    ks = [int(k) for k in ks]
    if not ks:
        return []
    lists = np.asarray(lists.cpu() if torch.is_tensor(lists) else lists).astype(np.int64)
    users = np.asarray(users.cpu() if torch.is_tensor(users) else users).astype(np.int64).reshape(-1)
    if lists.ndim != 2 or lists.shape[0] != len(users) or min(ks) < 1 or max(ks) > lists.shape[1]:
        raise ValueError("recall_of_lists: lists is [len(users), >= max(ks)] and every K >= 1, got %s for %d users and ks %s"
                         % (lists.shape, len(users), ks))
    off, held_items = held_out.host() if isinstance(held_out, (SeenItems, DeviceSeen)) else \
        (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in held_out)
    off, held_items = np.asarray(off, dtype=np.int64), np.asarray(held_items, dtype=np.int64)
    m = off[users + 1] - off[users]
    keep = m > 0
    if not keep.any():
        return [0.0 for _ in ks]
    lists, users, m = lists[keep], users[keep], m[keep]
    row = np.arange(len(users), dtype=np.int64)
    start = np.cumsum(m) - m
    pos_items = held_items[np.repeat(off[users] - start, m) + np.arange(int(m.sum()), dtype=np.int64)]
    base = int(max(lists.max(), pos_items.max())) + 1
    held = np.repeat(row, m) * base + pos_items                                 # ascending: rows ascend, items ascend inside a row
    keys = row[:, None] * base + lists
    at = np.minimum(np.searchsorted(held, keys), len(held) - 1)
    hit = (lists >= 0) & (held[at] == keys)
    hits = np.concatenate([np.zeros((len(users), 1), np.int64), np.cumsum(hit, axis=1)], axis=1)
    return [float(np.mean(hits[:, k].astype(np.float64) / m.astype(np.float64))) for k in ks]


def popularity_of_lists(lists, item_count):
    """{"mean_count", "coverage"} of lists that are given: lists int [n, K] (a tensor or an array; -1 pads a short list),
    item_count [n_item] the interaction count of every item.  mean_count: the mean of item_count over the listed slots (a listed
    item counts once per slot it fills; 0.0 when nothing is listed); coverage: the share of the catalogue that appears in some
    list.  Together they show what a popularity penalty (the beta of rp3beta) did to the lists.  Plain torch on the lists'
    device, float64."""
    lists = torch.as_tensor(lists).long()
    count = torch.as_tensor(item_count).to(device=lists.device, dtype=torch.float64).reshape(-1)
    if lists.dim() != 2 or (lists.numel() and int(lists.max()) >= count.shape[0]):
        raise ValueError("popularity_of_lists: lists is [n, K] with ids below len(item_count) = %d, got %s" % (count.shape[0], tuple(lists.shape)))
    listed = lists[lists >= 0]
    if listed.numel() == 0:
        return {"mean_count": 0.0, "coverage": 0.0}
    return {"mean_count": float(count[listed].mean()), "coverage": float(torch.unique(listed).numel()) / float(count.shape[0])}


def index_recall(model, index, users, topK=20, nprobe=None, exclude=None):
    """What the approximation of MFbasemode.recommend(index=) costs: the mean over `users` of
    |indexed list AND exact list| / (number of live slots of the exact list), the two lists being recommend(users, topK,
    exclude=) with and without the index (nprobe as recommend takes it); users whose exact list is empty do not count (0.0
    when none is left).  Exactly 1.0 when every list is probed.  The lists are compared on the host in float64."""
    users = torch.as_tensor(users).reshape(-1)
    exact = model.recommend(users, topK, exclude=exclude)[0].cpu().numpy()
    got = model.recommend(users, topK, exclude=exclude, index=index, nprobe=nprobe)[0].cpu().numpy()
    live = (exact >= 0).sum(1)
    both = ((got[:, :, None] == exact[:, None, :]) & (got >= 0)[:, :, None]).any(2).sum(1)
    keep = live > 0
    if not keep.any():
        return 0.0
    return float(np.mean(both[keep].astype(np.float64) / live[keep].astype(np.float64)))


def intra_list_similarity(model, lists, metric="cosine"):
    """float32 [n]: the mean pairwise similarity of each list's items -- the number that shows what
    MFbasemode.recommend(diversify=) did.  lists: item ids [n, m <= 128], padded with -1 (ids outside the catalogue and
    repeats of an id count as padding); metric "cosine" or "dot" of the item rows.  One HipEngine.rerank_mmr call with
    lam = 1, normalize=False and rel = -position: the order is kept, so the sum of the pairs' similarities runs in list
    order, and it is divided by m (m - 1) / 2 over the m live items (0 for m < 2)."""
    from .mf import _engine_for
    from .retrieval import rerank_args
    eng = _engine_for(model)
    dev = model.item_laten.weight.device
    lists = torch.as_tensor(lists).to(dev)
    if lists.dim() != 2:
        raise ValueError("lists is a matrix [n, m] of item ids padded with -1, got shape %s" % (tuple(lists.shape),))
    n, m = lists.shape
    rerank_args(m, 1.0, metric, m)
    rel = -torch.arange(m, device=dev, dtype=torch.float32).expand(n, m).contiguous()
    _, _, _, n_sel, sim_sum = eng.rerank_mmr(model.item_laten.weight.data, lists, rel, m, 1.0, metric=metric, normalize=False)
    cnt = n_sel.float()
    pairs = cnt * (cnt - 1.0) / 2.0
    return torch.where(pairs > 0, sim_sum / pairs.clamp(min=1.0), torch.zeros_like(sim_sum))
