"""Per-user ranking of held-out sets without a GPU: the numpy reference against brute force, the metric layer
(sml_amd.evaluation.user_metrics) against a transcription of the reference's per-user metrics, the held-out helpers
and the C entry points' argument checks."""
import numpy as np
import pytest
import torch

from _fp32_chain import near_tie_case, random_case, ref_topk, seen_csr
from _user_rank_ref import brute_user_rank, held_out_csr, ref_user_metrics, ref_user_rank, user_scores


def _small_case(d, seed, nan_items=()):
    c = random_case(d, seed, U=40, I=257, n=64)
    for i in nan_items:
        c["wi"][i] = np.nan
    rng = c["rng"]
    off, items = c["seen"]
    lists = []
    for x, u in enumerate(rng.choice(40, size=24, replace=False)):
        m = [0, 1, 3, 17, 60][x % 5]
        it = set(rng.choice(257, size=m, replace=False).tolist())
        s = items[off[u]:off[u + 1]]
        if len(s) and x % 3 == 0:
            it.add(int(s[0]))                          # a held-out item in Seen(u)
        it.update(i for i in nan_items if x % 2)       # held-out items scoring NaN
        lists.append((int(u), it))
    lists.append(lists[1])                             # a repeated user
    return c, held_out_csr(40, lists)


@pytest.mark.parametrize("d", [32, 64])
def test_reference_matches_brute_force(d):
    c, (users, off, items) = _small_case(d, d, nan_items=(5, 200))
    S = user_scores(c["wu"], c["wi"], users)
    a_ref, p_ref = ref_user_rank(c["wu"], c["wi"], users, off, items, c["seen"], S)
    a_bf, p_bf = brute_user_rank(c["wu"], c["wi"], users, off, items, c["seen"], S)
    np.testing.assert_array_equal(a_ref, a_bf)
    np.testing.assert_array_equal(p_ref, p_bf)
    assert (p_ref == -1).any() and (np.diff(off) == 0).any()


def test_reference_matches_brute_force_on_ties():
    c = near_tie_case(32, seed=3)
    rows = c["rows"][:96]
    users = np.unique(rows[:, 0])[:12]
    lists = {int(u): set(rows[rows[:, 0] == u, 1].tolist()) for u in users}
    users, off, items = held_out_csr(c["wu"].shape[0], lists)
    S = user_scores(c["wu"], c["wi"], users)
    a_ref, p_ref = ref_user_rank(c["wu"], c["wi"], users, off, items, c["seen"], S)
    a_bf, p_bf = brute_user_rank(c["wu"], c["wi"], users, off, items, c["seen"], S)
    np.testing.assert_array_equal(a_ref, a_bf)
    np.testing.assert_array_equal(p_ref, p_bf)


def test_reference_pos_is_topk_index():
    c, (users, off, items) = _small_case(32, 7)
    _, pos = ref_user_rank(c["wu"], c["wi"], users, off, items, c["seen"])
    lists, _ = ref_topk(c["wu"], c["wi"], users, 257, c["seen"])
    for x in range(len(users)):
        for e in range(off[x], off[x + 1]):
            hit = np.nonzero(lists[x] == items[e])[0]
            assert (pos[e] == hit[0]) if len(hit) else (pos[e] == -1)


# ---- the metric layer against the reference's per-user functions (evalution/evalution_function.py) ------------------

def _idcg(n):
    arr = torch.arange(n).float() + 2
    return (1.0 / torch.log2(arr)).sum()


def _match(ranklist, targets):
    return torch.tensor([1 if int(i) in targets else 0 for i in ranklist])


def _rec_ndcg(ranklist, targets):
    idcg = _idcg(len(targets))
    rank_of_target = torch.nonzero(_match(ranklist, targets))[:, 0]
    hits = rank_of_target.shape[0]
    if hits > 0:
        dcg = (1.0 / torch.log2(rank_of_target.float() + 2)).sum() / idcg
    else:
        dcg = 0
    return hits / len(targets), dcg


def _precision(ranklist, targets, topK):
    return torch.nonzero(_match(ranklist, targets))[:, 0].shape[0] / topK


def _mrr(ranklist, targets):
    rank_of_target = torch.nonzero(_match(ranklist, targets))[:, 0]
    return 1.0 / (rank_of_target[0] + 1).float() if rank_of_target.shape[0] > 0 else 0


def _map(ranklist, targets):
    rank_of_target = torch.nonzero(_match(ranklist, targets)).float()[:, 0]
    if rank_of_target.shape[0] > 0:
        rank_of_target = rank_of_target + 1
        hits = torch.arange(rank_of_target.shape[0]).float() + 1
        return torch.sum(hits / rank_of_target) / (min(ranklist.shape[0], len(targets)) * 1.0)
    return 0


@pytest.mark.parametrize("d", [32, 64])
def test_metric_layer_matches_reference_functions(d):
    from sml_amd.evaluation import user_metrics
    c, (users, off, items) = _small_case(d, 10 + d, nan_items=(9,))
    keep = np.diff(off) > 0                           # the layer averages over users with m > 0
    users, off, items = held_out_csr(40, [(u, items[off[x]:off[x + 1]]) for x, u in enumerate(users) if keep[x]])
    ks = (20, 10, 5, 1)
    _, pos = ref_user_rank(c["wu"], c["wi"], users, off, items, c["seen"])
    hits, dcg, ap, first = ref_user_metrics(pos, off, ks)
    out = dict(users=users, pos_off=off, pos_items=items, ks=ks, pos=pos, hits=hits, dcg=dcg, ap=ap, first=first)
    got = user_metrics(out)
    assert got["users"] == len(users)
    for K in ks:
        lists, _ = ref_topk(c["wu"], c["wi"], users, K, c["seen"])
        want = {k: [] for k in ("recall", "precision", "ndcg", "ndcg_ref", "map", "mrr")}
        for x in range(len(users)):
            targets = set(items[off[x]:off[x + 1]].tolist())
            rl = torch.from_numpy(lists[x])
            rec, ndcg_ref = _rec_ndcg(rl, targets)
            m = len(targets)
            want["recall"].append(rec)
            want["ndcg_ref"].append(float(ndcg_ref))
            want["ndcg"].append(float(ndcg_ref) * float(_idcg(m)) / float(_idcg(min(K, m))))
            want["precision"].append(_precision(rl, targets, K))
            want["map"].append(float(_map(rl, targets)))
            want["mrr"].append(float(_mrr(rl, targets)))
        for k, v in want.items():
            assert got[k][K] == pytest.approx(np.mean(v), rel=1e-6, abs=1e-9), (k, K)


def test_hit_shares():
    from sml_amd.evaluation import user_metrics
    users, off, items = held_out_csr(10, {1: [0, 5, 7], 2: [5, 6], 8: [1]})
    pos = np.array([0, 3, -1, 25, 1, 2])
    hits, dcg, ap, first = ref_user_metrics(pos, off, (5, 30))
    out = dict(users=users, pos_off=off, pos_items=items, ks=(5, 30), pos=pos, hits=hits, dcg=dcg, ap=ap, first=first)
    got = user_metrics(out, old_user={1, 2}, old_item=[0, 6])
    # hits @5: (1,0) oo, (1,5) on, (2,6) oo, (8,1) nn;  @30 adds (2,5) on
    assert got["hit_shares"][5] == (0.5, 0.25, 0.0, 0.25)
    assert got["hit_shares"][30] == (0.4, 0.4, 0.0, 0.2)
    assert got["recall"][5] == pytest.approx(np.mean([2 / 3, 1 / 2, 1.0]))
    assert got["mrr"][5] == pytest.approx(np.mean([1.0, 1 / 3, 1 / 2]))


def test_held_out_helpers():
    from sml_amd.retrieval import SeenItems, held_out, nonempty_users
    pairs = np.array([[3, 9, 1, 2], [0, 4, 5, 5], [3, 2, 0, 0], [3, 9, 7, 7], [6, 0, 1, 1]])
    sets = held_out(pairs, 8, 12)
    assert isinstance(sets, SeenItems) and len(sets) == 4
    users, off, items = nonempty_users(sets)
    assert users.tolist() == [0, 3, 6] and off.tolist() == [0, 1, 3, 4] and items.tolist() == [4, 2, 9, 0]
    assert users.dtype == np.int64 and off.dtype == np.int64 and items.dtype == np.int32
    u2, o2, i2 = nonempty_users(seen_csr(8, 12, {3: [9, 2], 0: [4], 6: [0]}))
    assert u2.tolist() == users.tolist() and o2.tolist() == off.tolist() and i2.tolist() == items.tolist()
    u3, o3, i3 = nonempty_users(held_out(np.zeros((0, 2), np.int64), 8, 12))
    assert len(u3) == 0 and o3.tolist() == [0] and len(i3) == 0


def test_entry_points_refuse_bad_arguments_without_a_context():
    from sml_amd import _lib
    lib = _lib.load()
    ks = np.array([20], np.int32)
    assert lib.sml_user_rank_scratch_bytes(None, 4, 10, 100) < 0
    assert lib.sml_user_rank(None, None, None, 100, None, 1, None, None, 1, None, None, None, None, None, None) != 0
    assert lib.sml_user_metrics(None, None, None, 1, ks.ctypes.data, 1, None, None, None, None, None) != 0
