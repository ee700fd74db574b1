"""Full-catalogue retrieval on fp16 tables on the MI355X (sml_full_rank_f16 / sml_topk_items_f16 / sml_user_rank_f16
through HipEngine, MFbasemode and sml_amd.evaluation).

d = 32 / 64: every output on fp16 tables equals, byte for byte, the fp32 entry points' output on `.float()` copies of the
same tables.  d = 128 (fp16 only): ranks, lists, score bits, above and pos against the exact emulation of the kernels'
fp32 chain on the widened tables (tests/_fp32_chain.py, tests/_user_rank_ref.py)."""
import numpy as np
import pytest
import torch

import _fp32_chain as F
from _half_cases import dyadic_half, half_near_tie_case, plant_specials, random_half_case, widen
from _user_rank_ref import held_out_csr, ref_user_metrics, ref_user_rank
from conftest import make_mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(seen):
    return None if seen is None else (gpu(seen[0]), gpu(seen[1]))


def held_out_sets(c, rng, n_users, extra=()):
    """Held-out sets for n_users of the case's users: sizes 0, 1, 4, 30, 200 in turn, the rows' positives, some Seen items,
    the items of `extra` for every third user; one user listed twice."""
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    off, items = c["seen"]
    rows = c["rows"]
    lists = []
    for x, u in enumerate(rng.choice(U, size=n_users, replace=False)):
        it = set(rows[rows[:, 0] == u, 1].tolist())
        it.update(rng.choice(I, size=min(I, [0, 1, 4, 30, 200][x % 5]), replace=False).tolist())
        s = items[off[u]:off[u + 1]]
        if len(s) and x % 4 == 1:
            it.update(s[:3].tolist())
        if x % 3 == 2:
            it.update(extra)
        if x % 11 == 10:
            it = set()
        lists.append((int(u), it))
    if len(lists) > 20:
        lists.insert(5, lists[20])
    return held_out_csr(U, lists)


# ---- d = 32 / 64: bit identity with the fp32 path on widened copies ---------------------------------------------------

def assert_same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    v = (lambda t: t.view(torch.int32)) if a.dtype == torch.float32 else (lambda t: t)
    assert torch.equal(v(a), v(b)), what


@pytest.mark.parametrize("with_seen", [False, True])
@pytest.mark.parametrize("n", [31, 33, 95, 97, 127, 129])
@pytest.mark.parametrize("d", [32, 64])
def test_bit_identical_to_fp32_path_on_widened_tables(d, n, with_seen):
    """Random fp16 values with subnormal halves, +-0, a NaN user row, a NaN item row and +-inf entries; 1,517 items (the
    last tile holds 13); n users / rows around a wave, a 3-wave and a 4-wave block."""
    c = random_half_case(d, seed=2000 + 10 * d + n, U=150, I=1517, n=n)
    rng = c["rng"]
    nan_item = plant_specials(c, rng)
    seen = csr_dev(c["seen"]) if with_seen else None
    hu, hi = gpu(c["wu"]), gpu(c["wi"])
    assert hu.dtype == torch.float16
    fu, fi = hu.float(), hi.float()
    eng = engine(d)
    rows = c["rows"].copy()
    rows[:3, 0] = 7                     # the NaN user
    rows[3, 1] = nan_item               # a NaN positive
    rows[4, 1] = 13                     # positives with an inf entry
    rows[5, 1] = 17
    rows = gpu(rows)
    assert_same_bytes(eng.full_rank(hu, hi, rows, seen), eng.full_rank(fu, fi, rows, seen), "rank")
    users = c["users"].copy()
    users[0] = 7
    users = gpu(users)
    for k in (1, 20, 128):
        hi_, hs_ = eng.topk_items(hu, hi, users, k, seen)
        fi_, fs_ = eng.topk_items(fu, fi, users, k, seen)
        assert hs_.dtype == torch.float32 and hi_.dtype == torch.int64
        assert_same_bytes(hi_, fi_, ("items", k))
        assert_same_bytes(hs_, fs_, ("scores", k))
    us, off, items = held_out_sets(c, rng, n, extra=(nan_item, 13, 17))
    ho = eng.user_ranks(hu, hi, us, off, items, seen, (20, 10, 5))
    fo = eng.user_ranks(fu, fi, us, off, items, seen, (20, 10, 5))
    for key in ("above", "pos", "hits", "dcg", "ap", "first"):
        assert_same_bytes(ho[key], fo[key], key)
    assert (ho["pos"] == -1).any()


# ---- d = 128: against the exact emulation of the fp32 chain on the widened tables -------------------------------------

def check_exact(eng, wu, wi, rows=None, users=None, ks=(), seen=None, ref_device="cpu", chunk=1 << 16):
    """wu / wi: numpy float16 arrays or fp16 device tensors.  Ranks of `rows` and the top-k lists of `users` for every k
    in ks, exactly as the fp32-chain reference (order="kernel") has them on the widened tables."""
    tu = wu if torch.is_tensor(wu) else gpu(wu)
    ti = wi if torch.is_tensor(wi) else gpu(wi)
    assert tu.dtype == torch.float16 and ti.dtype == torch.float16
    ru = wu if torch.is_tensor(wu) else widen(wu)
    ri = wi if torch.is_tensor(wi) else widen(wi)
    csr = csr_dev(seen)
    if rows is not None:
        got = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
        want = F.ref_full_rank(ru, ri, rows, seen, order="kernel", device=ref_device, chunk=chunk)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, ("rank", len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    if ks:
        want_i, want_s = F.ref_topk(ru, ri, users, max(ks), seen, order="kernel", device=ref_device, chunk=chunk)
        for k in ks:
            items, scores = eng.topk_items(tu, ti, gpu(users), k, csr)
            items, scores = items.cpu().numpy(), scores.cpu().numpy()
            wi_k, ws_k = want_i[:, :k], np.ascontiguousarray(want_s[:, :k])
            bad = np.nonzero((items != wi_k).any(1) | (scores.view(np.int32) != ws_k.view(np.int32)).any(1))[0]
            assert len(bad) == 0, ("topk", k, len(bad), bad[:4], items[bad[:1]], wi_k[bad[:1]])


def check_user_ranks(eng, wu, wi, users, off, items, seen, ks=(1, 5, 20, 128)):
    """above / pos exactly as the per-user reference; above = full_rank of every (u, p); pos = the index of p in u's
    top-128 list; metrics from pos."""
    tu, ti, csr = gpu(wu), gpu(wi), csr_dev(seen)
    out = {k: v.cpu().numpy() for k, v in eng.user_ranks(tu, ti, users, off, items, csr, ks).items()}
    above, pos = ref_user_rank(widen(wu), widen(wi), users, off, items, seen)
    np.testing.assert_array_equal(out["above"], above)
    np.testing.assert_array_equal(out["pos"], pos)
    hits, dcg, ap, first = ref_user_metrics(pos, off, ks)
    np.testing.assert_array_equal(out["hits"], hits)
    np.testing.assert_array_equal(out["first"], first)
    np.testing.assert_allclose(out["dcg"], dcg, rtol=2e-6, atol=0)
    np.testing.assert_allclose(out["ap"], ap, rtol=2e-6, atol=0)
    if len(items):
        rows = np.stack([np.repeat(users, np.diff(off)), items.astype(np.int64)], 1)
        rank = eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy()
        np.testing.assert_array_equal(out["above"], rank)
    k = 128
    lists, _ = eng.topk_items(tu, ti, gpu(users), k, csr)
    lists = lists.cpu().numpy()
    for x in range(len(users)):
        for e in range(off[x], off[x + 1]):
            at = np.nonzero(lists[x] == items[e])[0]
            if 0 <= pos[e] < k:
                assert len(at) == 1 and at[0] == pos[e], (x, e)
            else:
                assert len(at) == 0, (x, e)
    return out


def test_128_exact_on_dyadic_data():
    """Entries k/8: every order of summation is exact, so float64 matmul is the reference as well as the chain."""
    d, U, I, n = 128, 200, 2053, 129
    rng = np.random.RandomState(128)
    wu, wi = dyadic_half(rng, U, d), dyadic_half(rng, I, d)
    rows = np.stack([rng.randint(0, U, size=n), rng.randint(0, I, size=n)], 1).astype(np.int64)
    for r in range(0, n, 7):                                # exact ties with the positive
        for q in rng.choice(I, size=3, replace=False):
            wi[q] = wi[rows[r, 1]]
    seen = F.seen_csr(U, I, {u: rng.choice(I, size=rng.randint(0, 40), replace=False) for u in range(U)})
    users = rng.permutation(U)[:n]
    eng = engine(d)
    check_exact(eng, wu, wi, rows, users, (1, 20, 128), seen)
    S = wu.astype(np.float64) @ wi.astype(np.float64).T
    _, scores = eng.topk_items(gpu(wu), gpu(wi), gpu(users), 20, None)
    want = -np.sort(-S[users], axis=1)[:, :20]
    np.testing.assert_array_equal(scores.cpu().numpy().astype(np.float64), want)


def test_128_exact_on_random_halves():
    c = random_half_case(128, seed=928)
    nan_item = plant_specials(c, c["rng"])
    check_exact(engine(128), c["wu"], c["wi"], c["rows"], c["users"], (1, 20, 128), c["seen"])
    # 161 users: two 128-user groups of k_ur_count<128, half, ..>, every wave of the first with valid users, the second partial
    users, off, items = held_out_sets(c, np.random.RandomState(1), 160, extra=(nan_item, 13))
    assert len(users) == 161
    out = check_user_ranks(engine(128), c["wu"], c["wi"], users, off, items, c["seen"])
    assert (out["pos"] == -1).any() and (np.diff(off) == 0).any()


def test_128_exact_on_planted_near_ties():
    """Exact copies, next-fp16-value copies and rounding-only copies of the positives; k-th entries copied across slices
    (test_half_retrieval_host.py::test_exact_tests_have_teeth_at_128 shows another chain order fails on this data)."""
    c = half_near_tie_case(128, seed=0)
    check_exact(engine(128), c["wu"], c["wi"], c["rows"], c["users"], (1, 20, 128), c["seen"])
    users, off, items = held_out_sets(c, np.random.RandomState(2), 40)
    check_user_ranks(engine(128), c["wu"], c["wi"], users, off, items, c["seen"])


def _sweep_users(rng, U, n):
    users = rng.randint(0, U, size=n)
    if n > 2:
        users[n // 2] = users[0]
        users[-1] = users[1]
    return users


def test_128_every_topk_wave_count():
    """k in {1, 64, 65, 85, 86, 128}: the 4-, 3- and 2-wave blocks of k_topk_slice<128, half, ..>."""
    ks = (1, 64, 65, 85, 86, 128)
    assert {F.topk_waves(k) for k in ks} == {4, 3, 2}
    c = random_half_case(128, seed=929, U=200, I=3001)
    users = _sweep_users(c["rng"], 200, 200)
    check_exact(engine(128), c["wu"], c["wi"], None, users, ks, c["seen"])


@pytest.mark.parametrize("n_item", [1, 31, 32, 33])
def test_128_small_catalogue(n_item):
    """One tile or less (most slices empty), k above n_item, Seen covering all items / all but one."""
    d, U = 128, 40
    rng = np.random.RandomState(1280 + n_item)
    wu = rng.randn(U, d).astype(np.float16)
    wi = rng.randn(n_item, d).astype(np.float16)
    lists = {0: range(n_item), 1: [i for i in range(n_item) if i != n_item // 2], 2: {0, n_item - 1},
             3: {i for i in (31, 32) if i < n_item}}
    seen = F.seen_csr(U, n_item, lists)
    rows = np.stack([np.repeat(np.arange(U), 2)[:70], rng.randint(0, n_item, size=70)], 1).astype(np.int64)
    eng = engine(d)
    check_exact(eng, wu, wi, rows, _sweep_users(rng, U, 40), (1, 2, 33, 128), seen)
    items, _ = eng.topk_items(gpu(wu), gpu(wi), gpu(np.arange(4)), 128, csr_dev(seen))
    items = items.cpu().numpy()
    assert (items[0] == -1).all() and items[1, 0] == n_item // 2 and (items[1, 1:] == -1).all()
    held = [(u, rng.choice(n_item, size=rng.randint(0, n_item + 1), replace=False)) for u in range(U)]
    users, off, its = held_out_csr(U, held)
    for s in (None, seen):
        check_user_ranks(eng, wu, wi, users, off, its, s)


def _slice_edges(slices, slice_tiles, n_item):
    e = set()
    for q in range(slices):
        a, b = q * slice_tiles * 32, min((q + 1) * slice_tiles * 32, n_item)
        if a < b:
            e |= {a, b - 1}
    return e


@pytest.mark.parametrize("n_item,n_rows,n_users,empty_rank,empty_topk", [
    (288, 100, 100, 3, 3),          # 9 tiles over 8 slices: the last 3 empty
    (16411, 40, 3, 1, 1),           # 513 tiles, 32 slices (both kernels), the last one empty, the last tile partial
])
def test_128_slices_and_seen_edges(n_item, n_rows, n_users, empty_rank, empty_topk):
    """Empty trailing slices; Seen on items 0, 31, 32, n_item - 1 and on the first and last item of every slice; a user
    whose Seen is exactly one whole slice (its range starts and ends on slice edges), all items but one, and all items."""
    d, U = 128, 120
    rng = np.random.RandomState(1290 + n_item % 1000)
    rs, rst, rempty = F.rank_plan(n_rows, n_item)
    tw, ts, tst, tempty = F.topk_plan(n_users, 20, n_item)
    assert (rempty, tempty) == (empty_rank, empty_topk)
    wu = rng.randn(U, d).astype(np.float16)
    wi = rng.randn(n_item, d).astype(np.float16)
    edges = {0, 31, 32, n_item - 1} | _slice_edges(rs, rst, n_item) | _slice_edges(ts, tst, n_item)
    lists = {0: edges, 1: range(tst * 32, min(2 * tst * 32, n_item)), 2: range(rst * 32, min(2 * rst * 32, n_item)),
             3: [i for i in range(n_item) if i != n_item - 2], 4: range(n_item)}
    for u in range(5, U):
        lists[u] = rng.choice(n_item, size=min(n_item // 4, 50), replace=False)
    seen = F.seen_csr(U, n_item, lists)
    pos = np.array(sorted(edges))
    pos = rng.permutation(np.concatenate([pos, np.clip(pos + 1, 0, n_item - 1), rng.randint(0, n_item, size=n_rows)]))[:n_rows]
    pos[0] = n_item - 1                     # user 0's positive, inside its own Seen
    rows = np.stack([np.arange(n_rows) % U, pos], 1).astype(np.int64)
    users = np.concatenate([np.arange(min(5, n_users)), rng.randint(0, U, size=max(0, n_users - 5))])
    eng = engine(d)
    check_exact(eng, wu, wi, rows, users, (20, 128), seen)
    items, _ = eng.topk_items(gpu(wu), gpu(wi), gpu(np.arange(5)), 20, csr_dev(seen))
    items = items.cpu().numpy()
    assert (items[4] == -1).all() and items[3, 0] == n_item - 2 and (items[3, 1:] == -1).all()
    assert not (set(items[1].tolist()) & set(lists[1]))
    held = [(u, sorted(edges)[:40]) for u in range(5)] + [(u, rng.choice(n_item, size=6, replace=False)) for u in range(5, 12)]
    us, off, its = held_out_csr(U, held)
    check_user_ranks(eng, wu, wi, us, off, its, seen, ks=(5, 20))


@pytest.mark.parametrize("d", [32, 64, 128])
def test_determinism(d):
    c = random_half_case(d, seed=3000 + d, U=200, I=3000, n=300)
    nan_item = plant_specials(c, c["rng"])
    eng = engine(d)
    tu, ti, csr = gpu(c["wu"]), gpu(c["wi"]), csr_dev(c["seen"])
    rows, users = gpu(c["rows"]), gpu(np.arange(200))
    us, off, items = held_out_sets(c, np.random.RandomState(3), 60, extra=(nan_item,))

    def run():
        out = [eng.full_rank(tu, ti, rows, csr)]
        out += list(eng.topk_items(tu, ti, users, 20, csr))
        ur = eng.user_ranks(tu, ti, us, off, items, csr, (20, 10, 5))
        out += [ur[k] for k in sorted(ur)]
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in out]

    assert run() == run()


def test_item_table_above_2_to_the_31_bytes():
    """d = 128 fp16, 2^23 + 4,099 items (2.15 GB): item rows past 2^31 bytes, near-ties planted at the far end; 64 rank
    rows, the top-20 of 64 users and a few held-out sets, exact through the float64 filter (on the device)."""
    d, U, I = 128, 256, (1 << 23) + 4099
    assert I * d * 2 > (1 << 31) and I > 8388608
    free, _ = torch.cuda.mem_get_info()
    assert free > 16 * (1 << 30), free
    g = torch.Generator(device=DEV)
    g.manual_seed(1310)
    ti = torch.empty(I, d, device=DEV, dtype=torch.float16)
    for c0 in range(0, I, 1 << 21):
        ti[c0:c0 + (1 << 21)] = torch.randn(min(1 << 21, I - c0), d, generator=g, device=DEV).half()
    rng = np.random.RandomState(1310)
    wu = rng.randn(U, d).astype(np.float16)
    n = 64
    far = (1 << 23) + rng.randint(0, 4099, size=n)
    rows = np.stack([rng.randint(0, U, size=n), far], 1).astype(np.int64)
    rows[: n // 2, 1] = rng.randint(0, I, size=n // 2)
    src = torch.from_numpy(rows[:16, 1]).to(DEV)
    dst_far = torch.from_numpy(I - 1 - np.arange(16)).to(DEV)
    dst_near = torch.from_numpy(np.arange(16) * 1000 + 7).to(DEV)
    ti[dst_far] = ti[src]
    bits = ti[src].view(torch.int16)                        # the next fp16 value up: one step in the sign-magnitude bits
    ti[dst_near] = torch.where(bits >= 0, bits + 1, bits - 1).view(torch.float16)
    lists = {u: np.concatenate([[I - 1, I - 17, (1 << 23) + 3], rng.randint(0, I, size=20)]) for u in range(U)}
    seen = F.seen_csr(U, I, lists)
    users = rng.choice(U, size=64, replace=False)
    eng = engine(d)
    tu = gpu(wu)
    check_exact(eng, tu, ti, rows, users, (20,), seen, ref_device=DEV, chunk=1 << 19)
    # held-out sets at the far end: above = the rank of each (u, p), pos = its index in the user's list when inside it
    us = rows[:8, 0]
    order = np.argsort(us, kind="stable")
    held = {}
    for r in order:
        held.setdefault(int(rows[r, 0]), set()).update([int(rows[r, 1]), I - 2, (1 << 23) + 5])
    hu, off, its = held_out_csr(U, held)
    csr = csr_dev(seen)
    out = eng.user_ranks(tu, ti, hu, off, its, csr, (20,))
    prow = np.stack([np.repeat(hu, np.diff(off)), its.astype(np.int64)], 1)
    want = F.ref_full_rank(tu, ti, prow, seen, device=DEV, chunk=1 << 19)
    np.testing.assert_array_equal(out["above"].cpu().numpy(), want)
    li, _ = eng.topk_items(tu, ti, gpu(hu), 20, csr)
    li, pos = li.cpu().numpy(), out["pos"].cpu().numpy()
    for x in range(len(hu)):
        for e in range(off[x], off[x + 1]):
            at = np.nonzero(li[x] == its[e])[0]
            assert (len(at) == 1 and at[0] == pos[e]) if 0 <= pos[e] < 20 else len(at) == 0, (x, e)


def test_model_surface_at_width_128():
    """MFbasemode(...).cuda().half() at laten_factor 128: recommend, test_full, test_model_full and test_model_users
    agree with the engine calls on the same fp16 tables and with the exact reference."""
    from oracle.sml_oracle import eval_metrics
    from sml_amd.evaluation import test_model_full, test_model_users, user_metrics
    from sml_amd.retrieval import SeenItems, held_out
    c = random_half_case(128, seed=931, U=120, I=3000, n=200)
    wu, wi, rows = c["wu"], c["wi"], c["rows"]
    U, I = wu.shape[0], wi.shape[0]
    off, its = c["seen"]
    seen = SeenItems(U, I).add(np.stack([np.repeat(np.arange(U), np.diff(off)), its], 1))
    mf = make_mf(U, I, 128, widen(wu), widen(wi), device=DEV).half()
    assert mf.user_laten.weight.dtype == torch.float16 and mf.hidden_dim == 128
    assert torch.equal(mf.item_laten.weight.data.view(torch.int16), gpu(wi).view(torch.int16))
    eng = engine(128)
    tu, ti, csr = gpu(wu), gpu(wi), csr_dev(c["seen"])
    users = c["users"][:100]
    for k in (1, 20, 128):
        ri, rs = mf.recommend(gpu(users), topK=k, exclude=seen)
        ei, es = eng.topk_items(tu, ti, gpu(users), k, csr)
        assert torch.equal(ri, ei) and torch.equal(rs.view(torch.int32), es.view(torch.int32))
        want_i, want_s = F.ref_topk(widen(wu), widen(wi), users, k, c["seen"])
        np.testing.assert_array_equal(ri.cpu().numpy(), want_i)
        assert rs.cpu().numpy().tobytes() == want_s.tobytes()
    ranks = F.ref_full_rank(widen(wu), widen(wi), rows, c["seen"])
    np.testing.assert_array_equal(eng.full_rank(tu, ti, gpu(rows), csr).cpu().numpy(), ranks)
    for topK in (1, 10, 100):
        hits, ndcg = eval_metrics(torch.from_numpy(ranks), topK)
        h, nd, hit_rows = mf.test_full(gpu(rows), topK=topK, exclude=seen)
        assert h == hits and float(nd) == pytest.approx(ndcg, rel=1e-6, abs=1e-7)
        np.testing.assert_array_equal(hit_rows.cpu().numpy(), np.nonzero(ranks < topK)[0])
        r, nd = test_model_full(mf, [rows[:70], rows[70:]], seen=seen, topK=topK)
        assert r == hits / len(rows) and float(nd) == pytest.approx(ndcg / len(rows), rel=1e-6, abs=1e-7)
    rng = np.random.RandomState(9)
    test = np.stack([rng.randint(0, U, 900), rng.randint(0, I, 900), rng.randint(0, I, 900)], 1)
    got = test_model_users(mf, test, seen=seen, topK=(20, 10, 5))
    sets = held_out(test, U, I)
    out = mf.test_users(sets, topK=(20, 10, 5), exclude=seen)
    hu, hoff, hitems = out["users"], out["pos_off"], out["pos_items"]
    eo = eng.user_ranks(tu, ti, hu, hoff, hitems, csr, (20, 10, 5))
    for key in ("above", "pos", "hits", "dcg", "ap", "first"):
        assert out[key].cpu().numpy().tobytes() == eo[key].cpu().numpy().tobytes(), key
    above, pos = ref_user_rank(widen(wu), widen(wi), hu, hoff, hitems, c["seen"])
    np.testing.assert_array_equal(out["pos"].cpu().numpy(), pos)
    np.testing.assert_array_equal(out["above"].cpu().numpy(), above)
    hits, dcg, ap, first = ref_user_metrics(pos, hoff, (20, 10, 5))
    want = user_metrics(dict(users=hu, pos_off=hoff, pos_items=hitems, ks=(20, 10, 5), pos=pos, hits=hits, dcg=dcg, ap=ap,
                             first=first))
    for key in ("recall", "precision", "ndcg", "ndcg_ref", "map", "mrr"):
        for K in (20, 10, 5):
            assert got[key][K] == pytest.approx(want[key][K], rel=1e-5), (key, K)


def test_refusals():
    from sml_amd._lib import SmlError
    rows = torch.zeros(1, 2, dtype=torch.int64, device=DEV)
    users = torch.zeros(1, dtype=torch.int64, device=DEV)
    one = (np.array([0, 1]), torch.zeros(1, dtype=torch.int32, device=DEV))

    def tables(d, dt_u, dt_i):
        return torch.zeros(10, d, device=DEV, dtype=dt_u), torch.zeros(20, d, device=DEV, dtype=dt_i)

    for dt_u, dt_i in ((torch.float16, torch.float32), (torch.float32, torch.float16)):      # a mixed pair
        eng = engine(32)
        tu, ti = tables(32, dt_u, dt_i)
        with pytest.raises(ValueError):
            eng.full_rank(tu, ti, rows)
        with pytest.raises(ValueError):
            eng.topk_items(tu, ti, users, 5)
        with pytest.raises(ValueError):
            eng.user_ranks(tu, ti, users, *one)
    with pytest.raises(ValueError):
        engine(32).full_rank(*tables(32, torch.bfloat16, torch.bfloat16), rows)
    for d in (16, 256):         # a width without kernels: sml_ctx_create refuses it, so no engine exists to call retrieval on
        with pytest.raises(SmlError):
            engine(d)
    e128 = engine(128)                                                                       # fp32 at d = 128: as before
    tu, ti = tables(128, torch.float32, torch.float32)
    with pytest.raises(SmlError):
        e128.full_rank(tu, ti, rows)
    with pytest.raises(SmlError):
        e128.topk_items(tu, ti, users, 5)
    with pytest.raises(SmlError):
        e128.user_ranks(tu, ti, users, *one)
    hu, hi = tables(128, torch.float16, torch.float16)                                       # and fp16 at d = 128 runs
    assert e128.full_rank(hu, hi, rows).cpu().tolist() == [0]
    for k in (0, 129):
        with pytest.raises(SmlError):
            e128.topk_items(hu, hi, users, k)
    lib = e128.lib
    rank = torch.empty(1, dtype=torch.int32, device=DEV)
    off = torch.zeros(11, dtype=torch.int64, device=DEV)
    args = lambda n_item, n_cols, so, si: (e128._ctx, hu.data_ptr(), hi.data_ptr(), n_item, rows.data_ptr(), 1, n_cols,  # noqa: E731
                                           so, si, rank.data_ptr(), None)
    assert lib.sml_full_rank_f16(*args(20, 2, off.data_ptr(), None)) != 0      # exactly one of the CSR arrays
    assert lib.sml_full_rank_f16(*args(20, 1, None, None)) != 0                # n_cols < 2
    assert lib.sml_full_rank_f16(*args(0, 2, None, None)) != 0                 # n_item <= 0
    assert lib.sml_full_rank_f16(*args(1 << 31, 2, None, None)) != 0           # n_item >= 2^31
    assert lib.sml_full_rank_f16(*args(20, 2, None, None)) == 0
