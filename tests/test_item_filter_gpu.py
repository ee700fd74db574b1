"""The item filter of full-catalogue retrieval on the MI355X (sml_*_filtered through HipEngine, MFbasemode and
sml_amd.evaluation).

The oracle is the contract of include/sml_hip.h: a filtered call equals, byte for byte, the unfiltered call with
Seen'(u) = Seen(u) + ([0, n_item) - A) for every user (tests/_item_filter_cases.py builds Seen' on the host).  One case
per element type is also compared with the exact CPU references of the fp32 chain."""
import numpy as np
import pytest
import torch

import _fp32_chain as F
from _half_cases import half_near_tie_case, random_half_case, widen
from _item_filter_cases import near_tie_mask, pack, random_mask, seen_prime
from _user_rank_ref import held_out_csr, ref_user_metrics, ref_user_rank
from conftest import make_mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (20, 10, 5)


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(seen):
    return None if seen is None else (gpu(seen[0]), gpu(seen[1]))


def words_dev(words):
    return gpu(np.asarray(words, dtype=np.uint32).view(np.int32))


def same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    v = (lambda t: t.view(torch.int32)) if a.dtype == torch.float32 else (lambda t: t)
    assert torch.equal(v(a), v(b)), what


def held_sets(c, rng, n_users, extra=()):
    """Held-out sets for n_users of the case's users: sizes 0, 1, 4, 30 in turn, the rows' positives, some Seen items and
    the items of `extra` for every third user."""
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    off, items = c["seen"]
    rows = c["rows"]
    lists = []
    for x, u in enumerate(rng.choice(U, size=min(U, n_users), replace=False)):
        it = set(rows[rows[:, 0] == u, 1].tolist())
        it.update(rng.choice(I, size=min(I, [0, 1, 4, 30][x % 4]), replace=False).tolist())
        s = items[off[u]:off[u + 1]]
        if len(s) and x % 4 == 1:
            it.update(s[:3].tolist())
        if x % 3 == 2:
            it.update(extra)
        lists.append((int(u), it))
    return held_out_csr(U, lists)


def run_all(eng, tu, ti, rows, users, held, seen, allow, ks=(1, 20, 128)):
    """Every output of the three calls, as a flat dict of device tensors."""
    out = {"rank": eng.full_rank(tu, ti, rows, seen, allow=allow)}
    for k in ks:
        out["items%d" % k], out["scores%d" % k] = eng.topk_items(tu, ti, users, k, seen, allow=allow)
    if held is not None:
        ur = eng.user_ranks(tu, ti, held[0], held[1], held[2], seen, KS, allow=allow)
        out.update(("ur_" + k, v) for k, v in ur.items())
    return out


def check_identity(eng, tu, ti, c, mask, held, seen="case", words=None, ks=(1, 20, 128), rows=None, users=None):
    """Filtered (the mask's words, or `words` given by hand) against unfiltered with Seen'.  Returns the filtered outputs."""
    U = tu.shape[0]
    seen = c["seen"] if isinstance(seen, str) else seen
    rows = gpu(c["rows"] if rows is None else rows)
    users = gpu(c["users"] if users is None else users)
    allow = words_dev(pack(mask) if words is None else words)
    got = run_all(eng, tu, ti, rows, users, held, csr_dev(seen), allow, ks)
    want = run_all(eng, tu, ti, rows, users, held, csr_dev(seen_prime(seen, mask, U)), None, ks)
    for key in want:
        same_bytes(got[key], want[key], key)
    for k in ks:
        it = got["items%d" % k].cpu().numpy()
        assert np.asarray(mask)[it[it >= 0]].all()
    return got


def tables(c):
    return gpu(c["wu"]), gpu(c["wi"])


# ---- identity on random cases ------------------------------------------------------------------------------------------

CASES = [("fp32", 32), ("fp32", 64), ("fp16", 32), ("fp16", 64), ("fp16", 128)]


def make_case(dtype, d, seed=0):
    return F.random_case(d, seed) if dtype == "fp32" else random_half_case(d, seed)


@pytest.mark.parametrize("keep", [0.5, 0.05])
@pytest.mark.parametrize("dtype,d", CASES)
def test_filtered_equals_unfiltered_with_seen_prime(dtype, d, keep):
    """random_case / random_half_case: U = 300, I = 4,099 (a 3-bit last word), n = 256."""
    c = make_case(dtype, d, seed=7 * d + (1 if keep < 0.1 else 0))
    assert c["wi"].shape[0] == 4099 and c["wu"].shape[0] == 300 and len(c["rows"]) == 256
    mask = random_mask(4099, keep, seed=d)
    assert abs(mask.mean() - keep) < 0.03 and (~mask[c["rows"][:, 1]]).any()        # some positives are not allowed
    tu, ti = tables(c)
    held = held_sets(c, c["rng"], 120)
    assert (~mask[held[2]]).any() and mask[held[2]].any()
    got = check_identity(engine(d), tu, ti, c, mask, held)
    assert (got["ur_pos"].cpu().numpy()[~mask[held[2]]] == -1).all()
    if dtype == "fp16" and d != 128:        # fp16 against fp32 on .float() copies: the filtered calls agree bit for bit too
        rows, users, seen = gpu(c["rows"]), gpu(c["users"]), csr_dev(c["seen"])
        f32 = run_all(engine(d), tu.float(), ti.float(), rows, users, held, seen, words_dev(pack(mask)))
        for key in f32:
            same_bytes(got[key], f32[key], key)


@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp16", 128)])
def test_against_the_cpu_chain_references(dtype, d):
    """One case per element type: ranks, lists with score bits, above / pos and the metrics against the exact CPU
    references run with Seen'."""
    c = make_case(dtype, d, seed=91)
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    mask = random_mask(I, 0.5, seed=92)
    sp = seen_prime(c["seen"], mask, U)
    ru, ri = (c["wu"], c["wi"]) if dtype == "fp32" else (widen(c["wu"]), widen(c["wi"]))
    tu, ti = tables(c)
    eng, allow, seen = engine(d), words_dev(pack(mask)), csr_dev(c["seen"])
    rows, users = c["rows"][:128], c["users"][:64]
    got = eng.full_rank(tu, ti, gpu(rows), seen, allow=allow).cpu().numpy()
    np.testing.assert_array_equal(got, F.ref_full_rank(ru, ri, rows, sp))
    want_i, want_s = F.ref_topk(ru, ri, users, 20, sp)
    it, sc = eng.topk_items(tu, ti, gpu(users), 20, seen, allow=allow)
    np.testing.assert_array_equal(it.cpu().numpy(), want_i)
    np.testing.assert_array_equal(sc.cpu().numpy().view(np.int32), want_s.view(np.int32))
    hu, hoff, hit = held_sets(c, c["rng"], 24)
    out = {k: v.cpu().numpy() for k, v in eng.user_ranks(tu, ti, hu, hoff, hit, seen, KS, allow=allow).items()}
    above, pos = ref_user_rank(ru, ri, hu, hoff, hit, sp)
    np.testing.assert_array_equal(out["above"], above)
    np.testing.assert_array_equal(out["pos"], pos)
    hits, dcg, ap, first = ref_user_metrics(pos, hoff, KS)
    np.testing.assert_array_equal(out["hits"], hits)
    np.testing.assert_array_equal(out["first"], first)
    np.testing.assert_allclose(out["dcg"], dcg, rtol=2e-6, atol=0)
    np.testing.assert_allclose(out["ap"], ap, rtol=2e-6, atol=0)


# ---- near-ties ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp32", 64), ("fp16", 128)])
def test_near_ties(dtype, d):
    """The planted positives, their copies and their rounding-only neighbours stay; every third other item goes."""
    c = F.near_tie_case(d, seed=0) if dtype == "fp32" else half_near_tie_case(d, seed=0)
    mask = near_tie_mask(c)
    I = c["wi"].shape[0]
    assert mask[c["planted"][:, 1]].all() and 0.6 < mask.mean() < 0.8
    assert (~mask[(c["planted"][:, 1] + 1) % I]).any()                  # id neighbours of planted items are removed
    tu, ti = tables(c)
    check_identity(engine(d), tu, ti, c, mask, held_sets(c, c["rng"], 60))
    # and the references agree where they are cheap: the planted rows' ranks
    ru, ri = (c["wu"], c["wi"]) if dtype == "fp32" else (widen(c["wu"]), widen(c["wi"]))
    rows = c["planted"]
    got = engine(d).full_rank(tu, ti, gpu(rows), csr_dev(c["seen"]), allow=words_dev(pack(mask))).cpu().numpy()
    np.testing.assert_array_equal(got, F.ref_full_rank(ru, ri, rows, seen_prime(c["seen"], mask, tu.shape[0])))


# ---- filter edges ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[("fp32", 32), ("fp16", 128)], ids=["fp32-32", "fp16-128"])
def edge(request):
    dtype, d = request.param
    c = F.random_case(d, 3, U=100, I=4099, n=96) if dtype == "fp32" else random_half_case(d, 3, U=100, I=4099, n=96)
    tu, ti = tables(c)
    return dict(c=c, d=d, tu=tu, ti=ti, held=held_sets(c, np.random.RandomState(5), 40))


def edge_identity(e, mask, **kw):
    return check_identity(engine(e["d"]), e["tu"], e["ti"], e["c"], mask, e["held"], **kw)


def test_all_allowed_equals_no_filter(edge):
    e, c = edge, edge["c"]
    eng, seen = engine(e["d"]), csr_dev(c["seen"])
    rows, users = gpu(c["rows"]), gpu(c["users"])
    none = run_all(eng, e["tu"], e["ti"], rows, users, e["held"], seen, None)
    full = run_all(eng, e["tu"], e["ti"], rows, users, e["held"], seen, words_dev(pack(np.ones(4099, bool))))
    for key in none:
        same_bytes(full[key], none[key], key)
    ones = run_all(eng, e["tu"], e["ti"], rows, users, e["held"], seen, words_dev(np.full(129, 0xFFFFFFFF, np.uint32)))
    for key in none:
        same_bytes(ones[key], none[key], key)


def test_nothing_allowed(edge):
    got = edge_identity(edge, np.zeros(4099, bool))
    assert not got["rank"].any()
    for k in (1, 20, 128):
        assert (got["items%d" % k] == -1).all() and torch.isneginf(got["scores%d" % k]).all()
    assert (got["ur_pos"] == -1).all() and not got["ur_above"].any()
    assert not got["ur_hits"].any() and (got["ur_first"] == -1).all()


@pytest.mark.parametrize("item", [0, 2077, 4098])
def test_exactly_one_item_allowed(edge, item):
    mask = np.zeros(4099, bool)
    mask[item] = True
    got = edge_identity(edge, mask)
    it = got["items20"].cpu().numpy()
    assert set(np.unique(it).tolist()) <= {-1, item} and (it[:, 1:] == -1).all() and (it[:, 0] == item).any()
    assert int(got["rank"].max()) <= 1


def test_only_the_last_partial_word(edge):
    mask = np.zeros(4099, bool)
    mask[4096:] = True
    got = edge_identity(edge, mask)
    it = got["items128"].cpu().numpy()
    assert (it[:, 3:] == -1).all() and (it[:, :3] >= 4096).any()


def test_set_bits_past_n_item_change_nothing(edge):
    mask = random_mask(4099, 0.5, seed=8)
    words = pack(mask)
    assert words[-1] >> 3 == 0
    words[-1] |= np.uint32(0xFFFFFFF8)                        # by hand: ItemFilter never writes these
    edge_identity(edge, mask, words=words)
    none = np.zeros(129, np.uint32)
    none[-1] = 0xFFFFFFF8                                     # only tail bits: nothing is allowed
    got = edge_identity(edge, np.zeros(4099, bool), words=none)
    assert (got["items20"] == -1).all() and not got["rank"].any()


@pytest.mark.parametrize("pattern", ["alternating", "alternating_odd", "bit0_bit31"])
def test_word_patterns(edge, pattern):
    words = np.zeros(129, np.uint32)
    if pattern == "alternating":
        words[1::2] = 0xFFFFFFFF                              # 0x00000000 / 0xFFFFFFFF: every other tile is skipped
    elif pattern == "alternating_odd":
        words[0::2] = 0xFFFFFFFF
    else:
        words[:] = 0x80000001
    mask = np.unpackbits(words.view(np.uint8), bitorder="little")[:4099].astype(bool)
    edge_identity(edge, mask, words=words)


def test_fewer_than_k_allowed_pads(edge):
    mask = np.zeros(4099, bool)
    mask[np.random.RandomState(4).choice(4099, 10, replace=False)] = True
    got = edge_identity(edge, mask, ks=(20, 128))
    it, sc = got["items20"].cpu().numpy(), got["scores20"].cpu().numpy()
    assert (it[:, 10:] == -1).all() and np.isneginf(sc[:, 10:]).all() and (it[:, 0] >= 0).all()


# ---- skipped tiles and the Seen cursor ---------------------------------------------------------------------------------

def skip_filter(n_item, slice_tiles, slices, rng):
    """Per tile: slice 0 empty; slice 1 loses its first 10 tiles; slice 2 its last 10; slice 3 keeps tiles 5 and 18 only
    (isolated tiles between long empty runs); slice 4 keeps one bit in its last tile; the rest is random per item, with
    runs of empty tiles."""
    n_tiles = (n_item + 31) // 32
    tile_on = np.ones(n_tiles, bool)
    s = lambda q: slice(q * slice_tiles, (q + 1) * slice_tiles)        # noqa: E731
    tile_on[s(0)] = False
    tile_on[1 * slice_tiles:1 * slice_tiles + 10] = False
    tile_on[3 * slice_tiles - 10:3 * slice_tiles] = False
    tile_on[s(3)] = False
    tile_on[[3 * slice_tiles + 5, 3 * slice_tiles + 18]] = True
    tile_on[s(4)] = False
    mask = np.repeat(tile_on, 32)[:n_item] & (rng.rand(n_item) < 0.7)
    mask[(5 * slice_tiles - 1) * 32 + 17] = True
    for q in range(5, slices):                                         # random empty runs in the other slices
        a = q * slice_tiles + rng.randint(0, slice_tiles - 4)
        mask[a * 32:(a + rng.randint(1, 4)) * 32] = False
    mask[(3 * slice_tiles + 5) * 32:(3 * slice_tiles + 6) * 32] = True  # one isolated tile fully allowed
    return mask, tile_on


@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp32", 64), ("fp16", 128)])
def test_skipped_tiles_and_seen_cursor(dtype, d):
    U, I, n = 70, 32 * 8 * 24 + 5, 64
    slices, slice_tiles, _ = F.rank_plan(n, I)
    for k in (1, 20):
        w, s2, st2, _ = F.topk_plan(n, k, I)
        assert (s2, st2) == (slices, slice_tiles)
    s3, st3 = F.plan_slices((n + 127) // 128, I, 8192, 64)               # k_ur_count: the rank grid at 4 waves
    assert slices >= 2 and slices == 8 and slice_tiles == 25 and (s3, st3) == (slices, slice_tiles)
    c = F.random_case(d, 17, U=U, I=I, n=n) if dtype == "fp32" else random_half_case(d, 17, U=U, I=I, n=n)
    rng = np.random.RandomState(18)
    mask, tile_on = skip_filter(I, slice_tiles, slices, rng)
    # Seen: inside the skipped runs, directly before an allowed tile, at its first and last item, directly after it
    t_a, t_b = 3 * slice_tiles + 5, 3 * slice_tiles + 18
    marks = []
    for t in (t_a, t_b, slice_tiles + 10, 5 * slice_tiles - 1):
        marks += [t * 32 - 40, t * 32 - 1, t * 32, t * 32 + 31, t * 32 + 32, t * 32 + 70]
    marks += [0, 5, 31, 32, slice_tiles * 32 - 1, (3 * slice_tiles + 10) * 32 + 3, (4 * slice_tiles + 3) * 32, I - 1]
    off, items = c["seen"]
    lists = {}
    for u in range(U):
        own = set(items[off[u]:off[u + 1]].tolist())
        if u % 4 != 3:
            own.update(m for q, m in enumerate(marks) if (q + u) % 3 != 0 or u % 4 == 0)
        if u % 5 == 0:                                                  # a long run of Seen items across skipped tiles
            own.update(range(t_a * 32 - 200, t_a * 32 + 40))
        lists[u] = own
    c["seen"] = F.seen_csr(U, I, lists)
    assert not tile_on[(t_a * 32 - 1) // 32] and not tile_on[(t_a * 32 + 32) // 32] and mask[t_a * 32]
    tu, ti = tables(c)
    held = held_sets(c, rng, 40, extra=(t_a * 32, t_a * 32 - 1, t_b * 32 + 31, I - 1))
    check_identity(engine(d), tu, ti, c, mask, held, ks=(1, 20))
    check_identity(engine(d), tu, ti, c, mask, held, seen=None, ks=(20,))


@pytest.mark.parametrize("n_item", [1, 31, 33])
@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp16", 128)])
def test_catalogues_around_one_tile(dtype, d, n_item):
    rng = np.random.RandomState(100 + n_item)
    U = 40
    wu = rng.randn(U, d).astype(np.float32 if dtype == "fp32" else np.float16)
    wi = rng.randn(n_item, d).astype(wu.dtype)
    rows = np.stack([rng.randint(0, U, 40), rng.randint(0, n_item, 40)], 1).astype(np.int64)
    seen = F.seen_csr(U, n_item, {u: rng.choice(n_item, size=rng.randint(0, min(n_item, 6) + 1), replace=False) for u in range(U)})
    c = dict(wu=wu, wi=wi, rows=rows, users=np.arange(U), seen=seen)
    held = held_out_csr(U, [(u, rng.choice(n_item, size=min(n_item, 3), replace=False)) for u in range(0, U, 2)])
    tu, ti = tables(c)
    masks = [np.ones(n_item, bool), np.zeros(n_item, bool), rng.rand(n_item) < 0.5]
    if n_item > 1:
        last = np.zeros(n_item, bool)
        last[-1] = True
        masks.append(last)
    for mask in masks:
        check_identity(engine(d), tu, ti, c, mask, held, ks=(1, 20))


# ---- disallowed positives ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 64), ("fp16", 128)])
def test_disallowed_positives(dtype, d):
    c = make_case(dtype, d, seed=41)
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    mask = random_mask(I, 0.5, seed=42)
    rows = c["rows"][:96].copy()
    mask[rows[:48, 1]] = False                                          # half of the positives are not allowed
    mask[rows[48:, 1]] = True
    off, items = c["seen"]
    tu, ti = tables(c)
    ru, ri = (c["wu"], c["wi"]) if dtype == "fp32" else (widen(c["wu"]), widen(c["wi"]))
    eng, allow, seen = engine(d), words_dev(pack(mask)), csr_dev(c["seen"])
    # full_rank: p is never excluded; its rank counts the allowed, unseen items above it -- by the plain definition
    got = eng.full_rank(tu, ti, gpu(rows), seen, allow=allow).cpu().numpy()
    S = F.score_chain(ru[rows[:, 0]], ri)
    for r, (u, p) in enumerate(rows):
        ok = mask.copy()
        ok[items[off[u]:off[u + 1]]] = False
        ok[p] = False
        assert got[r] == int((S[r][ok] > S[r, p]).sum()), r
    assert got[:48].any()
    # user_ranks: a held-out item that is not allowed has pos -1; the user's other entries are what they are without it
    rng = np.random.RandomState(43)
    lists_a, lists_b = [], []
    for u in rng.choice(U, 30, replace=False):
        it = rng.choice(I, 12, replace=False)
        lists_a.append((int(u), it))
        lists_b.append((int(u), it[mask[it]]))
    ha, hb = held_out_csr(U, lists_a), held_out_csr(U, lists_b)
    oa = eng.user_ranks(tu, ti, ha[0], ha[1], ha[2], seen, KS, allow=allow)
    ob = eng.user_ranks(tu, ti, hb[0], hb[1], hb[2], seen, KS, allow=allow)
    keep = gpu(mask[ha[2]])
    assert (~mask[ha[2]]).sum() > 50 and (oa["pos"][~keep] == -1).all()
    same_bytes(oa["pos"][keep], ob["pos"], "pos of the allowed entries")
    same_bytes(oa["above"][keep], ob["above"], "above of the allowed entries")
    for key in ("hits", "dcg", "ap", "first"):
        same_bytes(oa[key], ob[key], key)
    check_identity(eng, tu, ti, c, mask, ha, rows=rows, ks=(20,))


# ---- large held-out sets -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 32), ("fp16", 128)])
def test_large_held_out_set_under_a_filter(dtype, d):
    """One user with 90 held-out items (about 45 allowed: more than the 32 thresholds kept in LDS, the global-memory path
    of k_ur_count) among users with short sets, under a 50 % filter."""
    c = make_case(dtype, d, seed=51)
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    mask = random_mask(I, 0.5, seed=52)
    rng = np.random.RandomState(53)
    big = rng.choice(I, 90, replace=False)
    off, items = c["seen"]
    u_big = 11
    n_live = int((mask[big] & ~np.isin(big, items[off[u_big]:off[u_big + 1]])).sum())
    assert n_live > 32
    lists = [(3, rng.choice(I, 5, replace=False)), (u_big, big), (20, rng.choice(I, 2, replace=False)),
             (21, np.nonzero(mask)[0][:40])]                            # 40 allowed items: all thresholds live
    held = held_out_csr(U, lists)
    tu, ti = tables(c)
    got = check_identity(engine(d), tu, ti, c, mask, held, ks=(20,))
    ru, ri = (c["wu"], c["wi"]) if dtype == "fp32" else (widen(c["wu"]), widen(c["wi"]))
    above, pos = ref_user_rank(ru, ri, held[0], held[1], held[2], seen_prime(c["seen"], mask, U))
    np.testing.assert_array_equal(got["ur_above"].cpu().numpy(), above)
    np.testing.assert_array_equal(got["ur_pos"].cpu().numpy(), pos)


# ---- the device builder ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_item", [4099, 64, 1])
def test_filter_from_ids_matches_numpy(n_item):
    eng = engine(32)
    rng = np.random.RandomState(n_item)
    ids = rng.randint(0, n_item, size=3 * n_item // 4 + 1)
    ids = np.concatenate([ids, ids[:50], [n_item - 1, 0]])               # duplicates, both ends
    for arr in (ids, np.zeros(0, np.int64), np.arange(n_item)):
        for invert in (False, True):
            mask = np.zeros(n_item, bool)
            mask[arr] = True
            want = pack(~mask if invert else mask)
            got = eng.item_filter_from_ids(gpu(arr.astype(np.int32)), n_item, invert=invert)
            assert got.dtype == torch.int32 and got.device.type == "cuda"
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want)
            again = eng.item_filter_from_ids(arr[::-1].copy(), n_item, invert=invert)      # a host array, another order
            assert torch.equal(got, again)
    for bad in ([-1], [n_item], [0, n_item + 5]):
        with pytest.raises(ValueError):
            eng.item_filter_from_ids(np.array(bad), n_item)


def test_device_built_filter_gives_the_same_bytes():
    from sml_amd.retrieval import ItemFilter, as_filter
    d = 64
    c = F.random_case(d, 61, U=100, I=4099, n=96)
    eng = engine(d)
    tu, ti = tables(c)
    rng = np.random.RandomState(62)
    ids = rng.choice(4099, 700, replace=False)
    held = held_sets(c, rng, 30)
    rows, users, seen = gpu(c["rows"]), gpu(c["users"]), csr_dev(c["seen"])
    for invert in (False, True):
        f = ItemFilter(4099)
        if invert:
            f.allow(np.arange(4099)).deny(ids)
        else:
            f.allow(ids)
        assert len(f) == (4099 - 700 if invert else 700)
        built = eng.item_filter_from_ids(ids, 4099, invert=invert)
        up = as_filter(f, 4099, DEV)
        assert torch.equal(built, up)
        a = run_all(eng, tu, ti, rows, users, held, seen, built, ks=(20,))
        b = run_all(eng, tu, ti, rows, users, held, seen, f, ks=(20,))                     # the engine takes an ItemFilter too
        m = run_all(eng, tu, ti, rows, users, held, seen, f.mask(), ks=(20,))              # and a bool mask
        for key in a:
            same_bytes(a[key], b[key], key)
            same_bytes(a[key], m[key], key)
        check_identity(eng, tu, ti, c, f.mask(), held, ks=(20,))


# ---- model surface -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d", [("fp32", 64), ("fp16", 128)])
def test_model_surface(dtype, d):
    from sml_amd.evaluation import test_model_full, test_model_users, user_metrics
    from sml_amd.retrieval import ItemFilter, SeenItems, held_out
    c = F.random_case(d, 71, U=120, I=3001, n=200) if dtype == "fp32" else random_half_case(d, 71, U=120, I=3001, n=200)
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    off, its = c["seen"]
    seen = SeenItems(U, I).add(np.stack([np.repeat(np.arange(U), np.diff(off)), its], 1))
    mask = random_mask(I, 0.3, seed=72)
    flt = ItemFilter.from_mask(mask)
    sp = seen_prime(c["seen"], mask, U)
    seen_p = SeenItems(U, I).add(np.stack([np.repeat(np.arange(U), np.diff(sp[0])), sp[1]], 1))
    mf = make_mf(U, I, d, widen(c["wu"]) if dtype == "fp16" else c["wu"], widen(c["wi"]) if dtype == "fp16" else c["wi"], device=DEV)
    if dtype == "fp16":
        mf = mf.half()
    eng = engine(d)
    tu, ti = mf.user_laten.weight.data, mf.item_laten.weight.data
    assert tu.dtype == (torch.float16 if dtype == "fp16" else torch.float32)
    users, rows = gpu(c["users"][:100]), gpu(c["rows"])
    csr, csr_p = seen.device(DEV), seen_p.device(DEV)
    for k in (1, 20):
        ri, rs = mf.recommend(users, topK=k, exclude=seen, items=flt)
        ei, es = eng.topk_items(tu, ti, users, k, csr_p)
        assert torch.equal(ri, ei) and torch.equal(rs.view(torch.int32), es.view(torch.int32))
        ni, ns = mf.recommend(users, topK=k, exclude=seen, items=None)          # items=None: what the call did before
        pi, ps = eng.topk_items(tu, ti, users, k, csr)
        assert torch.equal(ni, pi) and torch.equal(ns.view(torch.int32), ps.view(torch.int32))
        mi, _ = mf.recommend(users, topK=k, exclude=seen, items=mask)           # a bool mask is a filter too
        assert torch.equal(mi, ei)
    ranks = eng.full_rank(tu, ti, rows, csr_p)
    for topK in (1, 10, 100):
        h, nd, hit_rows = mf.test_full(rows, topK=topK, exclude=seen, items=flt)
        h2, nd2, hit_rows2 = mf.test_full(rows, topK=topK, exclude=seen_p)
        assert h == h2 and float(nd) == float(nd2) and torch.equal(hit_rows, hit_rows2)
        assert torch.equal(hit_rows, (ranks < topK).nonzero()[:, 0])
        a = test_model_full(mf, [c["rows"][:70], c["rows"][70:]], seen=seen, topK=topK, items=flt)
        b = test_model_full(mf, [c["rows"][:70], c["rows"][70:]], seen=seen_p, topK=topK)
        assert a[0] == b[0] and float(a[1]) == float(b[1])
        n0 = test_model_full(mf, c["rows"], seen=seen, topK=topK, items=None)
        p0 = test_model_full(mf, c["rows"], seen=seen, topK=topK)
        assert n0[0] == p0[0] and float(n0[1]) == float(p0[1])
    assert torch.equal(eng.full_rank(tu, ti, rows, csr, allow=flt), ranks)
    rng = np.random.RandomState(9)
    test = np.stack([rng.randint(0, U, 900), rng.randint(0, I, 900), rng.randint(0, I, 900)], 1)
    sets = held_out(test, U, I)
    out = mf.test_users(sets, topK=KS, exclude=seen, items=flt)
    ref = mf.test_users(sets, topK=KS, exclude=seen_p)
    eo = eng.user_ranks(tu, ti, out["users"], out["pos_off"], out["pos_items"], csr_p, KS)
    for key in ("above", "pos", "hits", "dcg", "ap", "first"):
        same_bytes(out[key], ref[key], key)
        same_bytes(out[key], eo[key], key)
    assert (out["pos"].cpu().numpy()[~mask[out["pos_items"]]] == -1).all()
    got = test_model_users(mf, test, seen=seen, topK=KS, items=flt)
    assert got == test_model_users(mf, test, seen=seen_p, topK=KS) == user_metrics(out)
    assert test_model_users(mf, test, seen=seen, topK=KS, items=None) == test_model_users(mf, test, seen=seen, topK=KS)
    plain = mf.test_users(sets, topK=KS, exclude=seen, items=None)
    eo0 = eng.user_ranks(tu, ti, plain["users"], plain["pos_off"], plain["pos_items"], csr, KS)
    for key in ("above", "pos", "hits", "dcg", "ap", "first"):
        same_bytes(plain[key], eo0[key], key)
