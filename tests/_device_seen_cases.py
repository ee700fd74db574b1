"""Cases and the numpy reference of the device interaction sets (sml_iset_*, sml_amd.retrieval.DeviceSeen).

The reference shares no code with SeenItems: np.unique over the key u * n_item + i, then the offsets by searchsorted on the
users.  tests/test_device_seen_host.py pins it against SeenItems.host() on every case; the GPU tests compare the device
results with it byte for byte."""
import numpy as np

# sizes on both sides of every block or tile edge of interaction_set.hip: the wavefront (64), the workgroup (256), the sort
# and scan tile (4096 = IS_TILE, 16 consecutive entries per lane in the scan); 70,001 needs 18 tiles and more than 256
# workgroups of 256
M_EDGES = (63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70001)
# further edges of the implementation: one scan lane's 16 entries, two tiles, and 256 tiles + 1 (the second trip of the
# loops over tile sums in k_is_scan / k_is_scan_sums)
M_EXTRA = (15, 16, 17, 8191, 8192, 8193, 256 * 4096 + 1)


def ref_set(pairs_list, n_user, n_item):
    """(off int64 [n_user + 1], items int32 [nnz]) of the union of the (user, item) columns of every array in pairs_list."""
    keys = [np.zeros(0, np.int64)]
    for p in pairs_list:
        p = np.asarray(p)
        if p.size:
            keys.append(p[:, 0].astype(np.int64) * n_item + p[:, 1].astype(np.int64))
    k = np.unique(np.concatenate(keys))
    users = k // n_item
    off = np.searchsorted(users, np.arange(n_user + 1, dtype=np.int64), side="left").astype(np.int64)
    return off, (k % n_item).astype(np.int32)


def ref_contains(set_pairs, n_item, probe):
    key = lambda p: np.asarray(p)[:, 0].astype(np.int64) * n_item + np.asarray(p)[:, 1].astype(np.int64)   # noqa: E731
    return np.isin(key(probe), key(set_pairs)) if len(set_pairs) else np.zeros(len(probe), bool)


def _pairs(u, i):
    return np.stack([np.asarray(u, np.int64), np.asarray(i, np.int64)], 1)


def random_pairs(rng, n_user, n_item, m):
    return _pairs(rng.randint(0, n_user, m), rng.randint(0, n_item, m))


def build_cases():
    """[(name, n_user, n_item, pairs int64 [m, >= 2])]: one add each."""
    rng = np.random.RandomState(1234)
    out = [("m0", 7, 9, np.zeros((0, 2), np.int64)),
           ("one_pair", 7, 9, _pairs([3], [8])),
           ("1x1_1000_copies", 1, 1, np.zeros((1000, 2), np.int64)),
           ("70x100_mostly_dups", 70, 100, random_pairs(rng, 70, 100, 150)[rng.randint(0, 150, 1000)])]
    p = random_pairs(rng, 48, 100, 600) + np.array([1, 0])            # users 1 .. 48 of 50: 0 and 49 absent
    out.append(("ends_absent", 50, 100, p))
    out.append(("ends_present", 50, 100, np.concatenate([p, _pairs([0, 49, 0, 49], [0, 99, 99, 0])])))
    out.append(("one_user_5000_items", 9, 6000, _pairs(np.full(5000, 4), rng.permutation(6000)[:5000])))
    out.append(("one_item_5000_users", 6000, 9, _pairs(rng.permutation(6000)[:5000], np.full(5000, 4))))
    p = random_pairs(rng, 300, 500, 3000)
    order = np.lexsort((p[:, 1], p[:, 0]))
    out.append(("sorted", 300, 500, p[order]))
    out.append(("reverse_sorted", 300, 500, p[order[::-1]]))
    out.append(("shuffled", 300, 500, p[rng.permutation(3000)]))
    out.append(("five_columns", 300, 500, np.concatenate([p, rng.randint(0, 500, (3000, 3))], 1)))
    edge = np.array([0, 255, 256, 257, 65535, 65536])
    u = rng.randint(0, 40, 600)
    out.append(("item_digit_edges", 40, 65537, _pairs(u, edge[rng.randint(0, 6, 600)])))
    out.append(("user_digit_edges", 65537, 40, _pairs(edge[rng.randint(0, 6, 600)], u)))
    p = random_pairs(rng, 70000, 70001, 4998)
    out.append(("key_above_2^32", 70000, 70001, np.concatenate([p, _pairs([0, 69999], [0, 70000])])[rng.permutation(5000)]))
    for m in M_EDGES + M_EXTRA:
        # few enough ids that duplicates occur, enough that several tiles hold every digit
        out.append(("m=%d" % m, 300, 1000, random_pairs(rng, 300, 1000, m)))
    return out


def union_cases():
    """[(name, n_user, n_item, [pairs, ...])]: a sequence of adds."""
    rng = np.random.RandomState(4321)
    out = []
    p = random_pairs(rng, 200, 700, 9000)
    for chunks in (1, 2, 7):
        out.append(("chunks_%d" % chunks, 200, 700, np.array_split(p, chunks)))
    out.append(("empty_add", 200, 700, [p[:4000], np.zeros((0, 2), np.int64), p[4000:]]))
    out.append(("subset_again", 200, 700, [p, p[rng.permutation(9000)[:2500]]]))
    lo, hi = random_pairs(rng, 100, 700, 3000), random_pairs(rng, 100, 700, 3000) + np.array([100, 0])
    out.append(("disjoint_users", 200, 700, [lo, hi]))
    out.append(("b_larger_than_a", 200, 700, [p[:300], p[300:]]))
    # user 3 grows from nothing to 5,000 even ids, then by the 5,000 odd ids between them; the others hold a few
    rest = random_pairs(rng, 9, 10000, 400)
    rest = rest[rest[:, 0] != 3]
    even, odd = _pairs(np.full(5000, 3), np.arange(0, 10000, 2)), _pairs(np.full(5000, 3), np.arange(1, 10000, 2))
    out.append(("range_grows_from_0_and_interleaved", 9, 10000, [rest, even[rng.permutation(5000)], odd[rng.permutation(5000)]]))
    out.append(("many_small_adds", 70000, 70001, [random_pairs(rng, 70000, 70001, 4097) for _ in range(3)]))
    return out
