"""Helpers shared by the item-filter tests (test_item_filter_host.py, test_item_filter_gpu.py): the oracle's Seen' on the
host, and the filters the tests use.

The contract (include/sml_hip.h): a filtered call with Seen and the filter A returns, byte for byte, what the unfiltered
call returns with Seen'(u) = Seen(u) + ([0, n_item) - A) for every user.  seen_prime builds that CSR."""
import numpy as np


def pack(mask):
    """bool [n_item] -> uint32 words, as np.packbits(bitorder="little") lays them out (tail bits 0)."""
    b = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    return np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)]).view("<u4").astype(np.uint32)


def seen_prime(seen, mask, n_user):
    """(seen_off int64, seen_items int32): every user's Seen range united with the items the mask does not allow."""
    mask = np.asarray(mask, dtype=bool)
    denied = np.nonzero(~mask)[0].astype(np.int64)
    if seen is None:
        off, items = np.zeros(n_user + 1, np.int64), np.zeros(0, np.int32)
    else:
        off, items = (np.asarray(t) for t in seen)
    lists = [np.union1d(items[off[u]:off[u + 1]].astype(np.int64), denied) for u in range(n_user)]
    new_off = np.zeros(n_user + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=new_off[1:])
    return new_off, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)


def random_mask(n_item, keep, seed):
    return np.random.RandomState(seed).rand(n_item) < keep


def near_tie_mask(c):
    """A filter for near_tie_case / half_near_tie_case: keeps the positives of the planted rows, every item whose row
    equals a planted positive's row bit for bit or differs from it in rounding only (all rows within the neighbourhood the
    case planted), and removes every third remaining item -- neighbours of the planted items in id included."""
    wi = np.asarray(c["wi"])
    I = wi.shape[0]
    mask = (np.arange(I) % 3) != 1
    keys = {np.sort(wi[p].astype(np.float64)).tobytes() for p in c["planted"][:, 1]}
    for i in range(I):                                   # copies and dim-permuted copies of a planted positive's row
        if np.sort(wi[i].astype(np.float64)).tobytes() in keys:
            mask[i] = True
    mask[c["planted"][:, 1]] = True
    return mask
