"""The item filter of full-catalogue retrieval, the parts that need no GPU: the C ABI surface of the _filtered entry points
and the filter builder, sml_amd.retrieval.ItemFilter, the register report of the filtered kernel instantiations, and the
proof that the filters of the GPU tests change the answers of the CPU references."""
import os
import subprocess

import numpy as np
import pytest
import torch

from _item_filter_cases import near_tie_mask, pack, random_mask, seen_prime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERED = ("sml_full_rank_filtered", "sml_topk_items_filtered", "sml_user_rank_filtered")
NEW = FILTERED + tuple(n + "_f16" for n in FILTERED) + ("sml_item_filter_words", "sml_item_filter_from_ids")


def test_abi_surface():
    import ctypes
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert len(NEW) == 8
    for name in NEW:
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert name in syms
    for name in FILTERED:
        assert _lib.SIGNATURES[name + "_f16"] == _lib.SIGNATURES[name]
        # the unfiltered argument list with `allow` (a pointer) inserted: one more argument, same result type
        res, args = _lib.SIGNATURES[name]
        res0, args0 = _lib.SIGNATURES[name.replace("_filtered", "")]
        assert res == res0 and len(args) == len(args0) + 1
        at = [q for q in range(len(args)) if args[:q] + args[q + 1:] == args0 and args[q] is ctypes.c_void_p]
        assert at, name
    # the header documents the layout, the ignored tail, the disallowed-positive rules and the identity
    for phrase in ("bit (i & 31) of word (i >> 5)", "are ignored, whatever they hold", "p itself is never excluded",
                   "treated exactly like one in Seen(u)", "Seen'(u) = Seen(u) united with"):
        assert phrase in header, phrase


def test_item_filter_words_and_composition():
    from sml_amd.retrieval import ItemFilter
    for n_item in (1, 31, 32, 33, 4099):
        rng = np.random.RandomState(n_item)
        mask = rng.rand(n_item) < 0.4
        f = ItemFilter.from_mask(mask)
        words = f.host()
        assert words.dtype == np.uint32 and words.shape == ((n_item + 31) // 32,)
        b = np.packbits(mask, bitorder="little")
        want = np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)]).view(np.uint32)
        np.testing.assert_array_equal(words, want)
        np.testing.assert_array_equal(words, pack(mask))
        assert len(f) == int(mask.sum())
        for i in range(n_item):                                       # the documented bit layout, item by item
            assert bool((int(words[i >> 5]) >> (i & 31)) & 1) == bool(mask[i])
        if n_item % 32:
            assert int(words[-1]) >> (n_item % 32) == 0               # ItemFilter keeps the tail bits 0
    f = ItemFilter(100)
    assert len(f) == 0 and not f.host().any()
    f.allow([3, 5, 5, 99]).allow(np.array([7], np.int32))
    assert len(f) == 4
    f.deny([5, 6])
    assert len(f) == 3 and sorted(np.nonzero(f.mask())[0].tolist()) == [3, 7, 99]
    f.allow(torch.tensor([5]))
    assert len(f) == 4
    np.testing.assert_array_equal(f.host(), pack(f.mask()))
    f.deny(np.arange(100))
    assert len(f) == 0
    f.allow([])
    assert len(f) == 0


def test_item_filter_refuses_bad_input():
    from sml_amd.retrieval import ItemFilter, as_filter
    f = ItemFilter(33)
    for bad in ([-1], [33], [0, 40], np.array([2 ** 31], np.int64)):
        with pytest.raises(ValueError):
            f.allow(bad)
        with pytest.raises(ValueError):
            f.deny(bad)
    with pytest.raises(ValueError):
        f.allow([0.5])
    assert len(f) == 0
    with pytest.raises(ValueError):
        ItemFilter(0)
    with pytest.raises(ValueError):
        ItemFilter.from_mask(np.zeros(5, np.int32))
    with pytest.raises(ValueError):
        as_filter(f, 34, "cpu")                                       # a filter over another catalogue
    with pytest.raises(ValueError):
        as_filter(np.zeros(32, bool), 33, "cpu")
    with pytest.raises(ValueError):
        as_filter(torch.zeros(1, dtype=torch.int32), 33, "cpu")       # 33 items need 2 words


def test_as_filter_forms_agree():
    from sml_amd.retrieval import ItemFilter, as_filter
    mask = random_mask(4099, 0.5, 3)
    f = ItemFilter.from_mask(mask)
    a = as_filter(f, 4099, "cpu")
    assert a.dtype == torch.int32 and a.shape == (129,)
    assert a is f.device("cpu")                                       # cached, like SeenItems.device
    np.testing.assert_array_equal(a.numpy().view(np.uint32), pack(mask))
    assert torch.equal(as_filter(mask, 4099, "cpu"), a)
    assert torch.equal(as_filter(torch.from_numpy(mask), 4099, "cpu"), a)
    assert torch.equal(as_filter(a.clone(), 4099, "cpu"), a)
    assert as_filter(None, 4099, "cpu") is None
    f.deny([int(np.nonzero(mask)[0][0])])
    assert f.device("cpu") is not a and len(f) == int(mask.sum()) - 1


def test_seen_prime_is_the_union():
    import _fp32_chain as F
    c = F.random_case(32, seed=1, U=20, I=300, n=8)
    mask = random_mask(300, 0.5, 2)
    off, items = seen_prime(c["seen"], mask, 20)
    o0, i0 = c["seen"]
    for u in range(20):
        want = sorted(set(i0[o0[u]:o0[u + 1]].tolist()) | set(np.nonzero(~mask)[0].tolist()))
        assert items[off[u]:off[u + 1]].tolist() == want
    off, items = seen_prime(None, mask, 3)
    assert items[off[1]:off[2]].tolist() == np.nonzero(~mask)[0].tolist()


@pytest.mark.parametrize("d", [32])
def test_filters_have_teeth_on_the_cpu_references(d):
    """On near_tie_case the references with Seen' differ from the references with plain Seen, for the near-tie filter and
    for the random 50 % filter of the GPU tests: a kernel that ignored the filter would fail the identity tests."""
    import _fp32_chain as F
    c = F.near_tie_case(d, seed=0)
    U, I = c["wu"].shape[0], c["wi"].shape[0]
    rows, users = c["rows"][:96], c["users"][:48]
    base_rank = F.ref_full_rank(c["wu"], c["wi"], rows, c["seen"])
    base_it, base_sc = F.ref_topk(c["wu"], c["wi"], users, 20, c["seen"])
    for mask in (near_tie_mask(c), random_mask(I, 0.5, 11)):
        assert 0 < mask.sum() < I
        sp = seen_prime(c["seen"], mask, U)
        rank = F.ref_full_rank(c["wu"], c["wi"], rows, sp)
        assert (rank <= base_rank).all() and (rank != base_rank).sum() >= 10
        it, sc = F.ref_topk(c["wu"], c["wi"], users, 20, sp)
        assert (it != base_it).any(1).sum() >= 10
        assert mask[it[it >= 0]].all()                          # the filtered lists hold allowed items only
    # the near-tie filter keeps the planted positives and their planted copies
    assert near_tie_mask(c)[c["planted"][:, 1]].all()
