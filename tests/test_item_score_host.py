"""The adjusted score of full-catalogue retrieval, the parts that need no GPU: the C ABI surface of the _adjusted entry points
and the term-table builders, sml_amd.retrieval.ItemScore, the register report of the adjusted kernel instantiations, and
the proof that the terms of the GPU cases change the answers of the CPU references -- and that the exact comparison tells
a fused multiply-add from a multiply followed by an add."""
import os
import subprocess

import numpy as np
import pytest
import torch

import _item_score_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("sml_full_rank", "sml_topk_items", "sml_user_rank")
NEW = tuple(n + "_adjusted" for n in CALLS) + ("sml_item_adjust_len", "sml_item_adjust_fill", "sml_item_adjust_cosine")


def test_abi_surface():
    import ctypes
    from sml_amd import _lib, build
    with open(os.path.join(REPO, "include", "sml_hip.h")) as f:
        header = f.read()
    lib = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert name in syms, name
    # header, binding and library agree symbol for symbol
    exported = {s for s in syms if s.startswith("sml_")}
    assert exported == set(_lib.SIGNATURES)
    for name in _lib.SIGNATURES:
        assert name + "(" in header, name
    for name in CALLS:
        # the _filtered argument list with elem_bytes (an int) after w_item and adj (a pointer) after allow
        res, args = _lib.SIGNATURES[name + "_adjusted"]
        res0, args0 = _lib.SIGNATURES[name + "_filtered"]
        assert res == res0 and len(args) == len(args0) + 2
        assert args[3] is ctypes.c_int and args[:3] + args[4:] != args0
        rest = args[:3] + args[4:]
        at = [q for q in range(len(rest)) if rest[:q] + rest[q + 1:] == args0 and rest[q] is ctypes.c_void_p]
        assert at, name
    flat = " ".join(" ".join(line.strip().lstrip("/*").strip() for line in header.splitlines()).split())     # comment text, unwrapped
    for phrase in ("A(u, i) = fmaf(S(u, i), scale[i], offset[i])", "Pad entries are ignored", "scale ≡ 1, offset ≡ +0",
                   "every integer output equals the unadjusted call's byte for byte",
                   "n2 > 0 ? 1.0f / sqrtf(n2) : 0.0f", "A zero row therefore scores 0 against everything instead of NaN",
                   "adj == NULL is refused", "32 * ceil(n_item / 32)"):
        assert phrase in flat, phrase


def test_item_adjust_len_needs_no_gpu():
    from sml_amd import _lib
    lib = _lib.load()
    for n_item, want in ((1, 32), (31, 32), (32, 32), (33, 64), (4099, 4128)):
        assert lib.sml_item_adjust_len(n_item) == want
    assert lib.sml_item_adjust_len(0) < 0 and lib.sml_item_adjust_len(1 << 31) < 0


def test_item_score_construction_and_editing():
    from sml_amd.retrieval import ItemScore, adjust_len
    for n_item, n_pad in ((1, 32), (31, 32), (32, 32), (33, 64), (4099, 4128)):
        assert adjust_len(n_item) == n_pad
        s = ItemScore(n_item)
        assert s.padded_len() == n_pad and not s.is_cosine
        adj = s.host()
        assert adj.dtype == np.float32 and adj.shape == (2, n_pad)
        assert (adj[0] == 1).all() and (adj[1] == 0).all() and not np.signbit(adj[1]).any()      # neutral: (1, +0)
        rng = np.random.RandomState(n_item)
        sc, of = rng.rand(n_item).astype(np.float32), rng.randn(n_item)
        assert s.scale(sc).offset(of) is s
        adj = s.host()
        np.testing.assert_array_equal(adj[0, :n_item], sc)
        np.testing.assert_array_equal(adj[1, :n_item], of.astype(np.float32))
        assert (adj[0, n_item:] == 1).all() and (adj[1, n_item:] == 0).all()                       # pads (1, 0)
        np.testing.assert_array_equal(adj, C.pad_adj(sc, of.astype(np.float32)))
    s = ItemScore(5).bias(np.arange(5, dtype=np.float64).reshape(5, 1))                           # an embedding's [n, 1] weight
    np.testing.assert_array_equal(s.host()[1, :5], np.arange(5, dtype=np.float32))
    s.bias(torch.arange(5).float().neg())                                                         # [n] and a tensor
    np.testing.assert_array_equal(s.host()[1, :5], -np.arange(5, dtype=np.float32))
    s.offset([0, -np.inf, np.nan, 1, 2]).scale([0, 1, 2, np.inf, -1])                              # any float may be given
    assert np.isneginf(s.host()[1, 1]) and np.isnan(s.host()[1, 2]) and np.isinf(s.host()[0, 3])
    s.cosine()
    assert s.is_cosine
    with pytest.raises(ValueError):
        s.host()                                                                                  # needs the item table
    with pytest.raises(ValueError):
        s.device(None, None)
    s.scale(np.ones(5))
    assert not s.is_cosine and (s.host()[0, :5] == 1).all()


def test_item_score_refuses_bad_input():
    from sml_amd.retrieval import ItemScore, as_score
    with pytest.raises(ValueError):
        ItemScore(0)
    s = ItemScore(33)
    for bad in (np.zeros(32), np.zeros((33, 2)), np.zeros((1, 33)), np.zeros(33, bool), np.array(["a"] * 33)):
        with pytest.raises(ValueError):
            s.scale(bad)
        with pytest.raises(ValueError):
            s.offset(bad)
        with pytest.raises(ValueError):
            s.bias(bad)
    with pytest.raises(ValueError):
        s.scale(np.zeros((33, 1)))                      # only bias() takes a column
    assert (s.host() == C.pad_adj(np.ones(33), np.zeros(33))).all()

    class Model(object):
        item_laten = torch.nn.Embedding(34, 4)
    assert as_score(None, Model()) is None and as_score("dot", Model()) is None
    with pytest.raises(ValueError):
        as_score(s, Model())                            # terms over another catalogue
    with pytest.raises(ValueError):
        as_score("euclid", Model())
    t = torch.zeros(2, 64)
    assert as_score(t, Model()) is t


def test_cosine_scale_reference():
    rng = np.random.RandomState(0)
    x = rng.randn(40, 32).astype(np.float32)
    x[7] = 0
    x[9] = np.float32(2.0 ** -72)                               # n2 underflows to a subnormal, not to 0
    s = C.cosine_scale(x)
    assert s.dtype == np.float32 and s[7] == 0 and np.isfinite(s).all() and s[9] > 0
    np.testing.assert_allclose(s[:7], 1.0 / np.linalg.norm(x[:7].astype(np.float64), axis=1), rtol=3e-7)
    e = np.zeros((1, 32), np.float32)
    e[0, 5] = 3.0
    assert C.cosine_scale(e)[0] == np.float32(1.0) / np.float32(3.0)


def test_terms_have_teeth_on_the_cpu_references():
    """The case the GPU exactness tests run (fp32, d = 32, seed C.SEED): the adjusted ranks and lists differ from the
    unadjusted ones, and a multiply-then-add emulation gives other score bits than the fma on listed items -- so a kernel
    that ignored the terms, or left the fmaf to two roundings, fails the exact comparison."""
    c = C.score_case("fp32", 32)
    S = C.case_scores(c)
    ones, zeros = np.ones_like(c["scale"]), np.zeros_like(c["offset"])
    A = C.adjusted(S, c["scale"][None], c["offset"][None])
    A2 = C.adjusted(S, c["scale"][None], c["offset"][None], rounding="two")
    neutral = C.adjusted(S, ones[None], zeros[None])
    assert np.array_equal(neutral, S)                            # A == S as values under (1, +0)
    rows, users = c["rows"], c["users"][:64]
    r0, r1 = C.ref_rank(S, rows, c["seen"]), C.ref_rank(A, rows, c["seen"])
    assert (r0 != r1).sum() >= 200
    np.testing.assert_array_equal(r0, F_ref_rank(c))             # the brute-force reference is the chain reference on S
    i0, s0 = C.ref_topk(S, users, 20, c["seen"])
    i1, s1 = C.ref_topk(A, users, 20, c["seen"])
    assert (i0 != i1).any(1).all()
    listed_one = A[users[:, None], i1]
    listed_two = A2[users[:, None], i1]
    assert np.array_equal(listed_one.view(np.int32), s1.view(np.int32))
    assert (listed_one.view(np.int32) != listed_two.view(np.int32)).sum() >= 10
    # the rules on A: NaN items enter no list, -inf items stay eligible and go last
    sp = c["special"]
    gone = np.concatenate([sp["nan_offset"], sp["nan_scale"]])
    full_i, full_s = C.ref_topk(A, users[:4], 4099, None)
    assert not np.isin(full_i, gone).any() and (full_i >= 0).sum(1).tolist() == [4099 - len(gone)] * 4
    tail = full_i[:, 4099 - len(gone) - len(sp["neg_inf"]):4099 - len(gone)]
    assert (np.sort(tail, 1) == np.sort(sp["neg_inf"])).all() and (np.diff(tail, axis=1) > 0).all()
    assert (r1[np.isin(rows[:, 1], gone)] == 0).all() and np.isin(rows[:, 1], gone).sum() >= 6
    # ties planted with identical rows and terms sit next to their positive, by id
    held = C.held_sets(c, 60)
    above, pos = C.ref_user_rank(A, *held, seen=c["seen"])
    assert (pos[np.isin(held[2], gone)] == -1).all() and (pos >= 0).sum() > 100


def F_ref_rank(c):
    import _fp32_chain as F
    return F.ref_full_rank(c["ru"], c["ri"], c["rows"], c["seen"])
