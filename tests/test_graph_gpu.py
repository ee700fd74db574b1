"""Graph propagation on the MI355X: sml_graph_propagate through HipEngine.graph_propagate, and sml_amd.graph (InteractionGraph,
propagate and its backward pass, LightGCN, fit).

Every comparison of propagated rows is byte equality against the host walk of the same definition, which tests/test_graph_host.py
holds to a restatement of the header.  Shapes: 48 rows over a table of 4,096 (tests/_graph_cases.py), set sizes 0 .. 3,000 on both
sides of the split threshold; the model tests use a planted-cluster set of 400 users x 800 items."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _graph_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def engine(d):
    from sml_amd.engine import get_engine
    return get_engine(DEV, d)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(t, a, what):
    """A device tensor and a numpy array, byte for byte."""
    G.same_bytes(t.detach().cpu().numpy(), a, what)


@functools.lru_cache(maxsize=None)
def dev_case(dtype, d):
    c = dict(G.case(dtype, d))
    c["t_src"], c["sets_dev"], c["t_a"], c["t_b"] = gpu(c["src"]), tuple(gpu(t) for t in c["csr"]), gpu(c["a"]), gpu(c["b"])
    return c


@pytest.mark.parametrize("dtype,d", G.PAIRS)
def test_device_equals_the_host_walk(dtype, d):
    c = dev_case(dtype, d)
    eng = engine(d)
    assert eng.graph_split_from() == G.split_from()
    for scaled in (True, False):
        want = G.host_rows(dtype, d, scaled)
        a, b = (c["t_a"], c["t_b"]) if scaled else (None, None)
        for path in (0, 1, 2):
            for mw in (0, 1, 3):
                same(eng.graph_propagate(c["t_src"], c["sets_dev"], a=a, b=b, max_workgroups=mw, path=path), want,
                     (dtype, d, scaled, path, mw))
        for path in (0, 1, 2):
            out = torch.full((len(G.ROWS), d), 7.0, device=DEV)
            got = eng.graph_propagate(c["t_src"], c["sets_dev"], out=out, rows=gpu(G.ROWS), a=a, b=b, path=path)
            assert got is out
            same(out, want[G.ROWS], (dtype, d, scaled, path, "rows: a permutation with a repeat"))


def test_a_refused_call_writes_nothing():
    from sml_amd import _lib
    c = dev_case("fp32", 32)
    eng = engine(32)
    lib = eng.lib
    off, items = c["sets_dev"]
    out = torch.full((G.N, 32), 7.0, device=DEV)
    nbytes = lib.sml_graph_scratch_bytes(eng._ctx, G.N, items.shape[0], 0)
    assert nbytes > 0
    scratch = torch.zeros(nbytes + 512, device=DEV, dtype=torch.uint8)
    assert scratch.data_ptr() % 256 == 0

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())

    def call(**kw):
        k = dict(src=c["t_src"], eb=4, n_src=G.n_src(), off=off, items=items, rows=None, n=G.N, a=c["t_a"], b=c["t_b"], mw=0, path=0,
                 scratch=scratch, out=out)
        k.update(kw)
        return lib.sml_graph_propagate(eng._ctx, ptr(k["src"]), k["eb"], k["n_src"], ptr(k["off"]), ptr(k["items"]), ptr(k["rows"]), k["n"],
                                       ptr(k["a"]), ptr(k["b"]), k["mw"], k["path"], ptr(k["scratch"]), ptr(k["out"]),
                                       eng._stream())

    for kw in (dict(eb=8), dict(eb=1), dict(n_src=0), dict(n_src=2 ** 31), dict(n=-1), dict(n=2 ** 31), dict(mw=-1), dict(path=3),
               dict(path=-1), dict(off=None), dict(items=None), dict(scratch=scratch.data_ptr() + 16), dict(scratch=None),
               dict(src=None), dict(out=None), dict(out=c["t_src"]), dict(out=off), dict(out=c["t_a"]), dict(out=c["t_b"]),
               dict(out=scratch), dict(out=out.data_ptr() + 4)):
        assert call(**kw) != 0 and lib.sml_last_error(), kw
    assert lib.sml_graph_scratch_bytes(eng._ctx, -1, 0, 0) < 0 and lib.sml_graph_scratch_bytes(eng._ctx, 1, -1, 0) < 0
    assert lib.sml_graph_scratch_bytes(eng._ctx, 1, 1, -1) < 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((scratch == 0).all())
    assert call(n=0, out=None, src=None, scratch=None) == 0                # n == 0 launches nothing
    assert call(path=1, scratch=None) == 0                                 # never split: no scratch
    same(out, G.host_rows("fp32", 32, True), "after the refusals")
    out.fill_(7.0)
    assert call(off=None, items=None, scratch=None) == 0                   # both NULL: every set is empty
    same(out, np.outer(c["a"], np.zeros(32, F32)).astype(F32), "no set")
    with pytest.raises(_lib.SmlError):
        eng.graph_propagate(c["t_src"], c["sets_dev"], path=5)


# ---- InteractionGraph on the case's 48 x n_src set -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph_case(dtype, d):
    from sml_amd.graph import InteractionGraph
    c = dev_case(dtype, d)
    rng = np.random.RandomState(2450 + d)
    by_item = G.transpose(c["sets"], G.n_src())
    g = dict(c, users=(rng.rand(G.N, d) - 0.5).astype(G.np_type(dtype)), by_item=by_item, csr_t=G.csr(by_item),
             du=G.degree_scale(c["sets"]), di=G.degree_scale(by_item))
    g["graph"] = InteractionGraph.build(c["sets_dev"], G.N, G.n_src(), engine=engine(d))
    g["t_users"] = gpu(g["users"])
    return g


def host_layer(g, users, items):
    return (G.host_propagate(items, g["d"], g["csr"], None, g["du"], g["di"]),
            G.host_propagate(users, g["d"], g["csr_t"], None, g["di"], g["du"]))


def host_read_out(g, users, items, weights):
    out_u, out_i = F32(weights[0]) * users.astype(F32), F32(weights[0]) * items.astype(F32)
    for w in weights[1:]:
        users, items = host_layer(g, users, items)
        out_u, out_i = out_u + F32(w) * users, out_i + F32(w) * items
    return out_u, out_i


@pytest.mark.parametrize("dtype,d", (("fp32", 32), ("fp16", 64), ("fp32", 128)))
def test_layer_equals_the_two_host_walks(dtype, d):
    g = graph_case(dtype, d)
    graph = g["graph"]
    same(graph.du, g["du"], "du")
    same(graph.di, g["di"], "di")
    same(graph.by_item[0], g["csr_t"][0], "the transpose's offsets")
    same(graph.by_item[1], g["csr_t"][1], "the transpose's members")
    u, i = graph.layer(g["t_users"], g["t_src"])
    want_u, want_i = host_layer(g, g["users"], g["src"])
    same(u, want_u, (dtype, d, "user half"))
    same(i, want_i, (dtype, d, "item half"))


@pytest.mark.parametrize("dtype,d", (("fp32", 64), ("fp16", 32)))
def test_propagate_equals_the_summed_host_layers(dtype, d):
    g = graph_case(dtype, d)
    for layers, weights in ((3, None), (2, None), (2, (0.2, 0.3, 0.5)), (0, None)):
        u, i = g["graph"].propagate(g["t_users"], g["t_src"], layers=layers, weights=weights)
        w = [1.0 / (layers + 1)] * (layers + 1) if weights is None else weights
        want_u, want_i = host_read_out(g, g["users"], g["src"], w)
        assert u.dtype == torch.float32 and i.dtype == torch.float32
        same(u, want_u, (dtype, d, layers, weights, "users"))
        same(i, want_i, (dtype, d, layers, weights, "items"))
    u, i = g["graph"].propagate(g["t_users"], g["t_src"], layers=0)
    same(u, g["users"].astype(F32), "layers = 0 returns the inputs widened")
    same(i, g["src"].astype(F32), "layers = 0 returns the inputs widened")


def test_backward_of_one_hop_is_the_transposed_call():
    g = graph_case("fp32", 32)
    rng = np.random.RandomState(2460)
    gu = (rng.rand(G.N, 32) - 0.5).astype(F32)
    users, items = g["t_users"].clone().requires_grad_(True), g["t_src"].clone().requires_grad_(True)
    u, i = g["graph"].propagate(users, items, layers=1)
    same(u, host_read_out(g, g["users"], g["src"], (0.5, 0.5))[0], "forward under autograd")
    u.backward(gpu(gu))
    # the incoming gradients are (g, 0); the read-out of the gradients is w_0 * g_l + w_1 * hop, summed as the forward sums
    zero_u, zero_i = np.zeros_like(gu), np.zeros((G.n_src(), 32), F32)
    hop_i = G.host_propagate(gu, 32, g["csr_t"], None, g["di"], g["du"])          # the transposed call on g
    hop_u = G.host_propagate(zero_i, 32, g["csr"], None, g["du"], g["di"])
    same(items.grad, F32(0.5) * zero_i + F32(0.5) * hop_i, "item table")
    same(users.grad, F32(0.5) * gu + F32(0.5) * hop_u, "user table")
    assert float(np.abs(hop_i).max()) > 0 and zero_u.shape == gu.shape


def test_backward_of_three_layers_is_close_to_float64_autograd():
    """Against dense float64 torch autograd on the 48 x n_src matrix P = diag(du) A diag(di) (du, di the float32 tables, widened).
    The gradient of sum_l w_l P^l E is sum_l w_l P^l g.  Bound: one hop errs by at most e_h |P| |x| per element, e_h = (40 +
    n_seg) 2^-23 with n_seg the largest segment count of any row (tests/test_graph_host.py derives it); hop l reads hop l - 1's
    rounded result, so |fl(P^l g) - P^l g| <= ((1 + e_h)^l - 1) |P|^l |g| <= l e_h (1 + e_h)^L |P|^l |g| (P has no negative
    entry, so |P| = P).  The read-out's products and adds, 2 L + 1 roundings of 2^-24 on partial sums bounded by
    sum_l w_l |P|^l |g|, add (2 L + 2) 2^-24 of that.  Together, per element:
        bound = (1 + e_h)^L sum_l w_l (l e_h + (2 L + 2) 2^-24) |P|^l |g|,
    the float64 reference's own error being some 2^-29 of that."""
    g = graph_case("fp32", 32)
    L, w = 3, [0.25] * 4
    rng = np.random.RandomState(2470)
    gu, gi = (rng.rand(G.N, 32) - 0.5).astype(F32), (rng.rand(G.n_src(), 32) - 0.5).astype(F32)
    users, items = g["t_users"].clone().requires_grad_(True), g["t_src"].clone().requires_grad_(True)
    u, i = g["graph"].propagate(users, items, layers=L)
    torch.autograd.backward([u, i], [gpu(gu), gpu(gi)])
    dense = torch.zeros(G.N, G.n_src(), dtype=torch.float64)
    for r, mem in enumerate(g["sets"]):
        dense[r, torch.from_numpy(mem)] = 1.0
    p = torch.from_numpy(g["du"]).double()[:, None] * dense * torch.from_numpy(g["di"]).double()[None, :]
    ru, ri = torch.from_numpy(g["users"]).double().requires_grad_(True), torch.from_numpy(g["src"]).double().requires_grad_(True)
    eu, ei, out_u, out_i = ru, ri, w[0] * ru, w[0] * ri
    for l in range(1, L + 1):
        eu, ei = p @ ei, p.t() @ eu
        out_u, out_i = out_u + w[l] * eu, out_i + w[l] * ei
    torch.autograd.backward([out_u, out_i], [torch.from_numpy(gu).double(), torch.from_numpy(gi).double()])
    n_seg = max((len(s) + G.SEG - 1) // G.SEG for s in list(g["sets"]) + list(g["by_item"]))
    e_h = (40 + n_seg) * 2.0 ** -23
    au, ai = torch.from_numpy(np.abs(gu)).double(), torch.from_numpy(np.abs(gi)).double()
    bound_u, bound_i = (2 * L + 2) * 2.0 ** -24 * w[0] * au, (2 * L + 2) * 2.0 ** -24 * w[0] * ai
    for l in range(1, L + 1):
        au, ai = p @ ai, p.t() @ au
        bound_u = bound_u + w[l] * (l * e_h + (2 * L + 2) * 2.0 ** -24) * au
        bound_i = bound_i + w[l] * (l * e_h + (2 * L + 2) * 2.0 ** -24) * ai
    for name, got, ref, bound in (("users", users.grad, ru.grad, bound_u), ("items", items.grad, ri.grad, bound_i)):
        bound = bound * (1 + e_h) ** L
        err = (got.cpu().double() - ref).abs()
        print("%s: largest error %.3g, in units of the bound %.4f" % (name, float(err.max()), float((err / bound.clamp(min=1e-300)).max())))
        assert bool((err <= bound).all()), (name, float(err.max()))
        assert float(ref.abs().max()) > 0


# ---- LightGCN on a planted-cluster set -----------------------------------------------------------------------------------------
N_USER, N_ITEM, D = 400, 800, 32


@functools.lru_cache(maxsize=None)
def cluster_case():
    sets = G.clusters(N_USER, N_ITEM)
    by_item = G.transpose(sets, N_ITEM)
    return dict(d=D, sets=sets, csr=G.csr(sets), csr_t=G.csr(by_item), du=G.degree_scale(sets), di=G.degree_scale(by_item),
                sets_dev=tuple(gpu(t) for t in G.csr(sets)))


def new_model(dtype=torch.float32):
    from sml_amd.graph import LightGCN
    torch.manual_seed(2480)
    model = LightGCN(N_USER, N_ITEM, D).to(device=DEV, dtype=dtype)
    return model.set_graph(cluster_case()["sets_dev"])


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
def test_materialise_serves_the_existing_calls(dtype):
    from sml_amd.mf import MFbasemode
    c = cluster_case()
    model = new_model(dtype)
    assert model.layers == 3 and isinstance(model, MFbasemode)
    m = model.materialise()
    assert type(m) is MFbasemode and m.user_laten.weight.dtype == dtype
    want_u, want_i = host_read_out(c, model.user_laten.weight.detach().cpu().numpy(), model.item_laten.weight.detach().cpu().numpy(),
                                   [0.25] * 4)
    np_t = F32 if dtype == torch.float32 else np.float16
    same(m.user_laten.weight, want_u.astype(np_t), "propagated user table")
    same(m.item_laten.weight, want_i.astype(np_t), "propagated item table")
    ref = MFbasemode(N_USER, N_ITEM, D).to(device=DEV, dtype=dtype)
    with torch.no_grad():
        pu, pi = model.propagated()
        ref.user_laten.weight.copy_(pu)
        ref.item_laten.weight.copy_(pi)
    users = torch.arange(0, N_USER, 7, device=DEV)
    got, want = m.recommend(users, 10, exclude=c["sets_dev"]), ref.recommend(users, 10, exclude=c["sets_dev"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got, want = m.similar_items(torch.arange(5, device=DEV), 5), ref.similar_items(torch.arange(5, device=DEV), 5)
    assert torch.equal(got[0], want[0])


def test_forward_is_bpr_and_l2_on_the_propagated_rows():
    model = new_model()
    rng = np.random.RandomState(2490)
    u, i, n = (gpu(rng.randint(0, hi, 256).astype(np.int64)) for hi in (N_USER, N_ITEM, N_ITEM))
    bpr, l2 = model(u, i, n)
    assert bpr.requires_grad and l2.requires_grad
    with torch.no_grad():
        _check_forward(model, u, i, n, bpr.detach(), l2.detach())
    (bpr + 1e-4 * l2).backward()
    assert model.user_laten.weight.grad is not None and float(model.item_laten.weight.grad.abs().max()) > 0


def _check_forward(model, u, i, n, bpr, l2):
    pu, pi = (t.double() for t in model.propagated())
    s = (pu[u] * pi[i]).sum(-1) - (pu[u] * pi[n]).sum(-1)
    w_u, w_i = model.user_laten.weight.double(), model.item_laten.weight.double()
    want_l2 = 0.5 * ((w_u[u] ** 2).sum(-1) + (w_i[i] ** 2).sum(-1) + (w_i[n] ** 2).sum(-1)).mean()
    assert abs(float(bpr) - float(-torch.nn.functional.logsigmoid(s).mean())) <= 1e-5 * max(1.0, abs(float(bpr)))
    assert abs(float(l2) - float(want_l2)) <= 1e-5 * float(want_l2)


def test_fit_lowers_the_loss():
    from sml_amd import graph
    model = new_model()
    before = model.user_laten.weight.detach().clone()
    losses = graph.fit(model, cluster_case()["sets_dev"], epochs=30)             # 8,000 pairs, one batch per epoch: 30 steps
    print("loss per step", ["%.4f" % x for x in losses])
    assert len(losses) == 30 and all(np.isfinite(losses))
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    assert not torch.equal(before, model.user_laten.weight.detach())
