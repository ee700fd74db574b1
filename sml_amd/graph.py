"""Graph propagation and the LightGCN baseline on the HIP engine (include/sml_hip.h, PROPAGATION).

One hop along the user-item graph is the symmetric-normalised product

    E' = D^-1/2 A D^-1/2 E,    U' = du * sum_{i in S(u)} di[i] * I[i],    I' = di * sum_{u in S^T(i)} du[u] * U[u]

(HipEngine.graph_propagate: a random-row gather whose bytes depend on no launch geometry).  InteractionGraph holds the set, its
transpose and the two scale tables; layer is one hop, propagate the LightGCN read-out sum_l w_l E^(l).  The operator is linear and
symmetric, so the backward pass of propagate is propagate itself applied to the incoming gradients: a trainable LightGCN costs no
second kernel.  LightGCN is the module, fit the BPR baseline loop.

layers = 3, lr = 1e-3 and reg = 1e-4 are conventions of the LightGCN paper, not values tuned for this project's data."""
import torch
import torch.nn as nn

from .mf import MFbasemode

WIDTHS = (32, 64, 128)


class InteractionGraph(object):
    """The user -> items set (by_user), its transpose (by_item) -- both (off int64, items int32) on the device -- and the fp32 scale
    tables du = deg_u^-1/2, di = deg_i^-1/2 (0 where the degree is 0; computed in float64 and rounded once)."""

    def __init__(self, by_user, by_item, du, di, n_user, n_item, engine=None):
        self.by_user, self.by_item, self.du, self.di = by_user, by_item, du, di
        self.n_user, self.n_item = int(n_user), int(n_item)
        self.device = du.device
        self._engine = engine

    @classmethod
    def build(cls, history, n_user, n_item, engine=None):
        """history: the users' interaction sets, anything sml_amd.retrieval.as_csr takes (a SeenItems, a DeviceSeen, an (off, items)
        pair).  engine: the HipEngine of the tables' width when the caller has one (its device is used; otherwise the current
        device, and every call finds the process-wide engine of its tables' width)."""
        from . import als
        from .engine import get_engine
        from .retrieval import as_csr
        n_user, n_item = int(n_user), int(n_item)
        eng = engine if engine is not None else get_engine(torch.device("cuda", torch.cuda.current_device()), WIDTHS[0])
        off, items = as_csr(history, eng.device)
        off = eng._dev(off, torch.int64)[:n_user + 1].contiguous()
        if off.shape[0] != n_user + 1:
            raise ValueError("InteractionGraph: the history has %d rows, n_user is %d" % (off.shape[0] - 1, n_user))
        items = eng._dev(items, torch.int32)[:int(off[-1])].contiguous()
        by_user = (off, items)
        by_item = als.transpose_sets(by_user, n_user, n_item, eng)
        return cls(by_user, by_item, cls._scale(off), cls._scale(by_item[0]), n_user, n_item, engine)

    @staticmethod
    def _scale(off):
        deg = (off[1:] - off[:-1]).double()
        return torch.where(deg > 0, deg.clamp(min=1.0).pow(-0.5), torch.zeros_like(deg)).float()

    def engine(self, tab):
        if tab.shape[-1] not in WIDTHS:
            raise ValueError("graph propagation exists at d = 32 / 64 / 128, got d = %d" % tab.shape[-1])
        if self._engine is not None and self._engine.d == tab.shape[-1]:
            return self._engine
        from .engine import get_engine
        return get_engine(self.device, tab.shape[-1])

    def _check(self, user_tab, item_tab):
        if user_tab.shape[0] != self.n_user or item_tab.shape[0] != self.n_item or user_tab.shape[1:] != item_tab.shape[1:]:
            raise ValueError("expected tables [%d, d] and [%d, d], got %s and %s"
                             % (self.n_user, self.n_item, tuple(user_tab.shape), tuple(item_tab.shape)))

    def layer(self, user_tab, item_tab):
        """(U', I'): one symmetric-normalised hop of fp32 or fp16 tables, as float32.  No autograd (propagate has it)."""
        self._check(user_tab, item_tab)
        eng = self.engine(user_tab)
        return (eng.graph_propagate(item_tab.detach(), self.by_user, a=self.du, b=self.di),
                eng.graph_propagate(user_tab.detach(), self.by_item, a=self.di, b=self.du))

    def _weights(self, layers, weights):
        layers = int(layers)
        if layers < 0:
            raise ValueError("layers must be >= 0, got %d" % layers)
        if weights is None:
            return [1.0 / (layers + 1)] * (layers + 1)
        weights = [float(w) for w in weights]
        if len(weights) != layers + 1:
            raise ValueError("weights holds one value per layer 0 .. %d, got %d" % (layers, len(weights)))
        return weights

    def _read_out(self, user_tab, item_tab, weights):
        """sum_l w_l E^(l) over l = 0 .. len(weights) - 1, the sum taken in torch in ascending l (a product, then an add, per
        layer).  Layer 1 reads the tables as they are, later layers read float32."""
        u, i = user_tab, item_tab
        out_u, out_i = weights[0] * u.float(), weights[0] * i.float()
        for w in weights[1:]:
            u, i = self.layer(u, i)
            out_u, out_i = out_u + w * u, out_i + w * i
        return out_u, out_i

    def propagate(self, user_tab, item_tab, layers=3, weights=None):
        """The float32 tables sum_l w_l E^(l), l = 0 .. layers (default w_l = 1 / (layers + 1); layers = 0 returns the inputs
        widened, times w_0).  fp32 tables that require grad get their gradients: the backward pass is the same read-out applied
        to the incoming gradients."""
        self._check(user_tab, item_tab)
        weights = self._weights(layers, weights)
        if torch.is_grad_enabled() and (user_tab.requires_grad or item_tab.requires_grad):
            if user_tab.dtype != torch.float32 or item_tab.dtype != torch.float32:
                raise ValueError("propagate is differentiable for float32 tables only")
            return _Propagate.apply(self, weights, user_tab, item_tab)
        return self._read_out(user_tab.detach(), item_tab.detach(), weights)


class _Propagate(torch.autograd.Function):
    """The read-out as one differentiable op.  With P the hop, P (U, I) = (Pu I, Pu^T U), the block operator is symmetric: the
    transpose of the user half is the item half -- the call on the other CSR with a and b swapped -- so the gradient of
    sum_l w_l P^l E with respect to E is sum_l w_l P^l applied to the incoming gradients."""

    @staticmethod
    def forward(ctx, graph, weights, user_tab, item_tab):
        ctx.graph, ctx.weights = graph, weights
        return graph._read_out(user_tab.detach(), item_tab.detach(), weights)

    @staticmethod
    def backward(ctx, g_user, g_item):
        gu, gi = ctx.graph._read_out(g_user.contiguous(), g_item.contiguous(), ctx.weights)
        return None, None, gu, gi


class LightGCN(MFbasemode):
    """LightGCN (He et al. 2020): the tables are the layer-0 embeddings, every score is taken on the propagated rows.  `layers`
    follows the paper, it is not a tuned value."""

    def __init__(self, num_user=0, num_item=0, laten_factor=32, layers=3):
        super(LightGCN, self).__init__(num_user, num_item, laten_factor)
        self.layers = int(layers)
        self.graph = None

    def set_graph(self, history):
        """history: an InteractionGraph, or the users' sets (anything as_csr takes) on the model's device."""
        if not isinstance(history, InteractionGraph):
            from .mf import _engine_for
            history = InteractionGraph.build(history, self.user_num, self.item_num, engine=_engine_for(self))
        self.graph = history
        return self

    def propagated(self):
        """(U, I): the float32 read-out of the current tables (differentiable when they are float32 and require grad)."""
        if self.graph is None:
            raise RuntimeError("LightGCN: set_graph(history) first")
        return self.graph.propagate(self.user_laten.weight, self.item_laten.weight, self.layers)

    def forward(self, user, item, neg_item):
        """(bpr, l2): -mean logsigmoid(s+ - s-) on the propagated rows, and half the mean squared norm of the three layer-0 rows."""
        dev = self.user_laten.weight.device
        user, item, neg_item = (torch.as_tensor(x).to(dev).long() for x in (user, item, neg_item))
        pu, pi = self.propagated()
        ue = pu[user]
        score = (ue * pi[item]).sum(-1) - (ue * pi[neg_item]).sum(-1)
        bpr = -torch.nn.functional.logsigmoid(score).mean()
        u0, i0, n0 = self.user_laten.weight[user].float(), self.item_laten.weight[item].float(), self.item_laten.weight[neg_item].float()
        l2 = 0.5 * (u0.pow(2).sum(-1) + i0.pow(2).sum(-1) + n0.pow(2).sum(-1)).mean()
        return bpr, l2

    def materialise(self):
        """An MFbasemode holding the propagated tables in this model's element type: recommend, test_users, similar_items,
        ItemIndex, fold_in_* and every other call of MFbasemode then work on the LightGCN scores unchanged."""
        w = self.user_laten.weight
        with torch.no_grad():
            pu, pi = self.propagated()
            out = MFbasemode(self.user_num, self.item_num, self.hidden_dim).to(device=w.device, dtype=w.dtype)
            out.user_laten.weight.copy_(pu)
            out.item_laten.weight.copy_(pi)
            out.user_bais.weight.copy_(self.user_bais.weight)
            out.item_bais.weight.copy_(self.item_bais.weight)
        return out


def fit(model, history, epochs, batch=8192, lr=1e-3, reg=1e-4, seed=0):
    """The LightGCN baseline: a plain torch Adam loop over the pairs of history (shuffled per epoch, batches of `batch`), one
    uniform negative outside the user's set per pair, loss = bpr + reg * l2.  Returns the loss of every step.  lr and reg follow
    the paper, they are not tuned values."""
    model.set_graph(history)
    g = model.graph
    dev = g.device
    off, items = g.by_user
    if items.shape[0] and int((off[1:] - off[:-1]).max()) >= g.n_item:
        raise ValueError("fit: a user holds every item, so it has no negative")
    users = torch.repeat_interleave(torch.arange(g.n_user, device=dev), off[1:] - off[:-1])
    items = items.long()
    keys = users * g.n_item + items                      # ascending: the CSR's own order
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    opt = torch.optim.Adam([model.user_laten.weight, model.item_laten.weight], lr=lr)
    losses = []
    for _ in range(int(epochs)):
        perm = torch.randperm(users.shape[0], device=dev, generator=gen)
        for b0 in range(0, perm.shape[0], int(batch)):
            idx = perm[b0:b0 + int(batch)]
            u, i = users[idx], items[idx]
            neg = torch.randint(0, g.n_item, u.shape, device=dev, generator=gen)
            while True:
                k = u * g.n_item + neg
                at = torch.searchsorted(keys, k).clamp(max=keys.shape[0] - 1)
                taken = keys[at] == k
                if not bool(taken.any()):
                    break
                neg = torch.where(taken, torch.randint(0, g.n_item, u.shape, device=dev, generator=gen), neg)
            bpr, l2 = model(u, i, neg)
            loss = bpr + reg * l2
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    return torch.stack(losses).tolist() if losses else []
