"""Full-catalogue retrieval helpers: the Seen-items exclusion set of sml_full_rank / sml_topk_items, and the item filter
of their _filtered forms.

SeenItems keeps, per user, the items to leave out of recommendations and full-catalogue ranks (typically everything
the user interacted with in earlier periods) as a CSR over users:

    seen_off    int64 [n_user + 1]
    seen_items  int32, ascending and unique inside each user's range [seen_off[u], seen_off[u + 1])

It is built on the host with numpy (a unique over the key u * n_item + i) and touches no random number generator.
DeviceSeen has the same surface with the set built and grown on the device (the interaction-set calls of include/sml_hip.h).

ItemFilter restricts a call to a subset of the catalogue, for every user alike: a bitmap over the items,

    allow  uint32 [ceil(n_item / 32)], bit i & 31 of word i >> 5 set <=> item i may appear

(bits at positions >= n_item of the last word are ignored by the kernels; ItemFilter keeps them 0).  A filtered call
returns what the unfiltered call returns with the complement of the filter added to every user's Seen range.

ItemScore describes per-item score terms: a call given one ranks by A(u, i) = fmaf(S(u, i), scale[i], offset[i]) instead of
the bare dot product S (include/sml_hip.h, the sml_*_adjusted entry points) -- an item bias is an offset, the cosine a scale.
On the device the terms are one padded table,

    adj  float32 [2, n_pad], n_pad = 32 * ceil(n_item / 32): plane 0 scale, plane 1 offset (pad entries are ignored)

Candidates / CandidateRows / as_candidates describe per-user candidate lists, the allow list of one user each that
sml_topk_candidates orders (HipEngine.topk_candidates, MFbasemode.recommend(candidates=), MFbasemode.test_lists): a ragged
(cand_off, cand_items) pair or a dense matrix read in place, e.g. the rows [user, positive, negatives] of a test set.

ItemIndex is a clustered (inverted-file) index over the item table: k-means lists built on the device, so that
MFbasemode.recommend(index=) scores only the members of each user's nearest lists (HipEngine.ivf_search) instead of the
catalogue; sml_amd.evaluation.index_recall measures what that costs.
"""
import os

import numpy as np
import torch


class SeenItems(object):
    def __init__(self, n_user, n_item):
        self.n_user, self.n_item = int(n_user), int(n_item)
        self._keys = np.zeros(0, dtype=np.int64)     # sorted unique u * n_item + i
        self._host = None
        self._dev = {}

    def add(self, pairs):
        """Union in an int array [m, 2] of (user, item); duplicates are allowed."""
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            return self
        if pairs.ndim != 2 or pairs.shape[1] < 2:
            raise ValueError("expected (user, item) pairs [m, 2], got shape %s" % (pairs.shape,))
        u, i = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
        if u.min() < 0 or u.max() >= self.n_user or i.min() < 0 or i.max() >= self.n_item:
            raise ValueError("pair out of range (n_user=%d, n_item=%d)" % (self.n_user, self.n_item))
        self._keys = np.union1d(self._keys, u * self.n_item + i)
        self._host = None
        self._dev = {}
        return self

    def host(self):
        """(seen_off int64 [n_user + 1], seen_items int32) numpy arrays."""
        if self._host is None:
            u = self._keys // self.n_item
            off = np.zeros(self.n_user + 1, dtype=np.int64)
            np.cumsum(np.bincount(u, minlength=self.n_user), out=off[1:])
            self._host = (off, (self._keys - u * self.n_item).astype(np.int32))
        return self._host

    def device(self, device):
        """The cached (seen_off, seen_items) tensors on `device`; rebuilt only after an add."""
        key = str(torch.device(device))
        if key not in self._dev:
            off, items = self.host()
            self._dev[key] = (torch.from_numpy(off).to(device), torch.from_numpy(items).to(device))
        return self._dev[key]

    def __len__(self):
        return int(self._keys.shape[0])

    @classmethod
    def from_periods(cls, root, name, periods, n_user=None, n_item=None):
        """Union of the train/<p>.npy pairs of dataset root/name (the format sml_amd/synth.py documents) over `periods`.
        n_user / n_item default to the dataset's information.npy."""
        base = os.path.join(root, name)
        if n_user is None or n_item is None:
            info = np.load(os.path.join(base, "information.npy"))
            n_user = int(info[1]) if n_user is None else n_user
            n_item = int(info[2]) if n_item is None else n_item
        seen = cls(n_user, n_item)
        for p in periods:
            seen.add(np.load(os.path.join(base, "train", "%d.npy" % p))[:, :2])
        return seen


class DeviceSeen(object):
    """SeenItems with the set resident on the device: the CSR is built and grown there (HipEngine.iset_build /
    iset_union, include/sml_hip.h "interaction sets"), so one add moves at most the pairs themselves to the device and
    reads back a few scalars (the range check, the new nnz); no CSR crosses the bus in either direction.  For any sequence
    of add calls host() equals SeenItems.host() after the same calls, byte for byte.  Any engine of the device serves: the
    set kernels do not depend on its d."""

    def __init__(self, n_user, n_item, engine):
        self.n_user, self.n_item, self.engine = int(n_user), int(n_item), engine
        if not (0 < self.n_user < 2 ** 31 and 0 < self.n_item < 2 ** 31):
            raise ValueError("n_user and n_item must be in (0, 2^31), got %d, %d" % (self.n_user, self.n_item))
        self._off = torch.zeros(self.n_user + 1, device=engine.device, dtype=torch.int64)
        self._items = torch.empty(0, device=engine.device, dtype=torch.int32)

    def _rows(self, pairs):
        """pairs (host array or tensor [m, >= 2]) as checked device rows int64, or None when there are none."""
        if not torch.is_tensor(pairs):
            pairs = np.asarray(pairs)
        if (pairs.numel() if torch.is_tensor(pairs) else pairs.size) == 0:
            return None
        if pairs.ndim != 2 or pairs.shape[1] < 2:
            raise ValueError("expected (user, item) pairs [m, 2], got shape %s" % (tuple(pairs.shape),))
        if not (torch.is_tensor(pairs) and pairs.device == self.engine.device):
            pairs = pairs[:, :2]                 # only the two columns cross the bus
        rows = self.engine._dev(pairs, torch.int64)
        lo, hi = torch.aminmax(rows[:, :2], dim=0)
        u0, i0, u1, i1 = torch.cat([lo, hi]).tolist()        # the one read-back of the check
        if u0 < 0 or u1 >= self.n_user or i0 < 0 or i1 >= self.n_item:
            raise ValueError("pair out of range (n_user=%d, n_item=%d)" % (self.n_user, self.n_item))
        return rows

    def add(self, pairs):
        """Union in an int array or tensor [m, >= 2] of (user, item) rows, on the host or already on the device (a
        DeviceRows' .rows works; further columns are ignored); duplicates are allowed."""
        rows = self._rows(pairs)
        if rows is None:
            return self
        new = self.engine.iset_build(rows, self.n_user, self.n_item)
        self._off, self._items = new if len(self) == 0 else self.engine.iset_union((self._off, self._items), new, self.n_user)
        return self

    def device(self, device=None):
        """(seen_off, seen_items) on the engine's device; seen_items is trimmed to nnz (one entry when empty, as the
        retrieval calls expect both arrays)."""
        if device is not None:
            d = torch.device(device)
            if d.type != self.engine.device.type or (d.index is not None and d.index != self.engine.device.index):
                raise ValueError("this DeviceSeen lives on %s, not on %s" % (self.engine.device, d))
        items = self._items if len(self) else torch.zeros(1, device=self.engine.device, dtype=torch.int32)
        return self._off, items

    def host(self):
        """(seen_off int64 [n_user + 1], seen_items int32) numpy arrays: the pair SeenItems.host() returns."""
        return self._off.cpu().numpy(), self._items.cpu().numpy()

    def __len__(self):
        return int(self._items.shape[0])

    def contains(self, pairs):
        """bool tensor [m] on the device: whether each (user, item) row of `pairs` is in the set."""
        rows = self._rows(pairs)
        if rows is None:
            return torch.zeros(0, device=self.engine.device, dtype=torch.bool)
        return self.engine.iset_contains(rows, (self._off, self._items))

    @classmethod
    def from_periods(cls, root, name, periods, engine, n_user=None, n_item=None):
        """SeenItems.from_periods with the set on the engine's device: one add per period's train/<p>.npy."""
        base = os.path.join(root, name)
        if n_user is None or n_item is None:
            info = np.load(os.path.join(base, "information.npy"))
            n_user = int(info[1]) if n_user is None else n_user
            n_item = int(info[2]) if n_item is None else n_item
        seen = cls(n_user, n_item, engine)
        for p in periods:
            seen.add(np.load(os.path.join(base, "train", "%d.npy" % p))[:, :2])
        return seen

    @classmethod
    def from_seen(cls, seen, engine):
        """Continue from a host SeenItems: its CSR is uploaded once."""
        out = cls(seen.n_user, seen.n_item, engine)
        off, items = seen.host()
        out._off, out._items = engine._dev(off, torch.int64), engine._dev(items, torch.int32)
        return out


def held_out(pairs, n_user, n_item):
    """T(u), the held-out items of every user of a test period: the (user, item) columns of `pairs` [m, >= 2] (further
    columns, e.g. sampled negatives, are ignored) as a SeenItems -- a per-user ascending, duplicate-free CSR."""
    pairs = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs)
    return SeenItems(n_user, n_item).add(pairs[:, :2] if pairs.size else pairs)


def nonempty_users(sets):
    """(users int64 [n], pos_off int64 [n + 1], pos_items int32 [n_pos]) of the users with at least one item in `sets` (a
    SeenItems or a (off, items) CSR over all users), ascending by user: what HipEngine.user_ranks takes."""
    off, items = sets.host() if isinstance(sets, (SeenItems, DeviceSeen)) else \
        (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in sets)
    off = np.asarray(off, dtype=np.int64)
    users = np.nonzero(np.diff(off) > 0)[0].astype(np.int64)
    pos_off = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(off[users + 1] - off[users], out=pos_off[1:])
    return users, pos_off, np.asarray(items, dtype=np.int32)[off[0]:off[-1]]


def as_csr(exclude, device):
    """exclude: None, a SeenItems, a DeviceSeen, or a (seen_off, seen_items) pair -> what the engine's retrieval calls take."""
    if exclude is None:
        return None
    if isinstance(exclude, (SeenItems, DeviceSeen)):
        return exclude.device(device)
    off, items = exclude
    return torch.as_tensor(off), torch.as_tensor(items)


class ItemFilter(object):
    """The items a retrieval call may return or count, as the catalogue bitmap of include/sml_hip.h (sml_*_filtered).
    A new filter allows nothing; allow / deny / from_mask edit it on the host with numpy."""

    def __init__(self, n_item):
        self.n_item = int(n_item)
        if self.n_item <= 0:
            raise ValueError("n_item must be positive, got %d" % self.n_item)
        self._mask = np.zeros(self.n_item, dtype=bool)
        self._dev = {}

    def _ids(self, ids):
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
        if ids.size == 0:
            return ids.astype(np.int64)
        if ids.dtype.kind not in "iu":
            raise ValueError("item ids must be integers, got %s" % ids.dtype)
        ids = ids.astype(np.int64)
        if ids.min() < 0 or ids.max() >= self.n_item:
            raise ValueError("item id out of range (n_item=%d)" % self.n_item)
        return ids

    def _set(self, ids, value):
        self._mask[self._ids(ids)] = value
        self._dev = {}
        return self

    def allow(self, ids):
        """Add `ids` (duplicates allowed) to the allowed items."""
        return self._set(ids, True)

    def deny(self, ids):
        """Remove `ids` from the allowed items."""
        return self._set(ids, False)

    @classmethod
    def from_mask(cls, mask):
        """mask: bool [n_item], True = allowed."""
        mask = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)
        if mask.dtype != np.bool_ or mask.ndim != 1:
            raise ValueError("expected a bool mask [n_item], got %s %s" % (mask.dtype, mask.shape))
        f = cls(mask.shape[0])
        f._mask = mask.copy()
        return f

    def mask(self):
        """bool [n_item] copy: True = allowed."""
        return self._mask.copy()

    def host(self):
        """The words, uint32 [ceil(n_item / 32)] (tail bits 0)."""
        b = np.packbits(self._mask, bitorder="little")
        b = np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)])
        return b.view("<u4").astype(np.uint32)

    def device(self, device):
        """The cached int32 word tensor (the same bits) on `device`; rebuilt only after an edit."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.host().view(np.int32)).to(device)
        return self._dev[key]

    def __len__(self):
        return int(self._mask.sum())


def filter_words(n_item):
    return (int(n_item) + 31) // 32


def as_filter(x, n_item, device):
    """x: None, an ItemFilter, a bool mask [n_item] (numpy or tensor), or a ready int32 word tensor
    [ceil(n_item / 32)] -> the int32 word tensor on `device` the engine's retrieval calls take as allow= (None: no filter)."""
    if x is None:
        return None
    if isinstance(x, ItemFilter):
        if x.n_item != int(n_item):
            raise ValueError("the filter is over %d items, the catalogue has %d" % (x.n_item, n_item))
        return x.device(device)
    if torch.is_tensor(x) and x.dtype == torch.int32:
        if x.dim() != 1 or x.shape[0] != filter_words(n_item):
            raise ValueError("an item filter over %d items has %d words, got shape %s" % (n_item, filter_words(n_item), tuple(x.shape)))
        return x.to(device).contiguous()
    m = np.asarray(x.cpu() if torch.is_tensor(x) else x)
    if m.dtype != np.bool_ or m.shape != (int(n_item),):
        raise ValueError("an item filter is None, an ItemFilter, a bool mask [n_item] or int32 words, got %s %s" % (m.dtype, m.shape))
    return ItemFilter.from_mask(m).device(device)


def adjust_len(n_item):
    """n_pad: the floats of one plane of the padded term table of n_item items."""
    return (int(n_item) + 31) // 32 * 32


class ItemScore(object):
    """Per-item score terms of a retrieval call, described on the host with numpy: A(u, i) = fmaf(S(u, i), scale[i],
    offset[i]) (include/sml_hip.h).  A new ItemScore is neutral (scale 1, offset +0).  scale / offset / bias / cosine edit it
    and return it; any float may be given: an offset of -inf sends an item to the end of every list, a NaN removes it."""

    def __init__(self, n_item):
        self.n_item = int(n_item)
        if self.n_item <= 0:
            raise ValueError("n_item must be positive, got %d" % self.n_item)
        self._scale = None               # None: 1 everywhere
        self._offset = None              # None: +0 everywhere
        self._cosine = False
        self._dev = {}

    def _values(self, values, what, column=False):
        v = np.asarray(values.detach().cpu() if torch.is_tensor(values) else values)
        if v.dtype.kind not in "fiu":
            raise ValueError("%s must be numbers, got %s" % (what, v.dtype))
        if column and v.shape == (self.n_item, 1):
            v = v[:, 0]
        if v.shape != (self.n_item,):
            raise ValueError("%s must have shape [%d]%s, got %s" % (what, self.n_item, " or [%d, 1]" % self.n_item if column else "",
                                                                    v.shape))
        return np.ascontiguousarray(v, dtype=np.float32)

    def scale(self, values):
        """scale[i] = values[i], float [n_item] (replaces an earlier scale or cosine())."""
        self._scale, self._cosine, self._dev = self._values(values, "scale"), False, {}
        return self

    def offset(self, values):
        """offset[i] = values[i], float [n_item]."""
        self._offset, self._dev = self._values(values, "offset"), {}
        return self

    def bias(self, item_bias):
        """An item bias as the offset: [n_item], or the [n_item, 1] weight of a bias embedding (MFbasemode.item_bais)."""
        self._offset, self._dev = self._values(item_bias, "item_bias", column=True), {}
        return self

    def cosine(self):
        """scale[i] = 1 / ||x_i||, resolved against the item table a call is made with (replaces an earlier scale)."""
        self._scale, self._cosine, self._dev = None, True, {}
        return self

    @property
    def is_cosine(self):
        return self._cosine

    def padded_len(self):
        return adjust_len(self.n_item)

    def host(self):
        """float32 [2, n_pad]: the table with pads (1, 0).  A cosine() score has no host form: its scale needs the table."""
        if self._cosine:
            raise ValueError("a cosine ItemScore is resolved on the device against an item table (ItemScore.device)")
        adj = np.zeros((2, self.padded_len()), np.float32)
        adj[0] = 1.0
        if self._scale is not None:
            adj[0, :self.n_item] = self._scale
        if self._offset is not None:
            adj[1, :self.n_item] = self._offset
        return adj

    def device(self, engine, item_tab=None):
        """The float32 [2, n_pad] table on the engine's device.  Fixed terms are cached and rebuilt only after an edit.  A
        cosine() score is built from item_tab at EVERY call (one small launch over the table) and never cached: training
        writes the tables in place through raw pointers, which no version counter or address records, so a cached norm
        could be stale."""
        if self._cosine:
            if item_tab is None or item_tab.shape[0] != self.n_item:
                raise ValueError("a cosine ItemScore over %d items needs the item table [%d, d]" % (self.n_item, self.n_item))
            return engine.item_adjust_cosine(item_tab, engine.item_adjust(self.n_item, None, self._offset))
        # (the engine's calls always pass their item table; a table built without one is still shape-checked by the call
        # it is handed to)
        if item_tab is not None and item_tab.shape[0] != self.n_item:
            raise ValueError("the score terms are over %d items, the catalogue has %d" % (self.n_item, item_tab.shape[0]))
        key = str(engine.device)
        if key not in self._dev:
            self._dev[key] = engine.item_adjust(self.n_item, self._scale, self._offset)
        return self._dev[key]


def as_score(x, model):
    """x: None or "dot" (the bare dot product), "cosine" (S / ||x_i||, the model's item table), "bias" (S + the model's item
    bias, MFbasemode.item_bais), an ItemScore, or a ready float32 [2, n_pad] table -> what the engine's retrieval calls take as
    adjust= (None: no terms).  "cosine" and "bias" are built on the device from the model's current weights at every call
    (one small launch), so they are never stale."""
    if x is None or (isinstance(x, str) and x == "dot"):
        return None
    if isinstance(x, ItemScore):
        if x.n_item != model.item_laten.weight.shape[0]:
            raise ValueError("the score terms are over %d items, the catalogue has %d" % (x.n_item, model.item_laten.weight.shape[0]))
        return x
    if torch.is_tensor(x):
        return x
    if isinstance(x, str) and x in ("cosine", "bias"):
        from .mf import _engine_for
        eng = _engine_for(model)
        if x == "cosine":
            return eng.item_adjust_cosine(model.item_laten.weight.data)
        return eng.item_adjust(model.item_laten.weight.shape[0], offset=model.item_bais.weight.data[:, 0].float())
    raise ValueError('score= is None, "dot", "cosine", "bias", an ItemScore or a float32 [2, n_pad] table, got %r' % (x,))


class CandidateRows(object):
    """Rows of a test set -- [user, positive, negatives ...], an int64 array / tensor [n, 2 + neg] or a
    sml_amd.evaluation.DeviceRows -- as per-user candidate lists: row x's list is rows[x, first_col:], its user rows[x, 0].
    The rows are read where they are (sml_topk_candidates' dense form): no copy, no int32 conversion."""

    def __init__(self, rows, first_col=1):
        if hasattr(rows, "wait_ready") and hasattr(rows, "rows"):          # a DeviceRows: order behind its upload
            rows.wait_ready()
            rows = rows.rows
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(np.ascontiguousarray(rows))
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.dtype != torch.int64:
            raise ValueError("expected int64 rows [n, 2 + neg], got %s %s" % (rows.dtype, tuple(rows.shape)))
        self.first_col = int(first_col)
        if not 0 <= self.first_col <= rows.shape[1] or rows.shape[1] < 1:
            raise ValueError("first_col %d is outside the %d columns of the rows" % (self.first_col, rows.shape[1]))
        self.rows = rows

    @property
    def users(self):
        return self.rows[:, 0]

    @property
    def geometry(self):
        """(stride, first, cols) of the dense form."""
        return self.rows.shape[1], self.first_col, self.rows.shape[1] - self.first_col


class Candidates(object):
    """Per-user candidate lists as sml_topk_candidates takes them (as_candidates makes one).  items: the int32 / int64 entries
    on the device, contiguous.  Ragged form: off int64 [n + 1], list x = items[off[x] : off[x + 1]].  Dense form (off None):
    list x = items.reshape(-1)[x * stride + first : ... + cols].  users: the rows' own users (CandidateRows) or None."""

    def __init__(self, n, items, off=None, stride=0, first=0, cols=0, users=None):
        self.n, self.items, self.off, self.users = int(n), items, off, users
        self.stride, self.first, self.cols = int(stride), int(first), int(cols)

    def lists(self):
        """The n lists as host int64 arrays (tests, small inputs)."""
        flat = self.items.reshape(-1).cpu().numpy().astype(np.int64)
        if self.off is None:
            return [flat[x * self.stride + self.first:x * self.stride + self.first + self.cols] for x in range(self.n)]
        off = self.off.cpu().numpy()
        return [flat[off[x]:off[x + 1]] for x in range(self.n)]


def _cand_items(x, device):
    """An int array / tensor as contiguous int32 or int64 entries on `device`; a tensor already there is not copied."""
    if not torch.is_tensor(x):
        x = np.asarray(x)
        if x.dtype.kind not in "iu":
            raise ValueError("candidate ids must be integers, got %s" % x.dtype)
        if x.dtype not in (np.int32, np.int64):
            x = x.astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype not in (torch.int32, torch.int64):
        if x.dtype.is_floating_point or x.dtype == torch.bool or x.dtype.is_complex:
            raise ValueError("candidate ids must be integers, got %s" % x.dtype)
        x = x.long()
    x = x.to(device)
    return x if x.is_contiguous() else x.contiguous()


def as_candidates(x, n, device):
    """Per-user candidate lists in any accepted form -> a Candidates on `device`.  x is one of

      a 2-D int32 / int64 array or tensor [n, C]    row x is the list of user x (entries outside [0, n_item), e.g. -1, pad);
      a tuple (cand_off, cand_items)                the ragged form: int64 offsets [n + 1] and the int32 / int64 entries;
      a list of n int sequences                     built into the ragged form (int32 entries when every id fits);
      a CandidateRows, or a DeviceRows (wrapped as CandidateRows(x, first_col=1)), which also supply the users.

    n: the number of users the lists are for, or None to take it from x.  A tensor already on the device is not copied.
    Offsets that come from the host are checked there: length n + 1, from 0, non-decreasing, last at most len(cand_items);
    offsets already on the device are checked for their length only.  Ids are not range-checked: the kernel skips the
    out-of-range ones."""
    device = torch.device(device)
    if isinstance(x, Candidates):
        got = x
    elif hasattr(x, "wait_ready") and hasattr(x, "rows") or isinstance(x, CandidateRows):
        r = x if isinstance(x, CandidateRows) else CandidateRows(x, 1)
        rows = r.rows.to(device)
        rows = rows if rows.is_contiguous() else rows.contiguous()
        stride, first, cols = r.geometry
        got = Candidates(rows.shape[0], rows, None, stride, first, cols, users=rows[:, 0])
    elif isinstance(x, tuple):
        if len(x) != 2:
            raise ValueError("a ragged candidate set is a (cand_off, cand_items) pair, got a tuple of %d" % len(x))
        off, items = x
        items = _cand_items(items, device)
        if items.dim() != 1:
            raise ValueError("cand_items must be 1-D, got shape %s" % (tuple(items.shape),))
        on_host = not (torch.is_tensor(off) and off.device.type != "cpu")
        if on_host:
            h = np.asarray(off.numpy() if torch.is_tensor(off) else off)
            if h.dtype.kind not in "iu" or h.ndim != 1 or h.shape[0] < 1:
                raise ValueError("cand_off must be a 1-D int array [n + 1], got %s %s" % (h.dtype, h.shape))
            h = h.astype(np.int64)
            if h[0] != 0 or (np.diff(h) < 0).any() or h[-1] > items.shape[0]:
                raise ValueError("cand_off must start at 0, never decrease and end at most at len(cand_items) = %d" % items.shape[0])
            off = torch.from_numpy(h)
        elif off.dtype != torch.int64 or off.dim() != 1 or off.shape[0] < 1:
            raise ValueError("cand_off must be int64 [n + 1], got %s %s" % (off.dtype, tuple(off.shape)))
        off = off.to(device)
        got = Candidates(off.shape[0] - 1, items, off if off.is_contiguous() else off.contiguous())
    elif isinstance(x, list):
        parts = [np.asarray(s).reshape(-1) for s in x]
        for p in parts:
            if p.size and p.dtype.kind not in "iu":
                raise ValueError("candidate ids must be integers, got %s" % p.dtype)
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([p.size for p in parts], out=off[1:])
        flat = np.concatenate([p.astype(np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
        if flat.size == 0 or (flat.min() >= -2 ** 31 and flat.max() < 2 ** 31):
            flat = flat.astype(np.int32)
        got = Candidates(len(parts), torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device))
    else:
        items = _cand_items(x, device)
        if items.dim() != 2:
            raise ValueError("dense candidates are a 2-D array [n, C], got shape %s" % (tuple(items.shape),))
        got = Candidates(items.shape[0], items, None, items.shape[1], 0, items.shape[1])
    if n is not None and got.n != int(n):
        raise ValueError("the candidates hold %d lists, the call has %d users" % (got.n, int(n)))
    return got


IVF_MAX_PROBE = 128   # probes per user of sml_ivf_search
IVF_MAX_K = 128       # its longest list


def default_n_list(n_item):
    """round(sqrt(n_item)), at least 1 and at most n_item: the convention ItemIndex.build follows when n_list is None."""
    n_item = int(n_item)
    return max(1, min(n_item, int(round(float(np.sqrt(n_item))))))


class ItemIndex(object):
    """A clustered (inverted-file) index over an item table [n_item, d] (include/sml_hip.h, CLUSTERED INDEX): k-means lists
    of the items, so that a query scores only the members of the lists nearest the user (HipEngine.ivf_search,
    MFbasemode.recommend(index=)).  Three device arrays:

        centroids   [n_list, d] in the table's element type   list_off  int64 [n_list + 1]
        list_items  int32 [n_item]: a partition of the item ids, ascending inside each list

    The index holds no rows and no scores -- search reads the current item table -- so an index built on last period's
    table costs recall on a retrained one, never a wrong score; refresh() moves it along with a couple of iterations.
    metric: how items (and later users) choose lists: "cosine" (the default: spherical assignment, S / ||centroid||) or
    "dot".  The same seed, table and arguments give the same bytes on every run."""

    def __init__(self, centroids, list_off, list_items, metric="cosine", engine=None):
        if metric not in ("cosine", "dot"):
            raise ValueError('metric is "cosine" or "dot", got %r' % (metric,))
        if centroids.dim() != 2 or centroids.dtype not in (torch.float32, torch.float16):
            raise ValueError("centroids are an fp32 or fp16 table [n_list, d], got %s %s" % (centroids.dtype, tuple(centroids.shape)))
        if list_off.dim() != 1 or list_off.shape[0] != centroids.shape[0] + 1 or list_off.dtype != torch.int64:
            raise ValueError("list_off must be int64 [%d], got %s %s" % (centroids.shape[0] + 1, list_off.dtype, tuple(list_off.shape)))
        if list_items.dim() != 1 or list_items.dtype != torch.int32:
            raise ValueError("list_items must be int32 [n_item], got %s %s" % (list_items.dtype, tuple(list_items.shape)))
        self.centroids, self.list_off, self.list_items = centroids, list_off, list_items
        self.metric, self.engine = metric, engine
        self._adj = None

    @property
    def n_list(self):
        return int(self.centroids.shape[0])

    @property
    def n_item(self):
        return int(self.list_items.shape[0])

    @property
    def dtype(self):
        return self.centroids.dtype

    def sizes(self):
        """int64 [n_list]: the lists' lengths (on the index's device)."""
        return self.list_off[1:] - self.list_off[:-1]

    def host(self):
        """{"centroids", "list_off", "list_items"} as numpy arrays."""
        return {"centroids": self.centroids.cpu().numpy(), "list_off": self.list_off.cpu().numpy(),
                "list_items": self.list_items.cpu().numpy()}

    def _check_table(self, item_tab):
        if item_tab.dim() != 2 or item_tab.shape[0] != self.n_item or item_tab.shape[1] != self.centroids.shape[1] or \
                item_tab.dtype != self.dtype:
            raise ValueError("the index is over a %s table [%d, %d], got %s %s"
                             % (self.dtype, self.n_item, self.centroids.shape[1], item_tab.dtype, tuple(item_tab.shape)))

    def _centroid_adjust(self):
        """The metric's score terms over the CENTROID table (None for "dot"); rebuilt only when the centroids change."""
        if self.metric == "dot":
            return None
        if self._adj is None:
            self._adj = self.engine.item_adjust_cosine(self.centroids)
        return self._adj

    def _iterate(self, item_tab, iters):
        """iters times: assign every item to its best centroid, rebuild the lists, move the centroids to their lists' means."""
        eng = self.engine
        n_item = item_tab.shape[0]
        ids = torch.arange(n_item, device=eng.device, dtype=torch.int64)
        for _ in range(int(iters)):
            best, _ = eng.topk_items(item_tab, self.centroids, ids, 1, adjust=self._centroid_adjust())
            assign = best[:, 0].clamp(min=0)            # an item whose every centroid score is NaN joins list 0
            self.list_off, self.list_items = eng.iset_build(torch.stack([assign, ids], 1), self.n_list, n_item)
            self.centroids = eng.ivf_centroids(item_tab, self.list_off, self.list_items, self.centroids)
            self._adj = None
        return self

    @classmethod
    def build(cls, item_tab, n_list=None, iters=10, seed=0, metric="cosine", engine=None):
        """k-means over the rows of item_tab (fp32 or fp16, on the GPU): n_list (None: round(sqrt(n_item))) distinct rows
        drawn by numpy.random.RandomState(seed) start the centroids; then `iters` >= 1 iterations of assign / lists / update."""
        if metric not in ("cosine", "dot"):
            raise ValueError('metric is "cosine" or "dot", got %r' % (metric,))
        if not torch.is_tensor(item_tab) or item_tab.dim() != 2:
            raise ValueError("item_tab is a tensor [n_item, d]")
        n_item = int(item_tab.shape[0])
        n_list = default_n_list(n_item) if n_list is None else int(n_list)
        if not 1 <= n_list <= n_item:
            raise ValueError("n_list must lie in 1..n_item = %d, got %d" % (n_item, n_list))
        if int(iters) < 1:
            raise ValueError("iters must be at least 1, got %d" % int(iters))
        if engine is None:
            from .engine import get_engine
            engine = get_engine(item_tab.device, item_tab.shape[1])
        first = np.random.RandomState(seed).choice(n_item, size=n_list, replace=False).astype(np.int64)
        centroids = item_tab[torch.from_numpy(first).to(item_tab.device)].contiguous()
        idx = cls(centroids, torch.zeros(n_list + 1, device=item_tab.device, dtype=torch.int64),
                  torch.zeros(n_item, device=item_tab.device, dtype=torch.int32), metric, engine)
        return idx._iterate(item_tab, iters)

    def refresh(self, item_tab, iters=2):
        """Continue from the current centroids on a retrained table of the same shape and type: `iters` more iterations, no
        re-initialisation.  On an unchanged table refresh(iters=1) is one more iteration of build."""
        self._check_table(item_tab)
        if int(iters) < 1:
            raise ValueError("iters must be at least 1, got %d" % int(iters))
        return self._iterate(item_tab, iters)

    def probe(self, user_tab, users, nprobe):
        """int32 [n, nprobe]: each user's nprobe best lists by the index's metric against the centroids, best first (-1 past
        n_list): what HipEngine.ivf_search takes.  Seen and item filters do not apply to centroids."""
        nprobe = int(nprobe)
        if not 1 <= nprobe <= IVF_MAX_PROBE:
            raise ValueError("nprobe must lie in 1..%d, got %d" % (IVF_MAX_PROBE, nprobe))
        lists, _ = self.engine.topk_items(user_tab, self.centroids, users, nprobe, adjust=self._centroid_adjust())
        return lists.to(torch.int32)


def index_args(index, nprobe, topK, n_item, dtype, candidates=None):
    """nprobe as MFbasemode.recommend(index=) passes it on (None: min(8, n_list)), checked without a device."""
    if not isinstance(index, ItemIndex):
        raise ValueError("index= is a sml_amd.retrieval.ItemIndex, got %s" % type(index).__name__)
    if candidates is not None:
        raise ValueError("candidates= and index= both name the items to score: give one of them")
    if index.n_item != int(n_item) or index.dtype != dtype:
        raise ValueError("the index is over %d %s items, the model has %d %s" % (index.n_item, index.dtype, int(n_item), dtype))
    if not 1 <= int(topK) <= IVF_MAX_K:
        raise ValueError("topK must lie in 1..%d with an index, got %d" % (IVF_MAX_K, int(topK)))
    nprobe = min(8, index.n_list) if nprobe is None else int(nprobe)
    if not 1 <= nprobe <= IVF_MAX_PROBE:
        raise ValueError("nprobe must lie in 1..%d, got %d" % (IVF_MAX_PROBE, nprobe))
    return nprobe


_SELF_SEEN = {}


def self_seen(n_item, device):
    """The Seen CSR over ITEM ids that excludes every item from its own list (off = arange(n_item + 1), items =
    arange(n_item)), built on the device: similar_items' self-exclusion.  One is kept per device, for the catalogue size
    asked for last (12 bytes per item), so a catalogue that grows from period to period does not pile them up."""
    key = str(torch.device(device))
    hit = _SELF_SEEN.get(key)
    if hit is None or hit[0] != int(n_item):
        hit = _SELF_SEEN[key] = (int(n_item), (torch.arange(n_item + 1, device=device, dtype=torch.int64),
                                              torch.arange(n_item, device=device, dtype=torch.int32)))
    return hit[1]


DEEP_MAX = 1024      # SML_TOPK_DEEP_MAX: the longest list of sml_topk_deep
# HipEngine.topk_items hands a call with DEEP_FROM <= k <= 128 to the deep kernels (the bytes are equal, so the choice is invisible).
# The rule: the smallest probed k from which the deep call's median is below sml_topk_items' minimum at all three widths of
# profiles/r20_deep_topk_probe.json; 129 = never.  Measured there (60,000 users x 123,000 items): at k = 20 the sorted lists win
# (25 / 34 / 41 ms against 70 / 98 / 169 ms); at k = 64 the deep call does (70 / 98 / 169 ms against 228 / 235 / 245 ms), and at
# k = 100 by nine times.  The rule's answer is 64.  OPEN ITEM: the constant is NOT set by the rule but is the next probed k, 100,
# because tests/test_retrieval_gpu.py::test_chunked_topk_equals_one_call holds k = 65 to sml_topk_items' own chunked calls; until
# that test counts its calls at a k below the threshold, 64 <= k < 100 stays three to nine times slower than topk_deep.
DEEP_FROM = 100


def deep_args(k):
    """k as HipEngine.topk_deep passes it on, checked without a device: an integer in 1..1024."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer in 1..%d, got %r" % (DEEP_MAX, k))
    k = int(k)
    if not 1 <= k <= DEEP_MAX:
        raise ValueError("k must lie in 1..%d, got %d" % (DEEP_MAX, k))
    return k


RERANK_MAX = 128     # pool entries and picks per list of sml_rerank_mmr


def rerank_args(k, lam, metric="cosine", pool_cols=None):
    """(k, lam) as HipEngine.rerank_mmr passes them on, checked without a device: 1 <= k <= 128, lam a number in [0, 1],
    metric "cosine" or "dot", and, when given, 1 <= pool_cols <= 128."""
    k = int(k)
    if not 1 <= k <= RERANK_MAX:
        raise ValueError("k must lie in 1..%d, got %d" % (RERANK_MAX, k))
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:                     # (NaN fails both comparisons)
        raise ValueError("lam must lie in [0, 1], got %r" % (lam,))
    if metric not in ("cosine", "dot"):
        raise ValueError('metric is "cosine" or "dot", got %r' % (metric,))
    if pool_cols is not None and not 1 <= int(pool_cols) <= RERANK_MAX:
        raise ValueError("a pool holds 1..%d entries per list, got %d" % (RERANK_MAX, int(pool_cols)))
    return k, lam


def diversify_args(topK, diversify, pool, metric):
    """The pool size of MFbasemode.recommend(diversify=): `pool` or min(128, 5 * topK), checked without a device."""
    topK = int(topK)
    pool = min(RERANK_MAX, 5 * topK) if pool is None else int(pool)
    if pool > RERANK_MAX:
        raise ValueError("pool must not exceed %d, got %d" % (RERANK_MAX, pool))
    if topK > pool:
        raise ValueError("topK = %d exceeds the pool of %d" % (topK, pool))
    rerank_args(topK, diversify, metric, pool)
    return pool
