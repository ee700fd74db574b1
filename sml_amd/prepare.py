"""Test-set preparation: the negatives of every test row, sampled on the device.

The reference writes its `test/<p>.npy` files -- rows (user, positive, neg_num negatives), the source of the MF stage's
pre-sampled negatives, the TR stage's rows and the sampled evaluation -- with data/dataset2.py select_neg_forinteraction, a
Python loop over every interaction.  This module is that step on the GPU: the same distribution (a row's negatives are a
uniformly random neg_num-subset, in uniformly random order, of the items that exist as of that row and that its user has not
interacted with as of that row), fixed to the byte by a counter-based stream instead of numpy's (include/sml_hip.h,
"test-set negatives"; DESIGN.md, "Test-set negatives on the device").

    Timeline(periods, n_user, n_item, engine)      the whole stream's catalogue order and per-user histories, on the device
    period_negatives(timeline, p, ...)             one period's rows with their negatives, a device tensor
    select_neg_forinteraction(path, name, files)   the reference's function: reads train/<f>.npy, writes test/<i>.npy

    python -m sml_amd.prepare --data_path dataset/ --data_name yelp --periods 40

Without a GPU the same bytes come from the library's single-threaded host walk (sml_host_neg_sets): pass engine="host"
(--host on the command line).  That route is asked for, never fallen back to.
"""
import argparse
import collections
import os
import sys

import numpy as np
import torch

from . import _lib

HOST = "host"
TimelineArrays = collections.namedtuple("TimelineArrays", "order n_cat h_off h_items h_since")


class Timeline(object):
    """What every row of the stream needs to draw its negatives, built once from all periods (the stream is their
    concatenation; row g is a global position):

        order     int32 [n_items_seen]   the items by first appearance: the catalogue as of row g is order[0 .. n_cat(g))
        n_cat     one int32 [n_p] per period (views of n_cat_all [total]): |C(g)|, row g's own item included
        h_off     int64 [n_user + 1]     } the CSR of the distinct (user, item) pairs, items ascending per user, with the
        h_items   int32 [n_pairs]        } global position of each pair's first row: user u's history as of row g is the
        h_since   int32 [n_pairs]        } entries of its range with h_since <= g
        room      int32 [total]          |C(g)| - |H(g)|: the largest neg_num row g can be served with

    all resident on the engine's device (engine="host": in host memory).  Plumbing, not a hot path: two stable sorts and a
    few scans in torch on that device; no host loop over rows.  periods: arrays or tensors int [n_p, >= 2] (columns 0 and 1),
    on the host or on the device.  The ids are range-checked here (one read-back) with SeenItems' error."""

    def __init__(self, periods, n_user, n_item, engine):
        self.n_user, self.n_item, self.engine = int(n_user), int(n_item), (None if engine in (None, HOST) else engine)
        if not (0 < self.n_user < 2 ** 31 and 0 < self.n_item < 2 ** 31):
            raise ValueError("n_user and n_item must be in (0, 2^31), got %d, %d" % (self.n_user, self.n_item))
        dev = self.device = self.engine.device if self.engine is not None else torch.device("cpu")
        parts = []
        for p in periods:
            if not torch.is_tensor(p):
                p = np.asarray(p)
            if p.ndim != 2 or p.shape[1] < 2:
                raise ValueError("expected (user, item) rows [n, >= 2], got shape %s" % (tuple(p.shape),))
            p = p[:, :2]                                   # only the two columns cross the bus
            if not torch.is_tensor(p):
                p = torch.from_numpy(np.ascontiguousarray(p))
            parts.append(p.to(device=dev, dtype=torch.int64))
        rows = torch.cat(parts).contiguous() if parts else torch.zeros((0, 2), device=dev, dtype=torch.int64)
        self.total = total = int(rows.shape[0])
        if total >= 2 ** 31:
            raise ValueError("the stream has %d rows; positions must stay below 2^31" % total)
        self.g0 = [0]
        for p in parts:
            self.g0.append(self.g0[-1] + int(p.shape[0]))
        self.rows = [rows[a:b] for a, b in zip(self.g0[:-1], self.g0[1:])]
        user, item = rows[:, 0], rows[:, 1]
        if total:
            lo, hi = torch.aminmax(rows, dim=0)
            u0, i0, u1, i1 = torch.cat([lo, hi]).tolist()
            if u0 < 0 or u1 >= self.n_user or i0 < 0 or i1 >= self.n_item:
                raise ValueError("pair out of range (n_user=%d, n_item=%d)" % (self.n_user, self.n_item))

        def heads(sorted_keys):
            h = torch.ones(total, device=dev, dtype=torch.bool)
            if total > 1:
                h[1:] = sorted_keys[1:] != sorted_keys[:-1]
            return h

        # catalogue: a stable sort by item puts each item's first position at the head of its run
        s_item, idx = torch.sort(item, stable=True)
        first_pos = torch.sort(idx[heads(s_item)]).values
        self.order = item[first_pos].to(torch.int32)
        flag = torch.zeros(total, device=dev, dtype=torch.int32)
        flag[first_pos] = 1
        self.n_cat_all = torch.cumsum(flag, 0).to(torch.int32)
        self.n_cat = [self.n_cat_all[a:b] for a, b in zip(self.g0[:-1], self.g0[1:])]
        # histories: the same over the key u * n_item + i; the sorted heads ARE the CSR
        s_key, idx = torch.sort(user * self.n_item + item, stable=True)
        head = heads(s_key)
        keys, since = s_key[head], idx[head]
        self.h_items = (keys % self.n_item).to(torch.int32)
        self.h_since = since.to(torch.int32)
        self.h_off = torch.searchsorted(torch.div(keys, self.n_item, rounding_mode="floor").contiguous(),
                                        torch.arange(self.n_user + 1, device=dev, dtype=torch.int64)).to(torch.int64)
        # |H(g)|: the pairs of row g's user that began at or before g = a running count of first rows inside the user
        flag.zero_()
        flag[since] = 1
        s_user, idx = torch.sort(user, stable=True)
        hist = torch.cumsum(flag[idx].to(torch.int64), 0) - self.h_off[s_user]
        self.room = torch.empty(total, device=dev, dtype=torch.int32)
        self.room[idx] = (self.n_cat_all[idx].to(torch.int64) - hist).to(torch.int32)

    def __len__(self):
        return len(self.rows)

    def host(self):
        """The numpy arrays (order, n_cat [total], h_off, h_items, h_since), a TimelineArrays."""
        return TimelineArrays(*(t.cpu().numpy() for t in (self.order, self.n_cat_all, self.h_off, self.h_items, self.h_since)))


def _host_neg_sets(timeline, p, neg_num, seed):
    lib = _lib.load()
    rows = timeline.rows[p].contiguous().numpy()
    n = rows.shape[0]
    a = [t.contiguous().numpy() for t in (timeline.n_cat[p], timeline.order, timeline.h_off, timeline.h_items, timeline.h_since)]
    out = np.empty((n, 2 + max(int(neg_num), 0)), dtype=np.int64)
    failed = np.zeros(1, dtype=np.int32)
    _lib.check(lib.sml_host_neg_sets(rows.ctypes.data, n, rows.shape[1], timeline.g0[p], a[0].ctypes.data, a[1].ctypes.data,
                                     a[2].ctypes.data, timeline.n_user, a[3].ctypes.data, a[4].ctypes.data, int(neg_num),
                                     int(seed) & (2 ** 64 - 1), out.ctypes.data, failed.ctypes.data), "sml_host_neg_sets")
    return torch.from_numpy(out), int(failed[0])


def period_negatives(timeline, p, neg_num=999, seed=2000, allow_short=False):
    """int64 tensor [n_p, 2 + neg_num] on the timeline's device: period p's rows (user, item) followed by their negatives --
    the contents of test/<p>.npy, and what DeviceRows and the evaluation calls take.  `seed` keys the whole preparation, a
    row's global position its own draws, so a period's result does not depend on which other periods are asked for.  One
    read-back: the count of rows that could not be served (fewer than neg_num eligible items).  Such a period raises
    ValueError unless allow_short, which returns it with -1 in the unfilled slots."""
    p, neg_num = int(p), int(neg_num)
    if not 0 <= p < len(timeline):
        raise ValueError("period %d is outside the timeline's %d" % (p, len(timeline)))
    if not 1 <= neg_num <= 4096:
        raise ValueError("neg_num must be in 1 .. 4096, got %d" % neg_num)
    if timeline.engine is None:
        out, n_failed = _host_neg_sets(timeline, p, neg_num, seed)
    else:
        out, failed = timeline.engine.neg_sets(timeline.rows[p], timeline.g0[p], timeline, neg_num, seed)
        n_failed = int(failed)                          # the one read-back
    if n_failed and not allow_short:
        fits = int(timeline.room[timeline.g0[p]:timeline.g0[p + 1]].min())
        raise ValueError("%d of the %d rows of period %d could not get %d negatives: the smallest row has %d eligible items "
                         "(neg_num <= %d fits every row of this period)" % (n_failed, out.shape[0], p, neg_num, fits, fits))
    return out


def _engine(engine):
    if engine is not None:
        return engine
    from .engine import get_engine
    return get_engine("cuda:0", 32)                     # (the width plays no part)


def select_neg_forinteraction(path='dataset/', datasetname='News', file_path_list=None, leave_for_init_train=0.7, neg_num=999,
                              seed=2000, engine=None):
    """reference data/dataset2.py:356-414 on the device: reads <path><datasetname>/train/<f>.npy for every name of
    file_path_list (<path><datasetname>/<f>.npy when that is where the file lies, as the reference has them) and writes
    <path><datasetname>/test/<i>.npy -- int64 [n, 2 + neg_num] -- for the list positions i >= round(len * leave_for_init_train).
    The same distribution as the reference, not numpy's random stream: `seed` replaces np.random.seed.  engine: a HipEngine
    (default: cuda:0's), or "host" for the single-threaded host walk.  Returns the paths written."""
    base = path + datasetname
    periods = []
    for f in file_path_list:
        name = os.path.join(base, "train", "%s.npy" % f)
        if not os.path.exists(name):
            name = os.path.join(base, "%s.npy" % f)
        periods.append(np.load(name)[:, :2])
    info = os.path.join(base, "information.npy")
    if os.path.exists(info):
        n_user, n_item = (int(x) for x in np.load(info)[1:3])
    else:
        n_user, n_item = (1 + max(int(p[:, c].max()) for p in periods if p.size) for c in (0, 1))
    start = round(len(periods) * leave_for_init_train)
    timeline = Timeline(periods, n_user, n_item, engine if engine == HOST else _engine(engine))
    os.makedirs(os.path.join(base, "test"), exist_ok=True)
    written = []
    for i in range(start, len(periods)):
        out = period_negatives(timeline, i, neg_num, seed)
        written.append(os.path.join(base, "test", "%d.npy" % i))
        np.save(written[-1], out.cpu().numpy())
    return written


def get_parse():
    ap = argparse.ArgumentParser(prog="python -m sml_amd.prepare",
                                 description="Write test/<p>.npy (rows with sampled negatives) from train/<p>.npy.")
    ap.add_argument("--data_path", default="dataset/", help="dataset root, with its trailing separator")
    ap.add_argument("--data_name", required=True, help="dataset directory under the root")
    ap.add_argument("--periods", type=int, required=True, help="number of periods: the files train/0.npy .. train/<N-1>.npy")
    ap.add_argument("--leave", type=float, default=0.7, help="share of the periods kept for initial training (no test file)")
    ap.add_argument("--neg_num", type=int, default=999, help="negatives per row")
    ap.add_argument("--seed", type=int, default=2000, help="keys the whole preparation")
    ap.add_argument("--cuda", type=int, default=0, help="which GPU")
    ap.add_argument("--host", action="store_true", help="the library's single-threaded host walk instead of the GPU (same bytes)")
    return ap


def main(argv=None):
    args = get_parse().parse_args(argv)
    if args.host:
        engine = HOST
    else:
        from .engine import get_engine
        engine = get_engine("cuda:%d" % args.cuda, 32)
    written = select_neg_forinteraction(args.data_path, args.data_name, [str(i) for i in range(args.periods)], args.leave,
                                        args.neg_num, args.seed, engine)
    for w in written:
        print(w)
    return 0


if __name__ == "__main__":
    sys.exit(main())
