"""The reference's MF baselines (model/baseline.py): SPMF, full-retrain and fine-tune, on the HIP engine.

SPMF (a streaming MF with a reservoir, sampling its training rows by rank weight) and the full-retrain / fine-tune
loops it is compared with, with the reference's class / method names, flags and printed
lines so its recorded runs (fixtures G10 and G16) replay against them:

- `Reservious` (model/baseline.py:68-100): the reservoir, its arithmetic as recorded, quirks included -- `pool_have`
  grows by the fill's END index, so it can exceed the rows actually filled and the zero rows (0, 0) behind them are
  trained on; the new rows are not trimmed when a fill ends exactly at `len`; the uniforms are still drawn when
  `len == 0`; init_pool draws (and drops) `len` random indices before it copies the last `len` rows in.
- `StreamingData` (model/baseline.py:558-587): the on-disk period stream.
- `SPMF.run_one_stage` (SPMF itself, model/baseline.py:227-304), with `compute_R_W_P` on the device
  (HipEngine.rank_weights: scores, a stable device radix sort, p) once per stage.  Default: stream-exact batches --
  the float64 CDF of p is built once per stage and every batch takes exactly the reference's numpy draws in the
  reference's order (random_sample searched in the CDF for the rows, then one legacy randint per negative candidate
  resolved by sml_host_resolve_negatives_csr; candidates are drawn one per unresolved row, so nothing is overdrawn
  and the next batch's draws are the reference's).  `--device_batches 1`: one HipEngine.weighted_epoch launch per
  epoch, the same distribution and not the same stream.  Both train through bare_adam_epoch + mf_flush and evaluate
  through the rank kernel.
- `SPMF.run_one_stage2` (model/baseline.py:306-386), the fine-tune / full-retrain inner loop (G10).
- `base_train_not_train`, `run` with its summary lines, and `main()` (model/baseline.py:149-160, 505-671): the
  `--method full|fine|spmf` program, plus `--device_batches` and `--pre_model ''` (no checkpoint: fresh tables).
- `--device_batches 1` with `full` / `fine`: every epoch is offlineDataset_withsample.epoch_triples_device, keyed by
  (stage, epoch) with the seed expression of SPMF's device mode; no numpy or torch draw is made for the batches.
- `--neg_pool M`, `--neg_pop_alpha A` (extensions, device batches only; anything else raises ValueError): the negatives
  of an epoch come from sml_amd.sampling.NegativeSampler(M, A) -- popularity-weighted candidates, the highest-scoring
  of the first M admissible ones -- through HipEngine.sample_negatives_ex.  The pool is scored by the tables as they
  are when the epoch starts.  With the defaults every printed line and trained byte is what it is without the flags.
- `--full_eval 1` (an extension): after the final test line of a stage, `SPMF.full_test` ranks every test user's held-out
  set against the whole catalogue minus the training history (a retrieval.DeviceSeen grown by one period per stage) and
  one `full-catalogue test---` line is printed.  No RNG draw: the training trajectory is the one without the flag.

Reference defects resolved here: `run_one_stage` unpacks two values from `test`, which returns four (the reference's
SPMF path raises as committed): the first two are taken.  `__main__` passes an undefined `start_idx` to
base_train_not_train: `args.start_idx` is used.  `run_one_stage` never appends to hit_new_user / hit_new_item: kept,
so `run` prints them empty for SPMF.  Only neg_num == 1 is provided (the bare step trains (user, item, neg) triples;
every reference script uses 1): any other value raises ValueError.  `base_train`, the pretraining run with
hard-coded checkpoint paths, is not provided.
"""
import argparse
import ctypes
import os
import time

import numpy as np
import torch

from . import datasets as D
from .datasets import offlineDataset_withsample
from .engine import get_engine
from .mf import MFbasemode
from .sampling import NegativeSampler


class Reservious(object):
    """The SPMF reservoir of (user, item) rows (model/baseline.py:68-100), arithmetic as recorded (G16)."""

    def __init__(self, length):
        self.t = 0
        self.len = length
        self.pool = np.zeros((length, 2), dtype=np.int64)
        print("pool size:", self.pool.shape)
        self.pool_have = 0

    def updata(self, new_data):
        if self.t <= self.len:                   # still filling: copy rows up to slot `len`
            end = min(self.len, self.pool_have + new_data.shape[0])
            self.pool[self.pool_have:end] = new_data[:end - self.pool_have]
            if end != self.len:
                new_data = new_data[end - self.pool_have:]
            self.pool_have = self.pool_have + end    # (sic) the end index, not the rows filled
            self.t = end
        m = new_data.shape[0]
        accept = np.random.rand(m) < self.len * 1.0 / (self.t + np.arange(m) + 1)
        for row in new_data[np.where(accept)]:
            self.pool[np.random.randint(0, self.len, 1)] = row
        self.t += m

    def init_pool(self, new_data):
        np.random.randint(0, new_data.shape[0], self.len)     # drawn and unused, as recorded
        self.pool[:] = new_data[-self.len:]
        self.pool_have = self.len
        self.t = new_data.shape[0]


class StreamingData(object):
    """Periods on disk (model/baseline.py:558-587): <path>information.npy = [n_interactions, n_user, n_item],
    test_new_user.npy, test_new_item.npy, train/<p>.npy (user, item), test/<p>.npy (user, pos, negs...)."""

    def __init__(self, file_pathe):
        information = np.load(file_pathe + "information.npy")
        self.user_num = information[1]
        self.item_num = information[2]
        self.itr_num = information[0]
        self.path = file_pathe
        self.test_new_user = np.load(file_pathe + "test_new_user.npy").astype(np.int64)
        self.test_new_item = np.load(file_pathe + "test_new_item.npy").astype(np.int64)

    def get_next(self, stage_id, types="not_only_new"):
        """(train, test) of stage `stage_id`: train = period stage_id-1 ('only_new') or periods 0..stage_id-1 (any other
        `types`), test = period stage_id; (None, None) once a file is missing."""
        try:
            if types == "not_only_new":
                train_data = np.concatenate([np.load(self.path + "train/" + str(i) + ".npy").astype(np.int64)
                                             for i in range(0, stage_id)], axis=0)
            else:
                train_data = np.load(self.path + "train/" + str(stage_id - 1) + ".npy").astype(np.int64)
        except Exception:
            print("read train data roung , may be there is no new data,finished")
            return None, None
        try:
            test_data = np.load(self.path + "test/" + str(stage_id) + ".npy").astype(np.int64)
        except Exception:
            print("read test data roung , may be there is no new data,finished")
            return None, None
        print("NOTICED: will train: {} , will test:{} ".format(stage_id - 1, stage_id))
        return train_data, test_data


class SPMF(object):
    """SPMF (`run_one_stage`) and the fine-tune / full-retrain baselines (`run_one_stage2`), one period at a time.

    `datasets` supplies `get_next(stage_id, types=...) -> (train [n,2], test [n,2+neg])` and the arrays
    `test_new_user` / `test_new_item` (the surface of the reference's StreamingData that this method touches)."""

    def __init__(self, args, datasets, user_num, item_num, laten_dim, device=None, engine=None):
        if engine is not None:                      # an injected engine (tests drive the control flow with a double)
            device = engine.device if device is None else device
        elif device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("the MF baseline step runs on the HIP engine only; there is no CPU path")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.MFbase = MFbasemode(num_user=user_num, num_item=item_num, laten_factor=laten_dim).to(self.device)
        self.lr = args.lr
        self.dataset = datasets
        self.new_user = np.asarray(datasets.test_new_user).astype(np.int64)
        self.new_item = np.asarray(datasets.test_new_item).astype(np.int64)
        self.batch_size = args.batch_size
        self.lambda_u, self.lambda_i = args.l2_u, args.l2_i
        self.epochs = args.epochs
        self.early_stop = getattr(args, "pool_init_type", 0) == 1     # the Adressa setting of the reference
        self.recall, self.ndcg, self.hit_new_user, self.hit_new_item, self.test_num = [], [], [], [], []
        self.neg_num = getattr(args, "neg_num", 1)
        if self.neg_num != 1:
            raise ValueError("neg_num must be 1: the bare MF step trains (user, item, negative) triples")
        self.pool_init_type = getattr(args, "pool_init_type", 0)
        self.pool_size = getattr(args, "pool_size", 0)
        self.Reservious = Reservious(self.pool_size)
        self.all_item = np.zeros(0, dtype=np.int64)
        self.user_hit = None                        # sorted unique codes user * item_num + item of every row trained so far
        self.item_num = int(item_num)
        self.user_num = int(user_num)
        self.device_batches = int(getattr(args, "device_batches", 0) or 0)
        self.sampler = NegativeSampler(getattr(args, "neg_pool", 1), getattr(args, "neg_pop_alpha", 0.0))
        if not self.sampler.is_default and not self.device_batches:
            raise ValueError("--neg_pool / --neg_pop_alpha select a sampler of the device batch supply: they need --device_batches 1 "
                             "(the host route draws the reference's numpy stream)")
        self.run_stage = 0
        self._order = None                          # device rank order of the stage's rows (device_batches)
        self.engine = engine if engine is not None else get_engine(self.device, laten_dim, max(int(args.batch_size), 4096))
        self.MFbase._sml_engine = self.engine
        self.full_eval = int(getattr(args, "full_eval", 0) or 0)
        self._seen, self._seen_periods = None, 0    # full_eval: train/0 .. train/(_seen_periods - 1) as a DeviceSeen

    def get_next_data(self, stage_id, types="only_new"):
        return self.dataset.get_next(stage_id, types=types)

    def _sampler_or_none(self):
        return None if self.sampler.is_default else self.sampler

    def _epoch(self, train, stage_id=0, epoch=0):
        """One shuffled pass: batches drawn with the reference's random-number consumption, trained in ONE engine
        call; returns the mean batch loss accumulated in fp32 as `loss_all += loss.data` does.

        `--device_batches 1`: the pass is built on the device instead (offlineDataset_withsample.epoch_triples_device, keyed
        by (stage_id, epoch) as SPMF's device mode keys its epochs): the same distribution, not the same stream, and no
        numpy or torch draw is made.  The negatives come from this run's NegativeSampler (--neg_pool, --neg_pop_alpha).
        Its pool is scored by the tables as they are at the epoch's start -- the previous epoch's mf_flush has made them
        current -- not by the tables as the epoch's own batches move them."""
        if self.device_batches:
            seed = (2002 * 1000003 + stage_id) * 1000003 + epoch
            tri = train.epoch_triples_device(self.engine, seed, sampler=self._sampler_or_none(), model=self.MFbase)
            failed = getattr(train, "_last_failed", None)
            if failed is not None and int(failed[0]):
                raise RuntimeError("negative sampling does not terminate: a user owns (almost) every item")
        else:
            tri = train.epoch_triples(D.loader_order(len(train), shuffle=True))
        self.MFbase.train()
        losses = self.engine.bare_adam_epoch(self.MFbase, tri, self.batch_size, self.lr, self.lambda_u, self.lambda_i, bce=True)
        self.engine.mf_flush(self.MFbase)          # dense-Adam state of every row is current again
        arr = losses.detach().cpu().numpy() if isinstance(losses, torch.Tensor) else np.asarray(losses)
        acc = np.float32(0)
        for l in arr.astype(np.float32):
            acc = np.float32(acc + l)
        return float(acc / np.float32(len(arr)))

    def run_one_stage2(self, stage_id, read_data_type='only_new'):
        """One period of the fine-tune ('only_new') / full-retrain ('not_only_new') baseline."""
        set_t, now_test = self.get_next_data(stage_id, types=read_data_type)
        if set_t is None:
            return False
        self.test_num.append(now_test.shape[0])
        train = offlineDataset_withsample(set_t)
        print("start train...")
        show = lambda tag, r, n, *more: print(tag, "recall(5,10,20):", r, "ndcg (5,10,20):", n, *more)
        rec, nd, _, _ = self.test(now_test)
        show("before train test---", rec, nd)
        best = (0, None, None)
        stale = 0
        for epoch in range(self.epochs):
            t0 = time.time()
            loss = self._epoch(train, stage_id, epoch)
            print("epoch: {} ,time:{:.1f}, loss:{:.4f}".format(epoch, time.time() - t0, loss))
            stale += 1
            if epoch % 5:
                continue
            rec, nd, _, _ = self.test(now_test)
            show("        epoch test---", rec, nd)
            if rec[-1] > best[0]:
                best, stale = (rec[-1], rec, nd), 0
            if self.early_stop and stale > 5:
                break
        rec, nd, hit_u, hit_i = self.test(now_test)
        print("max result ", best[1], best[2])
        show("FInal test---", rec, nd, "hit user:", hit_u, "hit item:", hit_i)
        self._show_full(stage_id, now_test)
        self.recall.append(rec)
        self.ndcg.append(nd)
        self.hit_new_user.append(hit_u)
        self.hit_new_item.append(hit_i)
        return True

    def full_test(self, stage_id, now_test, topk=(5, 10, 20)):
        """evaluation.test_model_users of the period's test rows over the whole catalogue minus everything trained on so
        far: Seen = train/0 .. train/(stage_id - 1), held on the device and grown by the periods' files that are new since
        the last call (one per stage in a run).  Makes no RNG draw."""
        from .evaluation import test_model_users
        from .retrieval import DeviceSeen
        if self._seen is None:
            self._seen = DeviceSeen(self.user_num, self.item_num, self.engine)
        for p in range(self._seen_periods, stage_id):
            self._seen.add(np.load(self.dataset.path + "train/" + str(p) + ".npy")[:, :2])
        self._seen_periods = max(self._seen_periods, stage_id)
        return test_model_users(self.MFbase, now_test, seen=self._seen, topK=topk)

    def _show_full(self, stage_id, now_test, topk=(5, 10, 20)):
        if not self.full_eval:
            return
        res = self.full_test(stage_id, now_test, topk)
        print("full-catalogue test---", "recall(5,10,20):", np.array([res["recall"][k] for k in topk]),
              "ndcg (5,10,20):", np.array([res["ndcg"][k] for k in topk]), "users:", res["users"])

    def test(self, test_data, topk=(5, 10, 20)):
        """(recall@k, ndcg@k for every k, share of @topk[-1] hits on new users, ... on new items) over the period's
        test rows (model/baseline.py:388-443)."""
        self.MFbase.eval()
        n = test_data.shape[0]
        rows = torch.from_numpy(np.ascontiguousarray(test_data)).to(self.device).long()
        ranks = self.engine.eval_ranks(self.MFbase.user_laten.weight.data, self.MFbase.item_laten.weight.data, rows)
        pairs = [self.engine.eval_metrics(ranks, k) for k in topk]
        hit_rows = np.asarray(test_data)[(ranks < topk[-1]).nonzero()[:, 0].cpu().numpy()]
        on_new_user = int(np.isin(hit_rows[:, 0], self.new_user).sum())
        on_new_item = int(np.isin(hit_rows[:, 1], self.new_item).sum())
        return (np.array([p[0] for p in pairs]) / n, np.array([p[1] for p in pairs]) / n, on_new_user / n, on_new_item / n)

    # ------------------------------------------------------------------ SPMF (model/baseline.py:227-304, 445-503)
    def updata_reservious(self, train_data):
        self.Reservious.updata(train_data)

    def compute_R_W_P(self, R_TR_data):
        """p[row] = exp(rank / N) / sum(exp(rank / N)) with rank 1 for the highest score (model/baseline.py:448-476), from
        HipEngine.rank_weights: float32 numpy [N].  Keeps the device rank order for the device batch supply."""
        self.MFbase.eval()
        _, _, order, p = self.engine.rank_weights(self.MFbase.user_laten.weight.data, self.MFbase.item_laten.weight.data,
                                                  np.ascontiguousarray(R_TR_data, dtype=np.int64))
        self._order = order
        return (p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)).astype(np.float32)

    def user_hit_num_in_W_R(self, data):
        """Adds data's (user, item) pairs to every user's items seen so far (model/baseline.py:478-487), kept as sorted
        unique codes user * item_num + item."""
        codes = data[:, 0].astype(np.int64) * self.item_num + data[:, 1].astype(np.int64)
        self.user_hit = np.unique(codes if self.user_hit is None else np.concatenate([self.user_hit, codes]))

    def _hit_csr(self):
        hu = self.user_hit // self.item_num
        n_users = max(self.user_num, int(hu.max()) + 1 if hu.size else 0)
        ptr = np.ascontiguousarray(np.searchsorted(hu, np.arange(n_users + 1)), dtype=np.int64)
        return ptr, np.ascontiguousarray(self.user_hit % self.item_num, dtype=np.int64)

    def _begin_sampling(self, p):
        """Per stage: the float64 CDF np.random.choice builds from p (cumsum, normalised by its last entry), and the
        negatives' CSR."""
        cdf = np.asarray(p, dtype=np.float64).cumsum()
        cdf /= cdf[-1]
        self._cdf = cdf
        self._csr = self._hit_csr()
        self._items = np.ascontiguousarray(self.all_item, dtype=np.int64)

    def sample_batch(self, data, batch_size, p, neg_num):
        """One batch of model/baseline.py:489-503 with the reference's numpy draws in the reference's order:
        np.random.choice(arange(N), B, p=p) is random_sample(B) searched in the CDF; each row's negative is
        np.random.choice(all_item, 1) redrawn while it is one of the user's items, i.e. one legacy randint per
        candidate -- drawn here one per still-unresolved row and walked by sml_host_resolve_negatives_csr.
        Returns (users [B,1], items [B,1], negs [B,1]).  (`p` must be the stage's p; _begin_sampling built its CDF.)"""
        from . import _lib
        lib = _lib.load()
        idx = self._cdf.searchsorted(np.random.random_sample(batch_size), side="right")
        bat = data[idx]
        users = np.ascontiguousarray(bat[:, 0], dtype=np.int64)
        ptr, items = self._csr
        pop = self._items.shape[0]
        negs = np.empty(batch_size, dtype=np.int64)
        used, got = ctypes.c_int64(0), ctypes.c_int64(0)
        done, drawn = 0, 0
        while done < batch_size:
            k = batch_size - done
            cand = np.ascontiguousarray(self._items[np.random.randint(0, pop, size=k)])
            _lib.check(lib.sml_host_resolve_negatives_csr(users.ctypes.data + 8 * done, k, cand.ctypes.data, k, ptr.ctypes.data,
                                                          ptr.shape[0] - 1, items.ctypes.data, negs.ctypes.data + 8 * done,
                                                          ctypes.byref(used), ctypes.byref(got)), "sml_host_resolve_negatives_csr")
            done += got.value
            drawn += k
            if drawn > 64 * (batch_size + 64):
                raise RuntimeError("negative sampling does not terminate: a user owns (almost) every item")
        return bat[:, 0].reshape(-1, 1), bat[:, 1].reshape(-1, 1), negs.reshape(-1, 1)

    def _spmf_epoch(self, train_data, p, itr, stage_id, epoch):
        """One SPMF epoch of itr batches, trained in ONE engine call; the mean batch loss in fp32 as `loss_all += loss.data`."""
        B = self.batch_size
        if self.device_batches:
            if self._dev_supply is None:
                dev = self.engine.device
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
                ptr, items = self._csr
                self._dev_supply = (t(train_data), t(self._items), t(ptr), t(items))
                self._dev_extra = {}                    # the stage's popularity cdf, built on first use
            rows, item_all, ptr, items = self._dev_supply
            seed = (2002 * 1000003 + stage_id) * 1000003 + epoch
            tri, failed = self.engine.weighted_epoch(rows, self._order, item_all, ptr, items, itr * B, seed)
            if int(failed[0]):
                raise RuntimeError("negative sampling does not terminate: a user owns (almost) every item")
            if not self.sampler.is_default:
                # another sampler: column 2 is redrawn for the users of column 0 (the pool scored by the epoch-start tables)
                if "cdf" not in self._dev_extra:
                    from . import sampling
                    cdf = self.sampler.cdf(self._items, train_data[:, 1])
                    self._dev_extra["cdf"] = None if cdf is None else sampling.device_cdf(cdf, self.engine.device)
                w_user, w_item = self.sampler.tables(self.MFbase)
                negs, failed = self.engine.sample_negatives_ex(tri[:, 0].contiguous(), item_all, ptr, items, seed + 1, pool=self.sampler.pool,
                                                               cdf=self._dev_extra["cdf"], w_user=w_user, w_item=w_item)
                if int(failed[0]):
                    raise RuntimeError("negative sampling does not terminate: a user owns (almost) every item")
                tri[:, 2] = negs
        else:
            tri = np.empty((itr * B, 3), dtype=np.int64)
            for b in range(itr):
                u, i, j = self.sample_batch(train_data, B, p, self.neg_num)
                tri[b * B:(b + 1) * B] = np.concatenate([u, i, j], axis=1)
        self.MFbase.train()
        losses = self.engine.bare_adam_epoch(self.MFbase, tri, B, self.lr, self.lambda_u, self.lambda_i, bce=True)
        self.engine.mf_flush(self.MFbase)
        arr = losses.detach().cpu().numpy() if isinstance(losses, torch.Tensor) else np.asarray(losses)
        acc = np.float32(0)
        for l in arr.astype(np.float32):
            acc = np.float32(acc + l)
        return float(acc / np.float32(len(arr)))

    def run_one_stage(self, stage_id):
        """One SPMF period (model/baseline.py:227-304): train on the reservoir + the period's rows, sampled by rank
        weight, then fold the period into the reservoir."""
        set_t, now_test = self.get_next_data(stage_id)
        if set_t is None:
            return False
        self.test_num.append(now_test.shape[0])
        self.all_item = np.union1d(self.all_item, set_t[:, 1])
        if self.Reservious.pool_have > 0:
            train_data = np.concatenate([self.Reservious.pool[0:self.Reservious.pool_have], set_t], axis=0)
        else:
            train_data = set_t
        self.user_hit_num_in_W_R(train_data)
        itr = round(train_data.shape[0] / self.batch_size)
        p = self.compute_R_W_P(train_data)
        self._begin_sampling(p)
        self._dev_supply = None
        show = lambda tag, r, n, *more: print(tag, "recall(5,10,20):", r, "ndcg (5,10,20):", n, *more)
        print("start train...")
        rec, nd = self.test(now_test)[:2]
        show("before train test---", rec, nd)
        best = 0
        stale = 0
        for epoch in range(self.epochs):
            t0 = time.time()
            loss = self._spmf_epoch(train_data, p, itr, stage_id, epoch)
            print("epoch: {} ,time:{:.1f}, loss:{:.4f}".format(epoch, time.time() - t0, loss))
            stale += 1
            rec, nd = self.test(now_test)[:2]
            show("        epoch test---", rec, nd)
            if best < rec[-1]:
                best, stale = rec[-1], 0
            if stale >= 5 and self.pool_init_type == 1:
                break
        self._dev_supply = None
        self.updata_reservious(set_t)
        rec, nd, hit_u, hit_i = self.test(now_test)
        show("FInal test---", rec, nd, "hit new user:", hit_u, "hit new item:", hit_i)
        self._show_full(stage_id, now_test)
        self.recall.append(rec)
        self.ndcg.append(nd)
        return True

    def base_train_not_train(self, stage_id):
        """Fills the reservoir from the history before the first SPMF period, without training (model/baseline.py:149-156)."""
        set_t, now_test = self.get_next_data(stage_id, types="not_only_new")
        if self.pool_init_type == 1:
            self.Reservious.init_pool(set_t)
        rec, nd = self.test(now_test)[:2]
        print("before train test---", "recall(5,10,20):", rec, "ndcg (5,10,20):", nd)
        if self.pool_init_type == 0:
            self.updata_reservious(set_t)

    def run(self, start_stage, method="full"):
        """Every period from start_stage until the stream ends, then the summary (model/baseline.py:505-556):
        the first round(n/3) periods are validation, the rest test, each averaged weighted by test rows."""
        self.run_stage = 0
        stage_id = start_stage
        while True:
            print("#################################runing stage:{}########################".format(stage_id))
            if method == "spmf":
                ok = self.run_one_stage(stage_id)
            elif method == "full":
                ok = self.run_one_stage2(stage_id, read_data_type="not_only_new")
            else:
                ok = self.run_one_stage2(stage_id, read_data_type="only_new")
            if ok:
                stage_id += 1
                self.run_stage += 1
                continue
            self._summary()
            break

    def _summary(self):
        test_num = np.array(self.test_num).reshape(-1, 1)
        recall = np.array(self.recall)
        ndcg = np.array(self.ndcg)
        print("average recall:", recall.mean(axis=0))
        print("average recall:", ndcg.mean(axis=0))     # (sic) the reference labels the ndcg mean so
        print(test_num)
        print(recall)
        print(ndcg)
        print("hit new user:", self.hit_new_user)
        print("hit new item:", self.hit_new_item)
        n3 = round(test_num.shape[0] * 1.0 / 3)
        head = test_num[0:n3] / test_num[0:n3].sum()
        print("pre 3 (val) reslut,recall,ndcg:", (recall[0:n3] * head).sum(axis=0), (ndcg[0:n3] * head).sum(axis=0))
        tail = test_num[n3:] / test_num[n3:].sum()
        print("last 7 (test) results,recall ,ndcg:", (recall[n3:] * tail).sum(axis=0), (ndcg[n3:] * tail).sum(axis=0))
        rate = test_num / test_num.sum()
        print("weight average recall@20:", (recall * rate).sum(axis=0))
        print("weight average ndcg@20:", (ndcg * rate).sum(axis=0))


def get_parse():
    """The reference's flags (model/baseline.py:592-626) plus --device_batches and --full_eval."""
    parser = argparse.ArgumentParser(description='MF and TR parameters.')
    parser.add_argument('--lr', type=float, default=0.01, help='Learning rate.')
    parser.add_argument('--l2_u', type=float, default=1e-5, help='user l2. should be same to l2_i')
    parser.add_argument('--l2_i', type=float, default=1e-5, help='item l2.should be same to l2_u ')
    parser.add_argument('--epochs', type=int, default=20, help='Number of epochs to train of each stage.')
    parser.add_argument('--batch_size', type=int, default=256, help='batch size of train.')
    parser.add_argument('--laten_dim', type=int, default=64, help='embedding width.')
    parser.add_argument('--neg_num', type=int, default=1, help='neg num (1 only).')
    parser.add_argument('--pool_size', type=int, default=0, help='SPMF reservoir rows.')
    parser.add_argument('--laten', type=int, default=64, help='(unused; --laten_dim sets the width)')
    parser.add_argument('--cuda', type=int, default=1, help='which GPU be used?.default 1')
    parser.add_argument('--method', default='full', help='full, fine, spmf')
    parser.add_argument('--pool_init_type', type=int, default=0,
                        help='Reservious of SPMF init methods, 0: update , 1: init, yelp=0, news (adressa) =1 ')
    parser.add_argument('--data_path', default='/home/wangpenghui/zhangyang/datasets/', help='data path')
    parser.add_argument('--data_name', default='yelp', help='dataset name')
    parser.add_argument('--pre_model', default="/home/wangpenghui/zhangyang/yelp_0113/save_model/best-mean-start29-spmf--1e-07-0.01lr.pt",
                        help="pretrained MFbase state dict; '' starts from fresh tables")
    parser.add_argument('--start_idx', type=int, default=30, help='retraining from which period: yelp 30, news(adressa) 48')
    # extension (not a reference flag): SPMF batches drawn on the device -- the same distribution, not the same numpy stream
    parser.add_argument('--device_batches', type=int, default=0, help='1: draw the epochs of every method on the device (not stream-exact)')
    parser.add_argument('--neg_pool', type=int, default=1,
                        help='with --device_batches 1: train on the highest-scoring of the first M admissible negatives (1..64)')
    parser.add_argument('--neg_pop_alpha', type=float, default=0.0,
                        help='with --device_batches 1: draw negatives with p(i) ~ count(i)^alpha over the training rows (0: uniform)')
    parser.add_argument('--full_eval', type=int, default=0,
                        help='1: after each stage also print the all-ranking metrics over the whole catalogue minus the history')
    return parser


def main(argv=None):
    """`python model/baseline.py --method full|fine|spmf ...` (model/baseline.py:628-671): one run with
    l2_i = l2_u, seeds 2000 / 2001 / 2002, pool_init_type from the dataset name."""
    print("start")
    args = get_parse().parse_args(argv)
    print("parameters:", args)
    data_path = args.data_path + args.data_name + "/"
    args.pool_init_type = 1 if args.data_name == 'news' else 0
    dataset = StreamingData(data_path)
    args.l2_i = args.l2_u
    print("*******************(l2_u,pool size):({},{})********".format(0, 0))
    print("*##**##*")
    print(args)
    torch.manual_seed(2000)
    torch.cuda.manual_seed(2001)
    np.random.seed(2002)
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    model = SPMF(args, dataset, int(dataset.user_num), int(dataset.item_num), args.laten_dim, device=device)
    if args.pre_model:
        sd = torch.load(args.pre_model, map_location=model.device)
        model.MFbase.load_state_dict(sd.state_dict() if hasattr(sd, "state_dict") else sd)
    if args.method == 'spmf':
        model.base_train_not_train(args.start_idx - 1)
    model.run(args.start_idx, method=args.method)
    print("\n *##**##* \n")


if __name__ == "__main__":
    main()
