"""HipEngine: the host-side handle on libsml_hip.so for one GPU.

Everything numerical on the SML hot path goes through this object; it owns the
sml_ctx (scratch), the flat theta buffer the transfer module's parameters are
re-pointed into, and the Adam state of both optimisers.  torch is used for device
memory, streams and (in sml_amd.dist) RCCL -- not for arithmetic on the path.
"""
import ctypes

import numpy as np
import torch

from . import _lib, switches
from ._lib import check

NET_PARAM_ORDER = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
                   "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class HipEngine(object):
    def __init__(self, device, d, max_batch=4096, lib=None):
        self.lib = _lib.load() if lib is None else lib           # (lib: a test hook -- _lib.load_other)
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs a GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HipEngine device must be a cuda (HIP) device, got %s" % device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.d = int(d)
        self.max_batch = int(max_batch)
        h = ctypes.c_void_p()
        check(self.lib.sml_ctx_create(ctypes.byref(h), self.device.index, self.d, self.max_batch), "sml_ctx_create")
        self._ctx = h
        self.net_size = int(self.lib.sml_theta_net_size(self.d))
        self.offsets = [int(self.lib.sml_theta_offset(self.d, w)) for w in range(8)]
        self._flat = {}       # id(transfer) -> (flat theta, [(param, off, numel)], transfer): the entry keeps the module alive
        self.mf_state = None  # lazy-Adam state of the MF tables
        self.mf_step = 0      # torch.optim.Adam's step counter; never resets (reference model/transfer.py:392)
        self.tr_state = None  # (m, v) flat, theta layout
        self.tr_step = 0
        self.grad_hook = None  # set by sml_amd.dist for the multi-GPU TR stage
        self.dist = None       # sml_amd.dist.DistContext when the job spans several GPUs
        self._plain_stream()   # (created before any CU-masked stream of the process: see there)

    _PLAIN = {}      # device index -> the process's one side stream over all CUs

    def _plain_stream(self):
        """The side stream for work that may use the whole chip (the bare step's index preparation).  ONE per process and
        device, created with the first engine -- before any CU-masked stream exists: the HIP runtime keeps a small pool
        of hardware queues and hands a new stream the least-used one, and a queue made for hipExtStreamCreateWithCUMask
        joins that pool WITH its mask.  A stream created after the masked ones can land on the 64-CU evaluation queue
        and run four times slower (measured: every third stream of torch's pool, in a process that had partitioned the
        chip).  A stream that exists already keeps the unmasked queue it was given."""
        key = self.device.index or 0
        st = HipEngine._PLAIN.get(key)
        if st is None:
            st = HipEngine._PLAIN[key] = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(st):                  # (the runtime binds the queue at the stream's first use)
                torch.empty(1, device=self.device).zero_()
            st.synchronize()
        return st

    def close(self):
        if getattr(self, "_side_ctx_h", None):
            self.lib.sml_ctx_destroy(self._side_ctx_h)
            self._side_ctx_h = None
        if getattr(self, "_ctx", None):
            self.lib.sml_ctx_destroy(self._ctx)
            self._ctx = None
            for p in self.__dict__.pop("_peer_opened", []):
                self.lib.sml_peer_close(self.device.index, ctypes.c_void_p(p))
            # (own regions are NOT freed here: a peer may still be writing into them; they go with the process,
            # or explicitly through sml_peer_free once every rank has detached)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, dtype):
        if isinstance(t, np.ndarray):
            # pinned staging (torch's caching host allocator) + an asynchronous copy: a pageable upload
            # would make the host wait for everything already queued on the stream
            t = torch.from_numpy(np.ascontiguousarray(t))
            if t.dtype != dtype:
                t = t.to(dtype)
            return t.pin_memory().to(device=self.device, non_blocking=True)
        t = t.to(device=self.device, dtype=dtype)
        return t if t.is_contiguous() else t.contiguous()

    def _table(self, t):
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != self.d:
            raise ValueError("expected a contiguous fp32 [rows,%d] tensor on %s, got %s %s on %s"
                             % (self.d, self.device, tuple(t.shape), t.dtype, t.device))
        return t

    def adopt(self, transfer):
        """Re-point the transfer module's parameters into one flat device buffer
        (user net then item net, layout sml_theta_offset) and return that buffer."""
        key = id(transfer)
        ent = self._flat.get(key)
        if ent is not None and ent[2] is transfer:
            flat, views = ent[0], ent[1]
            if all(p.data_ptr() == flat.data_ptr() + 4 * off for (p, off, _) in views):
                return flat
        flat = torch.zeros(2 * self.net_size, device=self.device, dtype=torch.float32)
        views = []
        for ni, net in enumerate((transfer.user_transfer, transfer.item_transfer)):
            named = dict(net.named_parameters())
            for w, name in enumerate(NET_PARAM_ORDER):
                p = named[name]
                off = ni * self.net_size + self.offsets[w]
                n = p.numel()
                if name == "conv1.weight" and p.shape[2] == 2:
                    # ConvTransfer's (2,1) kernel lives in the first two columns of the [10][3] block; the third
                    # column multiplies the zero x_com row and stays zero (its gradient is exactly zero)
                    block = flat[off:off + 30].view(10, 3)
                    block[:, :2].copy_(p.data.reshape(10, 2).to(self.device, torch.float32))
                    p.data = block[:, :2].view(10, 1, 2, 1)
                    views.append((p, off, n))
                    continue
                flat[off:off + n].copy_(p.data.reshape(-1).to(self.device, torch.float32))
                p.data = flat[off:off + n].view(p.shape)
                views.append((p, off, n))
        if len(self._flat) >= 8:                 # a long-lived engine does not collect every module it ever saw
            self._flat.pop(next(iter(self._flat)))
        self._flat[key] = (flat, views, transfer)
        return flat

    def load_optimizer_state(self, mfbase=None, mf_state=None, transfer=None, tr_state=None):
        """Resume from saved torch.optim.Adam states (the reference keeps both optimisers alive for the whole run,
        model/transfer.py:392-393; this is how a run is continued from a checkpoint of them).
        mf_state: dict(m_user, v_user, m_item, v_item, step) -- exp_avg / exp_avg_sq of the two tables, all rows
        current as of `step`.  tr_state: dict(m={param name: exp_avg}, v={param name: exp_avg_sq}, step) over
        transfer.named_parameters()."""
        if mf_state is not None:
            self._mf_tables(mfbase, None, None)
            s = self.mf_state
            for key, src in (("m_u", "m_user"), ("v_u", "v_user"), ("m_i", "m_item"), ("v_i", "v_item")):
                s[key].copy_(torch.as_tensor(mf_state[src]).to(self.device, torch.float32))
            self.mf_step = int(mf_state["step"])
            s["s_u"].fill_(self.mf_step)
            s["s_i"].fill_(self.mf_step)
        if tr_state is not None:
            theta = self._select(transfer)
            if self.tr_state is None or self.tr_state[0].shape != theta.shape:
                self.tr_state = (torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros_like(theta))
            names = {id(p): n for n, p in transfer.named_parameters()}
            for flat, src in ((self.tr_state[0], tr_state["m"]), (self.tr_state[1], tr_state["v"])):
                flat.zero_()
                for p, off, n in self._flat[id(transfer)][1]:
                    t = torch.as_tensor(src[names[id(p)]]).to(self.device, torch.float32)
                    if p.dim() == 4 and p.shape[2] == 2 and p.shape[0] == 10:   # ConvTransfer's (2,1) conv1 kernel: see adopt()
                        flat[off:off + 30].view(10, 3)[:, :2].copy_(t.reshape(10, 2))
                    else:
                        flat[off:off + n].copy_(t.reshape(-1))
            self.tr_step = int(tr_state["step"])

    def _select(self, transfer):
        """Tell the library which transfer architecture the next calls are for (0: ConvTransfer_com,
        1: ConvTransfer -- kernel-2 nets, unit-norm user output, BPR) and return the flat theta."""
        variant = 1 if int(getattr(transfer.user_transfer, "kernel", 3)) == 2 else 0
        if variant != getattr(self, "_variant", 0):
            check(self.lib.sml_ctx_set_variant(self._ctx, variant), "sml_ctx_set_variant")
            self._variant = variant
        return self.adopt(transfer)

    # ------------------------------------------------------------------ a5/a6/a10
    def transfer_forward(self, transfer, x_t, x_hat, which):
        net = {"user": 0, "item": 1}.get(which)
        if net is None:
            raise TypeError("convtransfer has not this type")
        theta = self._select(transfer)
        x_t = self._table(self._dev(x_t, torch.float32))
        x_hat = self._table(self._dev(x_hat.detach(), torch.float32))
        out = torch.empty_like(x_t)
        check(self.lib.sml_transfer_forward(self._ctx, _ptr(theta), net, _ptr(x_t), _ptr(x_hat), _ptr(out),
                                            x_t.shape[0], self._stream()), "sml_transfer_forward")
        return out

    def updata(self, transfer, last_user, hat_user, last_item, hat_item, out_user, out_item):
        theta = self._select(transfer)
        for net, (xt, xh, out) in enumerate(((last_user, hat_user, out_user), (last_item, hat_item, out_item))):
            xt, xh, out = self._table(xt), self._table(xh), self._table(out)
            if out.data_ptr() in (xt.data_ptr(), xh.data_ptr()):
                raise ValueError("updata output may not alias its inputs")
            check(self.lib.sml_transfer_forward(self._ctx, _ptr(theta), net, _ptr(xt), _ptr(xh), _ptr(out),
                                                xt.shape[0], self._stream()), "sml_transfer_forward")

    # ------------------------------------------------------------------ a8
    def _mf_tables(self, mfbase, last_user, last_item):
        wu, wi = self._table(mfbase.user_laten.weight.data), self._table(mfbase.item_laten.weight.data)
        if self.mf_state is None or self.mf_state["m_u"].shape != wu.shape or self.mf_state["m_i"].shape != wi.shape:
            z = lambda t: torch.zeros_like(t)
            self.mf_state = dict(m_u=z(wu), v_u=z(wu), m_i=z(wi), v_i=z(wi),
                                 # -1: never touched (m = v = 0: nothing to replay, nothing to flush)
                                 s_u=torch.full((wu.shape[0],), -1, device=self.device, dtype=torch.int32),
                                 s_i=torch.full((wi.shape[0],), -1, device=self.device, dtype=torch.int32))
        s = self.mf_state
        t = _lib.MFTables()
        t.w_user, t.w_item = wu.data_ptr(), wi.data_ptr()
        t.last_user = self._table(last_user).data_ptr() if last_user is not None else 0
        t.last_item = self._table(last_item).data_ptr() if last_item is not None else 0
        t.m_user, t.v_user, t.m_item, t.v_item = (s["m_u"].data_ptr(), s["v_u"].data_ptr(),
                                                  s["m_i"].data_ptr(), s["v_i"].data_ptr())
        t.step_user, t.step_item = s["s_u"].data_ptr(), s["s_i"].data_ptr()
        t.n_user, t.n_item = wu.shape[0], wi.shape[0]
        return t

    def _loss_kind(self, bce, norm):
        if getattr(self, "_variant", 0) == 1:
            # ConvTransfer.run_MF has one loss: BPR over the unit-norm user output (model/conv_transfer.py:71-85).  norm=True
            # (:79-81) divides the score by the norm of that unit-norm output WITHOUT detaching it: with u = x / stop(|x|) the
            # value is x.(i - n) / |x| and d/dx = (i - n) / |x| - (x.(i - n)) x / |x|^3 -- exactly the differentiable-norm BPR
            # (SML_LOSS_BPR_NORM) on the net's raw user rows
            return _lib.LOSS_BPR_NORM if norm else _lib.LOSS_BPR_UNIT
        if bce:
            return _lib.LOSS_BCE
        return _lib.LOSS_BPR_NORM if norm else _lib.LOSS_BPR

    def _plan(self, plan, n):
        """ctypes view of a batch plan {batch_off: int64 [nb+1] (numpy), loss_scale: float32 [nb] or None}: batches
        of unequal size (a global batch split over ranks by user owner).  Returns (struct pointer, keep-alive)."""
        if plan is None:
            return None, None
        off = np.ascontiguousarray(plan["batch_off"], dtype=np.int64)
        if off[0] != 0 or off[-1] != n:
            raise ValueError("batch plan does not cover the %d triples" % n)
        off_dev = torch.from_numpy(off.astype(np.int32)).pin_memory().to(self.device, non_blocking=True)
        sc = plan.get("loss_scale")
        sc = None if sc is None else np.ascontiguousarray(sc, dtype=np.float32)
        p = _lib.BatchPlan()
        p.n_batches = off.shape[0] - 1
        p.batch_off = off.ctypes.data
        p.batch_off_dev = off_dev.data_ptr()
        p.loss_scale = sc.ctypes.data if sc is not None else None
        return ctypes.byref(p), (p, off, off_dev, sc)

    def mf_stage_epoch(self, mfbase, transfer, last_user, last_item, triples, batch_size, lr, l2, norm=False, bce=True,
                       plan=None, exchange=None, adaptive_beta=None):
        """plan / exchange: the multi-GPU driver's per-epoch descriptors (sml_amd.dist.EpochRoute): batches of unequal
        local size, and the global item-occurrence list of the job.  adaptive_beta: the reference's --need_adaptive
        term (model/transfer.py:490-499; 0.1 there)."""
        check(self.lib.sml_ctx_set_adaptive(self._ctx, float(adaptive_beta or 0.0)), "sml_ctx_set_adaptive")
        theta = self._select(transfer)
        tri = self._dev(triples, torch.int64)
        n = tri.shape[0]
        nb = (n + batch_size - 1) // batch_size if plan is None else len(plan["batch_off"]) - 1
        t = self._mf_tables(mfbase, last_user, last_item)
        self._mf_lr = float(lr)
        losses = torch.empty(nb, device=self.device, dtype=torch.float32)
        step = ctypes.c_int64(self.mf_step)
        xp = None
        pp, keep = self._plan(plan, n)
        if self.dist is not None:
            ex = exchange if exchange is not None else self.dist.mf_exchange(tri, int(batch_size), self.d, self._loss_kind(bce, norm))
            hook_fn = ex["hook"]

            def _cb(_user, b):
                try:
                    hook_fn(int(b))
                    return 0
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return 1
            x = _lib.MFExchange()
            x.world = ex["world"]
            x.key_items, x.val_items = ex["keys"].data_ptr(), ex["vals"].data_ptr()
            x.dx_local, x.dx_items_all = ex["dx_local"].data_ptr(), ex["dx_all"].data_ptr()
            x.hook = _lib.MF_HOOK(_cb) if hook_fn is not None else ctypes.cast(None, _lib.MF_HOOK)
            x.hook_user = None
            x.loss_scale = ex["loss_scale"]
            x.slot_stride = int(ex.get("slot_stride", 0))
            ioff = ex.get("item_off")
            if ioff is not None:
                ioff = np.ascontiguousarray(ioff, dtype=np.int64)
                keep = (keep, ioff)
            x.item_off = ioff.ctypes.data if ioff is not None else None
            x.push_rows = int(ex.get("push_rows", 0))
            x.lists_unsorted = 1 if ex.get("unsorted") else 0
            xp = ctypes.byref(x)
        check(self.lib.sml_mf_stage_epoch(self._ctx, _ptr(theta), ctypes.byref(t), _ptr(tri), n, int(batch_size),
                                          float(lr), float(l2), self._loss_kind(bce, norm), ctypes.byref(step),
                                          _ptr(losses), xp, pp, self._stream()), "sml_mf_stage_epoch")
        self.mf_step = step.value
        return losses

    def mf_flush(self, mfbase):
        """Replay pending zero-gradient Adam steps so the tables can be read."""
        if self.mf_state is None or self.mf_step == 0:
            return
        t = self._mf_tables(mfbase, None, None)
        check(self.lib.sml_mf_adam_flush(self._ctx, ctypes.byref(t), float(self._mf_lr), self.mf_step, self._stream()),
              "sml_mf_adam_flush")

    # ------------------------------------------------------------------ a9
    def tr_stage_epoch(self, transfer, last_user, last_item, hat_user, hat_item, triples, batch_size, lr,
                       weight_decay, bce=True, loss_scale=None, plan=None, clip_max_norm=None):
        """clip_max_norm: the reference's --clip_grad / --maxnorm_grad (model/transfer.py:725-727)."""
        check(self.lib.sml_ctx_set_grad_clip(self._ctx, float(clip_max_norm or 0.0)), "sml_ctx_set_grad_clip")
        theta = self._select(transfer)
        if loss_scale is None:
            loss_scale = self.dist.tr_loss_scale(self._loss_kind(bce, False)) if self.dist is not None else 1.0
        if self.tr_state is None or self.tr_state[0].shape != theta.shape:
            self.tr_state = (torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros_like(theta))
        m, v, grad = self.tr_state
        tri = self._dev(triples, torch.int64)
        n = tri.shape[0]
        nb = (n + batch_size - 1) // batch_size if plan is None else len(plan["batch_off"]) - 1
        pp, keep = self._plan(plan, n)
        t = _lib.TRTables()
        t.last_user, t.last_item = self._table(last_user).data_ptr(), self._table(last_item).data_ptr()
        t.hat_user, t.hat_item = self._table(hat_user).data_ptr(), self._table(hat_item).data_ptr()
        t.n_user, t.n_item = last_user.shape[0], last_item.shape[0]
        losses = torch.empty(nb, device=self.device, dtype=torch.float32)
        step = ctypes.c_int64(self.tr_step)
        if self.grad_hook is not None:
            hook_fn = self.grad_hook

            def _cb(_user, _grad, _n, b):
                try:
                    hook_fn(grad, int(b))
                    return 0
                except Exception:  # surfaced as SML_ESTATE by the library
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = _lib.GRAD_HOOK(_cb)
        else:
            cb = ctypes.cast(None, _lib.GRAD_HOOK)
        # the flat theta-gradient is an output only where somebody reads it: the exchange on several GPUs, or a caller
        # that set keep_theta_grad (the G2 parity test); the fused single-GPU step does not write it otherwise
        want_grad = self.grad_hook is not None or self.dist is not None or getattr(self, "keep_theta_grad", False)
        check(self.lib.sml_tr_stage_epoch(self._ctx, _ptr(theta), _ptr(m), _ptr(v), _ptr(grad) if want_grad else None, ctypes.byref(t),
                                          _ptr(tri), n, int(batch_size), float(lr), float(weight_decay),
                                          self._loss_kind(bce, False), float(loss_scale), ctypes.byref(step),
                                          _ptr(losses), cb, None, pp, self._stream()), "sml_tr_stage_epoch")
        self.tr_step = step.value
        return losses

    # ------------------------------------------------------------------ a7 with gradients (the autograd surface)
    def run_mf_grad(self, transfer, user_last, user_hat, item_last, item_hat, bce=True, norm=False,
                    want_rows=True, want_theta=True):
        """run_MF of one batch given as row blocks (user_* [B,d]; item_* [2B,d]: positives then negatives) with its
        gradients: (loss 0-dim, d loss / d user_hat or None, d loss / d item_hat or None, flat theta gradient or None).
        No optimiser step -- this is what sml_amd.conv_transfer's autograd Function calls."""
        theta = self._select(transfer)
        ul, uh = self._table(user_last), self._table(user_hat)
        il, ih = self._table(item_last), self._table(item_hat)
        B = ul.shape[0]
        if uh.shape[0] != B or il.shape[0] != 2 * B or ih.shape[0] != 2 * B:
            raise ValueError("run_mf_grad: user blocks [B,d], item blocks [2B,d]")
        loss = torch.empty((), device=self.device, dtype=torch.float32)
        du = torch.empty_like(uh) if want_rows else None
        di = torch.empty_like(ih) if want_rows else None
        gt = torch.empty_like(theta) if want_theta else None
        check(self.lib.sml_run_mf_grad(self._ctx, _ptr(theta), _ptr(ul), _ptr(uh), _ptr(il), _ptr(ih), B, self._loss_kind(bce, norm),
                                       _ptr(loss), _ptr(du), _ptr(di), _ptr(gt), self._stream()), "sml_run_mf_grad")
        return loss, du, di, gt

    def theta_views(self, transfer):
        """[(parameter, offset, numel)] of the adopted transfer module inside its flat theta (adopt() first)."""
        self.adopt(transfer)
        return self._flat[id(transfer)][1]

    # ------------------------------------------------------------------ a3
    def _bare_exchange(self, ex):
        """ctypes view of sml_amd.dist.DistContext.bare_exchange(): (struct pointer or None, keep-alive)."""
        if ex is None:
            return None, None
        hook_fn = ex["hook"]

        def _cb(_user, b):
            try:
                hook_fn(int(b))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        x = _lib.BareExchange()
        x.world = ex["world"]
        x.items_all, x.dx_local, x.dx_items_all = ex["items_all"].data_ptr(), ex["dx_local"].data_ptr(), ex["dx_all"].data_ptr()
        cb = _lib.MF_HOOK(_cb) if hook_fn is not None else ctypes.cast(None, _lib.MF_HOOK)
        x.hook = cb
        x.hook_user = None
        x.loss_scale = ex["loss_scale"]
        return ctypes.byref(x), (x, cb, ex)

    def bare_prepare(self, triples, batch_size, n_user=0, n_item=0, exchange=None):
        """Build the index lists of a coming bare epoch on the engine's side stream (sort by (batch,row),
        unique marks, duplicates-only compaction) while earlier work keeps the main stream busy.
        n_user / n_item (the table heights; 0 = unknown) let the sort use 32-bit keys.
        exchange: several GPUs (DistContext.bare_exchange): the item lists are then the job's.
        Returns a handle for bare_epoch(prepared=...)."""
        if getattr(self, "_prep", None) is None:
            k = int(switches.get("SML_PREP_CUS"))
            if k > 0:                                    # the preparation confined to the last k compute units
                self._prep = self._masked_stream(self._n_cus() - k, self._n_cus())
            elif switches.get("SML_PREP_PRIO") in ("low", "high"):
                lo, hi = torch.cuda.Stream.priority_range()
                self._prep = torch.cuda.Stream(device=self.device, priority=int(lo if switches.get("SML_PREP_PRIO") == "low" else hi))
            else:
                self._prep = self._plain_stream()
        tri = self._dev(triples, torch.int64)
        slot = self._prep_slot = 1 - getattr(self, "_prep_slot", 1)
        cur = torch.cuda.current_stream(self.device)
        self._prep.wait_stream(cur)          # the slot's previous user (two epochs back) has been queued before this
        xp, keep = self._bare_exchange(exchange)
        with torch.cuda.stream(self._prep):
            check(self.lib.sml_embed_loss_sgd_prepare(self._ctx, _ptr(tri), tri.shape[0], int(batch_size), int(n_user),
                                                      int(n_item), slot, xp, self._stream()), "sml_embed_loss_sgd_prepare")
            ev = torch.cuda.Event()
            ev.record(self._prep)
        tri.record_stream(self._prep)
        return dict(slot=slot, event=ev, tri=tri, batch=int(batch_size), exchange=exchange)

    def index_lists(self, prepared):
        """Test hook: the lists a bare_prepare handle holds, as numpy arrays (see sml_index_lists_read)."""
        import numpy as np
        prepared["event"].synchronize()
        n, batch = int(prepared["tri"].shape[0]), prepared["batch"]
        nb = (n + batch - 1) // batch

        def rd(which, dtype, count):
            buf = np.zeros(max(int(count), 1), dtype)
            got = self.lib.sml_index_lists_read(self._ctx, prepared["slot"], which, buf.ctypes.data, buf.nbytes)
            if got < 0:
                check(int(got), "sml_index_lists_read")
            return buf[:got // buf.itemsize]

        two = rd(11, np.int32, 2)
        out = dict(runs_u=rd(0, np.uint32, 8 * (n // 2 + 8)).reshape(-1, 8), runs_i=rd(1, np.uint32, 8 * (n + 8)).reshape(-1, 8),
                   off_u=rd(2, np.int32, nb + 1), off_i=rd(3, np.int32, nb + 1), cnt_u=rd(4, np.int32, nb), cnt_i=rd(5, np.int32, nb),
                   val_u=rd(6, np.uint32, n), val_i=rd(7, np.uint32, 2 * n), uniq=rd(8, np.uint8, 3 * nb * batch),
                   max_len=int(two[0]), hot_cap=int(two[1]))
        out["hot_list"] = rd(9, np.uint32, nb * out["hot_cap"] * 3).reshape(nb, -1, 3) if out["hot_cap"] else None
        out["hot_count"] = rd(10, np.int32, nb) if out["hot_cap"] else None
        return out

    def bare_epoch(self, w_user, w_item, triples, batch_size, lr, lam_user, lam_item, bce=True, prepared=None, exchange=None):
        if w_user.dtype not in (torch.float32, torch.float16) or w_item.dtype != w_user.dtype:
            raise ValueError("tables must both be fp32 or both fp16")
        for w in (w_user, w_item):
            if w.device != self.device or not w.is_contiguous() or w.shape[-1] != self.d:
                raise ValueError("tables must be contiguous [rows,%d] on %s" % (self.d, self.device))
        slot = -1
        if prepared is not None:
            if prepared["batch"] != int(batch_size):
                raise ValueError("prepared for another batch size")
            tri, slot = prepared["tri"], prepared["slot"]
            exchange = prepared.get("exchange") if exchange is None else exchange
            torch.cuda.current_stream(self.device).wait_event(prepared["event"])
        else:
            tri = self._dev(triples, torch.int64)
        n = tri.shape[0]
        nb = (n + batch_size - 1) // batch_size
        losses = torch.empty(nb, device=self.device, dtype=torch.float32)
        xp, keep = self._bare_exchange(exchange)
        check(self.lib.sml_embed_loss_sgd_epoch(self._ctx, _ptr(w_user), _ptr(w_item), w_user.shape[0], w_item.shape[0],
                                                w_user.element_size(), _ptr(tri), n, int(batch_size), float(lr),
                                                float(lam_user), float(lam_item),
                                                _lib.LOSS_BCE if bce else _lib.LOSS_BPR, _ptr(losses), slot, xp,
                                                self._stream()),
              "sml_embed_loss_sgd_epoch")
        return losses

    def bare_epoch_sharded(self, w_user, triples, batch_size, lr, lam_user, lam_item, shard, bce=True):
        """The bare step with the item table SHARDED over the ranks (sml_embed_loss_sgd_epoch_sharded; peers attached):
        `shard` is sml_amd.dist.DistContext.bare_shard()'s descriptor -- head_rows / shard_rows, every rank's tail-shard
        address, this rank's head replica, the gathered item columns, the loss scale.  n_item = the GLOBAL table height."""
        if w_user.dtype not in (torch.float32, torch.float16) or not w_user.is_contiguous() or w_user.shape[-1] != self.d:
            raise ValueError("user table: contiguous fp32 / fp16 [rows,%d]" % self.d)
        tri = self._dev(triples, torch.int64)
        n = tri.shape[0]
        nb = (n + batch_size - 1) // batch_size
        losses = torch.empty(nb, device=self.device, dtype=torch.float32)
        world = int(shard["world"])
        ptrs = (ctypes.c_void_p * world)(*[int(p) for p in shard["item_shard"]])
        x = _lib.BareShard()
        x.world, x.rank = world, int(shard["rank"])
        x.head_rows, x.shard_rows = int(shard["head_rows"]), int(shard["shard_rows"])
        x.item_shard = ptrs
        head = shard.get("w_item_head")
        x.w_item_head = head.data_ptr() if head is not None and head.numel() else None
        x.items_all = shard["items_all"].data_ptr()
        x.loss_scale = float(shard["loss_scale"])
        check(self.lib.sml_embed_loss_sgd_epoch_sharded(self._ctx, _ptr(w_user), w_user.shape[0], int(shard["n_item"]), w_user.element_size(),
                                                        _ptr(tri), n, int(batch_size), float(lr), float(lam_user), float(lam_item),
                                                        _lib.LOSS_BCE if bce else _lib.LOSS_BPR, _ptr(losses), ctypes.byref(x), self._stream()),
              "sml_embed_loss_sgd_epoch_sharded")
        return losses

    def bare_adam_epoch(self, mfbase, triples, batch_size, lr, lam_user, lam_item, bce=True):
        """One epoch of the baselines' bare-MF step (reference model/baseline.py:343-361): BCE (or BPR) + L2 with
        the dense-Adam semantics of torch.optim.Adam over MFbase, replayed lazily per row.  Shares the MF
        optimiser state (m, v, step) with mf_stage_epoch; call mf_flush before reading the tables."""
        tri = self._dev(triples, torch.int64)
        n = tri.shape[0]
        nb = (n + batch_size - 1) // batch_size
        t = self._mf_tables(mfbase, None, None)
        self._mf_lr = float(lr)
        losses = torch.empty(nb, device=self.device, dtype=torch.float32)
        step = ctypes.c_int64(self.mf_step)
        check(self.lib.sml_embed_loss_adam_epoch(self._ctx, ctypes.byref(t), _ptr(tri), n, int(batch_size), float(lr),
                                                 float(lam_user), float(lam_item),
                                                 _lib.LOSS_BCE if bce else _lib.LOSS_BPR, ctypes.byref(step),
                                                 _ptr(losses), self._stream()), "sml_embed_loss_adam_epoch")
        self.mf_step = step.value
        return losses

    # ------------------------------------------------------------------ device batch supply (fast mode)
    def sample_negatives(self, users, item_all, user_ptr, user_items, seed):
        """A negative per element of `users` (device int64), uniform over item_all, never one of the user's own items
        (CSR user_ptr / user_items, device int64).  Distribution of the reference's sampler, not its numpy stream."""
        users = self._dev(users, torch.int64)
        n = users.shape[0]
        negs = torch.empty(n, device=self.device, dtype=torch.int64)
        failed = torch.zeros(1, device=self.device, dtype=torch.int32)
        check(self.lib.sml_sample_negatives(self._ctx, _ptr(users), n, _ptr(item_all), item_all.shape[0], _ptr(user_ptr),
                                            user_ptr.shape[0] - 1, _ptr(user_items), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                            _ptr(negs), _ptr(failed), self._stream()), "sml_sample_negatives")
        return negs, failed

    def sample_negatives_ex(self, users, item_all, user_ptr, user_items, seed, pool=1, cdf=None, w_user=None, w_item=None,
                            want_score=False, max_workgroups=0):
        """A training negative per element of `users` (sml_sample_negatives_ex, "training negatives" in include/sml_hip.h):
        candidates uniform over item_all -- or, with cdf (float64 [pop], nondecreasing, last entry exactly 1.0; a host
        array, validated here before it is uploaded, or what sml_amd.sampling.device_cdf returned), by that distribution --
        never one of the user's own items (CSR user_ptr / user_items, device int64); with pool = M > 1 the one of the first
        M admissible candidates that the fp32 tables w_user / w_item [rows, d], d = 32 / 64, score highest.  pool=1,
        cdf=None gives sample_negatives' bytes.  Returns (negs, failed[, score]); score (float32 [n], pool > 1 only, else
        None) with want_score.  With pool > 1 the users and item_all are range-checked against the tables, one read-back."""
        from . import sampling
        users = self._dev(users, torch.int64)
        item_all, user_ptr, user_items = (self._dev(t, torch.int64) for t in (item_all, user_ptr, user_items))
        n, pop, pool = users.shape[0], item_all.shape[0], int(pool)
        if pool < 1 or pool > 64:
            raise ValueError("sample_negatives_ex: pool must be in 1..64, got %d" % pool)
        if pop <= 0:
            raise ValueError("sample_negatives_ex: item_all is empty")
        if cdf is not None and not isinstance(cdf, sampling.DeviceCdf):
            cdf = sampling.device_cdf(cdf, self.device, pop)           # validated on the host, then uploaded
        if cdf is not None and (cdf.tensor.shape[0] != pop or cdf.tensor.device != self.device):
            raise ValueError("sample_negatives_ex: cdf must have one entry per item of item_all (%d), on %s" % (pop, self.device))
        wu = wi = score = None
        if pool > 1:
            if w_user is None or w_item is None:
                raise ValueError("sample_negatives_ex: pool > 1 scores the candidates: w_user and w_item are needed")
            if self.d not in (32, 64):
                raise ValueError("sample_negatives_ex: pool > 1 needs embedding width 32 or 64, got %d" % self.d)
            wu, wi = self._table(w_user), self._table(w_item)
            if n:
                lim = torch.stack([users.min(), users.max(), item_all.min(), item_all.max()]).tolist()      # one read-back
                if lim[0] < 0 or lim[1] >= wu.shape[0] or lim[2] < 0 or lim[3] >= wi.shape[0]:
                    raise ValueError("sample_negatives_ex: a user or an item of item_all is outside the tables")
            if want_score:
                score = torch.empty(n, device=self.device, dtype=torch.float32)
        negs = torch.empty(n, device=self.device, dtype=torch.int64)
        failed = torch.empty(1, device=self.device, dtype=torch.int32)
        check(self.lib.sml_sample_negatives_ex(self._ctx, _ptr(users), n, _ptr(item_all), pop, _ptr(user_ptr), user_ptr.shape[0] - 1,
                                               _ptr(user_items), _ptr(cdf.tensor if cdf is not None else None), pool, _ptr(wu), _ptr(wi),
                                               self.d, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(max_workgroups), _ptr(negs),
                                               _ptr(score), _ptr(failed), self._stream()), "sml_sample_negatives_ex")
        return (negs, failed, score) if want_score else (negs, failed)

    def device_epoch(self, ui, n, seed, mat=None, row_stride=1, col=0):
        """int64 [n,3] device triples of one shuffled pass (sml_device_epoch): columns 0, 1 = ui[perm(e)] (ui: device int64
        [n,2]); column 2 = mat[perm(e) * row_stride + col] when a device integer matrix / column vector is given, else
        left for sample_negatives.  perm: the counter-based permutation keyed by `seed`."""
        out = torch.empty((int(n), 3), device=self.device, dtype=torch.int64)
        eb = 8
        if mat is not None:
            if mat.dtype not in (torch.int32, torch.int64) or not mat.is_contiguous() or mat.device != self.device:
                raise ValueError("mat: a contiguous int32 / int64 device tensor")
            eb = mat.element_size()
        check(self.lib.sml_device_epoch(self._ctx, _ptr(ui), _ptr(mat), eb, int(row_stride), int(col), int(n),
                                        ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(out), self._stream()), "sml_device_epoch")
        return out

    # ------------------------------------------------------------------ SPMF rank-weighted sampling
    def rank_weights(self, w_user, w_item, rows):
        """SPMF.compute_R_W_P on the device (sml_rank_weights): rows int64 [N,2] -> (score f32 [N], rank int32 [N] in 1..N,
        order int32 [N] with order[k-1] the row of rank k, p f32 [N]).  Rank 1 is the highest score; ties keep row order."""
        wu, wi = self._table(w_user), self._table(w_item)
        rows = self._dev(rows, torch.int64).reshape(-1, 2).contiguous()
        n = rows.shape[0]
        if n and (int(rows.min()) < 0 or int(rows[:, 0].max()) >= wu.shape[0] or int(rows[:, 1].max()) >= wi.shape[0]):
            raise ValueError("rank_weights: a row's user or item is outside the tables")
        score = torch.empty(n, device=self.device, dtype=torch.float32)
        rank = torch.empty(n, device=self.device, dtype=torch.int32)
        order = torch.empty(n, device=self.device, dtype=torch.int32)
        p = torch.empty(n, device=self.device, dtype=torch.float32)
        nbytes = int(self.lib.sml_rank_weights_scratch_bytes(self._ctx, n))
        if nbytes < 0:
            check(-1, "sml_rank_weights_scratch_bytes")
        scratch = torch.empty(max(nbytes, 1), device=self.device, dtype=torch.uint8)
        check(self.lib.sml_rank_weights(self._ctx, _ptr(wu), _ptr(wi), _ptr(rows), n, _ptr(scratch), _ptr(score), _ptr(rank),
                                        _ptr(order), _ptr(p), self._stream()), "sml_rank_weights")
        return score, rank, order, p

    def weighted_epoch(self, rows, order, item_all, user_ptr, user_items, n_out, seed):
        """int64 [n_out,3] device triples drawn with SPMF's rank weights (sml_weighted_epoch): rows int64 [N,2] and `order`
        as rank_weights returned it; negatives by the rejection walk over item_all and the CSR user_ptr / user_items
        (device int64).  Returns (triples, failed) with failed a device int32 [1]."""
        rows = self._dev(rows, torch.int64).reshape(-1, 2).contiguous()
        order = self._dev(order, torch.int32)
        item_all, user_ptr, user_items = (self._dev(t, torch.int64) for t in (item_all, user_ptr, user_items))
        if order.shape[0] != rows.shape[0]:
            raise ValueError("weighted_epoch: order must have one entry per row")
        out = torch.empty((int(n_out), 3), device=self.device, dtype=torch.int64)
        failed = torch.zeros(1, device=self.device, dtype=torch.int32)
        check(self.lib.sml_weighted_epoch(self._ctx, _ptr(rows), rows.shape[0], _ptr(order), _ptr(item_all), item_all.shape[0],
                                          _ptr(user_ptr), user_ptr.shape[0] - 1, _ptr(user_items), int(n_out),
                                          ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(out), _ptr(failed), self._stream()),
              "sml_weighted_epoch")
        return out, failed

    # ------------------------------------------------------------------ interaction sets (interaction_set.hip)
    def _iset_rows(self, rows):
        rows = self._dev(rows, torch.int64)
        if rows.dim() != 2 or rows.shape[1] < 2:
            raise ValueError("expected (user, item) rows [m, >= 2], got shape %s" % (tuple(rows.shape),))
        return rows

    def _iset(self, s):
        off, items = self._dev(s[0], torch.int64), self._dev(s[1], torch.int32)
        return off, items, int(items.shape[0])

    def _scratch(self, nbytes, what):
        if nbytes < 0:
            check(-1, what)
        return torch.empty(max(int(nbytes), 16), device=self.device, dtype=torch.uint8)

    def iset_build(self, rows, n_user, n_item):
        """The set of the distinct (user, item) pairs of rows int [m, >= 2] (columns 0 and 1; duplicates allowed, any
        order, m = 0 allowed; a device tensor or a host array) as the Seen CSR on the device (sml_iset_build): (off int64
        [n_user + 1], items int32 [nnz]).  The ids are trusted: DeviceSeen.add checks their range.  One scalar (nnz) is read
        back to trim `items`."""
        rows = self._iset_rows(rows)
        m, n_user, n_item = rows.shape[0], int(n_user), int(n_item)
        scratch = self._scratch(self.lib.sml_iset_build_scratch_bytes(self._ctx, m, n_user, n_item), "sml_iset_build_scratch_bytes")
        off = torch.empty(n_user + 1, device=self.device, dtype=torch.int64)
        items = torch.empty(m, device=self.device, dtype=torch.int32)
        check(self.lib.sml_iset_build(self._ctx, _ptr(rows), m, rows.shape[1], n_user, n_item, _ptr(scratch), _ptr(off), _ptr(items),
                                      self._stream()), "sml_iset_build")
        return off, items[:int(off[-1])] if m else items

    def iset_union(self, a, b, n_user):
        """The union, user by user, of two sets (off, items) over n_user users (sml_iset_union) as a new pair; the inputs
        are left alone.  `items` of each input holds exactly its nnz entries.  One scalar (the new nnz) is read back."""
        n_user = int(n_user)
        a_off, a_items, nnz_a = self._iset(a)
        b_off, b_items, nnz_b = self._iset(b)
        if a_off.shape[0] != n_user + 1 or b_off.shape[0] != n_user + 1:
            raise ValueError("iset_union: both sets must be over %d users" % n_user)
        scratch = self._scratch(self.lib.sml_iset_union_scratch_bytes(self._ctx, nnz_a, nnz_b, n_user), "sml_iset_union_scratch_bytes")
        off = torch.empty(n_user + 1, device=self.device, dtype=torch.int64)
        items = torch.empty(nnz_a + nnz_b, device=self.device, dtype=torch.int32)
        check(self.lib.sml_iset_union(self._ctx, n_user, _ptr(a_off), _ptr(a_items), nnz_a, _ptr(b_off), _ptr(b_items), nnz_b,
                                      _ptr(scratch), _ptr(off), _ptr(items), self._stream()), "sml_iset_union")
        return off, items[:int(off[-1])] if nnz_a + nnz_b else items

    def iset_contains(self, rows, s):
        """bool tensor [m]: whether (rows[r][0], rows[r][1]) is in the set s = (off, items) (sml_iset_contains).  The ids
        are trusted: the users must be inside the set's user range."""
        rows = self._iset_rows(rows)
        off, items, _ = self._iset(s)
        out = torch.empty(rows.shape[0], device=self.device, dtype=torch.uint8)
        check(self.lib.sml_iset_contains(self._ctx, _ptr(rows), rows.shape[0], rows.shape[1], _ptr(off), _ptr(items), _ptr(out),
                                         self._stream()), "sml_iset_contains")
        return out.bool()

    # ------------------------------------------------------------------ test-set negatives (neg_sets.hip)
    def neg_sets(self, rows, g0, timeline, neg_num, seed, max_workgroups=0):
        """The negatives of the stream rows g0 .. g0 + n - 1 (sml_neg_sets): rows int [n, >= 2] (columns 0 and 1; a device
        tensor or a host array), timeline a sml_amd.prepare.Timeline of this device built from the whole stream.  Returns
        (out int64 [n, 2 + neg_num] on the device, failed device int32 [1]); a failed row keeps -1 in the slots it did not
        fill.  The ids are trusted: the Timeline checked their range.  Nothing is read back."""
        rows = self._iset_rows(rows)
        n, g0, neg_num = rows.shape[0], int(g0), int(neg_num)
        if g0 < 0 or g0 + n > timeline.total:
            raise ValueError("neg_sets: rows %d .. %d are outside the timeline's %d" % (g0, g0 + n, timeline.total))
        if timeline.order.device != self.device:
            raise ValueError("neg_sets: the timeline lives on %s, not on %s" % (timeline.order.device, self.device))
        n_cat = timeline.n_cat_all[g0:g0 + n]
        out = torch.empty((n, 2 + max(neg_num, 0)), device=self.device, dtype=torch.int64)
        failed = torch.empty(1, device=self.device, dtype=torch.int32)
        check(self.lib.sml_neg_sets(self._ctx, _ptr(rows), n, rows.shape[1], g0, _ptr(n_cat), _ptr(timeline.order), _ptr(timeline.h_off),
                                    timeline.n_user, _ptr(timeline.h_items), _ptr(timeline.h_since), neg_num,
                                    ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(max_workgroups), _ptr(out), _ptr(failed),
                                    self._stream()), "sml_neg_sets")
        return out, failed

    # ------------------------------------------------------------------ a2
    def mf_forward(self, w_user, w_item, user, item, norm=False):
        wu, wi = self._table(w_user), self._table(w_item)
        user, item = self._dev(user, torch.int64), self._dev(item, torch.int64)
        n = user.shape[0]
        ue = torch.empty(n, self.d, device=self.device, dtype=torch.float32)
        ie = torch.empty_like(ue)
        sc = torch.empty(n, device=self.device, dtype=torch.float32)
        check(self.lib.sml_mf_forward(self._ctx, _ptr(wu), _ptr(wi), _ptr(user), _ptr(item), n, int(bool(norm)),
                                      _ptr(ue), _ptr(ie), _ptr(sc), self._stream()), "sml_mf_forward")
        return ue, ie, sc

    # ------------------------------------------------------------------ a13
    BLOCKED_EVAL_MIN_ITEM_BYTES = 6 << 20   # L2-block the evaluation once the item table outgrows an XCD's 4 MB L2

    def _blocked_rows(self, rows, n_item):
        """Candidates of `rows` grouped by item range (built once per test set, kept while the tensor lives)."""
        key = (rows.data_ptr(), tuple(rows.shape), int(n_item))
        cache = self.__dict__.setdefault("_eval_blocked", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 3:
                cache.pop(next(iter(cache)))
            rows_b = torch.empty(rows.shape, device=self.device, dtype=torch.int32)
            off = torch.empty((rows.shape[0], 9), device=self.device, dtype=torch.int32)
            check(self.lib.sml_eval_prepare(self._ctx, _ptr(rows), rows.shape[0], rows.shape[1], int(n_item), _ptr(rows_b),
                                            _ptr(off), self._stream()), "sml_eval_prepare")
            rows.record_stream(torch.cuda.current_stream(self.device))      # (it may have been uploaded on another stream)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            hit = cache[key] = (rows_b, off, rows, ev)     # keeps `rows` alive: the key is its address
        else:
            torch.cuda.current_stream(self.device).wait_event(hit[3])   # built on another stream, perhaps
        return hit[0], hit[1]

    def _sliced_rows(self, rows, n_item):
        """Candidates of `rows` re-ordered slice-major for the LDS-sliced rank pass (built once per test set, kept while
        the tensor lives); None when the shape is outside that pass's range."""
        n, c = rows.shape
        ns = int(self.lib.sml_eval_sliced_slices(self._ctx, n, c, int(n_item)))
        if ns <= 0:
            return None
        key = (rows.data_ptr(), tuple(rows.shape), int(n_item))
        cache = self.__dict__.setdefault("_eval_sliced", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 3:
                cache.pop(next(iter(cache)))
            entries = torch.empty(int(self.lib.sml_eval_sliced_entries(self._ctx, n, c, int(n_item))), device=self.device, dtype=torch.int32)
            seg_off = torch.empty(ns * ((n + 63) // 64) + 1, device=self.device, dtype=torch.int32)
            work = torch.empty(int(self.lib.sml_eval_sliced_work_ints(self._ctx, n, c, int(n_item))), device=self.device, dtype=torch.int32)
            check(self.lib.sml_eval_prepare_sliced(self._ctx, _ptr(rows), n, c, int(n_item), _ptr(entries), _ptr(seg_off), _ptr(work),
                                                   self._stream()), "sml_eval_prepare_sliced")
            cur = torch.cuda.current_stream(self.device)
            rows.record_stream(cur)
            ev = torch.cuda.Event()
            ev.record(cur)
            hit = cache[key] = (entries, seg_off, rows, ev)     # keeps `rows` alive: the key is its address
        else:
            torch.cuda.current_stream(self.device).wait_event(hit[3])
        return hit[0], hit[1]

    # The form large test sets get: blocked (default) | sliced | plain.  The LDS-sliced pass is 1.8x faster on the evaluation
    # partition (1.38 against 2.55 ms per Yelp-shaped evaluation) and leaves that stream 45 % busy instead of 86 %, but the period
    # is 0.5-1 ms LONGER with it in a same-box A/B (the training kernels beside it run 1 % slower: profiles/r05s_*): the
    # evaluation stream is not the critical path, so the cheaper-to-sit-beside kernel stays the default.
    EVAL_MODE = switches.get("SML_EVAL")

    def eval_ranks(self, user_tab, item_tab, rows, blocked=None, max_workgroups=0, sliced=None):
        wu, wi = self._table(user_tab), self._table(item_tab)
        rows = self._dev(rows, torch.int64)
        n, c = rows.shape
        rank = torch.empty(n, device=self.device, dtype=torch.int32)
        if n == 0:                         # a rank that owns no row of this test set
            return rank
        if wi.numel() * 4 > (1 << 32):     # past the blocked kernel's 32-bit byte offsets: the plain kernel ranks it
            blocked = False
        large = wi.numel() * 4 >= self.BLOCKED_EVAL_MIN_ITEM_BYTES and n * c >= (1 << 22)
        if sliced is None:
            sliced = blocked is None and large and self.EVAL_MODE == "sliced"
        if sliced:
            prep = self._sliced_rows(rows, wi.shape[0])
            if prep is not None:
                entries, seg_off = prep
                # one scratch block per (stream, size), kept: passes queued on one stream use it one after the other (stream
                # order), and nothing of it outlives a pass
                nbytes = int(self.lib.sml_eval_sliced_scratch_bytes(self._ctx, n, c, wi.shape[0]))
                skey = (torch.cuda.current_stream(self.device).cuda_stream, nbytes)
                pool = self.__dict__.setdefault("_eval_sliced_scratch", {})
                scratch = pool.get(skey)
                if scratch is None:
                    if len(pool) >= 4:
                        pool.pop(next(iter(pool)))
                    scratch = pool[skey] = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
                check(self.lib.sml_eval_ranks_sliced(self._ctx, _ptr(wu), _ptr(wi), _ptr(rows), _ptr(entries), _ptr(seg_off), n, c,
                                                     wi.shape[0], _ptr(scratch), _ptr(rank), int(max_workgroups), self._stream()),
                      "sml_eval_ranks_sliced")
                for t in (entries, seg_off):
                    t.record_stream(torch.cuda.current_stream(self.device))
                return rank
        if blocked is None:
            blocked = large and self.EVAL_MODE != "plain"
        if blocked:
            rows_b, off = self._blocked_rows(rows, wi.shape[0])
            check(self.lib.sml_eval_ranks_blocked(self._ctx, _ptr(wu), _ptr(wi), _ptr(rows_b), _ptr(off), n, c,
                                                  _ptr(rank), int(max_workgroups), self._stream()), "sml_eval_ranks_blocked")
            for t in (rows_b, off):            # built on one stream, read here on another: not to be recycled under this launch
                t.record_stream(torch.cuda.current_stream(self.device))
        else:
            check(self.lib.sml_eval_ranks(self._ctx, _ptr(wu), _ptr(wi), _ptr(rows), n, c, _ptr(rank), self._stream()),
                  "sml_eval_ranks")
        return rank

    # ---- full-catalogue retrieval (retrieval.hip) ----
    TOPK_SCRATCH_BYTES = 256 << 20       # users of one sml_topk_items call are capped so its candidate scratch fits this

    def _seen(self, seen):
        if seen is None:
            return None, None
        off, items = seen
        off, items = self._dev(off, torch.int64), self._dev(items, torch.int32)
        if items.numel() == 0:           # an empty Seen still passes BOTH arrays (torch gives an empty tensor a null pointer)
            items = torch.zeros(1, device=self.device, dtype=torch.int32)
        return off, items

    def _allow(self, allow, n_item):
        """allow=: None, or the item filter of sml_*_filtered as an int32 word tensor [ceil(n_item / 32)] on this device
        (sml_amd.retrieval.as_filter makes one from an ItemFilter or a bool mask)."""
        if allow is None:
            return None
        if not torch.is_tensor(allow) or allow.dtype != torch.int32:
            from .retrieval import as_filter
            return as_filter(allow, n_item, self.device)
        if allow.device != self.device or allow.dim() != 1 or not allow.is_contiguous() or allow.shape[0] != (n_item + 31) // 32:
            raise ValueError("expected a contiguous int32 item filter [%d] on %s, got %s on %s"
                             % ((n_item + 31) // 32, self.device, tuple(allow.shape), allow.device))
        return allow

    def item_filter_from_ids(self, ids, n_item, invert=False):
        """The item filter (int32 words [ceil(n_item / 32)], tail bits 0) that allows exactly `ids` -- or, with invert,
        everything except `ids` -- built on the device (sml_item_filter_from_ids).  Duplicates are allowed; ids outside
        [0, n_item) raise."""
        n_item = int(n_item)
        n_words = int(self.lib.sml_item_filter_words(n_item))
        if n_words < 0:
            check(-1, "sml_item_filter_words")
        if not torch.is_tensor(ids):
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= n_item):        # checked before the ids narrow to int32
            raise ValueError("item id out of range (n_item=%d)" % n_item)
        ids = self._dev(ids, torch.int32).reshape(-1)
        words = torch.empty(n_words, device=self.device, dtype=torch.int32)
        check(self.lib.sml_item_filter_from_ids(self._ctx, _ptr(ids), ids.numel(), n_item, int(bool(invert)), _ptr(words),
                                                self._stream()), "sml_item_filter_from_ids")
        return words

    def _adjust(self, adjust, item_tab):
        """adjust=: None (the bare score), or the per-item score terms of sml_*_adjusted: a float32 tensor [2, n_pad] on this
        device (item_adjust / item_adjust_cosine build one), or a sml_amd.retrieval.ItemScore (resolved against item_tab)."""
        if adjust is None:
            return None
        if not torch.is_tensor(adjust):
            from .retrieval import ItemScore
            if not isinstance(adjust, ItemScore):
                raise ValueError("adjust= is None, an ItemScore or a float32 tensor [2, n_pad], got %s" % type(adjust).__name__)
            return adjust.device(self, item_tab)
        n_pad = (item_tab.shape[0] + 31) // 32 * 32
        if adjust.dtype != torch.float32 or adjust.device != self.device or not adjust.is_contiguous() or tuple(adjust.shape) != (2, n_pad):
            raise ValueError("expected a contiguous float32 item adjust [2, %d] on %s, got %s %s on %s"
                             % (n_pad, self.device, adjust.dtype, tuple(adjust.shape), adjust.device))
        if adjust.data_ptr() % 16:           # the walk reads it with 16-byte loads
            raise ValueError("the item adjust table must be 16-byte aligned (a view at an odd storage offset is not)")
        return adjust

    def item_adjust(self, n_item, scale=None, offset=None):
        """The padded per-item term table float32 [2, n_pad] (plane 0 scale, plane 1 offset; include/sml_hip.h) from optional
        per-item arrays [n_item]: scale None = 1, offset None = +0.  Built on the device (sml_item_adjust_fill)."""
        n_item = int(n_item)
        n_pad = int(self.lib.sml_item_adjust_len(n_item))
        if n_pad < 0:
            check(-1, "sml_item_adjust_len")
        parts = []
        for name, v in (("scale", scale), ("offset", offset)):
            if v is not None:
                v = self._dev(v, torch.float32).reshape(-1)
                if v.shape[0] != n_item:
                    raise ValueError("%s must have %d entries, got %d" % (name, n_item, v.shape[0]))
            parts.append(v)
        adj = torch.empty(2, n_pad, device=self.device, dtype=torch.float32)
        check(self.lib.sml_item_adjust_fill(self._ctx, _ptr(parts[0]), _ptr(parts[1]), n_item, _ptr(adj), self._stream()),
              "sml_item_adjust_fill")
        return adj

    def item_adjust_cosine(self, item_tab, adj=None):
        """Write scale[i] = 1 / ||item_tab[i]|| (0 for a zero row) into plane 0 of adj (a new table with offset 0 when adj is
        None) and return it: ranking by it is ranking by the cosine (sml_item_adjust_cosine; fp32 or fp16 table)."""
        _, wi, _ = self._retrieval_tables(item_tab, item_tab)
        adj = self.item_adjust(wi.shape[0]) if adj is None else self._adjust(adj, wi)
        check(self.lib.sml_item_adjust_cosine(self._ctx, _ptr(wi), wi.element_size(), wi.shape[0], _ptr(adj), self._stream()),
              "sml_item_adjust_cosine")
        return adj

    def _retrieval_call(self, base, wi, sfx, allow, adj):
        """(entry point, its name, what follows w_item, what follows seen_items): adj None -- the entry points without terms,
        exactly as before; else sml_<base>_adjusted, which takes elem_bytes, and allow (NULL: no filter) and adj."""
        if adj is None:
            name = base + ("" if allow is None else "_filtered") + sfx
            return getattr(self.lib, name), name, (), (() if allow is None else (_ptr(allow),))
        name = base + "_adjusted"
        return getattr(self.lib, name), name, (wi.element_size(),), (_ptr(allow), _ptr(adj))

    def _retrieval_tables(self, user_tab, item_tab):
        """(user table, item table, entry-point suffix): both fp32 (the sml_* entry points) or both fp16 (sml_*_f16; the
        rows are read as packed halves, no fp32 copy).  Which widths each element type has is the library's answer."""
        if user_tab.dtype not in (torch.float32, torch.float16) or item_tab.dtype != user_tab.dtype:
            raise ValueError("retrieval tables must both be fp32 or both fp16, got %s and %s" % (user_tab.dtype, item_tab.dtype))
        for t in (user_tab, item_tab):
            if t.device != self.device or t.dim() != 2 or not t.is_contiguous() or t.shape[-1] != self.d:
                raise ValueError("expected a contiguous [rows,%d] tensor on %s, got %s on %s"
                                 % (self.d, self.device, tuple(t.shape), t.device))
        return user_tab, item_tab, "_f16" if user_tab.dtype == torch.float16 else ""

    def full_rank(self, user_tab, item_tab, rows, seen=None, allow=None, adjust=None):
        """int32 [n]: per row (u, p, ...) the number of items i != p, not in Seen(u), scoring strictly above p over the
        WHOLE item table (include/sml_hip.h, sml_full_rank / sml_full_rank_f16: fp32 or fp16 tables).
        seen = (seen_off int64 [n_user + 1], seen_items int32).  allow: an item filter (_allow); the count then runs over
        the allowed items only (sml_full_rank_filtered).  adjust: per-item score terms (_adjust); the rank is then by
        A(u, i) = fmaf(S(u, i), scale[i], offset[i]) (sml_full_rank_adjusted)."""
        wu, wi, sfx = self._retrieval_tables(user_tab, item_tab)
        allow = self._allow(allow, wi.shape[0])
        call, name, eb, flt = self._retrieval_call("sml_full_rank", wi, sfx, allow, self._adjust(adjust, wi))
        rows = self._dev(rows, torch.int64)
        n, c = rows.shape
        rank = torch.empty(n, device=self.device, dtype=torch.int32)
        if n == 0:
            return rank
        off, items = self._seen(seen)
        check(call(self._ctx, _ptr(wu), _ptr(wi), *eb, wi.shape[0], _ptr(rows), n, c, _ptr(off), _ptr(items), *flt, _ptr(rank),
                   self._stream()), name)
        return rank

    def topk_items(self, user_tab, item_tab, users, k, seen=None, allow=None, adjust=None):
        """(int64 items [n, k], float32 scores [n, k]): each user's k best items not in Seen(u), score descending then id
        ascending; missing slots are (-1, -inf) (include/sml_hip.h, sml_topk_items / sml_topk_items_f16: fp32 or fp16 tables).
        allow: an item filter (_allow); only allowed items enter the lists (sml_topk_items_filtered).  adjust: per-item score
        terms (_adjust); order and returned scores are then A(u, i) (sml_topk_items_adjusted).  1 <= k <= 128.  A call with
        sml_amd.retrieval.DEEP_FROM <= k <= 128 is handed to topk_deep, which returns the same bytes from the radix select:
        its scratch is topk_deep's (about 1 KB per user) and an argument error then names sml_topk_deep."""
        from .retrieval import DEEP_FROM
        if DEEP_FROM <= int(k) <= 128:       # the same bytes from the radix select (sml_amd.retrieval.DEEP_FROM says from which k)
            return self.topk_deep(user_tab, item_tab, users, int(k), seen, allow, adjust)[:2]
        wu, wi, sfx = self._retrieval_tables(user_tab, item_tab)
        allow = self._allow(allow, wi.shape[0])
        call, name, eb, flt = self._retrieval_call("sml_topk_items", wi, sfx, allow, self._adjust(adjust, wi))
        users = self._dev(users, torch.int64).reshape(-1)
        n, k = users.shape[0], int(k)
        off, seen_items = self._seen(seen)
        total = int(self.lib.sml_topk_scratch_bytes(self._ctx, n, k, wi.shape[0]))
        if total < 0 or n == 0:          # argument checks (k, n_item) and the empty call go through the library
            check(call(self._ctx, _ptr(wu), _ptr(wi), *eb, wi.shape[0], _ptr(users), 0, k, _ptr(off), _ptr(seen_items), *flt, None, None, None,
                       self._stream()), name)
        items = torch.empty(n, k, device=self.device, dtype=torch.int32)
        scores = torch.empty(n, k, device=self.device, dtype=torch.float32)
        chunk = n if total <= self.TOPK_SCRATCH_BYTES else max(1, int(n * self.TOPK_SCRATCH_BYTES // total))
        scratch = None
        for c0 in range(0, n, chunk):
            m = min(chunk, n - c0)
            nbytes = int(self.lib.sml_topk_scratch_bytes(self._ctx, m, k, wi.shape[0]))
            if scratch is None or scratch.numel() < nbytes:
                scratch = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
            check(call(self._ctx, _ptr(wu), _ptr(wi), *eb, wi.shape[0], _ptr(users[c0:]), m, k, _ptr(off), _ptr(seen_items), *flt,
                       _ptr(scratch), _ptr(items[c0:]), _ptr(scores[c0:]), self._stream()), name)
        return items.long(), scores

    def topk_deep(self, user_tab, item_tab, users, k, seen=None, allow=None, adjust=None, slices=0):
        """(int64 items [n, k], float32 scores [n, k], int32 n_elig [n]): topk_items' lists for 1 <= k <= 1024, selected by
        radix instead of kept sorted -- a fixed number of catalogue walks whatever k is (include/sml_hip.h, DEEP LISTS;
        sml_topk_deep).  For k <= 128 items and scores equal topk_items' byte for byte; n_elig counts each user's eligible
        items.  seen, allow and adjust as in topk_items (adjust None: the bare score).  slices: 0 leaves the grid to the
        call, 1 .. 256 forces the number of item slices (the bytes do not depend on it).  The users are walked in chunks
        whose scratch (about 1 KB per user) fits TOPK_SCRATCH_BYTES."""
        from .retrieval import deep_args
        wu, wi, _ = self._retrieval_tables(user_tab, item_tab)
        allow = self._allow(allow, wi.shape[0])
        adj = self._adjust(adjust, wi)
        users = self._dev(users, torch.int64).reshape(-1)
        n, k, slices = users.shape[0], deep_args(k), int(slices)
        off, seen_items = self._seen(seen)
        items, scores, n_elig = self._list_out(n, k)
        total = int(self.lib.sml_topk_deep_scratch_bytes(self._ctx, n, k, wi.shape[0], slices))
        if total < 0:
            check(-1, "sml_topk_deep_scratch_bytes")
        chunk = n if total <= self.TOPK_SCRATCH_BYTES else max(1, int(n * self.TOPK_SCRATCH_BYTES // total))
        scratch = None
        for c0 in range(0, max(n, 1), max(chunk, 1)):        # (n == 0: one call, which checks the arguments and launches nothing)
            m = min(chunk, n - c0)
            nbytes = int(self.lib.sml_topk_deep_scratch_bytes(self._ctx, m, k, wi.shape[0], slices))
            if m and (scratch is None or scratch.numel() < nbytes):
                scratch = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
            check(self.lib.sml_topk_deep(self._ctx, _ptr(wu), _ptr(wi), wi.element_size(), wi.shape[0], _ptr(users[c0:]), m, k, _ptr(off),
                                         _ptr(seen_items), _ptr(allow), _ptr(adj), slices, _ptr(scratch), _ptr(items[c0:]),
                                         _ptr(scores[c0:]), _ptr(n_elig[c0:]), self._stream()), "sml_topk_deep")
        return items.long(), scores, n_elig

    def topk_candidates(self, user_tab, item_tab, users, candidates, k, seen=None, allow=None, adjust=None, max_workgroups=0):
        """(int64 items [n, k], float32 scores [n, k], int32 n_elig [n]): for each user the k best DISTINCT eligible ids of
        that user's own candidate list -- in the list, inside [0, n_item), not in Seen(u), allowed, score not NaN -- score
        descending then id ascending, missing slots (-1, -inf); n_elig counts the eligible entries, repeats included
        (include/sml_hip.h, sml_topk_candidates: one wavefront per list, no catalogue walk, no scratch).  candidates: anything
        sml_amd.retrieval.as_candidates takes; users may be None when the candidates carry their own (CandidateRows).  seen,
        allow and adjust as in topk_items; row x equals topk_items for users[x] alone with the filter `allow AND list x`.
        max_workgroups > 0 caps the grid (the bytes do not depend on it)."""
        from .retrieval import as_candidates
        wu, wi, _ = self._retrieval_tables(user_tab, item_tab)
        allow = self._allow(allow, wi.shape[0])
        adj = self._adjust(adjust, wi)
        if users is not None:
            users = self._dev(users, torch.int64).reshape(-1)
        cl = as_candidates(candidates, None if users is None else users.shape[0], self.device)
        if users is None:
            if cl.users is None:
                raise ValueError("users=None needs candidates that carry their users (a CandidateRows)")
            users = self._dev(cl.users, torch.int64)
        n, k = users.shape[0], int(k)
        off, seen_items = self._seen(seen)
        cand = cl.items if cl.items.numel() else torch.zeros(1, device=self.device, dtype=cl.items.dtype)   # (never a null pointer)
        items, scores, n_elig = self._list_out(n, k)
        check(self.lib.sml_topk_candidates(self._ctx, _ptr(wu), _ptr(wi), wi.element_size(), wi.shape[0], _ptr(users), n, _ptr(cand),
                                           cand.element_size(), _ptr(cl.off), cl.stride, cl.first, cl.cols, k, _ptr(off),
                                           _ptr(seen_items), _ptr(allow), _ptr(adj), int(max_workgroups), _ptr(items), _ptr(scores),
                                           _ptr(n_elig), self._stream()), "sml_topk_candidates")
        return items.long(), scores, n_elig

    def _ivf_lists(self, index_arrays, n_item):
        """index_arrays: an ItemIndex (anything with .list_off / .list_items) or a (list_off, list_items) pair -> (list_off int64
        [n_list + 1], list_items int32 [n_item]) on this device."""
        if hasattr(index_arrays, "list_off") and hasattr(index_arrays, "list_items"):
            index_arrays = (index_arrays.list_off, index_arrays.list_items)
        if not isinstance(index_arrays, (tuple, list)) or len(index_arrays) != 2:
            raise ValueError("an index is an ItemIndex or a (list_off, list_items) pair")
        off, items = (self._dev(t, dt) for t, dt in zip(index_arrays, (torch.int64, torch.int32)))
        if off.dim() != 1 or off.shape[0] < 2 or items.dim() != 1 or items.shape[0] != int(n_item):
            raise ValueError("expected list_off int64 [n_list + 1] and list_items int32 [%d], got %s and %s"
                             % (int(n_item), tuple(off.shape), tuple(items.shape)))
        return off, items

    def ivf_search(self, user_tab, item_tab, users, index_arrays, probes, k, seen=None, allow=None, adjust=None, max_workgroups=0):
        """(int64 items [n, k], float32 scores [n, k], int32 n_elig [n]): for each user the k best distinct eligible members of
        the lists it probes -- topk_candidates on "the members of probes[x, 0], then of probes[x, 1], ...", byte for byte, with
        no candidate matrix written (include/sml_hip.h, CLUSTERED INDEX; sml_ivf_search: one wavefront per user, no scratch).
        index_arrays: an ItemIndex or its (list_off, list_items); probes: int [n, nprobe], 1 <= nprobe <= 128, entries outside
        [0, n_list) are padding (ItemIndex.probe makes them).  seen, allow and adjust as in topk_candidates.  Probing every
        list once returns topk_items' bytes.  max_workgroups > 0 caps the grid (the bytes do not depend on it)."""
        wu, wi, _ = self._retrieval_tables(user_tab, item_tab)
        allow = self._allow(allow, wi.shape[0])
        adj = self._adjust(adjust, wi)
        users = self._dev(users, torch.int64).reshape(-1)
        list_off, list_items = self._ivf_lists(index_arrays, wi.shape[0])
        probes = self._dev(probes, torch.int32)
        n, k = users.shape[0], int(k)
        if probes.dim() != 2 or probes.shape[0] != n:
            raise ValueError("probes must be int [%d, nprobe], got shape %s" % (n, tuple(probes.shape)))
        off, seen_items = self._seen(seen)
        items, scores, n_elig = self._list_out(n, k)
        check(self.lib.sml_ivf_search(self._ctx, _ptr(wu), _ptr(wi), wi.element_size(), wi.shape[0], _ptr(users), n, _ptr(list_off),
                                      _ptr(list_items), list_off.shape[0] - 1, _ptr(probes), probes.shape[1], k, _ptr(off),
                                      _ptr(seen_items), _ptr(allow), _ptr(adj), int(max_workgroups), _ptr(items), _ptr(scores),
                                      _ptr(n_elig), self._stream()), "sml_ivf_search")
        return items.long(), scores, n_elig

    def ivf_centroids(self, item_tab, list_off, list_items, centroids, out=None):
        """The centroids [n_list, d] (the table's element type) of the lists (list_off, list_items) over item_tab: per list and
        dim the members' values added in member order in fp64, divided by the count and rounded to the element type; an empty
        list keeps its row of `centroids` (sml_ivf_centroids).  out: where to write (None: a new tensor; `centroids` itself:
        in place)."""
        _, wi, _ = self._retrieval_tables(item_tab, item_tab)
        off, items = self._ivf_lists((list_off, list_items), wi.shape[0])
        n_list = off.shape[0] - 1
        out = torch.empty_like(centroids) if out is None else out
        for t in (centroids, out):
            if t.dtype != wi.dtype or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n_list, self.d):
                raise ValueError("expected contiguous %s centroids [%d, %d] on %s, got %s %s on %s"
                                 % (wi.dtype, n_list, self.d, self.device, t.dtype, tuple(t.shape), t.device))
        check(self.lib.sml_ivf_centroids(self._ctx, _ptr(wi), wi.element_size(), wi.shape[0], _ptr(off), _ptr(items), n_list,
                                         _ptr(centroids), _ptr(out), self._stream()), "sml_ivf_centroids")
        return out

    def _als_table(self, t, what):
        if t.dtype not in (torch.float32, torch.float16) or t.device != self.device or t.dim() != 2 or not t.is_contiguous() \
                or t.shape[-1] != self.d:
            raise ValueError("%s: expected a contiguous fp32 or fp16 [rows,%d] tensor on %s, got %s %s on %s"
                             % (what, self.d, self.device, t.dtype, tuple(t.shape), t.device))
        return t

    def gram(self, table, n_rows=None):
        """float64 [d, d] on the device: G = Y^T Y over the first n_rows rows (default: all) of an fp32 or fp16 table, added in
        fp64 in the fixed chunk order of include/sml_hip.h, FOLD-IN (sml_gram: byte-defined, no atomics); d = 32 / 64."""
        w = self._als_table(table, "gram")
        n_rows = w.shape[0] if n_rows is None else int(n_rows)
        if n_rows > w.shape[0]:
            raise ValueError("gram: n_rows=%d exceeds the table's %d rows" % (n_rows, w.shape[0]))
        scratch = self._scratch(self.lib.sml_gram_scratch_bytes(self._ctx, n_rows), "sml_gram_scratch_bytes")
        g = torch.empty(self.d, self.d, device=self.device, dtype=torch.float64)
        check(self.lib.sml_gram(self._ctx, _ptr(w), w.element_size(), n_rows, _ptr(scratch), _ptr(g), self._stream()), "sml_gram")
        return g

    def als_solve(self, other_tab, gram, sets, out_tab, rows=None, reg=0.1, alpha0=0.1, max_workgroups=0):
        """The iALS half-step (include/sml_hip.h, FOLD-IN; sml_als_solve: one wavefront per row, no scratch): each named row of
        out_tab becomes (alpha0 G + sum_{i in S} y_i y_i^T + reg I)^-1 sum_{i in S} y_i over the rows y of other_tab, S being the
        row's range of sets = (off int64 [>= rows + 1], items int32), G = gram (float64 [d, d] from gram(); None only with
        alpha0 == 0).  rows: int64 ids of the rows to solve (None: all rows of out_tab); out_tab is written IN PLACE and has
        other_tab's element type.  Returns int32 status [n]: 0 solved, 1 empty set (the row is +0), 2 not solved (a pivot was
        not positive or the solution is not finite; the row is left untouched).  max_workgroups > 0 caps the grid (the bytes
        do not depend on it)."""
        wo = self._als_table(other_tab, "als_solve")
        out = self._als_table(out_tab, "als_solve")
        if out.dtype != wo.dtype:
            raise ValueError("als_solve: out_tab is %s, other_tab %s" % (out.dtype, wo.dtype))
        if gram is not None and (gram.dtype != torch.float64 or gram.device != self.device or not gram.is_contiguous()
                                 or tuple(gram.shape) != (self.d, self.d)):
            raise ValueError("als_solve: gram must be a contiguous float64 [%d, %d] tensor on %s" % (self.d, self.d, self.device))
        off, items = self._seen(sets)
        if rows is not None:
            rows = self._dev(rows, torch.int64).reshape(-1)
        n = out.shape[0] if rows is None else rows.shape[0]
        if off is not None and rows is None and off.shape[0] < n + 1:
            raise ValueError("als_solve: the set has %d rows, out_tab %d" % (off.shape[0] - 1, n))
        status = torch.empty(n, device=self.device, dtype=torch.int32)
        check(self.lib.sml_als_solve(self._ctx, _ptr(wo), wo.element_size(), wo.shape[0], _ptr(gram), float(alpha0), float(reg), _ptr(off),
                                     _ptr(items), _ptr(rows), n, _ptr(out), out.shape[0], int(max_workgroups), _ptr(status),
                                     self._stream()), "sml_als_solve")
        return status

    # ------------------------------------------------------------------ neighbourhood model (knn.hip)
    def knn_lds_limit(self):
        """The largest total list length of a row that accumulates on chip (sml_knn_lds_limit)."""
        return int(self.lib.sml_knn_lds_limit())

    def _knn_scratch(self, n_item, n, max_workgroups, kind):
        """(scratch, max_workgroups) of a call over n rows; kind 0 / 1 as sml_knn_scratch_bytes takes it, "weighted" for
        sml_cooc_weighted_scratch_bytes.  With the grid left to the call, a call of few rows asks for n workgroups when that makes
        the scratch smaller: a row never needs more than one, and the grid never changes a byte."""
        if kind == "weighted":
            what, size = "sml_cooc_weighted_scratch_bytes", lambda w: self.lib.sml_cooc_weighted_scratch_bytes(self._ctx, int(n_item), w)
        else:
            what, size = "sml_knn_scratch_bytes", lambda w: self.lib.sml_knn_scratch_bytes(self._ctx, int(n_item), w, kind)
        mw = int(max_workgroups)
        nbytes = size(mw)
        if mw == 0 and n > 0 and nbytes > 0:
            fewer = size(int(n))
            if 0 < fewer < nbytes:
                mw, nbytes = int(n), fewer
        return self._scratch(nbytes, what), mw

    def _list_out(self, n, k):
        """The (items int32 [n, k], scores float32 [n, k], n_elig int32 [n]) outputs of a list-producing call."""
        return (torch.empty(n, max(k, 0), device=self.device, dtype=torch.int32),
                torch.empty(n, max(k, 0), device=self.device, dtype=torch.float32),
                torch.empty(n, device=self.device, dtype=torch.int32))

    def cooc_topk(self, by_item, by_user, k, rows=None, norm=None, shrink=0.0, min_co=1, allow=None, max_workgroups=0, path=0):
        """(int64 items [n, k], float32 sims [n, k], int32 n_elig [n]): the co-occurrence neighbours of the query items (include/
        sml_hip.h, NEIGHBOURS; sml_cooc_topk: one wavefront per row, integer atomics only).  by_item = (off int64 [n_item + 1],
        users int32) and by_user = (off int64 [n_user + 1], items int32) are the set and its transpose as iset_build writes them.
        rows: int64 query items (None: all).  norm: None -- the score is the count -- or a float64 [n_item] table (a = b) or a
        pair (a, b) of them: sim = count / (a[i] * b[j] + shrink).  min_co: the smallest count that makes a neighbour; allow: an
        item filter on the neighbours.  Score descending then id ascending; missing slots (-1, -inf).  max_workgroups > 0 caps the
        grid and path forces the accumulator (0 auto, 1 dense, 2 LDS where it fits); neither changes a byte.  No read-back."""
        i_off, i_users = self._seen(by_item)
        u_off, u_items = self._seen(by_user)
        n_item, n_user = i_off.shape[0] - 1, u_off.shape[0] - 1
        allow = self._allow(allow, n_item)
        if norm is None:
            na = nb = None
        else:
            na, nb = norm if isinstance(norm, (tuple, list)) else (norm, norm)
            for t in (na, nb):
                if t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n_item,):
                    raise ValueError("cooc_topk: a norm table is a contiguous float64 [%d] tensor on %s" % (n_item, self.device))
        if rows is not None:
            rows = self._dev(rows, torch.int64).reshape(-1)
        n, k = n_item if rows is None else rows.shape[0], int(k)
        scratch, mw = self._knn_scratch(n_item, n, max_workgroups, 0)
        items, sims, n_elig = self._list_out(n, k)
        check(self.lib.sml_cooc_topk(self._ctx, _ptr(i_off), _ptr(i_users), _ptr(u_off), _ptr(u_items), n_user, n_item, _ptr(rows), n,
                                     _ptr(na), _ptr(nb), float(shrink), int(min_co), _ptr(allow), k, mw, int(path),
                                     _ptr(scratch), _ptr(items), _ptr(sims), _ptr(n_elig), self._stream()), "sml_cooc_topk")
        return items.long(), sims, n_elig

    def cooc_topk_weighted(self, by_item, by_user, k, user_w, frac_bits=30, rows=None, norm=None, shrink=0.0, allow=None,
                           max_workgroups=0, path=0):
        """cooc_topk with users that do not count equally (include/sml_hip.h, WEIGHTED NEIGHBOURS OF ITEMS; sml_cooc_topk_weighted):
        sim = (sum over the common users of user_w[u]) / (a[i] * b[j] + shrink), the sum taken in fixed point with frac_bits
        fractional bits by integer atomics.  user_w: a contiguous float32 [n_user] tensor on the engine's device; a user whose
        weight is not finite, not positive, rounds to 0 or exceeds 2^32 in fixed point contributes nothing.  There is no min_co.
        Everything else as in cooc_topk.  No read-back."""
        i_off, i_users = self._seen(by_item)
        u_off, u_items = self._seen(by_user)
        n_item, n_user = i_off.shape[0] - 1, u_off.shape[0] - 1
        if not torch.is_tensor(user_w) or user_w.dtype != torch.float32 or user_w.device != self.device or not user_w.is_contiguous() \
                or tuple(user_w.shape) != (n_user,):
            raise ValueError("cooc_topk_weighted: user_w is a contiguous float32 [%d] tensor on %s" % (n_user, self.device))
        allow = self._allow(allow, n_item)
        if norm is None:
            na = nb = None
        else:
            na, nb = norm if isinstance(norm, (tuple, list)) else (norm, norm)
            for t in (na, nb):
                if t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n_item,):
                    raise ValueError("cooc_topk_weighted: a norm table is a contiguous float64 [%d] tensor on %s" % (n_item, self.device))
        if rows is not None:
            rows = self._dev(rows, torch.int64).reshape(-1)
        n, k = n_item if rows is None else rows.shape[0], int(k)
        scratch, mw = self._knn_scratch(n_item, n, max_workgroups, "weighted")
        items, sims, n_elig = self._list_out(n, k)
        check(self.lib.sml_cooc_topk_weighted(self._ctx, _ptr(i_off), _ptr(i_users), _ptr(u_off), _ptr(u_items), n_user, n_item,
                                              _ptr(rows), n, _ptr(user_w), int(frac_bits), _ptr(na), _ptr(nb), float(shrink),
                                              _ptr(allow), k, mw, int(path), _ptr(scratch), _ptr(items), _ptr(sims), _ptr(n_elig),
                                              self._stream()), "sml_cooc_topk_weighted")
        return items.long(), sims, n_elig

    def knn_topk(self, nbr_items, nbr_sims, n_item, history, k, users=None, frac_bits=30, seen=None, allow=None, max_workgroups=0,
                 path=0):
        """(int64 items [n, k], float32 scores [n, k], int32 n_elig [n]): the list of each history under a neighbour table
        (include/sml_hip.h, NEIGHBOURS; sml_knn_topk).  nbr_items int [n_rows, k_nbr] / nbr_sims float32 [n_rows, k_nbr]: what
        cooc_topk returns, or any table of that shape; history = (off, items): the CSR of histories; users: int64 rows of
        history and seen (None: all).  A candidate's score is the sum, in fixed point with frac_bits fractional bits, of its sims
        over the history's members' lists; candidates in seen or outside allow are left out.  Score descending then id
        ascending; missing slots (-1, -inf).  max_workgroups and path as in cooc_topk.  No read-back."""
        nbr_items = self._dev(nbr_items, torch.int32)
        nbr_sims = self._dev(nbr_sims, torch.float32)
        if nbr_items.dim() != 2 or nbr_items.shape != nbr_sims.shape:
            raise ValueError("knn_topk: nbr_items and nbr_sims are [n_rows, k_nbr], got %s and %s"
                             % (tuple(nbr_items.shape), tuple(nbr_sims.shape)))
        n_item = int(n_item)
        h_off, h_items = self._seen(history)
        if users is not None:
            users = self._dev(users, torch.int64).reshape(-1)
        n, k = h_off.shape[0] - 1 if users is None else users.shape[0], int(k)
        s_off, s_items = self._seen(seen)
        allow = self._allow(allow, n_item)
        scratch, mw = self._knn_scratch(n_item, n, max_workgroups, 1)
        items, scores, n_elig = self._list_out(n, k)
        check(self.lib.sml_knn_topk(self._ctx, _ptr(nbr_items), _ptr(nbr_sims), nbr_items.shape[0], nbr_items.shape[1], n_item,
                                    _ptr(h_off), _ptr(h_items), _ptr(users), n, int(frac_bits), _ptr(s_off), _ptr(s_items), _ptr(allow),
                                    k, mw, int(path), _ptr(scratch), _ptr(items), _ptr(scores), _ptr(n_elig),
                                    self._stream()), "sml_knn_topk")
        return items.long(), scores, n_elig

    # ------------------------------------------------------------------ graph propagation (graph.hip)
    def graph_split_from(self):
        """The number of 256-member segments from which a row's segments are summed by separate wavefronts (sml_graph_split_from)."""
        return int(self.lib.sml_graph_split_from())

    def graph_propagate(self, src, sets, out=None, rows=None, a=None, b=None, max_workgroups=0, path=0):
        """float32 [n, d]: out[x] = a[row] * sum over the members m of row's set of b[m] * src[m], every fp32 operation in the fixed
        order of include/sml_hip.h, PROPAGATION (sml_graph_propagate: a random-row gather, no floating-point atomics).  src: a
        contiguous fp32 or fp16 [n_src, d] table; sets = (off int64 [>= rows + 1], items int32); rows: int64 ids of the rows to
        compute (None: every row of the set); a: float32 per row id, b: float32 [n_src] (None: 1).  out: where to write (None: a
        new tensor).  max_workgroups > 0 caps the grid and path forces the split of long rows (0 auto, 1 never, 2 every row of
        more than one segment); neither changes a byte.  No read-back unless rows is given (one scalar sizes the scratch)."""
        w = self._als_table(src, "graph_propagate")
        off, items = self._seen(sets)
        if off is None:
            raise ValueError("graph_propagate: sets is (off, items)")
        if rows is not None:
            rows = self._dev(rows, torch.int64).reshape(-1)
        n = off.shape[0] - 1 if rows is None else rows.shape[0]
        scales = []
        for t, need, name in ((a, off.shape[0] - 1, "a"), (b, w.shape[0], "b")):
            if t is not None and (t.dtype != torch.float32 or t.device != self.device or t.dim() != 1 or not t.is_contiguous()
                                  or t.shape[0] < need):
                raise ValueError("graph_propagate: %s is a contiguous float32 [>= %d] tensor on %s" % (name, need, self.device))
            scales.append(t)
        if out is None:
            out = torch.empty(n, self.d, device=self.device, dtype=torch.float32)
        elif out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous() or tuple(out.shape) != (n, self.d):
            raise ValueError("graph_propagate: out is a contiguous float32 [%d, %d] tensor on %s" % (n, self.d, self.device))
        if int(path) == 1 or n == 0:
            nnz = 0
        elif rows is None:
            nnz = int(items.shape[0])
        else:
            nnz = int((off[rows + 1] - off[rows]).sum())
        scratch = self._scratch(self.lib.sml_graph_scratch_bytes(self._ctx, n, nnz, int(max_workgroups)), "sml_graph_scratch_bytes")
        check(self.lib.sml_graph_propagate(self._ctx, _ptr(w), w.element_size(), w.shape[0], _ptr(off), _ptr(items), _ptr(rows), n,
                                           _ptr(scales[0]), _ptr(scales[1]), int(max_workgroups), int(path), _ptr(scratch), _ptr(out),
                                           self._stream()), "sml_graph_propagate")
        return out

    def rerank_mmr(self, item_tab, pool_items, pool_scores, k, lam, metric="cosine", normalize=True, max_workgroups=0, nrm=None):
        """Greedy MMR re-ranking of per-list pools (include/sml_hip.h, RE-RANKING; sml_rerank_mmr: one wavefront per list, no
        scratch).  pool_items int [n, C <= 128] (int64 as recommend returns them is narrowed on the device; entries outside
        the catalogue are padding) and pool_scores float32 [n, C]: each list's candidates and their relevance.  Each of up
        to k picks maximises lam * r - (1 - lam) * max sim(candidate, picks so far); r is the relevance, min-max scaled per
        list with normalize.  metric="cosine" builds the item norms from item_tab now (item_adjust_cosine) unless nrm= gives
        a ready table (float32 [>= n_item], or the [2, n_pad] table item_adjust_cosine returns); metric="dot" is the bare
        dot product.  Returns (items int64 [n, k], pos int32 [n, k] -- the pick's column in the pool --, value float32
        [n, k], n_sel int32 [n], sim_sum float32 [n] -- the sum of the picks' pairwise similarities); unused slots are
        (-1, -1, -inf).  max_workgroups > 0 caps the grid (the bytes do not depend on it)."""
        from .retrieval import rerank_args
        k, lam = rerank_args(k, lam, metric)
        _, wi, _ = self._retrieval_tables(item_tab, item_tab)
        pool_items = self._dev(pool_items, torch.int64 if not torch.is_tensor(pool_items) else pool_items.dtype)
        if pool_items.dtype not in (torch.int32, torch.int64) or pool_items.dim() != 2:
            raise ValueError("pool_items is an int32 / int64 matrix [n, C], got %s %s" % (pool_items.dtype, tuple(pool_items.shape)))
        pool_scores = self._dev(pool_scores, torch.float32)
        if pool_scores.shape != pool_items.shape:
            raise ValueError("pool_scores %s does not match pool_items %s" % (tuple(pool_scores.shape), tuple(pool_items.shape)))
        n, cols = pool_items.shape
        rerank_args(k, lam, metric, cols)
        if pool_items.dtype == torch.int64:              # ids beyond int32 are padding either way: they narrow to -1
            pool_items = torch.where((pool_items >= 0) & (pool_items < wi.shape[0]), pool_items, pool_items.new_full((), -1)).int()
        if metric == "dot":
            nrm = None
        elif nrm is None:
            nrm = self.item_adjust_cosine(wi)
        else:
            if not torch.is_tensor(nrm):
                nrm = self._dev(np.asarray(nrm), torch.float32)
            shape_ok = (nrm.dim() == 1 and nrm.shape[0] >= wi.shape[0]) or (nrm.dim() == 2 and nrm.shape[1] >= wi.shape[0])
            if nrm.dtype != torch.float32 or nrm.device != self.device or not nrm.is_contiguous() or not shape_ok:
                raise ValueError("nrm is a contiguous float32 table of at least %d entries on %s (plane 0 of item_adjust_cosine's table)"
                                 % (wi.shape[0], self.device))
        items = torch.empty(n, k, device=self.device, dtype=torch.int32)
        pos = torch.empty(n, k, device=self.device, dtype=torch.int32)
        value = torch.empty(n, k, device=self.device, dtype=torch.float32)
        n_sel = torch.empty(n, device=self.device, dtype=torch.int32)
        sim_sum = torch.empty(n, device=self.device, dtype=torch.float32)
        check(self.lib.sml_rerank_mmr(self._ctx, _ptr(wi), wi.element_size(), wi.shape[0], _ptr(pool_items), _ptr(pool_scores), n, cols, cols,
                                      _ptr(nrm), lam, int(bool(normalize)), k, int(max_workgroups), _ptr(items), _ptr(pos), _ptr(value),
                                      _ptr(n_sel), _ptr(sim_sum), self._stream()), "sml_rerank_mmr")
        return items.long(), pos, value, n_sel, sim_sum

    USER_RANK_SCRATCH_BYTES = 256 << 20  # held-out items of one sml_user_rank call are capped so its scratch fits this

    def user_ranks(self, user_tab, item_tab, users, pos_off, pos_items, seen=None, ks=(20,), allow=None, adjust=None):
        """Every user's held-out items ranked against the whole catalogue, and per-user metrics at each K in `ks`
        (include/sml_hip.h, sml_user_rank / sml_user_rank_f16 / sml_user_metrics: fp32 or fp16 tables).  users int64 [n]; pos_off int64 [n + 1] and pos_items
        int32 [n_pos]: users[x]'s held-out items, ascending and unique in [pos_off[x], pos_off[x + 1]).  Returns a dict:
        above, pos int32 [n_pos]; hits int32, dcg, ap float32 [n, len(ks)]; first int32 [n].  allow: an item filter (_allow);
        only allowed items are eligible, and a held-out item that is not allowed has pos -1 (sml_user_rank_filtered).
        adjust: per-item score terms (_adjust); above, pos and the metrics are then by A(u, i) (sml_user_rank_adjusted)."""
        wu, wi, sfx = self._retrieval_tables(user_tab, item_tab)
        allow = self._allow(allow, wi.shape[0])
        call, name, eb, flt = self._retrieval_call("sml_user_rank", wi, sfx, allow, self._adjust(adjust, wi))
        users = self._dev(users, torch.int64).reshape(-1)
        off_h = np.asarray(pos_off.cpu() if torch.is_tensor(pos_off) else pos_off, dtype=np.int64).reshape(-1)
        pos_items = self._dev(pos_items, torch.int32).reshape(-1)
        n, n_pos = users.shape[0], pos_items.shape[0]
        if off_h.shape[0] != n + 1 or off_h[0] != 0 or off_h[-1] != n_pos or (np.diff(off_h) < 0).any():
            raise ValueError("pos_off must be non-decreasing [n + 1] from 0 to len(pos_items)")
        ks_h = np.ascontiguousarray(np.asarray(ks, dtype=np.int32).reshape(-1))
        ks_p = ctypes.c_void_p(ks_h.ctypes.data)
        off, seen_items = self._seen(seen)
        n_k = ks_h.shape[0]
        out = dict(above=torch.empty(n_pos, device=self.device, dtype=torch.int32),
                   pos=torch.empty(n_pos, device=self.device, dtype=torch.int32),
                   hits=torch.empty(n, n_k, device=self.device, dtype=torch.int32),
                   dcg=torch.empty(n, n_k, device=self.device, dtype=torch.float32),
                   ap=torch.empty(n, n_k, device=self.device, dtype=torch.float32),
                   first=torch.empty(n, device=self.device, dtype=torch.int32))
        if n == 0 or n_pos == 0:         # argument checks (d, n_item, Seen, ks) go through the library
            check(call(self._ctx, _ptr(wu), _ptr(wi), *eb, wi.shape[0], None, 0, None, None, 0, _ptr(off), _ptr(seen_items), *flt, None, None,
                       None, self._stream()), name)
            check(self.lib.sml_user_metrics(self._ctx, None, None, 0, ks_p, n_k, None, None, None, None, self._stream()),
                  "sml_user_metrics")
            if n:
                out["hits"].zero_()
                out["dcg"].zero_()
                out["ap"].zero_()
                out["first"].fill_(-1)
            return out
        per_item = max(1, int(self.lib.sml_user_rank_scratch_bytes(self._ctx, n, n_pos, wi.shape[0])) // n_pos)
        cap = max(1, self.USER_RANK_SCRATCH_BYTES // per_item)
        scratch = None
        c0 = 0
        while c0 < n:                    # chunks of whole users with at most `cap` held-out items (or one user)
            c1 = max(c0 + 1, int(np.searchsorted(off_h, off_h[c0] + cap, side="right")) - 1)
            c1 = min(c1, n)
            e0, e1 = int(off_h[c0]), int(off_h[c1])
            sub_off = self._dev(off_h[c0:c1 + 1] - e0, torch.int64)
            m = c1 - c0
            nbytes = int(self.lib.sml_user_rank_scratch_bytes(self._ctx, m, e1 - e0, wi.shape[0]))
            if nbytes < 0:
                check(-1, "sml_user_rank_scratch_bytes")
            if scratch is None or scratch.numel() < nbytes:
                scratch = torch.empty(max(nbytes, 1), device=self.device, dtype=torch.uint8)
            check(call(self._ctx, _ptr(wu), _ptr(wi), *eb, wi.shape[0], _ptr(users[c0:]), m, _ptr(sub_off), _ptr(pos_items[e0:]), e1 - e0,
                       _ptr(off), _ptr(seen_items), *flt, _ptr(scratch), _ptr(out["above"][e0:]), _ptr(out["pos"][e0:]),
                       self._stream()), name)
            # a chunk of empty sets reads no pos; it still passes a valid pointer (an empty slice's may be null)
            pos_c = out["pos"][e0:] if e1 > e0 else out["pos"]
            check(self.lib.sml_user_metrics(self._ctx, _ptr(pos_c), _ptr(sub_off), m, ks_p, n_k,
                                            _ptr(out["hits"][c0:]), _ptr(out["dcg"][c0:]), _ptr(out["ap"][c0:]),
                                            _ptr(out["first"][c0:]), self._stream()), "sml_user_metrics")
            c0 = c1
        return out

    # Evaluations never sit on the training stream.  eval_submit copies the two tables into a snapshot (one copy
    # kernel, a few tens of MB) on the CURRENT stream and queues the rank pass over the snapshot on the engine's side
    # stream; the training kernels that follow on the current stream -- which may overwrite the tables at once -- do
    # not wait for it.
    SNAPSHOTS = 3
    # The chip is PARTITIONED between the two streams: the side stream owns the last SIDE_EVAL_CUS compute units of
    # the CU mask (mask bit i is a CU of XCD i % 8: a contiguous range takes the same share of every XCD), and the
    # training loop may run on the rest (`training_stream()`); the evaluation then neither shares SIMD issue slots
    # nor a CU's L2 port with the latency-bound training kernels.  SML_SIDE_EVAL_CUS=0 falls back to a low-priority
    # stream over all CUs with a capped grid.
    SIDE_EVAL_CUS = int(switches.get("SML_SIDE_EVAL_CUS"))      # -1: a quarter of the chip (64 of 256 CUs)
    SIDE_EVAL_WORKGROUPS = int(switches.get("SML_SIDE_EVAL_WGS"))   # grid cap of a side-stream evaluation

    def _n_cus(self):
        return int(torch.cuda.get_device_properties(self.device).multi_processor_count)

    def _side_cus(self):
        if self.SIDE_EVAL_CUS >= 0:
            return self.SIDE_EVAL_CUS
        n = self._n_cus()
        return (n // 4) // 8 * 8 if n >= 64 else 0       # whole CUs-per-XCD multiples; tiny parts are not partitioned

    _MASKED = {}     # (device index, lo, hi) -> ExternalStream: one pair of hardware queues per process, shared by its engines
    #                  and never destroyed (torch's allocator and events keep referring to a stream it has seen)

    def _masked_stream(self, lo, hi):
        key = (self.device.index or 0, int(lo), int(hi))
        st = HipEngine._MASKED.get(key)
        if st is None:
            h = ctypes.c_void_p()
            check(self.lib.sml_stream_create_cu_range(ctypes.byref(h), key[0], key[1], key[2]), "sml_stream_create_cu_range")
            st = HipEngine._MASKED[key] = torch.cuda.ExternalStream(h.value, device=self.device)
        return st

    def training_stream(self):
        """The stream over the CUs the side stream does NOT own (None when the chip is not partitioned)."""
        if self._side_cus() <= 0:
            return None
        if getattr(self, "_train", None) is None:
            self._train = self._masked_stream(0, self._n_cus() - self._side_cus())
        return self._train

    def partition(self):
        """Context manager: run the enclosed training loop on the training partition (no-op when the chip is not
        partitioned or SML_TRAIN_PARTITION=0).  The stream is ordered after the current stream on entry and the
        current stream after it on exit."""
        import contextlib, os

        @contextlib.contextmanager
        def scope():
            ts = self.training_stream() if switches.get("SML_TRAIN_PARTITION") != "0" else None
            if ts is None:
                yield
                return
            outer = torch.cuda.current_stream(self.device)
            ts.wait_stream(outer)
            with torch.cuda.stream(ts):
                yield
            outer.wait_stream(ts)
        return scope()

    def _side_eval_cap(self):
        if self.SIDE_EVAL_WORKGROUPS > 0:
            return self.SIDE_EVAL_WORKGROUPS
        return 4 * self._side_cus() if self._side_cus() > 0 else 256

    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            if self._side_cus() > 0:
                n = self._n_cus()
                self._side = self._masked_stream(n - self._side_cus(), n)
                return self._side
            prio = 0
            try:
                lo, _hi = torch.cuda.Stream.priority_range()
                prio = int(lo)                      # least urgent
            except Exception:
                prio = 0
            try:
                self._side = torch.cuda.Stream(device=self.device, priority=prio)
            except Exception:
                self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def copy_tables(self, pairs):
        """dst.copy_(src) for up to four (dst, src) pairs of same-shaped contiguous fp32 device tensors, in ONE launch
        on the current stream (save_MF_weight, model/transfer.py:911-943; evaluation snapshots).  The copies of one
        call run concurrently: no dst may be another pair's src."""
        pairs = list(pairs)
        for k in range(0, len(pairs), 4):
            chunk = pairs[k:k + 4]
            n = len(chunk)
            dst, src, nbytes = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)()
            for q, (d, s) in enumerate(chunk):
                if d.shape != s.shape or d.dtype != s.dtype or not (d.is_contiguous() and s.is_contiguous()) \
                        or (d.numel() * d.element_size()) % 16 or d.data_ptr() % 16 or s.data_ptr() % 16 or d.numel() == 0:
                    d.copy_(s)                    # odd shapes, misaligned views, empty tensors: torch's copy
                    dst[q], src[q], nbytes[q] = None, None, 0      # (a zero-byte job: the library skips it)
                    continue
                dst[q], src[q], nbytes[q] = d.data_ptr(), s.data_ptr(), d.numel() * d.element_size()
            check(self.lib.sml_copy_tables(n, dst, src, nbytes, self._stream()), "sml_copy_tables")

    def _snap_slot(self, cur):
        """Next snapshot slot of the ring; the current stream waits (on the device) for the evaluation that last read it."""
        ring = self.__dict__.setdefault("_snap", [])
        k = self.__dict__.get("_snap_next", 0) % self.SNAPSHOTS
        self._snap_next = k + 1
        while len(ring) <= k:
            ring.append(dict(ev=None))
        slot = ring[k]
        if slot["ev"] is not None:
            cur.wait_event(slot["ev"])          # the evaluation that last read this snapshot is done (device-side wait)
        return slot

    @staticmethod
    def _snap_buf(slot, key, like):
        if slot.get(key) is None or slot[key].shape != like.shape:
            slot[key] = torch.empty_like(like)
        return slot[key]

    def _side_order(self, cur, side):
        """The side stream may start on a snapshot once the copies queued on `cur` so far are done.  Device-side ordering
        (a flag kernel behind the copies, a polling kernel ahead of the side stream's work) instead of an event: a
        cross-queue barrier packet cost the training stream 2-4 ms per period (31 of them), the two tiny kernels cost
        nothing measurable."""
        mode = switches.get("SML_SIDE_SYNC")
        if mode == "event":
            check(self.lib.sml_stream_wait_stream(ctypes.c_void_p(side.cuda_stream), ctypes.c_void_p(cur.cuda_stream)),
                  "sml_stream_wait_stream")
            return
        if getattr(self, "_sync_flag", None) is None:
            self._sync_flag = torch.zeros(2, device=self.device, dtype=torch.int32)   # [sequence, time-outs]
            self._sync_seq = 0
            self._sync_seen = 0           # time-outs already reported
        self._sync_seq += 1
        check(self.lib.sml_flag_set(_ptr(self._sync_flag), self._sync_seq, ctypes.c_void_p(cur.cuda_stream)), "sml_flag_set")
        # The waiter starts polling as soon as the side stream is free, while its signal sits behind everything the
        # host has already queued on the training stream (the driver runs a whole stage ahead): the time-out is a
        # HANG GUARD, minutes not seconds (SML_FLAG_TIMEOUT_S).  A waiter that does give up is counted in flag[1]
        # (side_sync_check); the sequence word is untouched, so later evaluations stay ordered.
        check(self.lib.sml_flag_wait(_ptr(self._sync_flag), self._sync_seq, self._flag_timeout(),
                                     ctypes.c_void_p(side.cuda_stream)), "sml_flag_wait")

    def eval_submit(self, user_tab, item_tab, rows):
        """Queue the ranks of `rows` under the tables AS THEY ARE NOW (at this point of the current stream)
        and return a handle; the caller may modify the tables right away."""
        wu, wi = self._table(user_tab), self._table(item_tab)
        rows = self._dev(rows, torch.int64)
        side = self._side_stream()
        cur = torch.cuda.current_stream(self.device)
        slot = self._snap_slot(cur)
        su, si = self._snap_buf(slot, "u", wu), self._snap_buf(slot, "i", wi)
        self.copy_tables([(su, wu), (si, wi)])
        self._side_order(cur, side)
        with torch.cuda.stream(side):
            ranks = self.eval_ranks(su, si, rows, max_workgroups=self._side_eval_cap())
            ev = torch.cuda.Event()
            ev.record(side)
        slot["ev"] = ev
        rows.record_stream(side)
        return dict(ranks=ranks, event=ev, n=rows.shape[0])

    # A table-sized forward whose ONLY reader is an evaluation does not belong on the training stream either.  The
    # reference calls updata() ahead of every validation (model/transfer.py:737-739, 829-833); the one ahead of the "before
    # train transfer" test is overwritten by the next updata before any training kernel reads the tables: 10 of a period's
    # 21 table-sized forwards, 5 ms of its 110.  eval_submit_transferred snapshots what that forward READS (the four tables
    # and theta, one copy launch) and queues the forward itself, into the snapshot slot's own tables, ahead of the rank pass on
    # the evaluation stream's CUs.  Same kernels, same rows, same bits -- the tables the caller holds are not written.
    TRANSFERRED_MAX_BYTES = int(switches.get("SML_TRANSFERRED_MAX_BYTES"))   # ring budget

    def can_submit_transferred(self, user_tab, item_tab):
        """Whether the ring's six table copies per slot fit the budget (config-4-sized tables keep the in-place order)."""
        if switches.get("SML_EVAL_TRANSFERRED") == "0":
            return False
        per_slot = 3 * (user_tab.numel() + item_tab.numel()) * 4
        return per_slot * self.SNAPSHOTS <= self.TRANSFERRED_MAX_BYTES

    def _side_ctx(self):
        """A second library context for forwards on the side stream: its own MFMA operand images (the training context's
        are being stepped in place by the Adam kernels of the stream this does not wait for)."""
        if getattr(self, "_side_ctx_h", None) is None:
            h = ctypes.c_void_p()
            check(self.lib.sml_ctx_create(ctypes.byref(h), self.device.index or 0, self.d, 1024), "sml_ctx_create")
            self._side_ctx_h, self._side_variant = h, -1
        if self._side_variant != getattr(self, "_variant", 0):
            # (bit 1: an evaluation-stream context -- its table-sized forwards carry their own kernel name and timing class)
            check(self.lib.sml_ctx_set_variant(self._side_ctx_h, getattr(self, "_variant", 0) | 2), "sml_ctx_set_variant")
            self._side_variant = getattr(self, "_variant", 0)
        return self._side_ctx_h

    def eval_submit_transferred(self, transfer, last_user, hat_user, last_item, hat_item, rows):
        """Queue the ranks of `rows` under the tables updata(transfer, last_*, hat_*) WOULD produce now, without producing
        them on the current stream.  Returns a handle like eval_submit; the caller may modify all five inputs right away."""
        theta = self._select(transfer)
        tabs = [self._table(t) for t in (last_user, hat_user, last_item, hat_item)]
        rows = self._dev(rows, torch.int64)
        side = self._side_stream()
        cur = torch.cuda.current_stream(self.device)
        slot = self._snap_slot(cur)
        snaps = [self._snap_buf(slot, k, t) for k, t in zip(("lu", "hu", "li", "hi"), tabs)]
        su, si = self._snap_buf(slot, "u", tabs[0]), self._snap_buf(slot, "i", tabs[2])
        sth = self._snap_buf(slot, "theta", theta)
        self.copy_tables(list(zip(snaps, tabs)))
        sth.copy_(theta)
        self._side_order(cur, side)
        ctx = self._side_ctx()
        with torch.cuda.stream(side):
            for net, (xt, xh, out) in enumerate(((snaps[0], snaps[1], su), (snaps[2], snaps[3], si))):
                check(self.lib.sml_transfer_forward(ctx, _ptr(sth), net, _ptr(xt), _ptr(xh), _ptr(out), xt.shape[0],
                                                    self._stream()), "sml_transfer_forward")
            ranks = self.eval_ranks(su, si, rows, max_workgroups=self._side_eval_cap())
            ev = torch.cuda.Event()
            ev.record(side)
        slot["ev"] = ev
        rows.record_stream(side)
        return dict(ranks=ranks, event=ev, n=rows.shape[0])

    def eval_metrics_submit(self, handle, topk):
        """(hits, ndcg_sum) of a submitted evaluation at `topk`, on the side stream; returns (out, event)."""
        side = self._side_stream()
        with torch.cuda.stream(side):
            out = torch.empty(2, device=self.device, dtype=torch.float32)
            check(self.lib.sml_eval_metrics(self._ctx, _ptr(handle["ranks"]), handle["n"], int(topk), _ptr(out),
                                            self._stream()), "sml_eval_metrics")
            ev = torch.cuda.Event()
            ev.record(side)
        return (out, ev)

    @staticmethod
    def _flag_timeout():
        return float(switches.get("SML_FLAG_TIMEOUT_S"))

    def side_sync_check(self, block=True):
        """Raise if a side-stream evaluation gave up waiting for its table snapshot since the last check (its ranks
        were then computed over a snapshot that may have been incomplete).  Called wherever evaluation results are
        collected OR dropped (run_period without a record, bench.py).  block=True synchronises with the side stream;
        block=False never waits: it looks at the last asynchronous read-back of the counter that has completed and
        queues the next one (a period that drops its results checks the previous period's this way, and the caller
        ends the run with a blocking check).  An incident is reported once: the engine is re-armed, and later
        evaluations were ordered all along (the sequence word is never poisoned)."""
        flag = getattr(self, "_sync_flag", None)
        if flag is None:
            return
        side = self._side_stream()
        if block:
            with torch.cuda.stream(side):          # (read on the side stream: the training stream's backlog is not waited for)
                n = int(flag[1].item())
        else:
            n = self._sync_seen
            pend = getattr(self, "_sync_pending", None)
            if pend is not None and pend[1].query():
                n = int(pend[0][0])
                self._sync_pending = pend = None
            if pend is None:
                host = getattr(self, "_sync_host", None)
                if host is None:
                    host = self._sync_host = torch.zeros(1, dtype=torch.int32).pin_memory()
                with torch.cuda.stream(side):
                    host.copy_(flag[1:2], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(side)
                self._sync_pending = (host, ev)
        if n > self._sync_seen:
            new, self._sync_seen = n - self._sync_seen, n
            raise RuntimeError("%d side-stream evaluation(s) gave up waiting for their table snapshot (sml_flag_wait "
                               "timeout, SML_FLAG_TIMEOUT_S=%g): their results are not trustworthy" % (new, self._flag_timeout()))

    def eval_result(self, pending, check=True):
        """Wait (host) for an eval_metrics_submit result: (hits, ndcg_sum).  check=False: the caller collects many
        results and calls side_sync_check() once itself (each check is a device read-back)."""
        out, ev = pending[0], pending[1]
        ev.synchronize()
        if check:
            self.side_sync_check()
        h = out.cpu()
        return float(h[0]), float(h[1])

    def eval_metrics_device(self, ranks, topk):
        """(hits, ndcg_sum) as a 2-float DEVICE tensor: no synchronisation."""
        out = torch.empty(2, device=self.device, dtype=torch.float32)
        check(self.lib.sml_eval_metrics(self._ctx, _ptr(ranks), ranks.shape[0], int(topk), _ptr(out), self._stream()),
              "sml_eval_metrics")
        return out

    def eval_metrics(self, ranks, topk):
        h = self.eval_metrics_device(ranks, topk).cpu()
        return float(h[0]), float(h[1])

    # ------------------------------------------------------------------ native RCCL exchange
    def comm_init(self, dist, group=None):
        """Create the library's own RCCL communicator over the ranks of `group` (the unique id travels
        through torch.distributed) and verify it with a small all-reduce and all-gather.
        Returns True when the native exchange is usable on this rank."""
        import os
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if not os.path.exists(path):
            path = "librccl.so"
        loaded = self.lib.sml_comm_load(path.encode()) == 0
        # (a vote BEFORE the first collective of this function: a rank that cannot bind RCCL must not leave the others
        # inside the broadcast below)
        flag = torch.tensor([1.0 if loaded else 0.0], device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if float(flag.item()) < 0.5:
            return False
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        buf = ctypes.create_string_buffer(128)
        if rank == 0:
            check(self.lib.sml_comm_unique_id(buf), "sml_comm_unique_id")
        box = [bytes(buf.raw)]
        dist.broadcast_object_list(box, src=0, group=group)
        idb = ctypes.create_string_buffer(box[0], 128)
        check(self.lib.sml_comm_init(self._ctx, world, rank, idb), "sml_comm_init")
        t = torch.full((8,), float(rank + 1), device=self.device)
        check(self.lib.sml_comm_allreduce(self._ctx, _ptr(t), 8, self._stream()), "sml_comm_allreduce")
        src = torch.tensor([float(rank), rank + 0.5], device=self.device)
        dst = torch.empty(2 * world, device=self.device)
        check(self.lib.sml_comm_allgather(self._ctx, _ptr(src), _ptr(dst), 2, self._stream()), "sml_comm_allgather")
        want = torch.tensor([v for r in range(world) for v in (float(r), r + 0.5)], device=self.device)
        return bool(torch.all(t == world * (world + 1) / 2.0)) and bool(torch.equal(dst, want))

    def comm_destroy(self):
        self.lib.sml_comm_destroy(self._ctx)

    # ------------------------------------------------------------------ one-shot exchange over peer mappings
    def peer_region_bytes(self, world, rows_cap):
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self.lib.sml_peer_region_bytes(self._ctx, int(world), int(rows_cap), ctypes.byref(a), ctypes.byref(b)),
              "sml_peer_region_bytes")
        return a.value, b.value

    def peer_alloc(self, nbytes):
        """Zeroed device memory for an inbox / flags region (uncached or fine-grained: see sml_peer_alloc); an int address."""
        p = ctypes.c_void_p()
        check(self.lib.sml_peer_alloc(self.device.index, int(nbytes), ctypes.byref(p)), "sml_peer_alloc")
        self.__dict__.setdefault("_peer_owned", []).append(p.value)
        return p.value

    def peer_mem_kind(self, ptr):
        """0 uncached, 1 fine-grained, 2 plain device memory, -1 not a peer_alloc allocation."""
        return int(self.lib.sml_peer_mem_kind(ctypes.c_void_p(int(ptr))))

    def peer_free(self, ptr):
        """Free a peer_alloc region (only once every rank has detached and unmapped it)."""
        check(self.lib.sml_peer_free(self.device.index, ctypes.c_void_p(int(ptr))), "sml_peer_free")
        owned = self.__dict__.get("_peer_owned", [])
        if ptr in owned:
            owned.remove(ptr)

    def peer_close(self, ptr):
        check(self.lib.sml_peer_close(self.device.index, ctypes.c_void_p(int(ptr))), "sml_peer_close")
        opened = self.__dict__.get("_peer_opened", [])
        if ptr in opened:
            opened.remove(ptr)

    def peer_read(self, ptr, n_floats):
        """n_floats fp32 values at device address `ptr` (possibly another rank's memory), read with system-scope loads."""
        out = torch.empty(int(n_floats), device=self.device, dtype=torch.float32)
        check(self.lib.sml_peer_read(self.device.index, ctypes.c_void_p(int(ptr)), _ptr(out), int(n_floats) * 4, self._stream()),
              "sml_peer_read")
        return out

    def peer_tensor(self, shape, dtype=torch.float32):
        """A zeroed torch tensor over memory of its OWN device allocation (plain device memory, sml_peer_alloc): unlike a
        tensor from torch's caching allocator -- a slice of a larger segment -- its address can be exported whole with
        peer_export and opened by another process (an item-table shard other ranks read over the peer mapping)."""
        import os
        shape = tuple(int(v) for v in shape)
        n = 1
        for v in shape:
            n *= v
        nbytes = max(n * torch.empty((), dtype=dtype).element_size(), 16)
        old = os.environ.get("SML_PEER_MEM")
        os.environ["SML_PEER_MEM"] = "plain"
        try:
            ptr = self.peer_alloc(nbytes)
        finally:
            if old is None:
                del os.environ["SML_PEER_MEM"]
            else:
                os.environ["SML_PEER_MEM"] = old
        typestr = {torch.float32: "<f4", torch.float16: "<f2", torch.int32: "<i4", torch.int64: "<i8"}[dtype]

        class _Raw(object):
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        t = torch.as_tensor(_Raw(), device=self.device)
        t._sml_peer_ptr = ptr
        return t

    def peer_tensor_free(self, t):
        """Free a peer_tensor's allocation (the tensor must not be used afterwards; every rank must have unmapped it)."""
        ptr = getattr(t, "_sml_peer_ptr", None)
        if ptr is not None:
            torch.cuda.synchronize(self.device)
            t._sml_peer_ptr = None
            self.peer_free(ptr)

    def peer_export(self, ptr):
        buf = ctypes.create_string_buffer(64)
        check(self.lib.sml_peer_export(ctypes.c_void_p(ptr), buf), "sml_peer_export")
        return bytes(buf.raw)

    def peer_open(self, handle):
        p = ctypes.c_void_p()
        check(self.lib.sml_peer_open(self.device.index, ctypes.create_string_buffer(handle, 64), ctypes.byref(p)), "sml_peer_open")
        self.__dict__.setdefault("_peer_opened", []).append(p.value)
        return p.value

    def peer_attach(self, world, rank, inbox, flags, rows_cap, timeout_s=60.0):
        """inbox / flags: every rank's regions as addresses valid on THIS device (own allocations, sml_peer_open results,
        or -- several ranks in one process -- the other ranks' allocations)."""
        n = int(world)
        a, b = (ctypes.c_void_p * n)(*[int(x) for x in inbox]), (ctypes.c_void_p * n)(*[int(x) for x in flags])
        check(self.lib.sml_peer_attach(self._ctx, n, int(rank), a, b, int(rows_cap), float(timeout_s)), "sml_peer_attach")
        self.peer_world, self.peer_rows_cap = n, int(rows_cap)

    def peer_detach(self):
        self.lib.sml_peer_detach(self._ctx)
        self.peer_world = 0

    def peer_status(self):
        """Consumers that gave up waiting for a peer's push since attach (synchronous read)."""
        n = ctypes.c_int(0)
        check(self.lib.sml_peer_status(self._ctx, ctypes.byref(n)), "sml_peer_status")
        return n.value

    def peer_allreduce_check(self, src, timeout_s=0.0):
        dst = torch.empty_like(src)
        check(self.lib.sml_peer_allreduce_check(self._ctx, _ptr(src), _ptr(dst), src.numel(), float(timeout_s), self._stream()),
              "sml_peer_allreduce_check")
        return dst

    # ------------------------------------------------------------------ measurement
    def _prof_ctxs(self):
        """The library contexts whose launches are bracketed: the engine's own and, once it exists, the side stream's
        (eval_submit_transferred runs its table-sized forwards through it, on the evaluation stream)."""
        side = getattr(self, "_side_ctx_h", None)
        return [self._ctx] + ([side] if side else [])

    def profile(self, on):
        if on and hasattr(self, "_side_stream") and getattr(self, "_side_ctx_h", None) is None and self.device.type == "cuda":
            self._side_ctx()                       # (so that its launches are bracketed from their first one)
        for c in self._prof_ctxs():
            check(self.lib.sml_prof_enable(c, int(bool(on))), "sml_prof_enable")
            if on:
                check(self.lib.sml_prof_reset(c), "sml_prof_reset")

    def profile_pair_overhead(self, n=512):
        """Microseconds an EMPTY HIP-event pair reads on the current stream (subtract it from short kernels' averages)."""
        us = ctypes.c_double(0.0)
        check(self.lib.sml_prof_pair_overhead(self._ctx, int(n), self._stream(), ctypes.byref(us)), "sml_prof_pair_overhead")
        return us.value

    def profile_read(self, which="all"):
        """{kernel class: (launches, total ms)} measured with HIP events since profile(True).  which: "all" (both contexts,
        summed), "main" (the engine's own: the training stream) or "side" (the evaluation stream's forwards)."""
        out = {}
        ctxs = self._prof_ctxs()
        ctxs = ctxs[:1] if which == "main" else ctxs[1:] if which == "side" else ctxs
        for ctx in ctxs:
            for c in range(self.lib.sml_prof_classes()):
                cnt, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
                check(self.lib.sml_prof_get(ctx, c, ctypes.byref(cnt), ctypes.byref(ms)), "sml_prof_get")
                if cnt.value:
                    name = self.lib.sml_prof_name(c).decode()
                    have = out.get(name, (0, 0.0))
                    out[name] = (have[0] + cnt.value, have[1] + ms.value)
        return out

    def selftest(self):
        check(self.lib.sml_selftest(self.device.index), "sml_selftest")


_engines = {}


def get_engine(device, d, max_batch=4096):
    """Process-wide engine for (device, d)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (str(dev), int(d))
    eng = _engines.get(key)
    if eng is None or eng.max_batch < max_batch:
        eng_new = HipEngine(dev, d, max(max_batch, eng.max_batch if eng else 0))
        if eng is not None:   # keep optimiser state and adopted thetas across a scratch resize
            for k in ("_flat", "mf_state", "mf_step", "tr_state", "tr_step", "grad_hook"):
                setattr(eng_new, k, getattr(eng, k))
            if hasattr(eng, "_mf_lr"):
                eng_new._mf_lr = eng._mf_lr
        _engines[key] = eng = eng_new
    return eng
