/*
 * sml_hip.h -- C ABI of libsml_hip.so, the MI355X (gfx950) implementation of the
 * SML per-period retraining hot path.
 *
 * The reference (zyang1580/SML) has no FFI: the path sits behind a Python module
 * surface.  Each entry point below names the reference code it replaces
 * (paths relative to the reference checkout).  The Python host side
 * (sml_amd/engine.py) binds these with ctypes; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative SML_E* code and never
 *     throws; sml_last_error() returns a thread-local message for the last failure;
 *   - every device buffer is a caller-owned raw device pointer (e.g. a torch
 *     tensor's data_ptr()); the library never frees or retains it past the call;
 *   - every launch goes to the caller's hipStream_t (passed as void*), is
 *     asynchronous and performs no hidden synchronisation, except where noted;
 *   - scratch lives in an opaque sml_ctx; scalars (losses) are written to device
 *     memory supplied by the caller;
 *   - tables are row-major fp32 [rows, d]; d in {32, 64, 128}; indices are int64
 *     exactly as the reference's DataLoader yields them (model/transfer.py:466-468);
 *   - theta (the transfer net) is ONE flat fp32 buffer holding the user net then the
 *     item net, each laid out as sml_theta_offset() reports (16-byte aligned tensors
 *     in the reference's state_dict order: conv1.weight, conv1.bias, conv2.weight,
 *     conv2.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias; model/conv_transfer.py:23-34).
 */
#ifndef SML_HIP_H
#define SML_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SML_OK 0
#define SML_EINVAL (-1)   /* bad argument (unsupported d, null pointer, size mismatch) */
#define SML_EHIP (-2)     /* a HIP runtime call failed; see sml_last_error() */
#define SML_ENOMEM (-3)
#define SML_ESTATE (-4)   /* call sequence error (e.g. packed weights stale) */

/* loss selection: ConvTransfer_com.run_MF(BCE=True) is the reference default
 * (model/conv_transfer.py:113-126); BPR is its BCE=False branch (:128-134) */
#define SML_LOSS_BCE 0
#define SML_LOSS_BPR 1
#define SML_LOSS_BPR_NORM 2   /* BPR with score / ||u'|| (norm=True, :130-132) */
#define SML_LOSS_BPR_UNIT 3   /* ConvTransfer.run_MF (:71-85): BPR over u' / ||u'||.detach() */

typedef struct sml_ctx sml_ctx;

const char* sml_last_error(void);
int sml_version(void);

/* ---- context ------------------------------------------------------------------ */
/* Scratch for batches of up to max_batch triples at width d on `device`. */
int sml_ctx_create(sml_ctx** out, int device, int d, int max_batch);
int sml_ctx_destroy(sml_ctx* ctx);
/* Which of the reference's two convolutional transfers the following calls run
 * (model/transfer.py:377-382, --transfer_type):
 *   0  ConvTransfer_com (conv_com, the default; model/conv_transfer.py:87-135)
 *   1  ConvTransfer     (conv; :52-85): conv1 kernel (2,1) over (x_t, x_hat) -- theta keeps the [10][3]
 *      conv1 block with a zero third column -- no x_com row, user-net output divided by its detached norm
 *      (sml_transfer_forward with net 0 returns the normalised rows), loss SML_LOSS_BPR_UNIT -- or SML_LOSS_BPR_NORM for
 *      ConvTransfer.run_MF(norm=True), model/conv_transfer.py:79-81: the same value, the norm differentiated through.
 * + 2 (variant 2 / 3): the context is an EVALUATION-STREAM context -- a second context whose sml_transfer_forward calls over
 *      whole tables run beside the training context's on another stream (forwards that only an evaluation reads); nothing
 *      changes in what they compute, but those launches carry a kernel name (k_side_transfer_fwd) and a timing class of
 *      their own, so that traces and sml_prof_get tell them from the training stream's. */
int sml_ctx_set_variant(sml_ctx* ctx, int variant);
/* --clip_grad (reference model/transfer.py:725-727, torch.nn.utils.clip_grad_norm_(transfer.parameters(), max_norm, 2)
 * between backward and optimizer.step() in the TR loop): max_norm > 0 makes the TR stage epoch finish the flat theta
 * gradient (after the exchange on several GPUs; on the one-shot peer exchange the rank-order sum of the inbox slots is
 * materialised first), take its 2-norm and scale it by min(1, max_norm / (norm + 1e-6)) before Adam; the step then runs
 * un-fused (one reduction launch + one Adam launch more per batch).  0 switches it off. */
int sml_ctx_set_grad_clip(sml_ctx* ctx, float max_norm);
/* --need_adaptive (reference model/transfer.py:490-499, beta = 0.1 there): the MF stage's loss gains
 * sum over the batch's unique users of beta * count_u / ||w_u|| (detached) * ||w_u||^2; beta > 0 adds it (one small launch per
 * batch between the backward and the row update), 0 switches it off. */
int sml_ctx_set_adaptive(sml_ctx* ctx, float beta);

/* ---- theta layout ------------------------------------------------------------- */
/* Floats in one net's flat block / offset of tensor `which` (0..7 in state_dict
 * order) inside it.  The full theta buffer is 2 * sml_theta_net_size(d) floats. */
int64_t sml_theta_net_size(int d);
int64_t sml_theta_offset(int d, int which);
/* Rebuild the MFMA operand images of fc1/fc2 after theta was written by the host
 * (construction, load_state_dict).  The TR-stage Adam keeps them current itself. */
int sml_theta_pack(sml_ctx* ctx, const float* theta, void* stream);

/* ---- native RCCL exchange (multi-GPU) ------------------------------------------------ */
/* The library can issue the two exchange collectives itself, on the compute stream: no host
 * callback per batch.  It binds the RCCL that is ALREADY loaded in the process (the host passes
 * the path of that librccl.so; no link-time dependency), creates its own communicator from a
 * 128-byte unique id the host broadcasts (rank 0: sml_comm_unique_id), and then
 *   - sml_tr_stage_epoch with grad_hook == NULL all-reduces the flat theta gradient,
 *   - sml_mf_stage_epoch with xchg->hook == NULL all-gathers the item-gradient rows.
 * sml_comm_allreduce / sml_comm_allgather are exported for the host's start-up self-check. */
int sml_comm_load(const char* librccl_path);
int sml_comm_unique_id(void* out128);
int sml_comm_init(sml_ctx* ctx, int world, int rank, const void* id128);
int sml_comm_destroy(sml_ctx* ctx);
int sml_comm_allreduce(sml_ctx* ctx, float* buf, int64_t n, void* stream);
int sml_comm_allgather(sml_ctx* ctx, const float* src, float* dst, int64_t n_per_rank, void* stream);

/* ---- one-shot exchange over peer mappings (multi-GPU; no collective library on the data path) --------------
 * The reference is single-device (main_yelp.py:125, .cuda() throughout model/transfer.py:317-385): this wraps its
 * per-batch loops (theta-gradient of a 256-triple batch, model/transfer.py:701-728; item-gradient rows of a
 * 1,024-triple batch, :463-511) for one process per GPU.  At these sizes (0.79 MB of theta gradient, 262 KB of rows
 * per rank, every 26-42 us) a collective library's launch + protocol floor is longer than the step it sits in; with
 * 7 direct xGMI links per GPU every rank can instead WRITE its contribution straight into every peer's memory:
 *
 *   regions   every rank provides an `inbox` (theta slots [2 parities][world][G floats], then row slots
 *             [2 parities][world][rows_cap][d]) and a `flags` region (arrival counters), sized by
 *             sml_peer_region_bytes, allocated with sml_peer_alloc (uncached / fine-grained device memory: remote
 *             stores land in it without the owner's L2 holding stale lines) and ZEROED there.
 *   mapping   sml_peer_attach takes RAW POINTERS: inbox[q] / flags[q] = rank q's regions as addressable from this
 *             device.  One process per GPU: export with sml_peer_export (hipIpcGetMemHandle; dmabuf IPC:
 *             HSA_ENABLE_IPC_MODE_LEGACY=0), all-gather the 64-byte handles by any means, sml_peer_open them
 *             (hipIpcOpenMemHandle).  Several ranks inside one process (tests on one GPU): pass the allocations.
 *   push      TR stage: the epilogue of k_tr_wgrad2's tile workgroups stores every finished gradient tile into slot [step & 1][rank]
 *             of EVERY rank's inbox (system-scope write-through stores), then one system-scope counter increment
 *             per workgroup and destination.  MF stage / bare step: a copy kernel pushes the rank's item-gradient
 *             rows the same way.
 *   poll+sum  the consumer (theta Adam / the row update) polls its OWN counters for the step's value, then adds the
 *             world slots IN RANK ORDER: every rank forms bit-identical sums, replicas stay bit-identical without
 *             a broadcast.  Two parities are enough: a rank pushes step b+2 only after consuming step b+1, which
 *             needed every peer's b+1 push, issued after that peer consumed step b.
 *   errors    a consumer that is not released within the time-out (sml_peer_attach) counts an incident and goes
 *             on with what it has: sml_peer_status reports the count (synchronous).
 * With peers attached, sml_tr_stage_epoch (grad_hook == NULL) and sml_mf_stage_epoch / sml_embed_loss_sgd_epoch
 * (exchange hook == NULL) use this path instead of the RCCL communicator. */
#define SML_MAX_PEERS 8
int sml_peer_region_bytes(sml_ctx* ctx, int world, int64_t rows_cap, int64_t* inbox_bytes, int64_t* flags_bytes);
int sml_peer_alloc(int device, int64_t bytes, void** ptr);      /* zeroed; synchronous */
int sml_peer_free(int device, void* ptr);
/* What sml_peer_alloc got for `ptr`: 0 uncached, 1 fine-grained, 2 plain (coarse-grained) device memory, -1 not one of its
 * allocations.  Inboxes and flags that other DEVICES write must not be plain: sml_amd.dist refuses that combination. */
int sml_peer_mem_kind(void* ptr);
/* dst <- src (bytes, a multiple of 16; both 16-byte aligned) through system-scope loads that bypass this device's caches:
 * how a rank reads memory another device rewrites (an item shard of sml_embed_loss_sgd_epoch_sharded).  The start-up
 * visibility check of sml_amd.dist uses it on a probe allocation of the same kind as the shards. */
int sml_peer_read(int device, const void* src, void* dst, int64_t bytes, void* stream);
int sml_peer_export(void* ptr, void* handle64);
int sml_peer_open(int device, const void* handle64, void** ptr);
int sml_peer_close(int device, void* ptr);
int sml_peer_attach(sml_ctx* ctx, int world, int rank, void* const* inbox, void* const* flags, int64_t rows_cap,
                    double timeout_s);
int sml_peer_detach(sml_ctx* ctx);
int sml_peer_status(sml_ctx* ctx, int* timeouts);
/* start-up self-check: every rank pushes n floats of `src` into all inboxes' theta slots and reads back the rank-order
 * sum of all ranks' pushes into dst (device, n floats; n <= 2 * sml_theta_net_size).  Consumes one theta exchange step:
 * every rank must call it the same number of times.  timeout_s > 0 replaces the attach-time hang guard for this call. */
int sml_peer_allreduce_check(sml_ctx* ctx, const float* src, float* dst, int64_t n, double timeout_s, void* stream);

/* ---- a5/a6/a10: transfer net forward ------------------------------------------- */
/* ConvTransfer_com.forward (model/conv_transfer.py:92-110) for `net` (0 = user
 * transfer, 1 = item transfer): out[n,:] = net(x_t[n,:], x_hat[n,:]).  Rows are
 * contiguous; out may alias neither input.  Used for meta_train.updata
 * (model/transfer.py:884-902) over whole tables. */
int sml_transfer_forward(sml_ctx* ctx, const float* theta, int net, const float* x_t,
                         const float* x_hat, float* out, int64_t n_rows, void* stream);

/* ---- a8: MF stage (meta_train.MF_train_onestage inner loop, model/transfer.py:463-511) */
typedef struct {
    float* w_user;         /* MFbase.user_laten.weight [U,d] (trainable W_hat) */
    float* w_item;         /* MFbase.item_laten.weight [I,d] */
    const float* last_user;/* last_user_weight  W_{t-1} [U,d] */
    const float* last_item;/* last_item_weight  W_{t-1} [I,d] */
    float* m_user; float* v_user;   /* Adam exp_avg / exp_avg_sq, same shape as the tables */
    float* m_item; float* v_item;
    int32_t* step_user;    /* [U] last Adam step applied to each row (lazy replay); -1 = never touched (m = v = 0) */
    int32_t* step_item;    /* [I] */
    int64_t n_user, n_item;
} sml_mf_tables;

/* Multi-GPU exchange of the MF stage (NULL on one GPU).  Users are row-sharded: a rank only
 * sees triples of users it owns, so user rows never leave the rank.  Item tables are
 * replicated; every batch, after the backward pass has been queued on `stream`, `hook` is
 * called on the host to all-gather each rank's per-occurrence item-gradient rows
 * (dx_local[item_off .. item_off + 2*batch) -> dx_items_all[world][2*batch][d]); the item
 * update then runs over the GLOBAL occurrence list (key_items/val_items: every batch's
 * world*2*B_b occurrences as (batch << 32 | item row), sorted by the caller or -- lists_unsorted -- by the library,
 * value = slot in dx_items_all),
 * so all replicas apply the identical summed update.  loss_scale = B_local / B_global.
 * hook == NULL: the library's own RCCL communicator (sml_comm_init) does the all-gather. */
typedef int (*sml_mf_hook)(void* user, int64_t batch_index);
typedef struct {
    int world;
    const uint64_t* key_items;
    const uint32_t* val_items;
    float* dx_local;        /* caller-owned scratch, >= (3*batch + 64 + slot_stride) * d floats */
    float* dx_items_all;    /* caller-owned, world * slot_stride * d floats */
    sml_mf_hook hook;
    void* hook_user;
    float loss_scale;       /* used when no batch plan gives per-batch scales */
    int64_t slot_stride;    /* rows every rank contributes per batch to dx_items_all (0: 2*batch) */
    const int64_t* item_off;/* host [n_batches+1]: batch b's global item occurrences are key/val_items[item_off[b] .. item_off[b+1])
                               (NULL: world*2*batch per full batch, the uniform layout) */
    int64_t push_rows;      /* peer path only (sml_peer_attach, hook == NULL): rows a rank actually pushes per batch, the same
                               on every rank, 2*batch <= push_rows <= slot_stride (0: slot_stride).  There slot_stride must
                               equal the inboxes' rows_cap: the gathered buffer IS one parity of this rank's row slots, and
                               dx_items_all is not used. */
    int lists_unsorted;     /* 1: key_items / val_items are batch-major (batch b's occurrences at item_off[b] .. / the uniform layout) but
                               NOT sorted inside a batch: the library builds every batch's run list itself (index_prep.hip: stable, i.e.
                               a row's occurrences keep the caller's order -- the same on every rank).  0: sorted (stably) by the caller. */
} sml_mf_exchange;

/* Batches of unequal size.  A global batch split over ranks by user owner leaves every rank a DIFFERENT number of
 * triples per batch (possibly none).  With a plan, `triples` holds the rank's batches back to back, batch b =
 * rows [batch_off[b], batch_off[b+1]), each at most `batch` long (the size the scratch was made for), and
 * loss_scale[b] multiplies batch b's loss and gradients (B_local/B_global for the mean-type BCE, 1 for the
 * sum-type BPR kinds).  An empty batch still takes part in the exchange and in the optimiser step.
 * NULL plan: consecutive batches of `batch` triples, the last one ragged. */
typedef struct {
    int64_t n_batches;
    const int64_t* batch_off;       /* host [n_batches + 1] */
    const int32_t* batch_off_dev;   /* the same offsets as int32 on the device (the index preparation reads them there) */
    const float* loss_scale;        /* host [n_batches], or NULL for the call's scalar */
} sml_batch_plan;

/* One epoch over n pre-drawn triples (u,i,j) int64 [n,3], in batches of `batch`:
 * 6 gathers -> run_MF -> + l2*0.5*sum(x_hat^2) -> backward to the W_hat rows ->
 * Adam(lr, betas 0.9/0.999, eps 1e-8, wd 0) with the DENSE semantics of
 * torch.optim.Adam reproduced lazily per row (rows not in a batch still take their
 * zero-gradient steps; they are replayed when the row is next touched or flushed).
 * *step is the optimiser's global step counter (in: steps done; out: + n_batches).
 * batch_loss[n_batches] (device) receives each batch's loss as the reference's
 * loss_batch (model/transfer.py:488).  Asynchronous. */
int sml_mf_stage_epoch(sml_ctx* ctx, const float* theta, const sml_mf_tables* t,
                       const int64_t* triples, int64_t n, int batch, float lr, float l2,
                       int loss_kind, int64_t* step, float* batch_loss, const sml_mf_exchange* xchg,
                       const sml_batch_plan* plan, void* stream);
/* Replay every pending zero-gradient Adam step so the tables can be read out
 * (before save_MF_weight / updata / evaluation; model/transfer.py:518, 777, 832). */
int sml_mf_adam_flush(sml_ctx* ctx, const sml_mf_tables* t, float lr, int64_t step, void* stream);

/* ---- a9: TR stage (meta_train.transfer_train_onestage inner loop, model/transfer.py:701-728) */
typedef struct {
    const float* last_user; const float* last_item;   /* W_{t-1} */
    const float* hat_user;  const float* hat_item;    /* user_weight_hat / item_weight_hat */
    int64_t n_user, n_item;
} sml_tr_tables;

/* One epoch: per batch, run_MF(norm=False) forward, backward to theta, then
 * Adam(lr, weight_decay added to the gradient) on theta (and m, v: flat buffers of
 * the same layout).  theta_grad (2*net_size floats) receives each batch's flat
 * gradient; NULL: internal scratch on the exchange paths, and NOT WRITTEN AT ALL by the
 * single-GPU step (Adam is fused into the weight-gradient kernel there and nothing
 * reads the gradient).  With grad_hook == NULL the whole
 * epoch is queued asynchronously.  A non-NULL grad_hook is called on the host after
 * each batch's backward has been queued on `stream` and before its Adam step is
 * queued, with the flat theta-gradient buffer: the multi-GPU path all-reduces it
 * there (on the same stream).  loss_scale multiplies loss and gradients
 * (B_local / B_global when a global batch is split over ranks; 1 otherwise). */
typedef int (*sml_grad_hook)(void* user, float* grad, int64_t n_floats, int64_t batch_index);
int sml_tr_stage_epoch(sml_ctx* ctx, float* theta, float* adam_m, float* adam_v, float* theta_grad,
                       const sml_tr_tables* t, const int64_t* triples, int64_t n, int batch,
                       float lr, float weight_decay, int loss_kind, float loss_scale,
                       int64_t* step, float* batch_loss, sml_grad_hook grad_hook, void* hook_user,
                       const sml_batch_plan* plan, void* stream);

/* ---- a7 with gradients: ConvTransfer_com.run_MF for a caller that backpropagates it itself ------------------------
 * (reference model/conv_transfer.py:113-135 as called from model/transfer.py:476-502 and :714-723: the caller does
 * zero_grad -> run_MF -> loss.backward() -> optimizer.step()).  One batch of B triples given as ROW BLOCKS, not tables:
 * user_last / user_hat [B,d]; item_last / item_hat [2B,d] = the positives' rows then the negatives' rows.  Writes the
 * loss (device scalar), d loss / d user_hat [B,d], d loss / d item_hat [2B,d] (gradient reaches x_hat through the
 * stack's second row only: x_com is built from a detached x_hat, :93-99) and the flat theta gradient
 * (2 * sml_theta_net_size floats, theta layout); any of the three gradient outputs may be NULL.  No optimiser step, no
 * l2 term: the caller adds what its loop adds.  B <= the context's max_batch.  Asynchronous. */
int sml_run_mf_grad(sml_ctx* ctx, const float* theta, const float* user_last, const float* user_hat,
                    const float* item_last, const float* item_hat, int B, int loss_kind, float* loss,
                    float* d_user_hat, float* d_item_hat, float* theta_grad, void* stream);

/* ---- a3: bare fused embed + loss + SGD write-back ------------------------------ */
/* gather 3 rows, 2 dot products, BCE (model/baseline.py:188-201) or BPR
 * (model/MF.py:139-144 without biases) loss, gradients, and synchronous minibatch
 * SGD: W -= lr * dL/dW with duplicate rows' gradients summed before the write.
 * dtype_bytes: 4 (fp32 tables) or 2 (fp16 tables, fp32 arithmetic).
 * batch_loss[n_batches] as above.
 * prepared_slot: -1 builds the epoch's index lists (per batch: a stable partition of the occurrences
 * by low row bits, every bucket sorted in LDS -- packed 4-byte entries when n_user / n_item and the
 * batch size allow -- unique marks, compacted run records of the duplicated rows; index_prep.hip)
 * inline on `stream`; 0/1 uses the lists a previous
 * sml_embed_loss_sgd_prepare call built for the SAME triples/n/batch -- so a caller can
 * prepare epoch e+1 on a side stream while epoch e runs.  No host wait either way: the call QUERIES whether
 * the lists it uses are complete; if they are (prepared ahead) and hold no hot run, the hot-row kernels are
 * skipped; if they are still in flight the hot-row kernels are launched and find their lists empty on the device.
 * (The caller orders `stream` behind the preparation stream, as for any two streams.) */
/* Several GPUs (NULL on one): users are row-sharded -- w_user holds this rank's rows, `triples` its users' triples
 * (local user index), every rank brings the SAME n and batch -- and the item table is replicated.  The ranks'
 * global batch b is the union of their local batches b.  Item rows are then never updated in place: every item
 * occurrence emits its gradient row, the ranks all-gather those rows after the gradient pass (dx[B .. B + 2*batch)
 * -> dx_items_all[world][2*batch][d]; `hook` on the host, or the library's own communicator when hook == NULL),
 * and every rank applies the identical update over the job's global item-occurrence list, which the index
 * preparation builds from `items_all` (the item columns of every rank's triples, gathered once per epoch by the
 * caller): replicas stay bit-identical, the step is the synchronous SGD step of the global batch.  BCE's mean is
 * over the global batch: loss_scale = B_local / B_global (1 for BPR). */
typedef struct {
    int world;
    const int64_t* items_all;   /* device [world][n][2]: (positive, negative) of every rank's triples, rank-major */
    float* dx_local;            /* caller-owned, 3*batch * d floats: this rank's per-occurrence gradient rows (what a host-side
                                   hook gathers from) */
    float* dx_items_all;        /* caller-owned, world * 2*batch * d floats */
    sml_mf_hook hook;
    void* hook_user;
    float loss_scale;
} sml_bare_exchange;

int sml_embed_loss_sgd_prepare(sml_ctx* ctx, const int64_t* triples, int64_t n, int batch,
                               int64_t n_user, int64_t n_item, int slot, const sml_bare_exchange* xchg, void* stream);
/* Test hook: copies one of the prepared lists of `slot` to the host (blocking; the caller has synchronised the
 * preparation stream).  which: 0/1 run records of users/items (8 x uint32: row, pos, len, pad, slot[4]), 2/3 first run
 * of each batch, 4/5 runs per batch (-1 per batch when the lists carry nb+1 offsets instead), 6/7 sorted values,
 * 8 unique marks, 9 hot lists, 10 hot counts, 11 (max run length, hot_cap).  Returns the bytes copied (<= bytes), < 0 on error. */
int64_t sml_index_lists_read(sml_ctx* ctx, int slot, int which, void* host, int64_t bytes);
int sml_embed_loss_sgd_epoch(sml_ctx* ctx, void* w_user, void* w_item, int64_t n_user,
                             int64_t n_item, int dtype_bytes, const int64_t* triples, int64_t n,
                             int batch, float lr, float lam_user, float lam_item, int loss_kind,
                             float* batch_loss, int prepared_slot, const sml_bare_exchange* xchg, void* stream);

/* The bare step with the ITEM TABLE SHARDED over the ranks (configs 4 / 5: 10M x 1M and 50M x 5M over 8 GPUs), on the
 * one-shot peer exchange (sml_peer_attach; rows_cap >= 2*batch, head_rows * d <= 2 * sml_theta_net_size(d)).
 * Replicating the items makes the step exchange-bound by a factor of ten (every rank would receive every rank's
 * 2*batch gradient rows); here
 *   - the head rows [0, head_rows) -- the popular items of a Zipf catalogue, whose occurrences would otherwise all
 *     land on one owner -- are replicated (w_item_head): every rank sums its OWN occurrences' gradient rows into a
 *     dense [head_rows, d] partial, the partials are all-reduced one-shot (pushed into every rank's inbox, added in
 *     rank order) and every replica applies the identical update;
 *   - a tail row r >= head_rows lives on rank (r - head_rows) / shard_rows only (item_shard[q]: every rank's shard
 *     as addressable from this device): the gradient pass READS it from its owner over the peer mapping and STORES
 *     the occurrence's gradient row straight into the owner's inbox; the owner adds the rows of all ranks in a fixed
 *     order (job-wide occurrence list built from items_all) and writes its shard -- owner-computes, an all-to-all whose
 *     volume per rank does not grow with the world size.
 * Users are row-sharded as for the sml_bare_exchange path: w_user, triples with local user indices, the same n and batch on
 * every rank).  Per batch two counter rounds order the ranks: "all gradient rows of batch b have landed" before an
 * owner updates, "every owner has updated" before anybody reads rows for batch b + 1.  Exact synchronous SGD of the
 * GLOBAL batch; replicas of the head stay bit-identical.  dx scratch and index lists live in the context. */
typedef struct {
    int world, rank;
    int64_t head_rows, shard_rows;
    void* const* item_shard;    /* host array [world] of device pointers: rank q's tail shard [shard_rows, d] */
    void* w_item_head;          /* [head_rows, d] (NULL when head_rows == 0) */
    const int64_t* items_all;   /* device [world][n][2], as in sml_bare_exchange */
    float loss_scale;
} sml_bare_shard;
int sml_embed_loss_sgd_epoch_sharded(sml_ctx* ctx, void* w_user, int64_t n_user, int64_t n_item, int dtype_bytes,
                                     const int64_t* triples, int64_t n, int batch, float lr, float lam_user, float lam_item,
                                     int loss_kind, float* batch_loss, const sml_bare_shard* sh, void* stream);

/* The same step as the reference's baselines run it (model/baseline.py:188-201 in base_train, :343-361 in
 * run_one_stage2: fine-tune / full-retrain MF): BCE + L2 loss and torch.optim.Adam(lr, wd 0) over the DENSE
 * tables, reproduced lazily per row exactly as in sml_mf_stage_epoch (same sml_mf_tables; last_* are not
 * read).  Flush with sml_mf_adam_flush before the tables are read out.  fp32 tables. */
int sml_embed_loss_adam_epoch(sml_ctx* ctx, const sml_mf_tables* t, const int64_t* triples, int64_t n,
                              int batch, float lr, float lam_user, float lam_item, int loss_kind,
                              int64_t* step, float* batch_loss, void* stream);

/* ---- a2: MFbasemode.forward (model/MF.py:34-43) --------------------------------- */
int sml_mf_forward(sml_ctx* ctx, const float* w_user, const float* w_item, const int64_t* user,
                   const int64_t* item, int64_t n, int norm, float* uemb, float* iemb, float* score,
                   void* stream);

/* ---- a13: evaluation (MFbasemode.test, model/MF.py:45-80) ------------------------ */
/* rows int64 [n, n_cols]: col 0 user, col 1 the positive, cols 2.. negatives.
 * rank[r] = #{candidates scoring strictly above the positive} (= the position
 * torch.topk assigns it for tie-free scores). */
int sml_eval_ranks(sml_ctx* ctx, const float* w_user, const float* w_item, const int64_t* rows,
                   int64_t n, int n_cols, int32_t* rank, void* stream);
/* L2-blocked form for test sets that are evaluated repeatedly (the validation rows of a period):
 * sml_eval_prepare groups each row's candidates by item range ONCE into rows_b int32 [n, n_cols]
 * (half the index bytes of the int64 input; n_item < 2^31) and bucket_off int32 [n, 9];
 * sml_eval_ranks_blocked then yields the same ranks as sml_eval_ranks with every XCD gathering from
 * its own eighth of the item table.  max_workgroups > 0 caps the (persistent) grid: an evaluation
 * queued on a side stream underneath training kernels leaves them most of each CU's wave slots. */
int sml_eval_prepare(sml_ctx* ctx, const int64_t* rows, int64_t n, int n_cols, int64_t n_item,
                     int32_t* rows_b, int32_t* bucket_off, void* stream);
int sml_eval_ranks_blocked(sml_ctx* ctx, const float* w_user, const float* w_item, const int32_t* rows_b,
                           const int32_t* bucket_off, int64_t n, int n_cols, int32_t* rank,
                           int max_workgroups, void* stream);
/* LDS-sliced form (d = 32, n_item <= 2^20, at most 32767 candidates per row, fewer than 2^31 entries in all): the
 * candidates are re-ordered ONCE per test set slice-major (slice = 1,024 consecutive item rows, staged in LDS; inside a
 * slice by mini-block of 64 test rows, then by test row, every (row, slice) unit padded to an even count), and the rank pass
 * reads item rows from LDS instead of gathering them through L1 -- same ranks as sml_eval_ranks (same rounding of every
 * score), bit for bit.
 *   sml_eval_sliced_slices        number of slices, 0 when the shape is outside the range above (use the forms above)
 *   sml_eval_sliced_entries       uint32 words of `entries` (candidates + padding, an upper bound)
 *   sml_eval_sliced_work_ints     int32 words of `work` the preparation needs (contents not needed afterwards)
 *   sml_eval_sliced_scratch_bytes bytes of `scratch` one rank pass needs (contents not needed afterwards; 16-byte aligned)
 *   sml_eval_prepare_sliced       entries uint32 [sml_eval_sliced_entries], seg_off int32 [slices * ceil(n / 64) + 1]
 *   sml_eval_ranks_sliced         rows is the ORIGINAL int64 table (user and positive columns are read from it);
 *                                 max_workgroups > 0: grid size wanted (one workgroup occupies a whole CU's LDS). */
int sml_eval_sliced_slices(sml_ctx* ctx, int64_t n, int n_cols, int64_t n_item);
int64_t sml_eval_sliced_entries(sml_ctx* ctx, int64_t n, int n_cols, int64_t n_item);
int64_t sml_eval_sliced_work_ints(sml_ctx* ctx, int64_t n, int n_cols, int64_t n_item);
int64_t sml_eval_sliced_scratch_bytes(sml_ctx* ctx, int64_t n, int n_cols, int64_t n_item);
int sml_eval_prepare_sliced(sml_ctx* ctx, const int64_t* rows, int64_t n, int n_cols, int64_t n_item,
                            uint32_t* entries, int32_t* seg_off, int32_t* work, void* stream);
int sml_eval_ranks_sliced(sml_ctx* ctx, const float* w_user, const float* w_item, const int64_t* rows,
                          const uint32_t* entries, const int32_t* seg_off, int64_t n, int n_cols, int64_t n_item,
                          void* scratch, int32_t* rank, int max_workgroups, void* stream);
/* ---- a11: save_MF_weight (model/transfer.py:911-943) and evaluation snapshots ------- */
/* n <= 4 device-to-device copies (dst[q] <- src[q], bytes[q]; all multiples of 16) in one launch. */
int sml_copy_tables(int n, void* const* dst, const void* const* src, const int64_t* bytes, void* stream);

/* A HIP stream restricted to the compute units [cu_lo, cu_hi) of the device's CU mask (on MI355X mask bit i is a
 * CU of XCD i % 8, so a contiguous range takes the same number of CUs from every XCD: each range keeps all eight
 * L2s and an eighth of its CUs on each).  Evaluations queued on such a stream run beside the training kernels on
 * CUs of their own instead of sharing SIMDs and L2 ports with them.  The caller owns the stream. */
int sml_stream_create_cu_range(void** stream, int device, int cu_lo, int cu_hi);
int sml_stream_destroy(void* stream);
/* Orders `waiter` after everything queued on `signaler` so far, through a device-scope event (no system fence). */
int sml_stream_wait_stream(void* waiter, void* signaler);
/* The same ordering WITHOUT a cross-queue barrier packet: sml_flag_set (a one-thread kernel on the signalling stream,
 * after the work to be waited for) stores `value` into the device word flag[0]; sml_flag_wait (a kernel on the waiting
 * stream, before the dependent work) polls until flag[0] >= value.  `flag` points at TWO int32 words, both starting at
 * 0: flag[0] the sequence word (values must grow monotonically), flag[1] a counter of waiters that were not released
 * within timeout_s and gave up -- their dependent work then ran unordered.  The time-out is a hang guard (make it
 * long): it never touches the sequence word, so later waiters stay ordered; the host reads flag[1] when it collects
 * (or drops) results and treats a non-zero count as an error. */
int sml_flag_set(int32_t* flag, int value, void* stream);
int sml_flag_wait(int32_t* flag, int value, double timeout_s, void* stream);
/* hits = #{rank < topk}, ndcg = sum 1/log2(rank+2) over hits; out[0]=hits, out[1]=ndcg (device). */
int sml_eval_metrics(sml_ctx* ctx, const int32_t* rank, int64_t n, int topk, float* out, void* stream);

/* ---- full-catalogue retrieval ------------------------------------------------------ */
/* S(u, i) = <w_user[u], w_item[i]> in fp32 (no bias terms, as MFbasemode.test scores; the _adjusted entry points below
 * add per-item terms), one fmaf chain over the d
 * dims in a fixed order shared by both entry points: the two score every (u, i) to the same float, bit for bit.
 * The order pairs dim s with dim s + d/2: acc = 0; for s = 0 .. d/2 - 1 { acc = fmaf(x[s], u[s], acc);
 * acc = fmaf(x[s + d/2], u[s + d/2], acc); } with u = w_user[u], x = w_item[i], each fmaf rounded once (round to
 * nearest even, subnormals kept).
 * d (the ctx's) must be 32 or 64 for these fp32 entry points (the _f16 entry points below also take 128);
 * 0 < n_item < 2^31.  Seen(u), the items excluded for user u, is a CSR over users:
 * seen_off int64 [n_user + 1], seen_items int32 ascending and unique inside each user's range; both NULL = nothing
 * excluded, exactly one NULL is refused.  Exclusion is by item id, never by score.  Indices are trusted.
 *
 * sml_full_rank: rows int64 [n, n_cols >= 2] (col 0 user u, col 1 positive p, further columns ignored);
 *   rank[r] = #{i in [0, n_item): i != p, i not in Seen(u), S(u,i) > S(u,p)} -- strictly greater, IEEE (a NaN is never
 *   above, a NaN positive gets rank 0); p itself is never excluded.  The ranks feed sml_eval_metrics unchanged. */
int sml_full_rank(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item,
                  const int64_t* rows, int64_t n, int n_cols,
                  const int64_t* seen_off, const int32_t* seen_items, int32_t* rank, void* stream);
/* Bytes of `scratch` sml_topk_items needs for n users at this k (1 <= k <= 128) and n_item (16-byte aligned base;
 * contents not needed afterwards).  It grows linearly in n: callers with many users go in chunks.  < 0: bad argument. */
int64_t sml_topk_scratch_bytes(sml_ctx* ctx, int64_t n, int k, int64_t n_item);
/* sml_topk_items: for users int64 [n], items int32 [n, k] and scores float [n, k] = the k eligible items (not in
 * Seen(u), score not NaN) in order of score descending, then item id ascending; slots past the eligible count hold
 * item -1 and score -inf.  Deterministic (the same bytes whatever the schedule).  With the same Seen, the positive of
 * a row (u, p) sits at position rank + #{eligible i != p : S(u,i) == S(u,p), i < p} of u's list whenever that is < k. */
int sml_topk_items(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item,
                   const int64_t* users, int64_t n, int k,
                   const int64_t* seen_off, const int32_t* seen_items,
                   void* scratch, int32_t* items, float* scores, void* stream);
/* Per-user ranking of held-out sets (same S, d, n_item and Seen rules as above).  users int64 [n], n < 2^31 (a user may
 * appear more than once); pos_off int64 [n + 1] (pos_off[0] = 0, non-decreasing, pos_off[n] = n_pos < 2^31); pos_items int32
 * [n_pos]: T(x), the held-out items of users[x], ascending and unique inside [pos_off[x], pos_off[x + 1]) (may be empty).
 * (An item repeated inside a range is not refused: every copy gets that item's above / pos, and nothing is written
 * outside above / pos [n_pos].)
 * An item i is ELIGIBLE for u when i is not in Seen(u) and S(u, i) is not NaN.  For each held-out p of u:
 *   above[e] = #{eligible i != p : S(u,i) > S(u,p)} -- exactly sml_full_rank's rank of the row (u, p), NaN rule included;
 *   pos[e]   = #{eligible i : (S(u,i), i) before (S(u,p), p)} in the top-K order (score descending, then id ascending):
 *              p's index in u's sml_topk_items list; -1 when p itself is not eligible (in Seen(u) or scoring NaN).
 * pos is strictly increasing along a user's eligible held-out items taken in that order.  Integer counts: the same bytes
 * whatever the schedule.  The item table is read once per (32-user group, item slice); no score matrix is written.
 * sml_user_rank_scratch_bytes: bytes of `scratch` for n users and n_pos held-out items (16-byte aligned base; contents
 *   not needed afterwards), linear in n_pos.  < 0: bad argument. */
int64_t sml_user_rank_scratch_bytes(sml_ctx* ctx, int64_t n, int64_t n_pos, int64_t n_item);
int sml_user_rank(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item,
                  const int64_t* users, int64_t n, const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos,
                  const int64_t* seen_off, const int32_t* seen_items, void* scratch, int32_t* above, int32_t* pos,
                  void* stream);
/* The same three calls on HALF-PRECISION tables (IEEE binary16, row-major [rows, d], as sml_embed_loss_sgd_epoch trains
 * them with elem_bytes = 2): sml_full_rank_f16, sml_topk_items_f16, sml_user_rank_f16.  d (the ctx's) must be 32, 64 or
 * 128; fp32 tables at d = 128 stay refused by the entry points above.  Widening rule: every table entry is widened
 * EXACTLY to fp32 (each fp16 value -- subnormals, +-0, +-inf and NaN included -- is an fp32 value) and S(u, i) is the
 * fmaf chain defined above on the widened entries, accumulated in fp32: same dim order, each fmaf rounded once,
 * subnormals kept.  No fp32 copy of a table is made; rows are read as packed halves.  At d = 32 and d = 64 every output
 * equals, bit for bit, the output of the fp32 entry point on fp32 copies of the same tables; at d = 128 the same
 * definition holds.  Everything else carries over verbatim: Seen and its rules, the NaN rules, the (score descending,
 * id ascending) order, (-1, -inf) padding, rank / above / pos, 1 <= k <= 128, determinism, and the scratch sizes --
 * sml_topk_scratch_bytes and sml_user_rank_scratch_bytes serve both element types.  scores stay float32.
 * sml_user_metrics reads no table and serves both. */
int sml_full_rank_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item,
                      const int64_t* rows, int64_t n, int n_cols,
                      const int64_t* seen_off, const int32_t* seen_items, int32_t* rank, void* stream);
int sml_topk_items_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item,
                       const int64_t* users, int64_t n, int k,
                       const int64_t* seen_off, const int32_t* seen_items,
                       void* scratch, int32_t* items, float* scores, void* stream);
int sml_user_rank_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item,
                      const int64_t* users, int64_t n, const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos,
                      const int64_t* seen_off, const int32_t* seen_items, void* scratch, int32_t* above, int32_t* pos,
                      void* stream);
/* ITEM FILTER: the same six calls restricted to a subset of the catalogue, the same subset for every user.
 * allow uint32 [sml_item_filter_words(n_item) = ceil(n_item / 32)], device memory: bit (i & 31) of word (i >> 5) is set
 * exactly when item i may appear.  Bits at positions >= n_item of the last word are ignored, whatever they hold.
 * allow == NULL: no filter -- the call IS the unfiltered entry point (sml_full_rank is sml_full_rank_filtered with
 * allow = NULL, and so on).  An item is eligible when it is below n_item, not in Seen(u) and allowed (and, where the
 * unfiltered rule says so, scores no NaN).  Each _filtered entry point takes the argument list of its unfiltered form with
 * `allow` inserted after seen_items; each _f16 twin has the list of its fp32 form.  Scratch sizes do not depend on the
 * filter (sml_topk_scratch_bytes, sml_user_rank_scratch_bytes).
 * Defining identity: for any Seen and any filter A, every output of a filtered call -- rank; items, scores and their
 * (-1, -inf) padding; above, pos and, through sml_user_metrics, hits, dcg, ap and first -- equals byte for byte the output
 * of the unfiltered call with Seen'(u) = Seen(u) united with ([0, n_item) minus A) for every user.  In particular:
 *   sml_full_rank_filtered   rank[r] = #{allowed i != p, not in Seen(u), S(u,i) > S(u,p)}.  p itself is never excluded: a
 *                            positive that is not allowed still gets its rank among the allowed items.
 *   sml_topk_items_filtered  lists hold allowed items only; fewer than k eligible items leave (-1, -inf) padding, and a
 *                            filter that allows nothing leaves nothing else.
 *   sml_user_rank_filtered   a held-out p that is not allowed is treated exactly like one in Seen(u): pos = -1, above =
 *                            #{eligible i : S(u,i) > S(u,p)}, and p is no eligible item for the user's other entries.
 *                            With nothing allowed every pos is -1 and every above 0.
 * The fp16 statements above carry over: at d = 32 / 64 a filtered _f16 call equals the filtered fp32 call on fp32 copies
 * of the tables bit for bit; d = 128 exists for fp16 tables only.
 * Cost: a 32-item tile of the walk whose word allows no item below n_item is skipped by the whole wave (its item rows are
 * not read and not scored), so a call costs what its non-empty tiles cost. */
int sml_full_rank_filtered(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item,
                           const int64_t* rows, int64_t n, int n_cols,
                           const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, int32_t* rank, void* stream);
int sml_topk_items_filtered(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item,
                            const int64_t* users, int64_t n, int k,
                            const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow,
                            void* scratch, int32_t* items, float* scores, void* stream);
int sml_user_rank_filtered(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item,
                           const int64_t* users, int64_t n, const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos,
                           const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, void* scratch, int32_t* above,
                           int32_t* pos, void* stream);
int sml_full_rank_filtered_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item,
                               const int64_t* rows, int64_t n, int n_cols,
                               const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, int32_t* rank, void* stream);
int sml_topk_items_filtered_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item,
                                const int64_t* users, int64_t n, int k,
                                const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow,
                                void* scratch, int32_t* items, float* scores, void* stream);
int sml_user_rank_filtered_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item,
                               const int64_t* users, int64_t n, const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos,
                               const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, void* scratch,
                               int32_t* above, int32_t* pos, void* stream);
/* Words of an item filter over n_item items: ceil(n_item / 32); < 0: bad argument (0 < n_item < 2^31). */
int64_t sml_item_filter_words(int64_t n_item);
/* Build a filter on the device: words [sml_item_filter_words(n_item)] allows exactly the items of ids int32 [n_ids]
 * (device memory; duplicates allowed, n_ids = 0 allowed) or, with invert = 1, every item of [0, n_item) EXCEPT them (a
 * deny-list).  The tail bits of the last word are written 0.  Bits are set with atomic OR / AND: the same words whatever
 * the order.  ids must lie in [0, n_item); on the device they are trusted like every other index (a host-side caller
 * checks them: HipEngine.item_filter_from_ids does). */
int sml_item_filter_from_ids(sml_ctx* ctx, const int32_t* ids, int64_t n_ids, int64_t n_item, int invert, uint32_t* words,
                             void* stream);
/* ADJUSTED SCORE: the three calls ranking by a per-item affine function of the score instead of the bare dot product,
 *
 *     A(u, i) = fmaf(S(u, i), scale[i], offset[i])
 *
 * computed in fp32 and rounded once: S is the fmaf chain defined above (fp16 tables widened exactly as above), and the
 * term is one more fused multiply-add on its rounded value.  scale and offset are fp32 per-item arrays for both table
 * element types.  offset = an item bias ranks by dot + bias (a per-user bias cannot reorder a user's list and is left
 * out); scale[i] = 1 / ||x_i|| ranks by the cosine.
 * Everything the three calls do with S they do with A:
 *   rank / above   strict > against the positive's own A(u, p);
 *   top-K order    A descending, then item id ascending; the returned scores are A;
 *   pos            eligible means not in Seen(u), allowed, and A not NaN.
 * The NaN rules are stated on A: a NaN is never above anything, a NaN positive ranks 0, a NaN item enters no list, and as
 * a held-out item it has pos -1.  scale and offset may hold any float: an offset of -inf sends an item to the end of every
 * list but keeps it eligible (it fills a list that has room, after every finite score, by id); a NaN term removes the item.
 * With scale == 1 and offset == +0 everywhere (scale ≡ 1, offset ≡ +0), A == S as values: only the sign bit of a -0 score
 * changes (fmaf(-0, 1, +0) = +0), every integer output equals the unadjusted call's byte for byte, and every score
 * compares equal.
 * Layout: adj float [2][n_pad], device memory, 16-byte aligned, n_pad = sml_item_adjust_len(n_item) = 32 * ceil(n_item / 32);
 * plane 0 (adj[0 .. n_pad)) is scale, plane 1 (adj[n_pad .. 2 n_pad)) is offset.  Pad entries are ignored, whatever they
 * hold (the walk loads whole 32-item tiles; the items past n_item are masked by id).
 * Each _adjusted entry point takes the argument list of its _filtered form with `elem_bytes` (4: fp32 tables, d = 32 / 64;
 * 2: fp16 tables, d = 32 / 64 / 128; any other pair is refused) inserted after w_item and `adj` after allow.  allow may be
 * NULL: no filter.  adj == NULL is refused, and so is an adj that is not 16-byte aligned (the unadjusted entry points are
 * the calls without terms).  One entry point per
 * operation serves both element types.  Seen, the item filter and its identity, (-1, -inf) padding, 1 <= k <= 128,
 * determinism and the scratch sizes carry over verbatim: sml_topk_scratch_bytes and sml_user_rank_scratch_bytes serve
 * these calls, and sml_user_metrics is unchanged.  At d = 32 / 64 an adjusted call on fp16 tables equals the call on fp32
 * copies of them bit for bit, with the same adj.  With the same Seen, filter and adj, the positive of a row (u, p) sits at
 * position rank + #{eligible i != p : A(u,i) == A(u,p), i < p} of u's adjusted list whenever that is < k.
 * Cost: four 16-byte loads per plane per lane and tile, the same for the 32 user lanes of a lane half (they are served by
 * one cache line each), requested with the next tile's item rows; a tile the filter skips loads none. */
/* n_pad, the floats of one plane of adj for n_item items; < 0: bad argument (0 < n_item < 2^31). */
int64_t sml_item_adjust_len(int64_t n_item);
/* Build adj [2][n_pad] on the device from optional device arrays scale and offset, float [n_item] each: NULL scale means
 * 1 everywhere, NULL offset means +0 everywhere.  The pad entries are written (1, 0). */
int sml_item_adjust_fill(sml_ctx* ctx, const float* scale, const float* offset, int64_t n_item, float* adj, void* stream);
/* Cosine: write plane 0 of adj (only; plane 1 is not touched, the pad entries of plane 0 are written 1) from an item table
 * [n_item, d] of elem_bytes 4 or 2: n2 = the score chain of row i with itself (x_i on both sides, same dim order, fp16
 * widened exactly), scale[i] = n2 > 0 ? 1.0f / sqrtf(n2) : 0.0f with correctly rounded sqrtf and division.  A zero row
 * therefore scores 0 against everything instead of NaN (a row whose n2 is NaN gets scale 0 too, one whose n2 is +inf gets
 * 1 / inf = 0). */
int sml_item_adjust_cosine(sml_ctx* ctx, const void* w_item, int elem_bytes, int64_t n_item, float* adj, void* stream);
int sml_full_rank_adjusted(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item,
                           const int64_t* rows, int64_t n, int n_cols,
                           const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                           int32_t* rank, void* stream);
int sml_topk_items_adjusted(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item,
                            const int64_t* users, int64_t n, int k,
                            const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                            void* scratch, int32_t* items, float* scores, void* stream);
int sml_user_rank_adjusted(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item,
                           const int64_t* users, int64_t n, const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos,
                           const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                           void* scratch, int32_t* above, int32_t* pos, void* stream);
/* PER-USER CANDIDATE LISTS: "order these candidates for this user" -- the top k of a list of item ids given per user, without
 * a walk of the catalogue.  Tables, elem_bytes (4: d = 32 / 64; 2: d = 32 / 64 / 128; any other pair is refused), Seen, allow
 * and adj are exactly those of sml_topk_items_adjusted, except that here adj == NULL is accepted and means the bare score S (no
 * fmaf is applied: the unadjusted scores' bits are returned), as allow == NULL means no filter.  1 <= k <= 128.  users int64
 * [n]; a user may repeat.  cand holds int32 or int64 entries, cand_elem_bytes = 4 or 8.  The list of users[x] is
 *   ragged form  cand[cand_off[x] .. cand_off[x + 1]), cand_off int64 [n + 1], non-decreasing, from 0;
 *   dense form   (cand_off == NULL) cand[x * cand_stride + cand_first .. + cand_cols): rows [user, positive, negatives] of a
 *                test file go in as they are with cand_stride = 2 + neg_num, cand_first = 1, cand_cols = 1 + neg_num.
 * A list may be empty and may hold any id more than once, in any order.
 * Padding rule: an entry c outside [0, n_item) is padding and is skipped -- negative ids are how a dense matrix carries short
 * lists, and ids at or above n_item never touch memory (no address is formed from them).
 * An entry c is ELIGIBLE when 0 <= c < n_item, c is not in Seen(u), c is allowed and A(u, c) is not NaN, where A is S (the
 * fmaf chain above, fp16 entries widened exactly) or, with adj, one explicit fmaf(S, scale[c], offset[c]).
 * items[x] / scores[x] (int32 / float [n, k]) hold the DISTINCT eligible ids of list x in the top-K order (A descending, then
 * id ascending), at most k of them, then (-1, -inf).
 * Repeat rule: a repeated id appears once (the same id always scores the same bits, so an entry equal in score and id to one
 * already listed is dropped).
 * n_elig[x] (int32 [n]; may be NULL) = the number of eligible entries of list x, repeats counted as they occur.
 * Defining identity: row x equals, byte for byte in items and scores, row 0 of sml_topk_items_adjusted for the single user
 * users[x] with the same Seen and adj and the filter (allow AND bitmap(list x)) -- with adj == NULL, of
 * sml_topk_items_filtered[_f16].
 * The bytes are the same for every launch geometry: max_workgroups = 0 leaves the grid to the call, a positive value caps it
 * (lists are walked grid-stride, one wavefront per list).  No scratch, no allocation, no copy to the host, no synchronise.
 * Refused (sml_last_error): exactly one of seen_off / seen_items NULL; a (d, elem_bytes) pair the kernels do not exist for;
 * cand_elem_bytes other than 4 / 8; negative dense geometry; k out of range; max_workgroups < 0; a misaligned adj or table;
 * an output that overlaps an input or another output as far as the pointers and the sizes known to the call show it.
 * n == 0 is a valid call that launches nothing.  Indices (users, cand_off) are trusted.
 * Known limit: one wavefront walks a whole list, however long; a single list of hundreds of thousands of candidates belongs
 * to sml_topk_items_filtered with an item filter. */
int sml_topk_candidates(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item,
                        const int64_t* users, int64_t n,
                        const void* cand, int cand_elem_bytes, const int64_t* cand_off,
                        int64_t cand_stride, int64_t cand_first, int64_t cand_cols,
                        int k, const int64_t* seen_off, const int32_t* seen_items,
                        const uint32_t* allow, const float* adj, int max_workgroups,
                        int32_t* items, float* scores, int32_t* n_elig, void* stream);
/* ---- CLUSTERED INDEX: an inverted-file (IVF) index over the item table -- k-means lists, and a query that scores only the
 * members of the lists nearest the user instead of the whole catalogue.  The approximation lives ONLY in which lists are
 * probed: everything the calls below return is an exact, byte-defined function of (tables, lists, probes).
 * An index over an item table [n_item, d] of element type T (fp32: d = 32 / 64; fp16: d = 32 / 64 / 128; any other pair is
 * refused) is three device arrays:
 *   centroids   T [n_list, d], in the table's own element type, so that sml_topk_items[_adjusted][_f16] takes it as an item
 *               table: "assign each item to its nearest centroid" and "choose each user's lists" are that call;
 *   list_off    int64 [n_list + 1], from 0, non-decreasing, ending at n_item;
 *   list_items  int32 [n_item], a partition of [0, n_item), ids ascending inside each list (what sml_iset_build writes for
 *               the rows (list, item)).
 * The index holds no rows and no scores: search reads the CURRENT w_item, so a stale index can cost recall but can never
 * return a wrong score.
 * SEARCH.  probes int32 [n, nprobe], 1 <= nprobe <= 128: the lists of users[x] are probes[x][0], probes[x][1], ...  A probe
 * outside [0, n_list) is padding and forms no address; a list probed twice is walked twice.  1 <= k <= 128.  Seen, allow, adj
 * (NULL accepted: the bare score, no fmaf), eligibility, the order, the (-1, -inf) padding, the repeat rule and n_elig ("the
 * number of eligible entries, repeats counted as they occur") are exactly those of sml_topk_candidates.
 * Defining identity: row x equals, byte for byte in items, scores and n_elig, row x of sml_topk_candidates with the ragged list
 * "the members of probes[x][0], then of probes[x][1], ...".  Hence, through that call's own identity, row x also equals
 * sml_topk_items_filtered for that user alone under the filter (allow AND bitmap(union of the probed lists)).  Consequences:
 *   - probing every list once returns the bytes of sml_topk_items[_filtered|_adjusted][_f16] on the same arguments;
 *   - at d = 32 / 64 a call on fp16 tables equals the call on fp32 copies of them bit for bit;
 *   - the bytes are the same for every max_workgroups (0 leaves the grid to the call, a positive value caps it; one wavefront
 *     serves one user, users are walked grid-stride).
 * No scratch, no allocation, no copy to the host, no synchronise.  Refused (sml_last_error): what sml_topk_candidates refuses
 * (exactly one of seen_off / seen_items NULL; a (d, elem_bytes) pair the kernels do not exist for; k out of range;
 * max_workgroups < 0; a misaligned adj or table; an output that overlaps an input or another output as far as the pointers and
 * the sizes known to the call show it), and nprobe outside [1, 128] and n_list <= 0.  n == 0 is a valid call that launches
 * nothing.  Indices (users, list_off, list_items) are trusted.
 * sml_host_ivf_search: the same definition as a single-threaded walk over HOST memory (the host and the device share the text
 * of the score chain); d is the caller's (no context), and nothing has to be aligned.
 * CENTROID UPDATE.  For list c with members m_0 < m_1 < ... (len of them) and every dim s:
 *   acc = 0.0 as a double; acc += (double)x[m_j][s] for j ascending (the widening is exact);
 *   out[c][s] = (T)(float)(acc / (double)len) -- the fp64 division correctly rounded, each conversion to nearest even.
 * An empty list copies centroids_in[c].  centroids_in and centroids_out may be the same pointer (any other overlap is refused).
 * The order of the additions is part of the definition, so the bytes do not depend on the launch; there are no floating-point
 * atomics.  sml_host_ivf_centroids: the host walk of the same text, compiled so that nothing is contracted or reassociated.
 * Refused: a (d, elem_bytes) pair outside the family, n_item outside (0, 2^31), n_list <= 0, a null pointer, an output that
 * overlaps the table or the lists.
 * BUILD (sml_amd.retrieval.ItemIndex; plumbing over existing calls).  Initialise: n_list distinct item rows chosen on the host
 * from a seed.  Per iteration -- assign: item i joins the list of its best centroid, by sml_topk_items[_adjusted] with the item
 * table as the user table and k = 1 (metric "dot": the centroid maximising S(x_i, centroid_c); "cosine", the default: the
 * adjusted score fmaf(S, 1 / ||centroid_c||, +0) through sml_item_adjust_cosine on the centroid table; ties go to the lower list
 * id; an item whose every centroid score is NaN joins list 0, so the lists stay a partition); lists: sml_iset_build on the rows
 * (assign[i], i); update: sml_ivf_centroids.  Probe at query time: sml_topk_items[_adjusted] of the users against the centroids
 * with k = nprobe and the same metric's table, narrowed to int32; Seen and item filters do not apply to centroids.  The same
 * seed, table and arguments give the same index bytes on every run.
 * Not measured: trained (non-random) SML tables, and recall across periods under a refreshed index. */
int sml_ivf_search(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item,
                   const int64_t* users, int64_t n,
                   const int64_t* list_off, const int32_t* list_items, int n_list,
                   const int32_t* probes, int nprobe, int k,
                   const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                   int max_workgroups, int32_t* items, float* scores, int32_t* n_elig, void* stream);
int sml_host_ivf_search(const void* w_user, const void* w_item, int elem_bytes, int d, int64_t n_item,
                        const int64_t* users, int64_t n,
                        const int64_t* list_off, const int32_t* list_items, int n_list,
                        const int32_t* probes, int nprobe, int k,
                        const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                        int32_t* items, float* scores, int32_t* n_elig);
int sml_ivf_centroids(sml_ctx* ctx, const void* w_item, int elem_bytes, int64_t n_item,
                      const int64_t* list_off, const int32_t* list_items, int n_list,
                      const void* centroids_in, void* centroids_out, void* stream);
int sml_host_ivf_centroids(const void* w_item, int elem_bytes, int d, int64_t n_item,
                           const int64_t* list_off, const int32_t* list_items, int n_list,
                           const void* centroids_in, void* centroids_out);
/* ---- FOLD-IN: the closed-form row of a user or an item the last training run did not see -- the iALS half-step.  The other
 * side's table Y [n_other, d] is held fixed and the row solves its regularised least-squares problem from its interaction set S:
 *   p = argmin_p  sum_{i in S} (1 - p.y_i)^2 + alpha0 sum_{all i} (p.y_i)^2 + reg |p|^2
 *     = (alpha0 Y^T Y + sum_{i in S} y_i y_i^T + reg I)^-1 sum_{i in S} y_i.
 * With the user table as Y and the item -> users CSR the same call folds in items; alternating the two is iALS.
 * All arithmetic is fp64 and every rounding is named below, so the bytes depend on no launch geometry; the host walks share
 * the text of the steps with the kernels, compiled so that nothing is contracted or reassociated: every fused step is an explicit
 * fma().  There are no floating-point atomics and no matrix instructions.
 * Tables: element type T and width d of the retrieval family without d = 128 -- fp32: d = 32 / 64; fp16: d = 32 / 64; any other
 * pair is refused.  d = 128 needs a different register / LDS plan (one lane cannot hold a row of the triangle) and is out of scope.
 * GRAM.  G = Y^T Y over rows [0, n_rows) of a table, in chunks of SML_GRAM_CHUNK = 1024 rows, a constant of the definition.  For
 * chunk c and every (a, b): part = 0.0; for the chunk's rows i ascending: part = part + (double)y[i][a] * (double)y[i][b] -- the
 * product of two widened fp32 / fp16 values is exact in fp64, so fused or not gives the same bits and only the add rounds.  Then
 * G[a][b] = 0.0 and G[a][b] += part_c for c ascending.  G is double [d][d]; both triangles are written and are equal bit for bit
 * (the product commutes exactly).  NaN / Inf propagate.  scratch: sml_gram_scratch_bytes = n_chunks * d * d * 8 bytes, the
 * partials; scratch and gram 16-byte aligned.
 * ROW SOLVE, for a row with members m_0 < m_1 < ... (its range of the set CSR, ids ascending, as sml_iset_build writes them).
 * Only the lower triangle a >= b is formed:
 *   A[a][b] = fma(alpha0, G[a][b], a == b ? reg : 0.0); for members ascending: A[a][b] = A[a][b] + (double)y[m][a] * (double)y[m][b];
 *   rhs[a] = 0.0; for members ascending: rhs[a] += (double)y[m][a].
 * LDL^T without square roots, for j = 0 .. d - 1:
 *   v[k] = L[j][k] * D[k] for k < j;  D[j] = A[j][j]; for k = 0 .. j - 1: D[j] = fma(-L[j][k], v[k], D[j]);
 *   if !(D[j] > 0) the row fails;
 *   for i > j: t = A[i][j]; for k ascending: t = fma(-L[i][k], v[k], t); L[i][j] = t / D[j], the correctly rounded fp64 division.
 * Forward: z[j] = rhs[j]; for k < j ascending: z[j] = fma(-L[j][k], z[k], z[j]); then w[j] = z[j] / D[j].
 * Backward, j = d - 1 .. 0: p[j] = w[j]; for k = j + 1 .. d - 1 ascending: p[j] = fma(-L[k][j], p[k], p[j]).
 * Output: out[row][s] = (T)(float)p[s], each conversion to nearest even.
 * STATUS, int32 per solved row (status[x] belongs to rows[x]):
 *   0  solved and written;
 *   1  empty set: the row is written as +0.0 in every dim (the exact solution); nothing is factored;
 *   2  a pivot was not > 0, or some p[s] is not finite (reg = alpha0 = 0 with a rank-deficient set, a NaN / Inf member row, a
 *      NaN Gram): the output row is left untouched.
 * rows int64 [n]: which rows of w_out to solve; rows[x] also indexes set_off.  rows == NULL means rows 0 .. n - 1.  A row named
 * twice is written twice with the same bytes; rows not named are not touched.  w_out [n_out, d] has the element type of w_other.
 * gram == NULL is accepted only with alpha0 == 0 (G is then read as +0.0).  set_off == set_items == NULL: every set is empty.
 * max_workgroups = 0 leaves the grid to the call, a positive value caps it (one wavefront serves one row, rows are walked
 * grid-stride); it never changes a byte.  No allocation, no copy to the host, no synchronise; n == 0 launches nothing.  Indices
 * (rows, set_off, set_items) are trusted, like Seen.
 * Refused (sml_last_error): a (d, elem_bytes) pair outside the list above; reg or alpha0 negative or NaN; n_other, n_out outside
 * (0, 2^31); max_workgroups < 0; exactly one of set_off / set_items NULL; w_out overlapping w_other, gram, the set or status, where
 * the pointers and known sizes show it; a gram or scratch not 16-byte aligned.
 * sml_host_gram / sml_host_als_solve: the same definitions as single-threaded walks over HOST memory; d is the caller's (no
 * context), and nothing has to be aligned.
 * Not measured: trained (non-random) tables, recall of folded-in new users on real periods, shapes beyond the Yelp one. */
#define SML_GRAM_CHUNK 1024
/* n_chunks * d * d * 8; < 0: bad argument (0 < n_rows < 2^31) */
int64_t sml_gram_scratch_bytes(sml_ctx* ctx, int64_t n_rows);
int sml_gram(sml_ctx* ctx, const void* w, int elem_bytes, int64_t n_rows, void* scratch, double* gram, void* stream);
int sml_host_gram(const void* w, int elem_bytes, int d, int64_t n_rows, double* gram);
int sml_als_solve(sml_ctx* ctx, const void* w_other, int elem_bytes, int64_t n_other, const double* gram,
                  double alpha0, double reg, const int64_t* set_off, const int32_t* set_items,
                  const int64_t* rows, int64_t n, void* w_out, int64_t n_out, int max_workgroups,
                  int32_t* status, void* stream);
int sml_host_als_solve(const void* w_other, int elem_bytes, int d, int64_t n_other, const double* gram,
                       double alpha0, double reg, const int64_t* set_off, const int32_t* set_items,
                       const int64_t* rows, int64_t n, void* w_out, int64_t n_out, int32_t* status);
/* ---- NEIGHBOURS: the neighbourhood model (ItemKNN) -- item-to-item neighbours from co-occurrence, and the list of a history that
 * has no row in any table.  One sparse operation underlies both: for a row x, accumulate over the lists of x's members and keep
 * the K best,  out(x) = top-K over j of sum_{m in R(x)} W[m, j].  The device entry points take a context and read no embedding
 * table, so any engine's context serves (any width, d = 128 included); the host walks take none.  All pointers of the device calls
 * are device memory.  The only atomics are integer, exact and order-free; similarities are accumulated in fixed point; there are no
 * floating-point atomics, so the bytes depend on no launch geometry.
 * NEIGHBOURS OF ITEMS (sml_cooc_topk).  by_item_off / by_item_users (int64 [n_item + 1] / int32): the item -> users CSR;
 * by_user_off / by_user_items (int64 [n_user + 1] / int32): the user -> items CSR -- the same set and its transpose, both as
 * sml_iset_build writes them.  rows int64 [n]: the query items; rows == NULL means 0 .. n - 1.  norm_a, norm_b: double [n_item],
 * both NULL or both given.  shrink: double >= 0.  min_co: int >= 1.  allow: filter words (ITEM FILTER), may be NULL.  1 <= k <= 128.
 * For query item i with users U(i), S(u) the items of user u:
 *   c(j) = #{u in U(i) : j in S(u)}, an integer;
 *   the candidates are the j != i with c(j) >= min_co that are allowed;
 *   without norms the score is s = (float)c;
 *   with norms, four roundings and no contraction:  den = norm_a[i] * norm_b[j], one fp64 rounding;  den = den + shrink;
 *     s64 = (double)c / den, the correctly rounded fp64 division;  s = (float)s64, to nearest even;
 *   an s that is NaN is not eligible (den = 0 gives inf, which is eligible, as in the family);
 *   the order is the family's: s descending, then id ascending.
 * Outputs: items int32 [n, k] and sims float [n, k], missing slots hold (-1, -inf); n_elig int32 [n] (may be NULL) = the number
 * of eligible candidates.  The definition contains no square root: the metric lives in the tables, which the caller makes (cosine:
 * a = b = deg^1/2; asymmetric: a = deg^alpha, b = deg^(1 - alpha)).  With norm_a == norm_b the product commutes exactly, so
 * sim(i, j) and sim(j, i) are the same bits.  With norms NULL and k >= the number of neighbours, the row is exactly the non-zero
 * off-diagonal of row i of X^T X, X the 0/1 interaction matrix.
 * WEIGHTED NEIGHBOURS OF ITEMS (sml_cooc_topk_weighted): the call above in which users do not count equally -- the random-walk
 * similarities P3alpha and RP3beta (user_w = deg_u^-alpha, norm_a = deg^alpha, norm_b = deg^beta), inverse-user-frequency cosine,
 * Adamic-Adar / resource allocation, any trust or recency weight per user.  Inputs are those of sml_cooc_topk, except: user_w float
 * [n_user], required; frac_bits F in [0, 32]; there is no min_co.  For query item i:
 *   a user's weight in fixed point is q(u) = llrint(ldexp((double)user_w[u], F)), round to nearest even (the quantisation of the
 *     list of a history below, the same text);
 *   a user contributes nothing when user_w[u] is not finite, or |q(u)| > 2^32, or q(u) <= 0; a user that contributes nothing
 *     creates no candidate;
 *   cw(j) = sum of q(u) over the contributing u in U(i) with j in S(u), an int64.  It cannot overflow: fewer than 2^31 users, each
 *     at most 2^32;
 *   the candidates are the j != i with cw(j) > 0 that are allowed;
 *   num = ldexp((double)cw, -F); the int64 -> double conversion rounds to nearest even and is exact below 2^53;
 *   without norms the score is s = (float)num;
 *   with norms:  den = norm_a[i] * norm_b[j], one fp64 rounding;  den = den + shrink;  s64 = num / den, correctly rounded;
 *     s = (float)s64;
 *   a NaN score is not eligible, an inf score is;
 *   order, padding (-1, -inf), n_elig, rows == NULL, 1 <= k <= 128 and a row named twice being written twice are the family's.
 * Defining identities of the weighted call:
 *   (a) unit weights: user_w == 1.0f everywhere with F = 0 returns sml_cooc_topk's bytes at min_co = 1 (items, sims, n_elig),
 *       with norms and without;
 *   (b) dropped users: a user that contributes nothing behaves like that user removed from both CSRs;
 *   (c) power-of-two scaling: doubling every weight while lowering F by one leaves every q(u) and so every cw, the items and
 *       n_elig the same bytes; num carries the scale 2^-F, so every sim is exactly doubled -- the same bytes once halved;
 *   (d) symmetry: with norm_a == norm_b, weighted sim(i, j) and sim(j, i) are the same bits;
 *   (e) prefix: a k'-call of the weighted call is the prefix of its k-call;
 *   (f) geometry: max_workgroups and path never change a byte of the weighted call;
 *   (g) filter: a filtered call returns the unfiltered row with the disallowed candidates removed, and its n_elig counts the rest.
 * Paths: as above, with int64 sums in the on-chip table and one int64 [n_item] accumulator per wavefront in scratch; every
 * contributing q is >= 1, so a touched slot is a non-zero slot and the claim is the exchange that returns a non-zero sum -- no
 * bitmap.  scratch: sml_cooc_weighted_scratch_bytes(ctx, n_item, max_workgroups) bytes (< 0: bad argument), 256-byte aligned,
 * zeroed by the call at the start as far as it is used and left zero.  Refused, a refused call writing nothing: everything
 * sml_cooc_topk refuses; user_w NULL; F outside [0, 32]; a misaligned scratch.  sml_host_cooc_topk_weighted: the single-threaded
 * walk over HOST memory (a dense int64 array, then a full sort), sharing the quantisation and the score text with the kernel.
 * Not measured for the weighted call: real periods, trained comparisons, shapes beyond the Yelp one, sums above 2^53.
 * THE LIST OF A HISTORY (sml_knn_topk).  nbr_items int32 and nbr_sims float, both [n_rows_nbr, k_nbr], 1 <= k_nbr <= 128: the
 * output form of the call above, but any table of that shape is accepted.  hist_off / hist_items: the CSR of histories.  users
 * int64 [n] indexes hist_off and seen_off; users == NULL means 0 .. n - 1.  frac_bits F in [0, 32].  seen_off / seen_items, allow:
 * the family's exclusion forms.  1 <= k <= 128.
 *   A history member m outside [0, n_rows_nbr) is skipped before any address is formed.
 *   A neighbour slot contributes nothing when its id is outside [0, n_item), or its sim is not finite, or |q| > 2^32, where
 *     q = llrint(ldexp((double)sim, F)), round to nearest even.
 *   acc(j) = sum of q, an int64.  It cannot overflow: a history has < 2^31 members and j occurs at most once per list.
 *   A candidate is every j that occurs in a contributing slot, whatever its sum: a j whose sum cancels to 0 is still a candidate
 *     with score 0.
 *   A candidate is eligible if it is allowed and not in Seen(users[x]).  History members are not excluded unless Seen says so.
 *   Score A = (float)ldexp((double)acc, -F); both conversions round to nearest even.
 *   Order, padding and n_elig are the family's.
 * Defining identities:
 *   - a k'-call is the prefix of a k-call;
 *   - a filtered call equals the unfiltered call with the filter's complement added to every Seen range;
 *   - max_workgroups and path never change a byte;
 *   - a row named twice is written twice with the same bytes;
 *   - a history {i} with no Seen and no filter returns item i's neighbour list, ids in the same order, and the scores are bit-equal
 *     when every sim is a multiple of 2^-F (with F = 30: every float >= 2^-7 in magnitude).
 * Two paths, one definition.  A row whose total list length (sum over its members of their lists' lengths, a bound on its distinct
 * ids known before the walk) is at most sml_knn_lds_limit() accumulates in an open-addressing table in LDS of at least twice that
 * many slots, which therefore can never fill; any other row owns a dense accumulator over [0, n_item) in scratch (int32 counts for
 * the neighbours of items; int64 sums plus a touched bitmap for the list of a history), adds with integer atomics, and then
 * claims every touched candidate once -- on a second walk of its lists, or from the bitmap's words when a history's lists hold more
 * slots than the catalogue has items -- and the lane that claims it takes its sum and resets the slot.  path: 0 auto, 1 dense
 * everywhere, 2 LDS wherever it fits.  max_workgroups = 0 leaves the grid to the call, a positive value caps it (one wavefront serves one row, rows
 * are walked grid-stride).
 * scratch: sml_knn_scratch_bytes(ctx, n_item, max_workgroups, kind) bytes (kind 0: neighbours of items, 1: the list of a history;
 * < 0: bad argument) for the same n_item and max_workgroups, 256-byte aligned.  The call zeroes what it uses of its scratch at the
 * start and leaves it zero.  No allocation, no copy to the host and no synchronise inside; n == 0 launches nothing.  Indices (rows,
 * users, the CSRs' offsets and entries) are trusted, like Seen.
 * Refused (sml_last_error; a refused call writes nothing): k, k_nbr, frac_bits, min_co, max_workgroups or path out of range;
 * shrink negative or NaN; exactly one of a CSR's two pointers NULL; exactly one of the norms NULL; n_item or n_user outside
 * (0, 2^31); a misaligned scratch; an output overlapping an input or another output, where pointers and known sizes show it.
 * sml_host_cooc_topk / sml_host_knn_topk: the same definitions as single-threaded walks over HOST memory (a plain dense array, then
 * a full sort by the order); they share the text of the scores with the kernels.
 * Not measured: real periods, trained tables as the neighbour table, anything beyond the Yelp shape. */
int sml_knn_lds_limit(void);
int64_t sml_knn_scratch_bytes(sml_ctx* ctx, int64_t n_item, int max_workgroups, int kind);
int sml_cooc_topk(sml_ctx* ctx, const int64_t* by_item_off, const int32_t* by_item_users,
                  const int64_t* by_user_off, const int32_t* by_user_items, int64_t n_user, int64_t n_item,
                  const int64_t* rows, int64_t n, const double* norm_a, const double* norm_b, double shrink, int min_co,
                  const uint32_t* allow, int k, int max_workgroups, int path, void* scratch,
                  int32_t* items, float* sims, int32_t* n_elig, void* stream);
int sml_host_cooc_topk(const int64_t* by_item_off, const int32_t* by_item_users,
                       const int64_t* by_user_off, const int32_t* by_user_items, int64_t n_user, int64_t n_item,
                       const int64_t* rows, int64_t n, const double* norm_a, const double* norm_b, double shrink, int min_co,
                       const uint32_t* allow, int k, int32_t* items, float* sims, int32_t* n_elig);
int64_t sml_cooc_weighted_scratch_bytes(sml_ctx* ctx, int64_t n_item, int max_workgroups);
int sml_cooc_topk_weighted(sml_ctx* ctx, const int64_t* by_item_off, const int32_t* by_item_users,
                           const int64_t* by_user_off, const int32_t* by_user_items, int64_t n_user, int64_t n_item,
                           const int64_t* rows, int64_t n, const float* user_w, int frac_bits,
                           const double* norm_a, const double* norm_b, double shrink,
                           const uint32_t* allow, int k, int max_workgroups, int path, void* scratch,
                           int32_t* items, float* sims, int32_t* n_elig, void* stream);
int sml_host_cooc_topk_weighted(const int64_t* by_item_off, const int32_t* by_item_users,
                                const int64_t* by_user_off, const int32_t* by_user_items, int64_t n_user, int64_t n_item,
                                const int64_t* rows, int64_t n, const float* user_w, int frac_bits,
                                const double* norm_a, const double* norm_b, double shrink,
                                const uint32_t* allow, int k, int32_t* items, float* sims, int32_t* n_elig);
int sml_knn_topk(sml_ctx* ctx, const int32_t* nbr_items, const float* nbr_sims, int64_t n_rows_nbr, int k_nbr, int64_t n_item,
                 const int64_t* hist_off, const int32_t* hist_items, const int64_t* users, int64_t n, int frac_bits,
                 const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, int k,
                 int max_workgroups, int path, void* scratch, int32_t* items, float* scores, int32_t* n_elig, void* stream);
int sml_host_knn_topk(const int32_t* nbr_items, const float* nbr_sims, int64_t n_rows_nbr, int k_nbr, int64_t n_item,
                      const int64_t* hist_off, const int32_t* hist_items, const int64_t* users, int64_t n, int frac_bits,
                      const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, int k,
                      int32_t* items, float* scores, int32_t* n_elig);
/* ---- PROPAGATION: one hop along the user-item graph -- the LightGCN layer E' = D^-1/2 A D^-1/2 E, and a plain smoothing operator
 * in its own right.  One sparse-times-dense product underlies it:  out[x] = a[row] * sum_{m in S(row)} b[m] * src[m].
 * With src the item table, S the user -> items set, a = deg_u^-1/2 and b = deg_i^-1/2 it is the user half of a layer; the item half
 * is the same call on the transposed set with the two scale tables swapped, and so is the transpose of either (the operator is
 * linear), which makes the backward pass the same call.  Every fp32 operation and its order are named below, so the bytes depend
 * on no launch geometry; the host walk shares the text of the steps with the kernels, compiled so that nothing is contracted or
 * reassociated: every fused step is an explicit fmaf().  There are no floating-point atomics and no matrix instructions.
 * Inputs: src [n_src, d] of element type T -- fp32 (elem_bytes 4) or fp16 (elem_bytes 2) -- and width d = 32 / 64 / 128, the
 * context's; all six pairs are accepted.  set_off int64 / set_items int32: the CSR of members, ids ascending, as sml_iset_build
 * writes them.  rows int64 [n], may be NULL: rows == NULL means rows 0 .. n - 1; rows[x] indexes set_off and a.  a: float indexed
 * by row id (at least max(rows) + 1 entries); b: float [n_src]; either may be NULL, which means 1.0f.  out: float [n, d] whatever
 * T is; out[x] belongs to rows[x].
 * For a row with members m_0 < m_1 < ... < m_{L-1} at positions p = 0 .. L - 1, and for every dimension s:
 *   1. position p belongs to segment c = p / SML_PROP_SEG and to strand j = p % SML_PROP_STRANDS; SML_PROP_SEG = 256 and
 *      SML_PROP_STRANDS = 8 are constants of the definition;
 *   2. per (c, j), over the positions of that segment and strand ascending: acc = +0.0f, then
 *      acc = fmaf(b[m_p], (float)src[m_p][s], acc);
 *   3. the segment value is a fixed tree of fp32 adds: u_j = acc_j + acc_{j+4} for j = 0 .. 3; v_j = u_j + u_{j+2} for j = 0, 1;
 *      seg_c = v_0 + v_1;
 *   4. tot = +0.0f, then for c ascending: tot = tot + seg_c;
 *   5. out[x][s] = a[row] * tot, one fp32 rounding.
 * An empty set gives a[row] * +0.0f.  NaN / Inf propagate with no special case.  A row named twice is written twice with the same
 * bytes.  The fp16 result equals the result on the widened fp32 copy bit for bit (the widening is exact).
 * Two paths, one definition.  A row of fewer than sml_graph_split_from() segments is summed by one wavefront; any other row has
 * its segments summed by separate wavefronts into scratch, and a further pass adds them in segment order (step 4).  path: 0 auto,
 * 1 never split (scratch is not touched and may be NULL), 2 split every row of more than one segment.  max_workgroups = 0 leaves
 * the grid to the call, a positive value caps it.  Neither ever changes a byte.
 * scratch: sml_graph_scratch_bytes(ctx, n, nnz, max_workgroups) bytes of device memory, 256-byte aligned, for the same n; nnz is
 * the number of members of the n named rows, a row named twice counted twice (rows == NULL: set_off[n]) -- a larger value is
 * fine, a smaller one is not: the call cannot check it.  < 0: bad argument.  The scratch holds nothing between calls.
 * No allocation, no copy to the host and no synchronise inside; n == 0 launches nothing.  The only atomic is an integer one (a
 * split row reserves its slots of scratch).  Indices (rows, set_off, set_items) are trusted, like Seen.
 * Refused (sml_last_error; a refused call writes nothing): elem_bytes outside {2, 4}; a width other than 32 / 64 / 128; n_src
 * outside (0, 2^31) or n outside [0, 2^31); max_workgroups < 0 or path outside 0 .. 2; exactly one of set_off / set_items NULL
 * (both NULL: every set is empty); a scratch not 256-byte aligned, or a src or out not 16-byte aligned; out overlapping src, the
 * set, rows, a, b or the scratch, where the pointers and known sizes show it.
 * sml_host_graph_propagate: the same definition as a single-threaded walk over HOST memory; d is the caller's (no context),
 * there is no scratch and nothing has to be aligned.
 * Not measured: trained tables, the recall of a fitted LightGCN on real periods, shapes beyond the Yelp one. */
#define SML_PROP_SEG 256
#define SML_PROP_STRANDS 8
/* the number of segments from which a row is split (a measured value) */
int sml_graph_split_from(void);
int64_t sml_graph_scratch_bytes(sml_ctx* ctx, int64_t n, int64_t nnz, int max_workgroups);
int sml_graph_propagate(sml_ctx* ctx, const void* src, int elem_bytes, int64_t n_src,
                        const int64_t* set_off, const int32_t* set_items, const int64_t* rows, int64_t n,
                        const float* a, const float* b, int max_workgroups, int path, void* scratch,
                        float* out, void* stream);
int sml_host_graph_propagate(const void* src, int elem_bytes, int d, int64_t n_src,
                             const int64_t* set_off, const int32_t* set_items, const int64_t* rows, int64_t n,
                             const float* a, const float* b, float* out);
/* ---- DEEP LISTS: candidate generation at depth -- lists of up to 1,024 items per user over the whole catalogue, for a
 * downstream re-ranker, a recall@K curve or a pool.  sml_topk_items keeps a sorted list per (user, slice) and its cost grows
 * with k; sml_topk_deep selects by radix: a fixed number of catalogue walks (four counting passes over the order-preserving
 * bits of the score, one or two collecting passes) and one sort per user, whatever k is and whatever the data are.
 * Arguments: the tables, elem_bytes (4: d = 32 / 64; 2: d = 32 / 64 / 128; any other pair is refused), Seen and allow are
 * those of sml_topk_items_adjusted, and so is adj, except that here adj == NULL is accepted and means the bare score S (no fmaf
 * is applied: the chain's bits are returned, as sml_topk_candidates reads it).  allow == NULL: no filter.
 * 1 <= k <= SML_TOPK_DEEP_MAX.  users int64 [n]; a user may repeat.
 * Outputs: items / scores (int32 / float [n, k]) are exactly the top-K family's definition: the ELIGIBLE items -- below n_item,
 * not in Seen(u), allowed, and A not NaN -- in the order A descending, then item id ascending; slots past the eligible count
 * hold (-1, -inf).  n_elig[x] (int32 [n]; may be NULL) = the number of eligible items of users[x].  Every output is written.
 * Defining identities:
 *   - for k <= 128, items and scores equal those of sml_topk_items[_filtered|_adjusted][_f16] on the same arguments byte for
 *     byte;
 *   - for any k' < k, row x of the k'-call is the first k' slots of row x of the k-call;
 *   - a filtered call returns what the unfiltered call returns with the complement of the filter added to every user's Seen
 *     range (Seen' = Seen U complement); at d = 32 / 64 a call on fp16 tables equals the call on fp32 copies of them bit for
 *     bit; with the same Seen, filter and adj, the positive of a row (u, p) sits at position
 *     rank + #{eligible i != p : A(u,i) == A(u,p), i < p} of u's list (rank: sml_full_rank's) whenever that is < k.
 * Ties: the order compares floats, so -0 and +0 tie and the id decides (with adj, fmaf(+0, -1, -0) is -0); the integer key
 * the selection derives from a score sends both zeros to one key, and the returned score keeps its own sign bit.  NaN never
 * enters a list.  -inf is eligible and orders last.
 * Geometry: slices = 0 leaves the grid to the call, a value in [1, 256] forces the number of item slices; the bytes are the
 * same for every value, empty slices included.
 * scratch: sml_topk_deep_scratch_bytes(ctx, n, k, n_item, slices) bytes of device memory, 256-byte aligned, for the same n,
 * n_item and slices (< 0: bad argument); about 1 KB per user.  It is written by the call and holds nothing afterwards.
 * n == 0 is a valid call that launches nothing.  No allocation, no copy to the host and no synchronise happen inside; counts
 * are added with integer atomics (exact, order-free) and there are no floating-point atomics.
 * Refused (sml_last_error): k outside [1, 1024] or slices outside [0, 256]; exactly one of seen_off / seen_items NULL; a
 * (d, elem_bytes) pair the kernels do not exist for; a misaligned table, adj or scratch; an output that overlaps an input or
 * another output as far as the pointers and the sizes known to the call show it.  Indices (users) are trusted.
 * Not measured beyond the shapes profiles/ records; sml_topk_candidates and sml_rerank_mmr keep their limit of 128.
 * sml_host_topk_items: the same definition as a single-threaded walk over HOST memory, for any k in [1, 1024] -- every item's
 * score by the same chain (the host and the device share its text), no GPU needed; d is the caller's (no context).  It
 * refuses what sml_topk_deep refuses, except that nothing has to be aligned. */
#define SML_TOPK_DEEP_MAX 1024
int64_t sml_topk_deep_scratch_bytes(sml_ctx* ctx, int64_t n, int k, int64_t n_item, int slices);
int sml_topk_deep(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item,
                  const int64_t* users, int64_t n, int k,
                  const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                  int slices, void* scratch, int32_t* items, float* scores, int32_t* n_elig, void* stream);
int sml_host_topk_items(const void* w_user, const void* w_item, int elem_bytes, int d, int64_t n_item,
                        const int64_t* users, int64_t n, int k,
                        const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                        int32_t* items, float* scores, int32_t* n_elig);
/* Per-user metrics from pos (as sml_user_rank writes it; any value < 0 is never a hit) over the ranges of pos_off,
 * n < 2^31.  ks: HOST int32 [n_k], 1 <= n_k <= 8, every K >= 1.  For user x with m = |T(x)| and each K (outputs [n, n_k], row-major):
 *   hits = #{p : 0 <= pos(p) < K};  dcg = sum over hits of 1/log2(pos + 2), fp32, summed in ascending pos;
 *   ap = sum over the j-th hit (j = 1, 2, ... in ascending pos) of j / (pos + 1), fp32, same order;
 *   first[x] = the smallest pos >= 0, -1 if none.  Normalisation (by m, K, IDCG) is the caller's.
 * The sums take each non-negative pos value once: a value repeated inside a range (sml_user_rank never writes one for
 * unique held-out items) counts in hits once per copy but adds one term to dcg / ap.  Every output is written. */
int sml_user_metrics(sml_ctx* ctx, const int32_t* pos, const int64_t* pos_off, int64_t n, const int32_t* ks, int n_k,
                     int32_t* hits, float* dcg, float* ap, int32_t* first, void* stream);

/* ---- measurement ------------------------------------------------------------------ */
/* Optional HIP-event timing of every kernel launch on the caller's stream, by kernel class
 * (bench.py's roofline leg).  Off by default; when on, each launch is bracketed by two
 * event records.  sml_prof_get synchronises on the last recorded event. */
int sml_prof_enable(sml_ctx* ctx, int on);
/* In-kernel timeline of the training kernels (measurement builds only: -DSML_TIMELINE, see tools/timeline_probe.py;
 * returns -1 otherwise).  buf: device int64, [0] = record counter (zero it), 16-stamp records from [16]; NULL: off. */
int sml_debug_timeline(long long* buf);
int sml_prof_reset(sml_ctx* ctx);
/* Average reading (microseconds) of n EMPTY event pairs on `stream`: the cost of the bracket itself, which a caller
 * subtracts from per-launch averages of short kernels.  Synchronous. */
int sml_prof_pair_overhead(sml_ctx* ctx, int n, void* stream, double* avg_us);
int sml_prof_classes(void);
const char* sml_prof_name(int cls);
int sml_prof_get(sml_ctx* ctx, int cls, int64_t* count, double* total_ms);

/* ---- device batch supply (fast mode) --------------------------------------------------- */
/* offlineDataset_withsample's negatives (reference data/dataset.py:63-71) drawn ON THE DEVICE: for every
 * element e, candidates uniform over item_all[0..pop) are redrawn while they are one of users[e]'s own
 * items (CSR: user_ptr [n_users+1] into ascending user_items; all device pointers).  Same distribution as
 * the reference's loop, NOT its numpy random stream: the driver uses it only when asked
 * (--device_batches); the stream-exact host path (sml_host_resolve_negatives_csr) is the default.
 * Counter-based generator keyed by (seed, e): reproducible for a given seed.  *failed (device int32) counts
 * elements whose 4096 draws were all rejected; such an element still gets a valid item, its last candidate. */
int sml_sample_negatives(sml_ctx* ctx, const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop,
                         const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, uint64_t seed,
                         int64_t* negs, int32_t* failed, void* stream);

/* One shuffled pass over a period's rows assembled on the device -- the device form of a DataLoader(shuffle=True) pass over
 * trainDataset_withPreSample (reference data/dataset2.py:172-201: rows [user, item, c2, c3, ...], ONE pre-sampled column per
 * pass is the negative) and of the (user, item) half of offlineDataset_withsample (data/dataset.py:41-71).  ui: device int64
 * [n,2]; mat (or NULL): device integer matrix (elem_bytes 4 or 8) with row_stride elements per row -- out3[e] = (ui[r][0],
 * ui[r][1], mat[r*row_stride + col]) with r = perm(e); NULL leaves column 2 alone (sml_sample_negatives fills it).  perm is a
 * counter-based permutation of [0, n) keyed by `seed` (a Feistel network, cycle-walked): the same distribution as the
 * reference's shuffle, NOT torch's randperm stream -- used only under --device_batches; every rank of a job derives the
 * same epoch from the same seed without communication.  Asynchronous. */
int sml_device_epoch(sml_ctx* ctx, const int64_t* ui, const void* mat, int elem_bytes, int64_t row_stride, int64_t col, int64_t n,
                     uint64_t seed, int64_t* out3, void* stream);

/* ---- SPMF rank-weighted sampling (reference model/baseline.py:448-503) ----------------- */
/* sml_rank_weights replaces SPMF.compute_R_W_P (model/baseline.py:448-476): rows int64 [n,2] (user, item), 0 <= n < 2^31,
 * d = 32 / 64 / 128.  score[r] = MFbasemode.forward's score of row r, the same bytes as sml_mf_forward's `score`.  The rows
 * are ranked by score descending with a stable device radix sort: equal scores by row index ascending, -0.0 equal to
 * +0.0, NaN before everything (as torch.argsort(descending=True, stable=True) places it).  order[k-1] (int32) = the row
 * of rank k, rank[row] (int32) = its rank in 1..n, and p[row] = w / S with w = expf(__fdiv_rn((float)rank, (float)n))
 * and S the fp32 rounding of a fixed-order float64 sum of all w: the same bytes whatever the launch shape.
 * sml_rank_weights_scratch_bytes: bytes of `scratch` (256-byte aligned base; contents not needed afterwards), linear in
 * n; < 0: bad argument.  Asynchronous. */
int64_t sml_rank_weights_scratch_bytes(sml_ctx* ctx, int64_t n);
int sml_rank_weights(sml_ctx* ctx, const float* w_user, const float* w_item, const int64_t* rows, int64_t n, void* scratch,
                     float* score, int32_t* rank, int32_t* order, float* p, void* stream);
/* sml_weighted_epoch: the device form of SPMF.sample_batch (model/baseline.py:489-503) for a whole epoch.  Element e of
 * [0, n_out) draws u in [0, 1) from the counter-based stream keyed by (seed, e) and takes rank
 * k = ceil(n * ln(1 + u (e - 1))) clamped to [1, n] -- the exact inverse of the rank-order CDF of w = exp(k / n) -- then
 * out3[e] = (rows[r][0], rows[r][1], neg) with r = order[k-1] (as sml_rank_weights wrote it).  neg is drawn by
 * sml_sample_negatives' rejection walk over item_all[0..pop) and the CSR user_ptr [n_users+1] / user_items (every user's
 * items ascending); *failed (device int32, zeroed here) counts elements still rejected after 4096 draws.  The same
 * distribution as the reference's numpy draws, NOT its random stream.  All pointers are device memory.  Asynchronous. */
int sml_weighted_epoch(sml_ctx* ctx, const int64_t* rows, int64_t n, const int32_t* order, const int64_t* item_all, int64_t pop,
                       const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, int64_t n_out, uint64_t seed,
                       int64_t* out3, int32_t* failed, void* stream);

/* ---- interaction sets ------------------------------------------------------------------ */
/* A set over (n_user, n_item), 0 < n_user < 2^31, 0 < n_item < 2^31, is exactly the Seen CSR of the retrieval section:
 *   off    int64 [n_user + 1], off[0] = 0
 *   items  int32 [nnz], ascending and unique inside each user's range [off[u], off[u + 1])
 * so every output of these calls goes to sml_full_rank*, sml_topk_items* and sml_user_rank* as seen_off / seen_items or
 * pos_off / pos_items without a copy.  m, nnz < 2^31.  Indices are trusted on the device, like every other index of the
 * library (sml_amd.retrieval.DeviceSeen range-checks them).
 *
 * Rules for all of them: integer work only; the output bytes are the same whatever the schedule (the only atomics are
 * order-free digit counters in LDS); no workgroup waits on another -- every dependency is a launch boundary, so the
 * calls suit hipGraph capture; the launch functions do no allocation, no copy to the host and no synchronise: the
 * workspace is the caller's `scratch` (16-byte aligned base; contents not needed afterwards; the _scratch_bytes calls
 * return its size, < 0: bad argument).  All pointers are device memory.  Asynchronous.
 *
 * sml_iset_build: rows int64 [m, n_cols >= 2], column 0 the user, column 1 the item, further columns ignored (a test
 *   period's rows with their sampled negatives go in as they are).  Duplicates are allowed, in any order; m = 0 is
 *   allowed.  Writes all of off [n_user + 1] and items[0 .. nnz), nnz = off[n_user] = the number of distinct pairs.  The
 *   caller gives `items` room for m entries; entries past nnz are unspecified.  A stable LSD radix sort by item and then
 *   by user (8 bits per pass, only the passes that cover n_item - 1 and n_user - 1), adjacent-unique flags, one scan.
 * sml_iset_union: out = the union of a and b, user by user, in the same format.  out_items has room for nnz_a + nnz_b
 *   (nnz_a = a_off[n_user], nnz_b = b_off[n_user], given by the caller); entries past out_off[n_user] are unspecified.
 *   Outputs must not alias inputs: overlap of an output with an input is refused where the pointers show it.  Either
 *   side may be empty (its items pointer may then be NULL).  Element-parallel: every element of b bisects its user's
 *   range of a, every element of a its user's range of b, and each computes its output slot; nobody walks a range.
 *   One call reads and writes O(nnz_a + nnz_b): the history is copied once per union.
 * sml_iset_contains: rows as above; out uint8 [m] is 1 exactly when (rows[r][0], rows[r][1]) is in the set. */
int64_t sml_iset_build_scratch_bytes(sml_ctx* ctx, int64_t m, int64_t n_user, int64_t n_item);
int sml_iset_build(sml_ctx* ctx, const int64_t* rows, int64_t m, int n_cols, int64_t n_user, int64_t n_item, void* scratch,
                   int64_t* off, int32_t* items, void* stream);
int64_t sml_iset_union_scratch_bytes(sml_ctx* ctx, int64_t nnz_a, int64_t nnz_b, int64_t n_user);
int sml_iset_union(sml_ctx* ctx, int64_t n_user, const int64_t* a_off, const int32_t* a_items, int64_t nnz_a,
                   const int64_t* b_off, const int32_t* b_items, int64_t nnz_b, void* scratch,
                   int64_t* out_off, int32_t* out_items, void* stream);
int sml_iset_contains(sml_ctx* ctx, const int64_t* rows, int64_t m, int n_cols, const int64_t* off, const int32_t* items,
                      uint8_t* out, void* stream);

/* ---- test-set negatives ---------------------------------------------------------------- */
/* The negatives of a test period's rows -- the device form of the reference's data/dataset2.py select_neg_forinteraction:
 * the same distribution, NOT numpy's random stream (the contract of sml_sample_negatives and sml_weighted_epoch).
 *
 * The stream is every period's rows one after the other; row g (a global position, < 2^31) is (u, i).  C(g) is the set of
 * items of rows 0..g and H(g) the set of items of user u in rows 0..g, row g included in both.  A row's negatives are a
 * uniformly random neg_num-subset of C(g) \ H(g) in uniformly random order, fixed to the byte as follows.
 *   order   int32: the items by first appearance; C(g) = order[0 .. n_cat(g)), n_cat(g) = |C(g)|
 *   H       a CSR over the users: h_off int64 [n_user + 1], h_items int32 ascending and unique per user, h_since int32 the
 *           global position of the pair's first row; H(g) = the entries of u's range with h_since <= g
 *   draws   row g owns the stream s0 = neg_stream(seed, g); candidate number c = 0, 1, 2, ... is
 *             order[umul64hi(mix(s0 + (c + 1) * 0x9e3779b97f4a7c15), n_cat(g))]
 *           -- the c-th output of splitmix64 from state s0, addressed by c.  Walking c upwards, a candidate in H(g) or equal
 *           to an earlier accepted candidate of the row is rejected, anything else accepted; the negatives are the first
 *           neg_num accepted candidates in acceptance order.
 *   fails   a row with n_cat(g) - |H(g)| < neg_num (decided before any draw), or with fewer than neg_num accepted among
 *           262,144 candidates, keeps -1 in every slot it did not fill and adds 1 to *failed.
 * sml_neg_sets: rows int64 [n, n_cols >= 2] are the rows g0 .. g0 + n - 1 of the stream (column 0 the user, column 1 the item),
 *   n_cat int32 [n] their catalogue sizes.  out int64 [n, 2 + neg_num]: out[r] = (rows[r][0], rows[r][1], negatives...), the
 *   format of a test/<p>.npy file and of the evaluation calls.  1 <= neg_num <= 4096; anything else is refused, and so is an
 *   out that overlaps an input where the pointers show it.  One wavefront per row takes 64 candidates per round; rows are
 *   walked grid-stride, max_workgroups = 0 leaves the grid to the call, and any grid gives the same bytes whatever the
 *   schedule.  *failed (device int32) is zeroed by the call.  No allocation, no copy to the host, no synchronise.  Indices
 *   are trusted on the device (sml_amd.prepare.Timeline range-checks them).  All pointers are device memory.  Asynchronous. */
int sml_neg_sets(sml_ctx* ctx, const int64_t* rows, int64_t n, int n_cols, int64_t g0, const int32_t* n_cat, const int32_t* order,
                 const int64_t* h_off, int64_t n_user, const int32_t* h_items, const int32_t* h_since, int neg_num, uint64_t seed,
                 int max_workgroups, int64_t* out, int32_t* failed, void* stream);

/* ---- training negatives ---------------------------------------------------------------- */
/* One training negative per element, drawn uniformly or by popularity and, with a pool, the hardest of M: the sampler of
 * the device batch supply beyond sml_sample_negatives.  The kernel (sml_sample_negatives_ex), the host walk
 * (sml_host_sample_negatives_ex) and the tests' restatement all implement this definition.
 *
 * Inputs.  For element e of [0, n) with user u = users[e]: item_all[0..pop); the CSR user_ptr [n_users + 1] / user_items
 *   (ascending per user); an optional cdf; pool = M, 1 <= M <= 64; seed; for M > 1, fp32 tables w_user, w_item of width
 *   d = 32 or 64 (fp16 tables are out of scope).
 * Draws.  s0 = neg_stream(seed, e) = seed ^ (e * 0xd1342543de82ef95 + 0x632be59bd9b4e019); output number c = 0, 1, 2, ... is
 *   z_c = splitmix64_mix(s0 + (c + 1) * 0x9e3779b97f4a7c15) -- the c-th splitmix64() call from state s0, the stream
 *   sml_sample_negatives consumes, addressed by c.
 * Candidate c.  cdf == NULL: cand_c = item_all[umulhi64(z_c, pop)], sml_sample_negatives' expression.  cdf given: cdf is
 *   float64 [pop], nondecreasing, cdf[pop - 1] == 1.0; u_c = (z_c >> 11) * 2^-53; idx_c = the first index with
 *   cdf[idx] > u_c (bisect right); cand_c = item_all[idx_c].  Entries of zero mass are never drawn.
 * Admissible.  cand_c is admissible when it is not in u's CSR range, tested by bisection.  A user outside [0, n_users) has
 *   an empty range.
 * Pool.  The first M admissible candidates in order of c, restricted to c < 4096.  The pool may hold the same item twice.
 * Choice.  M == 1: the first admissible candidate; no table is read, the table pointers may be NULL.  M > 1: the pool
 *   member with the greatest S = the fp32 fmaf chain of the retrieval section over (w_user[u], w_item[cand]): acc = 0, then
 *   for s = 0 .. d/2 - 1: acc = fmaf(x[s], u[s], acc); acc = fmaf(x[s + d/2], u[s + d/2], acc).  A NaN score loses to every
 *   non-NaN score; among equal scores, or among all-NaN scores, the smaller c wins.  Fewer than M admissible candidates
 *   below the cap: the choice is among those found; this is not a failure.  No admissible candidate below the cap:
 *   *failed += 1 and the result is cand_4095, a valid item, which is what sml_sample_negatives returns.
 * Outputs.  negs int64 [n]; score float32 [n] (optional, may be NULL), S(u, negs[e]), written for M > 1 only; failed
 *   int32 [1], zeroed by the call.
 * Identity.  The bytes do not depend on launch geometry: elements are walked grid-stride, max_workgroups = 0 leaves the
 *   grid to the call, any grid gives the same bytes.  With cdf == NULL and M == 1, negs and failed equal
 *   sml_sample_negatives' output for the same arguments, byte for byte (with max_workgroups = 0 that case launches
 *   sml_sample_negatives' own kernel: the new one-lane kernel measured 1.3 - 3.8 % slower).
 * Properties.  The pool for M is a prefix of the pool for M' > M, so the chosen score never decreases as M grows; for
 *   M = 1 it is the score of sml_sample_negatives' negative.
 * Refused (SML_EINVAL): pool outside 1..64; pool > 1 with a NULL table, with d not 32 or 64, or with a table that is not
 *   16-byte aligned; a NULL users, item_all, user_ptr, user_items, negs or failed; pop <= 0; n, n_users or max_workgroups
 *   < 0.  Indices are trusted on the device (HipEngine.sample_negatives_ex range-checks users and item_all against the
 *   tables).  No allocation, no copy to the host, no synchronise.  All pointers are device memory.  Asynchronous. */
int sml_sample_negatives_ex(sml_ctx* ctx, const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop,
                            const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, const double* cdf, int pool,
                            const float* w_user, const float* w_item, int d, uint64_t seed, int max_workgroups, int64_t* negs,
                            float* score, int32_t* failed, void* stream);

/* ---- RE-RANKING ------------------------------------------------------------------------ */
/* Greedy MMR (maximal marginal relevance) re-ranking: from each list's pool of (item, relevance) entries pick up to k, one at
 * a time, trading relevance against the similarity to what is already picked, and report how alike the picks are.  The
 * kernel (sml_rerank_mmr), the host walk (sml_host_rerank_mmr) and the tests' restatement all implement this definition.
 *
 * Inputs per list x of [0, n).  A pool of at most 128 entries: pool_items[x * pool_stride + e] (int32) and
 *   pool_rel[x * pool_stride + e] (float) for e in [0, pool_cols); 1 <= pool_cols <= 128, pool_stride >= pool_cols,
 *   1 <= k <= 128.
 * Tables.  The item table w_item [n_item, d], elem_bytes 4 (fp32, d = 32 / 64) or 2 (fp16, d = 32 / 64 / 128): the pairs
 *   sml_retrieval_supports answers for; fp16 entries are widened exactly.
 * Norms.  nrm float [>= n_item] or NULL: plane 0 of the table sml_item_adjust_cosine writes is exactly this.
 * Trade-off.  lam in [0, 1]; oml = 1.0f - lam, formed once in fp32; normalize is 0 or 1.
 * Eligible.  Entry e is ELIGIBLE when 0 <= id < n_item (any other id is padding and no address is formed from it: the
 *   (-1, -inf) padding of the top-K calls is skipped), rel is not NaN, and no e' < e has the same id and a non-NaN rel: the
 *   first occurrence wins.
 * Relevance r(e).  normalize == 0: rel as given.  normalize == 1: min-max scaled over the list's eligible entries:
 *   lo = min rel, hi = max rel (-0 orders below +0), span = hi - lo, r = span > 0 ? (rel - lo) / span : +0 -- an fp32
 *   subtraction and a correctly rounded fp32 division.
 * Similarity of candidate c against a picked item s.  S = the retrieval score chain with x_s on the user side and x_c on the
 *   item side: acc = 0, then for q = 0 .. d/2 - 1: acc = fmaf(x_c[q], x_s[q], acc); acc = fmaf(x_c[q + d/2], x_s[q + d/2],
 *   acc).  nrm == NULL: sim = S.  Otherwise sim = (S * nrm[c]) * nrm[s]: two fp32 multiplies in that order, the candidate's
 *   norm first.
 * State.  Per entry pen = -inf, sum = +0; per list total = +0.
 * Selection, for t = 0, 1, ... while t < k and an eligible entry is unpicked:
 *   q(e) = +0 when t == 0, otherwise q(e) = -(oml * pen(e)): one fp32 multiply, then an exact negation;
 *   v(e) = fmaf(lam, r(e), q(e));
 *   the pick is the unpicked eligible entry that comes first in the total order (NaN last, then v descending, then pool
 *   position ascending);
 *   items[x, t] = id, pos[x, t] = e, value[x, t] = v;  total = total + sum(pick), an fp32 add, in pick order;
 *   for every other unpicked eligible entry, with sim taken against the pick: pen = sim > pen ? sim : pen (a NaN sim never
 *   replaces pen); sum = sum + sim, an fp32 add.
 * Outputs.  items, pos int32 [n, k], value float [n, k]; n_sel[x] (int32 [n]) = the number of picks = min(k, eligible
 *   entries); sim_sum[x] (float [n]) = total, which the caller divides by m (m - 1) / 2 to get the intra-list similarity of
 *   the m picks.  Unused slots hold (-1, -1, -inf).  Every output is written.
 * Rounding rule.  Each named multiply, add and subtract is a single rounding: sum + sim does not fuse with sim's last
 *   multiply and oml * pen does not fuse into anything; the only fused operations are the fmaf calls named above.  This
 *   holds on the device and in the host walk alike.
 * Consequences.  With lam == 1 and normalize == 0 the picks are the pool in order of (rel descending, position ascending)
 *   and value holds rel's bits (oml is 0, so q is a zero as long as pen is finite; a rel of -0 may read +0): on a pool that a
 *   top-K call returned, items is the pool's first k columns byte for byte.
 *   With lam == 0 the first pick is the pool position of the first eligible entry.  The bytes are the same for every launch
 *   geometry: max_workgroups = 0 leaves the grid to the call, a positive value caps it (lists are walked grid-stride, one
 *   wavefront per list).  At d = 32 / 64 a call on fp16 tables equals the call on exact fp32 copies bit for bit.
 * Refused (sml_last_error): a (d, elem_bytes) pair without kernels; pool_cols, pool_stride or k out of range; lam outside
 *   [0, 1] or NaN; normalize not 0 / 1; max_workgroups < 0; a table that is not 16-byte aligned; an output that overlaps an
 *   input or another output as far as the pointers and the sizes show it.  n == 0 is a valid call that launches nothing.
 *   No allocation, no scratch, no copy to the host, no synchronise.  All pointers are device memory.  Asynchronous. */
int sml_rerank_mmr(sml_ctx* ctx, const void* w_item, int elem_bytes, int64_t n_item, const int32_t* pool_items,
                   const float* pool_rel, int64_t n, int pool_cols, int64_t pool_stride, const float* nrm, float lam,
                   int normalize, int k, int max_workgroups, int32_t* items, int32_t* pos, float* value, int32_t* n_sel,
                   float* sim_sum, void* stream);

/* ---- host helper: batch supply ------------------------------------------------------- */
/* Sequential rejection sampling of offlineDataset_withsample.__getitem__ (reference
 * data/dataset.py:63-71) over a pre-drawn candidate stream, on the HOST (no GPU involved):
 * element e takes candidates cand[ptr], cand[ptr+1], ... until one is not an item of user[e]
 * ((user,item) pairs given sorted as user*stride+item), exactly as the per-item loop consumes the
 * random stream.  *consumed = candidates used, *resolved = elements that got their negative; when
 * the stream runs out first (*resolved < n, *consumed == m) the caller continues from element
 * *resolved with the next draws.  Drawing exactly as many candidates as there are unresolved
 * elements per call therefore consumes the generator exactly as the per-item loop does. */
int sml_host_resolve_negatives(const int64_t* users, int64_t n, const int64_t* cand, int64_t m,
                               const int64_t* pairs_sorted, int64_t n_pairs, int64_t stride,
                               int64_t* negs, int64_t* consumed, int64_t* resolved);

/* The same walk with the users' items in CSR form (user_ptr int64 [n_users + 1] into user_items, each user's
 * items ascending): two memory touches per candidate instead of a 17-step bisection of the pair list. */
/* Host-side gathers of the same batch supply: out3 is the epoch's int64 [n,3] triple array.  gather_pairs: columns 0, 1 <-
 * ui[order[e]] (ui = contiguous int64 [n_rows,2]); gather_column: column out_col <- element `col` of row order[e] of a
 * row-major integer matrix (elem_bytes 4 or 8).  data/dataset2.py:172-201 (pre-sampled column), data/dataset.py:41-71. */
int sml_host_gather_pairs(const int64_t* ui, int64_t n_rows, const int64_t* order, int64_t n, int64_t* out3);
int sml_host_gather_column(const void* mat, int64_t n_rows, int64_t row_stride_bytes, int elem_bytes, int64_t col,
                           const int64_t* order, int64_t n, int64_t* out3, int out_col);
int sml_host_resolve_negatives_csr(const int64_t* users, int64_t n, const int64_t* cand, int64_t m,
                                   const int64_t* user_ptr, int64_t n_users, const int64_t* user_items,
                                   int64_t* negs, int64_t* consumed, int64_t* resolved);

/* sml_neg_sets (test-set negatives) over HOST memory: a single-threaded walk of the same definition, one candidate at a
 * time, drawing through the same candidate function as the kernel -- the same bytes in out and the same count in *failed
 * (host int32).  The route of a machine without a GPU. */
int sml_host_neg_sets(const int64_t* rows, int64_t n, int n_cols, int64_t g0, const int32_t* n_cat, const int32_t* order,
                      const int64_t* h_off, int64_t n_user, const int32_t* h_items, const int32_t* h_since, int neg_num, uint64_t seed,
                      int64_t* out, int32_t* failed);

/* sml_sample_negatives_ex (training negatives) over HOST memory: a single-threaded walk of the same definition, one
 * candidate at a time, drawing through the same functions as the kernels -- the same bytes in negs and score and the same
 * count in *failed (host int32).  The route of a machine without a GPU. */
int sml_host_sample_negatives_ex(const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop, const int64_t* user_ptr,
                                 int64_t n_users, const int64_t* user_items, const double* cdf, int pool, const float* w_user,
                                 const float* w_item, int d, uint64_t seed, int64_t* negs, float* score, int32_t* failed);

/* sml_rerank_mmr (re-ranking) over HOST memory: the single-threaded walk of the same definition, one entry at a time, built
 * from the same functions as the kernel -- the same bytes in every output, fp16 tables included (d is given since there is
 * no context).  The refusals are the kernel entry's.  The route of a machine without a GPU. */
int sml_host_rerank_mmr(const void* w_item, int elem_bytes, int d, int64_t n_item, const int32_t* pool_items,
                        const float* pool_rel, int64_t n, int pool_cols, int64_t pool_stride, const float* nrm, float lam,
                        int normalize, int k, int32_t* items, int32_t* pos, float* value, int32_t* n_sel, float* sim_sum);

/* ---- self test ------------------------------------------------------------------ */
/* Checks the MFMA operand/accumulator lane maps this library assumes against a
 * scalar loop on the device.  Synchronous.  Returns 0 if they hold. */
int sml_selftest(int device);

#ifdef __cplusplus
}
#endif
#endif /* SML_HIP_H */
