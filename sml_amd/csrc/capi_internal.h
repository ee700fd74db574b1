// What capi.hip (the context and the stateful training / evaluation / exchange drivers) and capi_ops.hip (the stateless
// operations) share: error reporting, the device guard, deferred frees, growing buffers, per-class timing, and the context.
#ifndef SML_CAPI_INTERNAL_H
#define SML_CAPI_INTERNAL_H
#include <hip/hip_runtime.h>
#ifdef SML_TEST_PREP_REFERENCE     // (test build only, tests/build_reference.py: the library-sort reference of the index preparation)
#include <hipcub/hipcub.hpp>
#endif
#include <rccl/rccl.h>      // types only: the functions are bound at run time from the loaded librccl

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sml_hip.h"
#include "sml_kernels.h"

// Everything but the context itself (the C ABI's `struct sml_ctx`) sits in a namespace of the library's own, and the two objects
// the files share are hidden: libsml_hip.so exports neither them nor a generic name another library could interpose.
namespace sml_capi {

__attribute__((visibility("hidden"))) extern thread_local std::string g_err;      // (defined in capi.hip, like g_graveyard below)

inline int fail(int code, const char* what, const char* detail) {
    g_err = std::string(what) + ": " + (detail ? detail : "");
    return code;
}
template <typename T> T zeroed() { T x; memset(&x, 0, sizeof(x)); return x; }     // (memset: padding bytes too -- the structs travel as kernel arguments)
#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) return fail(SML_EHIP, #expr, hipGetErrorString(_e));    \
    } while (0)

struct DevGuard {
    int prev = -1;
    bool changed = false;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~DevGuard() { if (changed) (void)hipSetDevice(prev); }
};

// Buffers that were outgrown are NOT freed on the spot: hipFree waits for the whole device, and on a device that
// another rank's kernel is polling on (peer exchange: a consumer spinning for THIS host thread's next launch) that wait
// never ends before the poller's time-out.  They are parked here and freed when a context is destroyed.
// The same holds for destroying a whole context (Python's garbage collector may finalise an old engine on ANY thread,
// e.g. inside a rank thread whose peer is polling -- found with a stack dump of a stalled thread-rank test): everything a
// context owns is parked, and the yard is emptied only while no context of the process has peer mappings attached.
struct Graveyard {
    std::vector<void*> dead, dead_host;
    std::vector<sml_ctx*> zombies;   // whole contexts whose destruction (RCCL communicator, events, frees) has to wait
    std::mutex mu;
    bool defer(sml_ctx* c) { std::lock_guard<std::mutex> g(mu); if (peers_live <= 0) return false; zombies.push_back(c); return true; }
    std::vector<sml_ctx*> take_zombies() { std::lock_guard<std::mutex> g(mu); std::vector<sml_ctx*> z; if (peers_live <= 0) z.swap(zombies); return z; }
    int peers_live = 0;          // contexts with peer mappings attached (their consumers may be polling on the device)
    void park(void* p) { if (p) { std::lock_guard<std::mutex> g(mu); dead.push_back(p); } }
    void park_host(void* p) { if (p) { std::lock_guard<std::mutex> g(mu); dead_host.push_back(p); } }
    void peers(int delta) { std::lock_guard<std::mutex> g(mu); peers_live += delta; }
    void reap() {
        std::vector<void*> d, h;
        { std::lock_guard<std::mutex> g(mu); if (peers_live > 0) return; d.swap(dead); h.swap(dead_host); }
        for (void* p : d) (void)hipFree(p);
        for (void* p : h) (void)hipHostFree(p);
    }
};
__attribute__((visibility("hidden"))) extern Graveyard g_graveyard;

// A device buffer that grows on demand.  Whoever declares one owns it: the destructor parks the pointer (never hipFree on the
// spot, for the reasons above), so no owner keeps a list of its buffers to release -- and none can be copied by accident.
template <typename T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { g_graveyard.park(p); }
    hipError_t ensure(size_t need) {
        if (need <= cap) return hipSuccess;
        if (p) { g_graveyard.park(p); p = nullptr; cap = 0; }
        size_t want = need + need / 8;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
        if (e != hipSuccess) return e;
        cap = want;
        return hipSuccess;
    }
};

// ---- optional per-kernel-class timing with HIP events on the caller's stream -------------
enum ProfClass { PC_FWD = 0, PC_BWD, PC_WGRAD, PC_THETA_ADAM, PC_PAIR_LOSS /* hot-row kernels */, PC_SEG_ADAM, PC_SEG_SGD, PC_BARE_GRAD,
                 PC_EVAL_RANKS, PC_FLUSH, PC_PACK, PC_SORT, PC_MISC, PC_FWD_SIDE, PC_COUNT };
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;     // pairs
    std::vector<int> cls;
    size_t used = 0;                // pairs in flight
    double total_ms[PC_COUNT] = {0};
    int64_t count[PC_COUNT] = {0};
    static constexpr size_t kPairs = 4096;
    int64_t lost = 0;               // pairs whose elapsed time could not be read (reported by sml_prof_get's caller as missing)
    void drain() {
        if (!used) return;
        // the ring is shared by every stream the context is used on (training stream, side-stream evaluations):
        // wait for EACH pair's end event, not just the newest one
        for (size_t i = 0; i < used; ++i) {
            float ms = 0.f;
            (void)hipEventSynchronize(ev[2 * i + 1]);
            if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { total_ms[cls[i]] += ms; count[cls[i]]++; }
            else ++lost;
        }
        used = 0;
    }
    void begin(int c, hipStream_t st) {
        if (!on) return;
        if (ev.empty()) { ev.resize(2 * kPairs); cls.resize(kPairs); for (auto& e : ev) (void)hipEventCreate(&e); }
        if (used == kPairs) drain();
        cls[used] = c;
        (void)hipEventRecord(ev[2 * used], st);
    }
    void end(hipStream_t st) {
        if (!on) return;
        (void)hipEventRecord(ev[2 * used + 1], st);
        ++used;
    }
    void release() { drain(); for (auto& e : ev) (void)hipEventDestroy(e); ev.clear(); }
};
// `body` (statements; every launch in it under its own HIPCHK) timed as ONE pair of profile class `cls` on stream `st` of `ctx`.
// A failed launch returns from the function between the two: no end event is recorded on a failing stream (so no scope object).
#define PROFILED(cls, ...) do { ctx->prof.begin(cls, st); __VA_ARGS__; ctx->prof.end(st); } while (0)

// sorted occurrence lists and run records of one epoch (two sets: one may be prepared on a side
// stream while the other is in use).  Keys are uint32 ((batch << row_bits) | row) when that fits,
// else uint64 ((batch << 32) | row); the key buffers are sized for the wider form.
struct IndexSet {
    Buf<uint64_t> key_u, key_u2, key_i, key_i2;
    Buf<uint32_t> val_u2, val_i2;      // values (slots) in sorted order
    Buf<SmlRun> rec_u, rec_i;          // one record per sorted position
    Buf<SmlRun> runs_u, runs_i;        // compacted: duplicated runs only (bare step)
    Buf<uint32_t> hot_list;            // [nb][hot_cap][3] hot runs of every batch (bare step, large batches)
    Buf<int> hot_count;                // [nb]
    int hot_cap = 0;                   // 0: the hot-row path is off for this epoch's batch size
    Buf<uint8_t> uniq;
    Buf<uint32_t> slot_info;           // records mode, by hand: per slot, "once" or the position of its run's record (SmlFusedUpdate)
    int64_t slot_stride = 0;           // ... slots per batch; 0: this set has none
    int64_t dense_stride = 0;          // distinct-row records per batch (whole tiles of both lists)
    // MF stage, distinct-row form (SmlDense): records by scratch row, distinct rows per (batch, table), per-tile headers / entry blocks / spill
    Buf<SmlRun> dense_rec; Buf<int> dense_n; Buf<SmlTileHdr> tile_hdr; Buf<uint2> tile_ent, tile_spill; Buf<int> spill_cnt;
    bool dense = false; int tiles_cap = 0;
    Buf<int> off_u, off_i, n_sel;
    // index_prep.hip (the by-hand preparation): tile histograms, bucket offsets, run counts, oversized buckets
    Buf<uint32_t> hist_u, hist_i, bko_u, bko_i, large, medium;
    Buf<int> cnt_u, cnt_i;
    Buf<int> rank_viol;      // [0]: lanes the start-up probe found served out of lane order by a returning LDS atomic (wave_rank)
    bool rank_probed = false;
    bool by_hand = false;              // the lists were built by index_prep.hip: a batch's runs are off[b] .. off[b] + cnt[b]
#ifdef SML_TEST_PREP_REFERENCE         // what only the library-sort reference (tests/csrc/prep_cub_reference.inc) uses
    Buf<uint32_t> val_u, val_i;        // values in occurrence order, the sort's input
    Buf<uint32_t> heads_u, heads_i;    // sorted positions of the duplicated-run heads
    Buf<char> cub_tmp;
    int key_bytes = 8, row_bits_u = 32, row_bits_i = 32;
#endif
    int* viol_host = nullptr;          // pinned: entries emit_bucket found out of (row, value) order, ever (SmlPrepArgs.order_viol)
    hipEvent_t viol_ready = nullptr;
    int* max_len_host = nullptr;       // pinned: longest duplicated run of the prepared epoch (0 if none exceeds SML_HOT)
    int* lists_host = nullptr;         // pinned, compact lists by hand: [off_u (nb+1)][off_i (nb+1)][cnt_u (nb*STRIDE)][cnt_i (nb*STRIDE)] -- the
    int64_t lists_host_nb = 0, lists_nb = 0;   // (capacity; batches of the prepared epoch, 0: not read back) batches' places in the run lists, read back with max_len (same event): the run kernel then needs no offset / count loads
    hipEvent_t ready = nullptr;        // recorded after the copy into max_len_host
    int64_t n = -1; int batch = 0; const void* triples = nullptr; int world = 1;   // what was prepared here
    void release() {                   // what is not a Buf: the pinned blocks and the events
        if (max_len_host) { g_graveyard.park_host(max_len_host); max_len_host = nullptr; }
        if (viol_host) { g_graveyard.park_host(viol_host); viol_host = nullptr; }
        if (viol_ready) { (void)hipEventDestroy(viol_ready); viol_ready = nullptr; }
        if (lists_host) { g_graveyard.park_host(lists_host); lists_host = nullptr; lists_host_nb = 0; }
        if (ready) { (void)hipEventDestroy(ready); ready = nullptr; }
    }
};

struct SchedRetired { SmlSched* dev; SmlSched* host; hipEvent_t done; };

}  // namespace sml_capi
using namespace sml_capi;

struct sml_ctx {
    int device = 0, d = 32, max_batch = 0;
    int variant = 0;         // 0: ConvTransfer_com, 1: ConvTransfer (sml_ctx_set_variant)
    bool side = false;       // an evaluation-stream context (sml_ctx_set_variant, bit 1): its table-sized forwards run under their own name / class
    float clip_max_norm = 0.0f;   // > 0: the TR stage clips the theta gradient's norm (sml_ctx_set_grad_clip)
    float adaptive_beta = 0.0f;   // > 0: the MF stage adds the reference's --need_adaptive user-norm term (sml_ctx_set_adaptive)
    Buf<float> clip_sumsq;
    IndexSet ix[2];
    // transfer-net workspaces, 3*B slots each
    Buf<float> out, dout, dx, xin, z1, a1, a2, dz1, mrep, vrep;
    Buf<float> pk, grad, convg, loss_part;
    Buf<float> pkx;          // bf16x3 operand images of the table-sized forward (both nets)
    Buf<float> cstate;       // [2 parities][2 nets][3][SML_CG]: the conv parameters' working copy of a TR epoch (deferred conv step)
    int pk_set = 0;          // which of the two operand-image sets is current
    Buf<int> arrive;         // k_tr_wgrad2's tail-workgroup arrival counter (0 between launches)
    Buf<int> run_arrive;     // MF stage, fused row update: per-run arrival counters of a batch (0 between launches)
    // Adam schedule of the MF optimiser
    Buf<SmlSched> sched;
    int sched_len = 0;
    float sched_lr = -1.0f;
    std::vector<SchedRetired> sched_retired;     // replaced schedule tables / their pinned sources, freed once idle
    hipEvent_t sched_ready = nullptr;            // behind the newest table's upload
    hipStream_t sched_stream = nullptr;
    Buf<SmlRun> rec_x;       // run records of the multi-GPU global item list (caller-sorted keys)
    Buf<int32_t> xoff;       // ... and, for lists the library builds itself, the batches' offsets in the occurrence stream
    ncclComm_t comm = nullptr;
    int comm_world = 1, comm_rank = 0;
    // one-shot exchange over peer mappings (sml_peer_attach): world == 0 means detached
    struct Peer {
        int world = 0, rank = 0;
        char* inbox[SML_MAX_PEERS] = {nullptr};
        unsigned long long* flags[SML_MAX_PEERS] = {nullptr};
        int64_t theta_slot = 0;          // floats per (parity, source) theta slot
        int64_t rows_cap = 0;            // rows per (parity, source) row slot
        int64_t tick[3] = {0, 0, 0};     // exchanges done, per kind (0: theta / dense head, 1: rows, 2: "owner has updated")
        unsigned long long expect[3][2] = {{0, 0}, {0, 0}, {0, 0}};   // [kind][parity]: counter value after the last push
        bool done_pending = false;       // sharded bare step: the last batch's "owner done" round has not been waited for yet
        SmlPeerPoll done_poll;
        long long timeout = 0;           // 100 MHz ticks
        int* err = nullptr;              // device: incidents
    } peer;
    Buf<int> hot_first;
    Buf<float> hot_part;
    Buf<float> head_part;    // sharded bare step: this rank's dense [head_rows, d] gradient partial
    Buf<void*> ptr_tab;      // sharded bare step: [0..8) shard pointers, [8..16) inbox bases (device table, per-lane indexed)
    Prof prof;

    void release_all() {               // what is not a Buf (those park themselves when the context is deleted)
        prof.release();
        ix[0].release(); ix[1].release();
        for (auto& r : sched_retired) { g_graveyard.park(r.dev); g_graveyard.park_host(r.host); (void)hipEventDestroy(r.done); }
        sched_retired.clear();
        if (sched_ready) { (void)hipEventDestroy(sched_ready); sched_ready = nullptr; }
        if (peer.err) { g_graveyard.park(peer.err); peer.err = nullptr; }
    }
};

#endif
