// C ABI of libsml_hip.so (see include/sml_hip.h), the stateless operations: each needs the context's d, device and profile only.
// One argument check, one launch (or one host walk); no state survives a call.  The context and the training drivers: capi.hip.
#include <cmath>
#include <cstdint>

#include "capi_internal.h"

namespace {

// The bytes of one argument as far as the call's arguments give them: an array whose extent only the device knows counts from its
// first entry (4 or 8 bytes).  A null pointer or a length <= 0 overlaps nothing.
struct Span { const void* p; int64_t bytes; };

bool spans_overlap(const Span& a, const Span& b) {
    const char *p = (const char*)a.p, *q = (const char*)b.p;
    return p && q && a.bytes > 0 && b.bytes > 0 && p < q + b.bytes && q < p + a.bytes;
}

// The one overlap check: `out_in` if an output overlaps an input; failing that, `out_out` if two outputs overlap each other
// (NULL: this caller's outputs are not compared); NULL if nothing was found.  Each caller supplies its own two messages.
template <int NI, int NO>
const char* overlap_refusal(const Span (&in)[NI], const Span (&out)[NO], const char* out_in, const char* out_out) {
    for (const Span& o : out)
        for (const Span& i : in)
            if (spans_overlap(o, i)) return out_in;
    for (int a = 0; out_out && a < NO; ++a)
        for (int b = a + 1; b < NO; ++b)
            if (spans_overlap(out[a], out[b])) return out_out;
    return nullptr;
}
const char* const kOutIn = "an output overlaps an input";
const char* const kOutOut = "the outputs overlap each other";

bool count_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31); }      // 0 <= n < 2^31
bool size_ok(int64_t n) { return n > 0 && n < ((int64_t)1 << 31); }        // 0 < n < 2^31
bool elem_ok(int elem_bytes) { return elem_bytes == 4 || elem_bytes == 2; }

}  // namespace

extern "C" {

// ---- full-catalogue retrieval (retrieval.hip) ----------------------------------------------------------------------

// Every table-reading entry point fills a catalogue (sml_kernels.h) and makes one call.  elem_bytes: 4 for the fp32 entry points
// (d = 32 / 64), 2 for the _f16 ones (d = 32 / 64 / 128), the caller's for the _adjusted ones; allow / adj: NULL where the form
// has none.  The refusals they share, in order: with_adj (the _adjusted forms: adj is required) a bad elem_bytes, a null or
// misaligned adj; then the common arguments and the operation's own ranges (own_ok; `ranges` names them all).  c.d: the context's
static int catalogue_ok(const char* what, sml_ctx* ctx, SmlCatalogue& c, bool with_adj, bool own_ok, const char* ranges) {
    if (with_adj && !elem_ok(c.elem_bytes)) return fail(SML_EINVAL, what, "bad argument (elem_bytes must be 4 or 2)");
    if (with_adj && (!c.adj || ((uintptr_t)c.adj & 15))) return fail(SML_EINVAL, what, "adj must be non-null and 16-byte aligned");
    if (!ctx || !sml_retrieval_supports(ctx->d, c.elem_bytes) || !size_ok(c.n_item) || (!c.seen_off) != (!c.seen_items) || !own_ok)
        return fail(SML_EINVAL, what, ranges);
    c.d = ctx->d;
    return SML_OK;
}

static int full_rank_impl(const char* what, sml_ctx* ctx, SmlCatalogue c, bool with_adj, const int64_t* rows, int64_t n, int n_cols,
                          int32_t* rank, void* stream) {
    if (int rc = catalogue_ok(what, ctx, c, with_adj, n_cols >= 2 && n >= 0,
                              "bad argument (d must be 32/64, or 128 for fp16 tables; 0 < n_item < 2^31, n_cols >= 2, seen_off and seen_items both or neither)"))
        return rc;
    if (n == 0) return SML_OK;
    if (!c.wu || !c.wi || !rows || !rank) return fail(SML_EINVAL, what, "null argument");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_full_rank(c, rows, n, n_cols, rank, st)));
    return SML_OK;
}

int sml_full_rank(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item, const int64_t* rows, int64_t n,
                  int n_cols, const int64_t* seen_off, const int32_t* seen_items, int32_t* rank, void* stream) {
    return full_rank_impl("sml_full_rank", ctx, {0, 4, w_user, w_item, n_item, seen_off, seen_items}, false, rows, n, n_cols, rank, stream);
}

int sml_full_rank_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item, const int64_t* rows, int64_t n,
                      int n_cols, const int64_t* seen_off, const int32_t* seen_items, int32_t* rank, void* stream) {
    return full_rank_impl("sml_full_rank_f16", ctx, {0, 2, w_user, w_item, n_item, seen_off, seen_items}, false, rows, n, n_cols, rank, stream);
}

int sml_full_rank_filtered(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item, const int64_t* rows, int64_t n,
                           int n_cols, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, int32_t* rank,
                           void* stream) {
    return full_rank_impl("sml_full_rank_filtered", ctx, {0, 4, w_user, w_item, n_item, seen_off, seen_items, allow}, false, rows, n, n_cols, rank,
                          stream);
}

int sml_full_rank_filtered_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item, const int64_t* rows, int64_t n,
                               int n_cols, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, int32_t* rank,
                               void* stream) {
    return full_rank_impl("sml_full_rank_filtered_f16", ctx, {0, 2, w_user, w_item, n_item, seen_off, seen_items, allow}, false, rows, n, n_cols,
                          rank, stream);
}

int64_t sml_topk_scratch_bytes(sml_ctx* ctx, int64_t n, int k, int64_t n_item) {
    if (!ctx || n < 0 || k < 1 || k > 128 || !size_ok(n_item)) return fail(SML_EINVAL, "sml_topk_scratch_bytes", "bad argument");
    return n == 0 ? 0 : sml_topk_scratch_size(n, k, n_item);
}

static int topk_items_impl(const char* what, sml_ctx* ctx, SmlCatalogue c, bool with_adj, const int64_t* users, int64_t n, int k,
                           void* scratch, int32_t* items, float* scores, void* stream) {
    if (int rc = catalogue_ok(what, ctx, c, with_adj, k >= 1 && k <= 128 && n >= 0,
                              "bad argument (d must be 32/64, or 128 for fp16 tables; 1 <= k <= 128, 0 < n_item < 2^31, seen_off and seen_items both or neither)"))
        return rc;
    if (n == 0) return SML_OK;
    if (!c.wu || !c.wi || !users || !scratch || !items || !scores) return fail(SML_EINVAL, what, "null argument");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_topk(c, users, n, k, scratch, items, scores, st)));
    return SML_OK;
}

int sml_topk_items(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item, const int64_t* users, int64_t n, int k,
                   const int64_t* seen_off, const int32_t* seen_items, void* scratch, int32_t* items, float* scores, void* stream) {
    return topk_items_impl("sml_topk_items", ctx, {0, 4, w_user, w_item, n_item, seen_off, seen_items}, false, users, n, k, scratch, items, scores,
                           stream);
}

int sml_topk_items_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item, const int64_t* users, int64_t n, int k,
                       const int64_t* seen_off, const int32_t* seen_items, void* scratch, int32_t* items, float* scores, void* stream) {
    return topk_items_impl("sml_topk_items_f16", ctx, {0, 2, w_user, w_item, n_item, seen_off, seen_items}, false, users, n, k, scratch, items,
                           scores, stream);
}

int sml_topk_items_filtered(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item, const int64_t* users, int64_t n, int k,
                            const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, void* scratch, int32_t* items,
                            float* scores, void* stream) {
    return topk_items_impl("sml_topk_items_filtered", ctx, {0, 4, w_user, w_item, n_item, seen_off, seen_items, allow}, false, users, n, k, scratch,
                           items, scores, stream);
}

int sml_topk_items_filtered_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item, const int64_t* users, int64_t n, int k,
                                const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, void* scratch, int32_t* items,
                                float* scores, void* stream) {
    return topk_items_impl("sml_topk_items_filtered_f16", ctx, {0, 2, w_user, w_item, n_item, seen_off, seen_items, allow}, false, users, n, k,
                           scratch, items, scores, stream);
}

int64_t sml_user_rank_scratch_bytes(sml_ctx* ctx, int64_t n, int64_t n_pos, int64_t n_item) {
    if (!ctx || !count_ok(n) || !count_ok(n_pos) || !size_ok(n_item))
        return fail(SML_EINVAL, "sml_user_rank_scratch_bytes", "bad argument");
    return n == 0 || n_pos == 0 ? 0 : sml_user_rank_scratch_size(n_pos);
}

static int user_rank_impl(const char* what, sml_ctx* ctx, SmlCatalogue c, bool with_adj, const int64_t* users, int64_t n,
                          const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos, void* scratch, int32_t* above, int32_t* pos,
                          void* stream) {
    if (int rc = catalogue_ok(what, ctx, c, with_adj, count_ok(n) && count_ok(n_pos),
                              "bad argument (d must be 32/64, or 128 for fp16 tables; 0 < n_item < 2^31, 0 <= n, n_pos < 2^31, seen_off and seen_items both or neither)"))
        return rc;
    if (n == 0 || n_pos == 0) return SML_OK;
    if (!c.wu || !c.wi || !users || !pos_off || !pos_items || !scratch || !above || !pos)
        return fail(SML_EINVAL, what, "null argument");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_user_rank(c, users, n, pos_off, pos_items, n_pos, scratch, above, pos, st)));
    return SML_OK;
}

int sml_user_rank(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item, const int64_t* users, int64_t n,
                  const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos, const int64_t* seen_off,
                  const int32_t* seen_items, void* scratch, int32_t* above, int32_t* pos, void* stream) {
    return user_rank_impl("sml_user_rank", ctx, {0, 4, w_user, w_item, n_item, seen_off, seen_items}, false, users, n, pos_off, pos_items, n_pos,
                          scratch, above, pos, stream);
}

int sml_user_rank_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item, const int64_t* users, int64_t n,
                      const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos, const int64_t* seen_off,
                      const int32_t* seen_items, void* scratch, int32_t* above, int32_t* pos, void* stream) {
    return user_rank_impl("sml_user_rank_f16", ctx, {0, 2, w_user, w_item, n_item, seen_off, seen_items}, false, users, n, pos_off, pos_items, n_pos,
                          scratch, above, pos, stream);
}

int sml_user_rank_filtered(sml_ctx* ctx, const float* w_user, const float* w_item, int64_t n_item, const int64_t* users, int64_t n,
                           const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos, const int64_t* seen_off,
                           const int32_t* seen_items, const uint32_t* allow, void* scratch, int32_t* above, int32_t* pos, void* stream) {
    return user_rank_impl("sml_user_rank_filtered", ctx, {0, 4, w_user, w_item, n_item, seen_off, seen_items, allow}, false, users, n, pos_off,
                          pos_items, n_pos, scratch, above, pos, stream);
}

int sml_user_rank_filtered_f16(sml_ctx* ctx, const void* w_user, const void* w_item, int64_t n_item, const int64_t* users, int64_t n,
                               const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos, const int64_t* seen_off,
                               const int32_t* seen_items, const uint32_t* allow, void* scratch, int32_t* above, int32_t* pos,
                               void* stream) {
    return user_rank_impl("sml_user_rank_filtered_f16", ctx, {0, 2, w_user, w_item, n_item, seen_off, seen_items, allow}, false, users, n, pos_off,
                          pos_items, n_pos, scratch, above, pos, stream);
}

// the adjusted score A(u, i) = fmaf(S(u, i), scale[i], offset[i]): one entry point per operation serves both element types
int sml_full_rank_adjusted(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* rows,
                           int64_t n, int n_cols, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow,
                           const float* adj, int32_t* rank, void* stream) {
    return full_rank_impl("sml_full_rank_adjusted", ctx, {0, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj}, true, rows, n,
                          n_cols, rank, stream);
}

int sml_topk_items_adjusted(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* users,
                            int64_t n, int k, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                            void* scratch, int32_t* items, float* scores, void* stream) {
    return topk_items_impl("sml_topk_items_adjusted", ctx, {0, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj}, true, users, n,
                           k, scratch, items, scores, stream);
}

int sml_user_rank_adjusted(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* users,
                           int64_t n, const int64_t* pos_off, const int32_t* pos_items, int64_t n_pos, const int64_t* seen_off,
                           const int32_t* seen_items, const uint32_t* allow, const float* adj, void* scratch, int32_t* above, int32_t* pos,
                           void* stream) {
    return user_rank_impl("sml_user_rank_adjusted", ctx, {0, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj}, true, users, n,
                          pos_off, pos_items, n_pos, scratch, above, pos, stream);
}

// per-user candidate lists: allow and adj are both optional here (adj == NULL: the bare score, no fmaf)
int sml_topk_candidates(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* users, int64_t n,
                        const void* cand, int cand_elem_bytes, const int64_t* cand_off, int64_t cand_stride, int64_t cand_first,
                        int64_t cand_cols, int k, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj,
                        int max_workgroups, int32_t* items, float* scores, int32_t* n_elig, void* stream) {
    const char* what = "sml_topk_candidates";
    SmlCatalogue c = {0, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj};
    if (!elem_ok(elem_bytes)) return fail(SML_EINVAL, what, "bad argument (elem_bytes must be 4 or 2)");
    if (adj && ((uintptr_t)adj & 15)) return fail(SML_EINVAL, what, "adj must be 16-byte aligned");
    if (cand_elem_bytes != 4 && cand_elem_bytes != 8) return fail(SML_EINVAL, what, "bad argument (cand_elem_bytes must be 4 or 8)");
    if (!cand_off && (cand_stride < 0 || cand_first < 0 || cand_cols < 0))
        return fail(SML_EINVAL, what, "bad argument (dense candidates: cand_stride, cand_first and cand_cols must not be negative)");
    if (int rc = catalogue_ok(what, ctx, c, false, k >= 1 && k <= 128 && n >= 0 && max_workgroups >= 0,
                              "bad argument (d must be 32/64, or 128 for fp16 tables; 1 <= k <= 128, 0 < n_item < 2^31, n >= 0, max_workgroups >= 0, seen_off and seen_items both or neither)"))
        return rc;
    if (n == 0) return SML_OK;
    const bool empty = !cand_off && cand_cols == 0;              // dense lists of no columns: cand is never read
    if (!w_user || !w_item || !users || (!cand && !empty) || !items || !scores) return fail(SML_EINVAL, what, "null argument");
    if (((uintptr_t)w_user | (uintptr_t)w_item) & 15) return fail(SML_EINVAL, what, "the tables must be 16-byte aligned");
    // the inputs' extents as far as the arguments give them: a ragged cand and the tables of unknown height count from their
    // first byte only
    const int64_t out_bytes = 4 * n * (int64_t)k;
    const int64_t cand_bytes = cand_off ? cand_elem_bytes : ((n - 1) * cand_stride + cand_first + cand_cols) * cand_elem_bytes;
    const int64_t n_pad = sml_item_adjust_pad(n_item);
    const Span in[] = {{users, 8 * n}, {cand, cand_bytes}, {cand_off, 8 * (n + 1)}, {w_user, (int64_t)ctx->d * elem_bytes},
                       {w_item, n_item * ctx->d * elem_bytes}, {seen_off, 8}, {seen_items, 4}, {allow, n_pad / 8}, {adj, 8 * n_pad}};
    const Span out[] = {{items, out_bytes}, {scores, out_bytes}, {n_elig, 4 * n}};
    if (const char* why = overlap_refusal(in, out, kOutIn, kOutOut)) return fail(SML_EINVAL, what, why);
    const SmlCandidates l = {cand, cand_elem_bytes, cand_off, cand_stride, cand_first, cand_cols};
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_topk_candidates(c, users, n, l, k, max_workgroups, items, scores, n_elig, st)));
    return SML_OK;
}

// clustered index: what sml_ivf_search and sml_host_ivf_search refuse alike (NULL: nothing), in sml_topk_candidates' order.  The
// tables, the lists and Seen are of unknown extent: they count from their first entry only
static const char* ivf_search_refusal(int d, int elem_bytes, const void* w_user, const void* w_item, int64_t n_item, const int64_t* users,
                                      int64_t n, const int64_t* list_off, const int32_t* list_items, int n_list, const int32_t* probes,
                                      int nprobe, int k, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow,
                                      const float* adj, int max_workgroups, const int32_t* items, const float* scores, const int32_t* n_elig) {
    if (!elem_ok(elem_bytes)) return "bad argument (elem_bytes must be 4 or 2)";
    if (nprobe < 1 || nprobe > 128) return "bad argument (1 <= nprobe <= 128)";
    if (n_list <= 0) return "bad argument (n_list must be positive)";
    if (!sml_retrieval_supports(d, elem_bytes) || !size_ok(n_item) || (!seen_off) != (!seen_items) || k < 1 || k > 128 ||
        n < 0 || max_workgroups < 0)
        return "bad argument (d must be 32/64, or 128 for fp16 tables; 1 <= k <= 128, 0 < n_item < 2^31, n >= 0, max_workgroups >= 0, seen_off and seen_items both or neither)";
    if (n == 0) return nullptr;
    if (!w_user || !w_item || !users || !list_off || !list_items || !probes || !items || !scores) return "null argument";
    const int64_t out_bytes = 4 * n * (int64_t)k;
    const int64_t n_pad = sml_item_adjust_pad(n_item);
    const Span in[] = {{users, 8 * n}, {list_off, 8 * ((int64_t)n_list + 1)}, {list_items, 4}, {probes, 4 * n * (int64_t)nprobe},
                       {w_user, (int64_t)d * elem_bytes}, {w_item, n_item * d * elem_bytes}, {seen_off, 8}, {seen_items, 4},
                       {allow, n_pad / 8}, {adj, 8 * n_pad}};
    const Span out[] = {{items, out_bytes}, {scores, out_bytes}, {n_elig, 4 * n}};
    return overlap_refusal(in, out, kOutIn, kOutOut);
}

int sml_ivf_search(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* users, int64_t n,
                   const int64_t* list_off, const int32_t* list_items, int n_list, const int32_t* probes, int nprobe, int k,
                   const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj, int max_workgroups,
                   int32_t* items, float* scores, int32_t* n_elig, void* stream) {
    const char* what = "sml_ivf_search";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    if (adj && ((uintptr_t)adj & 15)) return fail(SML_EINVAL, what, "adj must be 16-byte aligned");
    if (const char* why = ivf_search_refusal(ctx->d, elem_bytes, w_user, w_item, n_item, users, n, list_off, list_items, n_list, probes, nprobe, k,
                                             seen_off, seen_items, allow, adj, max_workgroups, items, scores, n_elig))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    if (((uintptr_t)w_user | (uintptr_t)w_item) & 15) return fail(SML_EINVAL, what, "the tables must be 16-byte aligned");
    const SmlCatalogue c = {ctx->d, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj};
    const SmlIvfLists l = {list_off, list_items, n_list, probes, nprobe};
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_ivf_search(c, users, n, l, k, max_workgroups, items, scores, n_elig, st)));
    return SML_OK;
}

int sml_host_ivf_search(const void* w_user, const void* w_item, int elem_bytes, int d, int64_t n_item, const int64_t* users, int64_t n,
                        const int64_t* list_off, const int32_t* list_items, int n_list, const int32_t* probes, int nprobe, int k,
                        const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj, int32_t* items,
                        float* scores, int32_t* n_elig) {
    const char* what = "sml_host_ivf_search";
    if (const char* why = ivf_search_refusal(d, elem_bytes, w_user, w_item, n_item, users, n, list_off, list_items, n_list, probes, nprobe, k,
                                             seen_off, seen_items, allow, adj, 0, items, scores, n_elig))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    const SmlCatalogue c = {d, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj};
    const SmlIvfLists l = {list_off, list_items, n_list, probes, nprobe};
    if (!sml_ivf_host_walk(c, users, n, l, k, items, scores, n_elig)) return fail(SML_EINVAL, what, "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

// the centroid update: what the device call and the host walk refuse alike (NULL: nothing).  centroids_in == centroids_out is the
// in-place call; any other overlap of the two, or of the output with the table or the lists, is refused
static const char* ivf_centroids_refusal(int d, int elem_bytes, const void* w_item, int64_t n_item, const int64_t* list_off,
                                         const int32_t* list_items, int n_list, const void* cin, const void* cout) {
    if (!elem_ok(elem_bytes)) return "bad argument (elem_bytes must be 4 or 2)";
    if (!sml_retrieval_supports(d, elem_bytes) || !size_ok(n_item) || n_list <= 0)
        return "bad argument (d must be 32/64, or 128 for fp16 tables; 0 < n_item < 2^31, n_list > 0)";
    if (!w_item || !list_off || !list_items || !cin || !cout) return "null argument";
    const int64_t cb = (int64_t)n_list * d * elem_bytes;
    if (cin != cout && spans_overlap({cin, cb}, {cout, cb})) return "centroids_in and centroids_out overlap without being the same array";
    const Span in[] = {{w_item, n_item * d * elem_bytes}, {list_off, 8 * ((int64_t)n_list + 1)}, {list_items, 4 * n_item}};
    const Span out[] = {{cout, cb}};
    return overlap_refusal(in, out, kOutIn, nullptr);
}

int sml_ivf_centroids(sml_ctx* ctx, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* list_off, const int32_t* list_items,
                      int n_list, const void* centroids_in, void* centroids_out, void* stream) {
    const char* what = "sml_ivf_centroids";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    if (const char* why = ivf_centroids_refusal(ctx->d, elem_bytes, w_item, n_item, list_off, list_items, n_list, centroids_in, centroids_out))
        return fail(SML_EINVAL, what, why);
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_ivf_centroids(ctx->d, elem_bytes, w_item, list_off, list_items, n_list, centroids_in, centroids_out, st)));
    return SML_OK;
}

int sml_host_ivf_centroids(const void* w_item, int elem_bytes, int d, int64_t n_item, const int64_t* list_off, const int32_t* list_items,
                           int n_list, const void* centroids_in, void* centroids_out) {
    const char* what = "sml_host_ivf_centroids";
    if (const char* why = ivf_centroids_refusal(d, elem_bytes, w_item, n_item, list_off, list_items, n_list, centroids_in, centroids_out))
        return fail(SML_EINVAL, what, why);
    if (!sml_ivf_centroids_host_walk(d, elem_bytes, w_item, list_off, list_items, n_list, centroids_in, centroids_out))
        return fail(SML_EINVAL, what, "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

// fold-in: what the device calls and the host walks refuse alike (NULL: nothing)
static const char* gram_refusal(int d, int elem_bytes, const void* w, int64_t n_rows, const void* scratch, int64_t scratch_bytes, const double* gram,
                                bool device) {
    if (!sml_als_supports(d, elem_bytes)) return "bad argument (fp32 or fp16 tables of d = 32 / 64; d = 128 is out of scope)";
    if (!size_ok(n_rows)) return "bad argument (0 < n_rows < 2^31)";
    if (!w || !gram || (device && !scratch)) return "null argument";
    if (device && (((uintptr_t)scratch | (uintptr_t)gram) & 15)) return "scratch and gram must be 16-byte aligned";
    const int64_t gb = (int64_t)d * d * 8, wb = n_rows * d * elem_bytes;
    const Span in[] = {{w, wb}}, out[] = {{gram, gb}, {scratch, scratch_bytes}};
    const char* const why = "an output overlaps an input or the scratch";
    return overlap_refusal(in, out, why, why);
}

int64_t sml_gram_scratch_bytes(sml_ctx* ctx, int64_t n_rows) {
    if (!ctx || !size_ok(n_rows)) return fail(SML_EINVAL, "sml_gram_scratch_bytes", "bad argument (0 < n_rows < 2^31)");
    return sml_gram_chunks(n_rows) * ctx->d * ctx->d * 8;
}

int sml_gram(sml_ctx* ctx, const void* w, int elem_bytes, int64_t n_rows, void* scratch, double* gram, void* stream) {
    const char* what = "sml_gram";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    const int64_t sb = n_rows > 0 ? sml_gram_chunks(n_rows) * ctx->d * ctx->d * 8 : 0;
    if (const char* why = gram_refusal(ctx->d, elem_bytes, w, n_rows, scratch, sb, gram, true)) return fail(SML_EINVAL, what, why);
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_gram(ctx->d, elem_bytes, w, n_rows, (double*)scratch, gram, st)));
    return SML_OK;
}

int sml_host_gram(const void* w, int elem_bytes, int d, int64_t n_rows, double* gram) {
    const char* what = "sml_host_gram";
    if (const char* why = gram_refusal(d, elem_bytes, w, n_rows, nullptr, 0, gram, false)) return fail(SML_EINVAL, what, why);
    if (!sml_gram_host_walk(d, elem_bytes, w, n_rows, gram)) return fail(SML_EINVAL, what, "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

static const char* als_refusal(int d, int elem_bytes, const void* w_other, int64_t n_other, const double* gram, double alpha0, double reg,
                               const int64_t* set_off, const int32_t* set_items, const int64_t* rows, int64_t n, const void* w_out, int64_t n_out,
                               int max_workgroups, const int32_t* status, bool device) {
    if (!sml_als_supports(d, elem_bytes)) return "bad argument (fp32 or fp16 tables of d = 32 / 64; d = 128 is out of scope)";
    if (!(reg >= 0.0) || !(alpha0 >= 0.0)) return "bad argument (reg and alpha0 must be >= 0)";
    if (!size_ok(n_other) || !size_ok(n_out) || !count_ok(n))
        return "bad argument (0 < n_other < 2^31, 0 < n_out < 2^31, 0 <= n < 2^31)";
    if (max_workgroups < 0) return "bad argument (max_workgroups >= 0)";
    if ((!set_off) != (!set_items)) return "bad argument (set_off and set_items both or neither)";
    if (!gram && alpha0 != 0.0) return "bad argument (gram == NULL only with alpha0 == 0)";
    if (device && ((uintptr_t)gram & 15)) return "gram must be 16-byte aligned";
    if (n == 0) return nullptr;
    if (!w_other || !w_out || !status) return "null argument";
    const int64_t ob = n_out * d * elem_bytes;
    // w_out against the inputs and status; status against the five inputs only
    const Span in[] = {{w_other, n_other * d * elem_bytes}, {gram, (int64_t)d * d * 8}, {set_off, rows ? 8 : 8 * (n + 1)}, {set_items, 4},
                       {rows, 8 * n}};
    const Span wo[] = {{w_out, ob}}, st[] = {{status, 4 * n}};
    if (overlap_refusal(in, wo, kOutIn, nullptr) || spans_overlap(wo[0], st[0])) return "w_out overlaps an input or status";
    return overlap_refusal(in, st, "status overlaps an input", nullptr);
}

int sml_als_solve(sml_ctx* ctx, const void* w_other, int elem_bytes, int64_t n_other, const double* gram, double alpha0, double reg,
                  const int64_t* set_off, const int32_t* set_items, const int64_t* rows, int64_t n, void* w_out, int64_t n_out,
                  int max_workgroups, int32_t* status, void* stream) {
    const char* what = "sml_als_solve";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    if (const char* why = als_refusal(ctx->d, elem_bytes, w_other, n_other, gram, alpha0, reg, set_off, set_items, rows, n, w_out, n_out,
                                      max_workgroups, status, true))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_als_solve(ctx->d, elem_bytes, w_other, gram, alpha0, reg, set_off, set_items, rows, n, w_out,
                                                  max_workgroups, status, st)));
    return SML_OK;
}

int sml_host_als_solve(const void* w_other, int elem_bytes, int d, int64_t n_other, const double* gram, double alpha0, double reg,
                       const int64_t* set_off, const int32_t* set_items, const int64_t* rows, int64_t n, void* w_out, int64_t n_out,
                       int32_t* status) {
    const char* what = "sml_host_als_solve";
    if (const char* why = als_refusal(d, elem_bytes, w_other, n_other, gram, alpha0, reg, set_off, set_items, rows, n, w_out, n_out, 0, status,
                                      false))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    if (!sml_als_host_walk(d, elem_bytes, w_other, gram, alpha0, reg, set_off, set_items, rows, n, w_out, status))
        return fail(SML_EINVAL, what, "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

// neighbours: what the device calls and the host walks refuse alike (NULL: nothing).  The CSRs, Seen and the neighbour table's
// height are of unknown extent where the arguments do not give it: they count from their first entry only
// weighted: the call takes the users' weights user_w (required) in fixed point with frac_bits fractional bits
static const char* cooc_refusal(const SmlCooc& a, int max_workgroups, int path, const void* scratch, int64_t scratch_bytes, const int32_t* items,
                                const float* sims, const int32_t* n_elig, bool device, bool weighted = false, const float* user_w = nullptr,
                                int frac_bits = 0) {
    if (a.k < 1 || a.k > 128) return "bad argument (1 <= k <= 128)";
    if (a.min_co < 1) return "bad argument (min_co >= 1)";
    if (weighted && (frac_bits < 0 || frac_bits > 32)) return "bad argument (0 <= frac_bits <= 32)";
    if (weighted && !user_w) return "null argument";
    if (max_workgroups < 0 || path < 0 || path > 2) return "bad argument (max_workgroups >= 0, path 0 / 1 / 2)";
    if (!(a.shrink >= 0.0)) return "bad argument (shrink must be >= 0)";
    if ((!a.item_off) != (!a.item_users) || (!a.user_off) != (!a.user_items)) return "bad argument (a CSR's two pointers both or neither)";
    if ((!a.norm_a) != (!a.norm_b)) return "bad argument (norm_a and norm_b both or neither)";
    if (!size_ok(a.n_item) || !size_ok(a.n_user) || !count_ok(a.n))
        return "bad argument (0 < n_user < 2^31, 0 < n_item < 2^31, 0 <= n < 2^31)";
    if (device && ((uintptr_t)scratch & 255)) return "scratch must be 256-byte aligned";
    if (a.n == 0) return nullptr;
    if (!items || !sims || (device && !scratch) || (a.item_off && !a.user_off)) return "null argument";
    const int64_t ob = 4 * a.n * (int64_t)a.k;
    const Span in[] = {{a.item_off, 8 * (a.n_item + 1)}, {a.item_users, 4}, {a.user_off, 8 * (a.n_user + 1)}, {a.user_items, 4},
                          {a.rows, 8 * a.n}, {a.norm_a, 8 * a.n_item}, {a.norm_b, 8 * a.n_item}, {a.allow, (a.n_item + 31) / 32 * 4},
                          {user_w, 4 * a.n_user}};
    const Span out[] = {{items, ob}, {sims, ob}, {n_elig, 4 * a.n}, {scratch, scratch_bytes}};
    return overlap_refusal(in, out, kOutIn, kOutOut);
}

static const char* knn_refusal(const SmlKnn& a, int max_workgroups, int path, const void* scratch, int64_t scratch_bytes, const int32_t* items,
                               const float* scores, const int32_t* n_elig, bool device) {
    if (a.k < 1 || a.k > 128 || a.k_nbr < 1 || a.k_nbr > 128) return "bad argument (1 <= k <= 128, 1 <= k_nbr <= 128)";
    if (a.frac_bits < 0 || a.frac_bits > 32) return "bad argument (0 <= frac_bits <= 32)";
    if (max_workgroups < 0 || path < 0 || path > 2) return "bad argument (max_workgroups >= 0, path 0 / 1 / 2)";
    if ((!a.hist_off) != (!a.hist_items) || (!a.seen_off) != (!a.seen_items)) return "bad argument (a CSR's two pointers both or neither)";
    if (!size_ok(a.n_item) || !count_ok(a.n_rows_nbr) || !count_ok(a.n))
        return "bad argument (0 < n_item < 2^31, 0 <= n_rows_nbr < 2^31, 0 <= n < 2^31)";
    if (device && ((uintptr_t)scratch & 255)) return "scratch must be 256-byte aligned";
    if (a.n == 0) return nullptr;
    if (!items || !scores || (device && !scratch) || (a.n_rows_nbr > 0 && (!a.nbr_items || !a.nbr_sims))) return "null argument";
    const int64_t ob = 4 * a.n * (int64_t)a.k, nb = 4 * a.n_rows_nbr * (int64_t)a.k_nbr;
    const Span in[] = {{a.nbr_items, nb}, {a.nbr_sims, nb}, {a.hist_off, a.users ? 8 : 8 * (a.n + 1)}, {a.hist_items, 4},
                          {a.users, 8 * a.n}, {a.seen_off, a.users ? 8 : 8 * (a.n + 1)}, {a.seen_items, 4}, {a.allow, (a.n_item + 31) / 32 * 4}};
    const Span out[] = {{items, ob}, {scores, ob}, {n_elig, 4 * a.n}, {scratch, scratch_bytes}};
    return overlap_refusal(in, out, kOutIn, kOutOut);
}

int sml_knn_lds_limit(void) { return sml_knn_lds_entries(); }

int64_t sml_knn_scratch_bytes(sml_ctx* ctx, int64_t n_item, int max_workgroups, int kind) {
    if (!ctx || !size_ok(n_item) || max_workgroups < 0 || (kind != 0 && kind != 1))
        return fail(SML_EINVAL, "sml_knn_scratch_bytes", "bad argument (0 < n_item < 2^31, max_workgroups >= 0, kind 0 / 1)");
    return sml_knn_scratch_size(n_item, max_workgroups, kind);
}

int sml_cooc_topk(sml_ctx* ctx, const int64_t* by_item_off, const int32_t* by_item_users, const int64_t* by_user_off,
                  const int32_t* by_user_items, int64_t n_user, int64_t n_item, const int64_t* rows, int64_t n, const double* norm_a,
                  const double* norm_b, double shrink, int min_co, const uint32_t* allow, int k, int max_workgroups, int path, void* scratch,
                  int32_t* items, float* sims, int32_t* n_elig, void* stream) {
    const char* what = "sml_cooc_topk";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    const SmlCooc a = {by_item_off, by_item_users, by_user_off, by_user_items, n_user, n_item, rows, n, norm_a, norm_b, shrink, min_co, allow, k};
    const int64_t sb = size_ok(n_item) && max_workgroups >= 0 ? sml_knn_scratch_size(n_item, max_workgroups, 0) : 0;
    if (const char* why = cooc_refusal(a, max_workgroups, path, scratch, sb, items, sims, n_elig, true)) return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_cooc_topk(a, max_workgroups, path, scratch, items, sims, n_elig, st)));
    return SML_OK;
}

int sml_host_cooc_topk(const int64_t* by_item_off, const int32_t* by_item_users, const int64_t* by_user_off, const int32_t* by_user_items,
                       int64_t n_user, int64_t n_item, const int64_t* rows, int64_t n, const double* norm_a, const double* norm_b,
                       double shrink, int min_co, const uint32_t* allow, int k, int32_t* items, float* sims, int32_t* n_elig) {
    const char* what = "sml_host_cooc_topk";
    const SmlCooc a = {by_item_off, by_item_users, by_user_off, by_user_items, n_user, n_item, rows, n, norm_a, norm_b, shrink, min_co, allow, k};
    if (const char* why = cooc_refusal(a, 0, 0, nullptr, 0, items, sims, n_elig, false)) return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    sml_cooc_host_walk(a, items, sims, n_elig);
    return SML_OK;
}

int64_t sml_cooc_weighted_scratch_bytes(sml_ctx* ctx, int64_t n_item, int max_workgroups) {
    if (!ctx || !size_ok(n_item) || max_workgroups < 0)
        return fail(SML_EINVAL, "sml_cooc_weighted_scratch_bytes", "bad argument (0 < n_item < 2^31, max_workgroups >= 0)");
    return sml_cooc_weighted_scratch_size(n_item, max_workgroups);
}

int sml_cooc_topk_weighted(sml_ctx* ctx, const int64_t* by_item_off, const int32_t* by_item_users, const int64_t* by_user_off,
                           const int32_t* by_user_items, int64_t n_user, int64_t n_item, const int64_t* rows, int64_t n, const float* user_w,
                           int frac_bits, const double* norm_a, const double* norm_b, double shrink, const uint32_t* allow, int k,
                           int max_workgroups, int path, void* scratch, int32_t* items, float* sims, int32_t* n_elig, void* stream) {
    const char* what = "sml_cooc_topk_weighted";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    const SmlCooc c = {by_item_off, by_item_users, by_user_off, by_user_items, n_user, n_item, rows, n, norm_a, norm_b, shrink, 1, allow, k};
    const int64_t sb = size_ok(n_item) && max_workgroups >= 0 ? sml_cooc_weighted_scratch_size(n_item, max_workgroups) : 0;
    if (const char* why = cooc_refusal(c, max_workgroups, path, scratch, sb, items, sims, n_elig, true, true, user_w, frac_bits))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    const SmlCoocWeighted a = {by_item_off, by_item_users, by_user_off, by_user_items, n_user, n_item, rows, n, user_w, frac_bits,
                               norm_a, norm_b, shrink, allow, k};
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_cooc_topk_weighted(a, max_workgroups, path, scratch, items, sims, n_elig, st)));
    return SML_OK;
}

int sml_host_cooc_topk_weighted(const int64_t* by_item_off, const int32_t* by_item_users, const int64_t* by_user_off,
                                const int32_t* by_user_items, int64_t n_user, int64_t n_item, const int64_t* rows, int64_t n,
                                const float* user_w, int frac_bits, const double* norm_a, const double* norm_b, double shrink,
                                const uint32_t* allow, int k, int32_t* items, float* sims, int32_t* n_elig) {
    const char* what = "sml_host_cooc_topk_weighted";
    const SmlCooc c = {by_item_off, by_item_users, by_user_off, by_user_items, n_user, n_item, rows, n, norm_a, norm_b, shrink, 1, allow, k};
    if (const char* why = cooc_refusal(c, 0, 0, nullptr, 0, items, sims, n_elig, false, true, user_w, frac_bits))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    const SmlCoocWeighted a = {by_item_off, by_item_users, by_user_off, by_user_items, n_user, n_item, rows, n, user_w, frac_bits,
                               norm_a, norm_b, shrink, allow, k};
    sml_cooc_weighted_host_walk(a, items, sims, n_elig);
    return SML_OK;
}

int sml_knn_topk(sml_ctx* ctx, const int32_t* nbr_items, const float* nbr_sims, int64_t n_rows_nbr, int k_nbr, int64_t n_item,
                 const int64_t* hist_off, const int32_t* hist_items, const int64_t* users, int64_t n, int frac_bits, const int64_t* seen_off,
                 const int32_t* seen_items, const uint32_t* allow, int k, int max_workgroups, int path, void* scratch, int32_t* items,
                 float* scores, int32_t* n_elig, void* stream) {
    const char* what = "sml_knn_topk";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    const SmlKnn a = {nbr_items, nbr_sims, n_rows_nbr, k_nbr, n_item, hist_off, hist_items, users, n, frac_bits, seen_off, seen_items, allow, k};
    const int64_t sb = size_ok(n_item) && max_workgroups >= 0 ? sml_knn_scratch_size(n_item, max_workgroups, 1) : 0;
    if (const char* why = knn_refusal(a, max_workgroups, path, scratch, sb, items, scores, n_elig, true)) return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_knn_topk(a, max_workgroups, path, scratch, items, scores, n_elig, st)));
    return SML_OK;
}

int sml_host_knn_topk(const int32_t* nbr_items, const float* nbr_sims, int64_t n_rows_nbr, int k_nbr, int64_t n_item, const int64_t* hist_off,
                      const int32_t* hist_items, const int64_t* users, int64_t n, int frac_bits, const int64_t* seen_off,
                      const int32_t* seen_items, const uint32_t* allow, int k, int32_t* items, float* scores, int32_t* n_elig) {
    const char* what = "sml_host_knn_topk";
    const SmlKnn a = {nbr_items, nbr_sims, n_rows_nbr, k_nbr, n_item, hist_off, hist_items, users, n, frac_bits, seen_off, seen_items, allow, k};
    if (const char* why = knn_refusal(a, 0, 0, nullptr, 0, items, scores, n_elig, false)) return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    sml_knn_host_walk(a, items, scores, n_elig);
    return SML_OK;
}

// propagation: what the device call and the host walk refuse alike (NULL: nothing).  The set's items, a and the scratch's slot
// records are of unknown extent: they count from their first entry, respectively up to what n alone fixes
static const char* graph_refusal(int d, int elem_bytes, const void* src, int64_t n_src, const int64_t* set_off, const int32_t* set_items,
                                 const int64_t* rows, int64_t n, const float* a, const float* b, int max_workgroups, int path,
                                 const void* scratch, const float* out, bool device) {
    if (!elem_ok(elem_bytes)) return "bad argument (elem_bytes 4: fp32 rows, 2: fp16 rows)";
    if (!sml_graph_supports(d, elem_bytes)) return "bad argument (d = 32 / 64 / 128)";
    if (!size_ok(n_src) || !count_ok(n)) return "bad argument (0 < n_src < 2^31, 0 <= n < 2^31)";
    if (max_workgroups < 0 || path < 0 || path > 2) return "bad argument (max_workgroups >= 0, path 0 / 1 / 2)";
    if ((!set_off) != (!set_items)) return "bad argument (set_off and set_items both or neither)";
    if (device && ((uintptr_t)scratch & 255)) return "scratch must be 256-byte aligned";
    if (device && (((uintptr_t)src | (uintptr_t)out) & 15)) return "src and out must be 16-byte aligned";
    if (n == 0) return nullptr;
    if (!src || !out || (device && !scratch && path != 1 && set_off)) return "null argument";
    const int64_t ob = 4 * n * (int64_t)d;
    const Span in[] = {{src, n_src * d * elem_bytes}, {set_off, rows ? 8 : 8 * (n + 1)}, {set_items, 4}, {rows, 8 * n}, {a, rows ? 4 : 4 * n},
                          {b, 4 * n_src}, {scratch, scratch ? sml_graph_scratch_size(d, n, 0) : 0}};
    const Span o[] = {{out, ob}};
    return overlap_refusal(in, o, "out overlaps an input or the scratch", nullptr);
}

int sml_graph_split_from(void) { return sml_graph_split_segments(); }

int64_t sml_graph_scratch_bytes(sml_ctx* ctx, int64_t n, int64_t nnz, int max_workgroups) {
    if (!ctx || !count_ok(n) || nnz < 0 || max_workgroups < 0)
        return fail(SML_EINVAL, "sml_graph_scratch_bytes", "bad argument (0 <= n < 2^31, nnz >= 0, max_workgroups >= 0)");
    return sml_graph_scratch_size(ctx->d, n, nnz);
}

int sml_graph_propagate(sml_ctx* ctx, const void* src, int elem_bytes, int64_t n_src, const int64_t* set_off, const int32_t* set_items,
                        const int64_t* rows, int64_t n, const float* a, const float* b, int max_workgroups, int path, void* scratch,
                        float* out, void* stream) {
    const char* what = "sml_graph_propagate";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    if (const char* why = graph_refusal(ctx->d, elem_bytes, src, n_src, set_off, set_items, rows, n, a, b, max_workgroups, path, scratch, out, true))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_graph_propagate(ctx->d, elem_bytes, src, set_off, set_items, rows, n, a, b, max_workgroups, path, scratch,
                                                        out, st)));
    return SML_OK;
}

int sml_host_graph_propagate(const void* src, int elem_bytes, int d, int64_t n_src, const int64_t* set_off, const int32_t* set_items,
                             const int64_t* rows, int64_t n, const float* a, const float* b, float* out) {
    const char* what = "sml_host_graph_propagate";
    if (const char* why = graph_refusal(d, elem_bytes, src, n_src, set_off, set_items, rows, n, a, b, 0, 0, nullptr, out, false))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    if (!sml_graph_host_walk(d, elem_bytes, src, set_off, set_items, rows, n, a, b, out))
        return fail(SML_EINVAL, what, "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

// deep lists: what sml_topk_deep and sml_host_topk_items refuse alike (NULL: nothing).  The tables' heights are unknown: they
// count from their first row only
static const char* deep_refusal(int d, int elem_bytes, const void* w_user, const void* w_item, int64_t n_item, const int64_t* users, int64_t n,
                                int k, const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj, int slices,
                                const void* scratch, int64_t scratch_bytes, const int32_t* items, const float* scores, const int32_t* n_elig) {
    if (!elem_ok(elem_bytes)) return "bad argument (elem_bytes must be 4 or 2)";
    if (k < 1 || k > SML_TOPK_DEEP_MAX) return "bad argument (1 <= k <= 1024)";
    if (slices < 0 || slices > 256) return "bad argument (0 <= slices <= 256)";
    if (!sml_retrieval_supports(d, elem_bytes)) return "bad argument (d must be 32/64, or 128 for fp16 tables)";
    if (!size_ok(n_item) || !count_ok(n)) return "bad argument (0 < n_item < 2^31, 0 <= n < 2^31)";
    if ((!seen_off) != (!seen_items)) return "bad argument (seen_off and seen_items both or neither)";
    if (n == 0) return nullptr;
    if (!w_user || !w_item || !users || !items || !scores) return "null argument";
    const int64_t out_bytes = 4 * n * (int64_t)k;
    const int64_t n_pad = sml_item_adjust_pad(n_item);
    const Span in[] = {{users, 8 * n}, {w_user, (int64_t)d * elem_bytes}, {w_item, n_item * d * elem_bytes}, {seen_off, 8}, {seen_items, 4},
                       {allow, n_pad / 8}, {adj, 8 * n_pad}};
    const Span out[] = {{items, out_bytes}, {scores, out_bytes}, {n_elig, 4 * n}, {scratch, scratch_bytes}};
    return overlap_refusal(in, out, kOutIn, kOutOut);
}

int64_t sml_topk_deep_scratch_bytes(sml_ctx* ctx, int64_t n, int k, int64_t n_item, int slices) {
    if (!ctx || !count_ok(n) || k < 1 || k > SML_TOPK_DEEP_MAX || !size_ok(n_item) || slices < 0 || slices > 256)
        return fail(SML_EINVAL, "sml_topk_deep_scratch_bytes", "bad argument (1 <= k <= 1024, 0 <= slices <= 256, 0 < n_item < 2^31, 0 <= n < 2^31)");
    return n == 0 ? 0 : sml_topk_deep_scratch_size(n, n_item, slices);
}

int sml_topk_deep(sml_ctx* ctx, const void* w_user, const void* w_item, int elem_bytes, int64_t n_item, const int64_t* users, int64_t n, int k,
                  const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj, int slices, void* scratch,
                  int32_t* items, float* scores, int32_t* n_elig, void* stream) {
    const char* what = "sml_topk_deep";
    if (!ctx) return fail(SML_EINVAL, what, "null argument");
    if (adj && ((uintptr_t)adj & 15)) return fail(SML_EINVAL, what, "adj must be 16-byte aligned");
    const int64_t scratch_bytes = size_ok(n) && size_ok(n_item) && slices >= 0 && slices <= 256
                                      ? sml_topk_deep_scratch_size(n, n_item, slices) : 0;
    if (const char* why = deep_refusal(ctx->d, elem_bytes, w_user, w_item, n_item, users, n, k, seen_off, seen_items, allow, adj, slices, scratch,
                                       scratch_bytes, items, scores, n_elig))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    if (!scratch) return fail(SML_EINVAL, what, "null argument");
    if (((uintptr_t)w_user | (uintptr_t)w_item) & 15) return fail(SML_EINVAL, what, "the tables must be 16-byte aligned");
    if ((uintptr_t)scratch & 255) return fail(SML_EINVAL, what, "scratch must be 256-byte aligned");
    const SmlCatalogue c = {ctx->d, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj};
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_topk_deep(c, users, n, k, slices, scratch, items, scores, n_elig, st)));
    return SML_OK;
}

int sml_host_topk_items(const void* w_user, const void* w_item, int elem_bytes, int d, int64_t n_item, const int64_t* users, int64_t n, int k,
                        const int64_t* seen_off, const int32_t* seen_items, const uint32_t* allow, const float* adj, int32_t* items,
                        float* scores, int32_t* n_elig) {
    const char* what = "sml_host_topk_items";
    if (const char* why = deep_refusal(d, elem_bytes, w_user, w_item, n_item, users, n, k, seen_off, seen_items, allow, adj, 0, nullptr, 0, items,
                                       scores, n_elig))
        return fail(SML_EINVAL, what, why);
    if (n == 0) return SML_OK;
    const SmlCatalogue c = {d, elem_bytes, w_user, w_item, n_item, seen_off, seen_items, allow, adj};
    if (!sml_topk_host_walk(c, users, n, k, items, scores, n_elig)) return fail(SML_EINVAL, what, "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

int64_t sml_item_adjust_len(int64_t n_item) {
    if (!size_ok(n_item)) return fail(SML_EINVAL, "sml_item_adjust_len", "bad argument (0 < n_item < 2^31)");
    return sml_item_adjust_pad(n_item);
}

int sml_item_adjust_fill(sml_ctx* ctx, const float* scale, const float* offset, int64_t n_item, float* adj, void* stream) {
    if (!ctx || !size_ok(n_item)) return fail(SML_EINVAL, "sml_item_adjust_fill", "bad argument (0 < n_item < 2^31)");
    if (!adj || ((uintptr_t)adj & 15)) return fail(SML_EINVAL, "sml_item_adjust_fill", "adj must be non-null and 16-byte aligned");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_item_adjust_fill(scale, offset, n_item, adj, st)));
    return SML_OK;
}

int sml_item_adjust_cosine(sml_ctx* ctx, const void* w_item, int elem_bytes, int64_t n_item, float* adj, void* stream) {
    if (!ctx || !elem_ok(elem_bytes) || !sml_retrieval_supports(ctx->d, elem_bytes) || !size_ok(n_item))
        return fail(SML_EINVAL, "sml_item_adjust_cosine", "bad argument (d must be 32/64, or 128 for fp16 tables; elem_bytes 4 or 2; 0 < n_item < 2^31)");
    if (!w_item || !adj || ((uintptr_t)adj & 15)) return fail(SML_EINVAL, "sml_item_adjust_cosine", "null argument, or adj not 16-byte aligned");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_item_adjust_cosine(ctx->d, elem_bytes, w_item, n_item, adj, st)));
    return SML_OK;
}

int64_t sml_item_filter_words(int64_t n_item) {
    if (!size_ok(n_item)) return fail(SML_EINVAL, "sml_item_filter_words", "bad argument (0 < n_item < 2^31)");
    return (n_item + 31) / 32;
}

int sml_item_filter_from_ids(sml_ctx* ctx, const int32_t* ids, int64_t n_ids, int64_t n_item, int invert, uint32_t* words, void* stream) {
    if (!ctx || !count_ok(n_ids) || !size_ok(n_item) || (invert != 0 && invert != 1))
        return fail(SML_EINVAL, "sml_item_filter_from_ids", "bad argument (0 <= n_ids < 2^31, 0 < n_item < 2^31, invert 0 or 1)");
    if (!words || (n_ids && !ids)) return fail(SML_EINVAL, "sml_item_filter_from_ids", "null argument");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_item_filter(ids, n_ids, n_item, invert, words, st)));
    return SML_OK;
}

int sml_user_metrics(sml_ctx* ctx, const int32_t* pos, const int64_t* pos_off, int64_t n, const int32_t* ks, int n_k,
                     int32_t* hits, float* dcg, float* ap, int32_t* first, void* stream) {
    bool ok = ctx && count_ok(n) && ks && n_k >= 1 && n_k <= 8;
    for (int q = 0; ok && q < n_k; ++q) ok = ks[q] >= 1;
    if (!ok) return fail(SML_EINVAL, "sml_user_metrics", "bad argument (ks: 1 to 8 host values >= 1, 0 <= n < 2^31)");
    if (n == 0) return SML_OK;
    if (!pos || !pos_off || !hits || !dcg || !ap || !first) return fail(SML_EINVAL, "sml_user_metrics", "null argument");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_user_metrics(pos, pos_off, n, ks, n_k, hits, dcg, ap, first, st)));
    return SML_OK;
}

int sml_host_resolve_negatives(const int64_t* users, int64_t n, const int64_t* cand, int64_t m,
                               const int64_t* pairs, int64_t n_pairs, int64_t stride, int64_t* negs,
                               int64_t* consumed, int64_t* resolved) {
    if (!users || !cand || !pairs || !negs || !consumed || !resolved || n < 0 || m < 0 || n_pairs < 0 || stride <= 0)
        return fail(SML_EINVAL, "sml_host_resolve_negatives", "bad argument");
    int64_t ptr = 0, e = 0;
    for (; e < n; ++e) {
        bool placed = false;
        while (ptr < m) {
            const int64_t c = cand[ptr++];
            const int64_t code = users[e] * stride + c;
            int64_t lo = 0, hi = n_pairs;                      // is (user, candidate) one of the user's own pairs?
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (pairs[mid] < code) lo = mid + 1; else hi = mid; }
            if (!(lo < n_pairs && pairs[lo] == code)) { negs[e] = c; placed = true; break; }
        }
        if (!placed) break;                                    // stream ran out inside element e
    }
    *consumed = ptr;
    *resolved = e;
    return SML_OK;
}

int sml_sample_negatives(sml_ctx* ctx, const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop,
                         const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, uint64_t seed, int64_t* negs,
                         int32_t* failed, void* stream) {
    if (!ctx || !users || !item_all || !user_ptr || !user_items || !negs || !failed || n < 0 || pop <= 0 || n_users < 0)
        return fail(SML_EINVAL, "sml_sample_negatives", "bad argument");
    if (n == 0) return SML_OK;
    DevGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(failed, 0, sizeof(int32_t), st));
    PROFILED(PC_MISC, HIPCHK(sml_launch_sample_negatives(users, n, item_all, pop, user_ptr, n_users, user_items, seed, negs, failed, st)));
    return SML_OK;
}

int sml_device_epoch(sml_ctx* ctx, const int64_t* ui, const void* mat, int elem_bytes, int64_t row_stride, int64_t col, int64_t n,
                     uint64_t seed, int64_t* out3, void* stream) {
    if (!ctx || !ui || !out3 || n < 0 || (mat && (elem_bytes != 4 && elem_bytes != 8)) || (mat && (row_stride <= 0 || col < 0 || col >= row_stride)))
        return fail(SML_EINVAL, "sml_device_epoch", "bad argument");
    DevGuard g(ctx->device);
    HIPCHK(sml_launch_device_epoch(ui, mat, elem_bytes, row_stride, col, n, seed, out3, (hipStream_t)stream));
    return SML_OK;
}

int64_t sml_rank_weights_scratch_bytes(sml_ctx* ctx, int64_t n) {
    if (!ctx || !count_ok(n)) return fail(SML_EINVAL, "sml_rank_weights_scratch_bytes", "bad argument");
    return sml_rank_weights_scratch_size(n);
}

int sml_rank_weights(sml_ctx* ctx, const float* w_user, const float* w_item, const int64_t* rows, int64_t n, void* scratch,
                     float* score, int32_t* rank, int32_t* order, float* p, void* stream) {
    if (!ctx || !count_ok(n) || (ctx->d != 32 && ctx->d != 64 && ctx->d != 128))
        return fail(SML_EINVAL, "sml_rank_weights", "bad argument (0 <= n < 2^31, d must be 32/64/128)");
    if (n == 0) return SML_OK;
    if (!w_user || !w_item || !rows || !scratch || !score || !rank || !order || !p) return fail(SML_EINVAL, "sml_rank_weights", "null argument");
    DevGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_rank_weights(ctx->d, w_user, w_item, rows, n, scratch, score, rank, order, p, st)));
    return SML_OK;
}

int sml_weighted_epoch(sml_ctx* ctx, const int64_t* rows, int64_t n, const int32_t* order, const int64_t* item_all, int64_t pop,
                       const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, int64_t n_out, uint64_t seed,
                       int64_t* out3, int32_t* failed, void* stream) {
    if (!ctx || !size_ok(n) || pop <= 0 || n_users < 0 || !count_ok(n_out))
        return fail(SML_EINVAL, "sml_weighted_epoch", "bad argument (0 < n < 2^31, pop > 0, 0 <= n_out < 2^31)");
    if (!rows || !order || !item_all || !user_ptr || !user_items || !out3 || !failed)
        return fail(SML_EINVAL, "sml_weighted_epoch", "null argument");
    DevGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(failed, 0, sizeof(int32_t), st));
    if (n_out == 0) return SML_OK;
    PROFILED(PC_MISC, HIPCHK(sml_launch_weighted_epoch(rows, n, order, item_all, pop, user_ptr, n_users, user_items, n_out, seed, out3, failed, st)));
    return SML_OK;
}

// ---- interaction sets (interaction_set.hip) ----
int64_t sml_iset_build_scratch_bytes(sml_ctx* ctx, int64_t m, int64_t n_user, int64_t n_item) {
    if (!ctx || !count_ok(m) || !size_ok(n_user) || !size_ok(n_item))
        return fail(SML_EINVAL, "sml_iset_build_scratch_bytes", "bad argument (0 <= m < 2^31, 0 < n_user, n_item < 2^31)");
    return sml_iset_build_scratch_size(m);
}

int sml_iset_build(sml_ctx* ctx, const int64_t* rows, int64_t m, int n_cols, int64_t n_user, int64_t n_item, void* scratch,
                   int64_t* off, int32_t* items, void* stream) {
    if (!ctx || !count_ok(m) || n_cols < 2 || !size_ok(n_user) || !size_ok(n_item))
        return fail(SML_EINVAL, "sml_iset_build", "bad argument (0 <= m < 2^31, n_cols >= 2, 0 < n_user, n_item < 2^31)");
    if (!scratch || !off || (m && (!rows || !items))) return fail(SML_EINVAL, "sml_iset_build", "null argument");
    if (((uintptr_t)scratch & 15) != 0) return fail(SML_EINVAL, "sml_iset_build", "scratch must be 16-byte aligned");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_iset_build(rows, m, n_cols, n_user, n_item, scratch, off, items, st)));
    return SML_OK;
}

int64_t sml_iset_union_scratch_bytes(sml_ctx* ctx, int64_t nnz_a, int64_t nnz_b, int64_t n_user) {
    if (!ctx || !count_ok(nnz_a) || !count_ok(nnz_b) || !count_ok(nnz_a + nnz_b) || !size_ok(n_user))
        return fail(SML_EINVAL, "sml_iset_union_scratch_bytes", "bad argument (0 <= nnz_a, nnz_b, nnz_a + nnz_b < 2^31, 0 < n_user < 2^31)");
    return sml_iset_union_scratch_size(nnz_b);
}

int sml_iset_union(sml_ctx* ctx, int64_t n_user, const int64_t* a_off, const int32_t* a_items, int64_t nnz_a, const int64_t* b_off,
                   const int32_t* b_items, int64_t nnz_b, void* scratch, int64_t* out_off, int32_t* out_items, void* stream) {
    if (!ctx || !count_ok(nnz_a) || !count_ok(nnz_b) || !count_ok(nnz_a + nnz_b) || !size_ok(n_user))
        return fail(SML_EINVAL, "sml_iset_union", "bad argument (0 <= nnz_a, nnz_b, nnz_a + nnz_b < 2^31, 0 < n_user < 2^31)");
    if (!scratch || !a_off || !b_off || !out_off || (nnz_a && !a_items) || (nnz_b && !b_items) || ((nnz_a + nnz_b) && !out_items))
        return fail(SML_EINVAL, "sml_iset_union", "null argument");
    if (((uintptr_t)scratch & 15) != 0) return fail(SML_EINVAL, "sml_iset_union", "scratch must be 16-byte aligned");
    const int64_t off_bytes = 8 * (n_user + 1), out_bytes = 4 * (nnz_a + nnz_b);
    const Span in[] = {{a_off, off_bytes}, {b_off, off_bytes}, {a_items, 4 * nnz_a}, {b_items, 4 * nnz_b}};
    const Span out[] = {{out_off, off_bytes}, {out_items, out_bytes}};
    if (const char* why = overlap_refusal(in, out, kOutIn, nullptr)) return fail(SML_EINVAL, "sml_iset_union", why);
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_iset_union(n_user, a_off, a_items, nnz_a, b_off, b_items, nnz_b, scratch, out_off, out_items, st)));
    return SML_OK;
}

int sml_iset_contains(sml_ctx* ctx, const int64_t* rows, int64_t m, int n_cols, const int64_t* off, const int32_t* items, uint8_t* out,
                      void* stream) {
    if (!ctx || !count_ok(m) || n_cols < 2) return fail(SML_EINVAL, "sml_iset_contains", "bad argument (0 <= m < 2^31, n_cols >= 2)");
    if (m == 0) return SML_OK;
    if (!rows || !off || !out) return fail(SML_EINVAL, "sml_iset_contains", "null argument");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_iset_contains(rows, m, n_cols, off, items, out, st)));
    return SML_OK;
}

// ---- test-set negatives (neg_sets.hip) ----
static const char* const kNegSetsArgs = "bad argument (n >= 0, n_cols >= 2, g0 >= 0, g0 + n < 2^31, 0 < n_user < 2^31, 1 <= neg_num <= 4096)";
static bool neg_sets_dims_ok(int64_t n, int n_cols, int64_t g0, int64_t n_user, int neg_num) {
    return count_ok(n) && n_cols >= 2 && count_ok(g0) && count_ok(g0 + n) && size_ok(n_user) && neg_num >= 1 &&
           neg_num <= 4096;
}
// out against every input, as far as the pointers show it: the arrays whose length only the device knows count as one entry
static bool neg_sets_overlap(const int64_t* rows, int64_t n, int n_cols, const int32_t* n_cat, const int32_t* order, const int64_t* h_off,
                             int64_t n_user, const int32_t* h_items, const int32_t* h_since, int neg_num, const int64_t* out,
                             const int32_t* failed) {
    const Span in[] = {{rows, 8 * n * n_cols}, {n_cat, 4 * n}, {h_off, 8 * (n_user + 1)}, {order, 4}, {h_items, 4}, {h_since, 4}, {failed, 4}};
    const Span o[] = {{out, 8 * n * (2 + (int64_t)neg_num)}};
    return overlap_refusal(in, o, kOutIn, nullptr) != nullptr;
}

int sml_neg_sets(sml_ctx* ctx, const int64_t* rows, int64_t n, int n_cols, int64_t g0, const int32_t* n_cat, const int32_t* order,
                 const int64_t* h_off, int64_t n_user, const int32_t* h_items, const int32_t* h_since, int neg_num, uint64_t seed,
                 int max_workgroups, int64_t* out, int32_t* failed, void* stream) {
    if (!ctx || !neg_sets_dims_ok(n, n_cols, g0, n_user, neg_num) || max_workgroups < 0) return fail(SML_EINVAL, "sml_neg_sets", kNegSetsArgs);
    if (!failed || !h_off || (n && (!rows || !n_cat || !order || !out))) return fail(SML_EINVAL, "sml_neg_sets", "null argument");
    if (neg_sets_overlap(rows, n, n_cols, n_cat, order, h_off, n_user, h_items, h_since, neg_num, out, failed))
        return fail(SML_EINVAL, "sml_neg_sets", "out overlaps an input");
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(failed, 0, sizeof(int32_t), st));
    if (n == 0) return SML_OK;
    PROFILED(PC_MISC, HIPCHK(sml_launch_neg_sets(rows, n, n_cols, g0, n_cat, order, h_off, h_items, h_since, neg_num, seed, max_workgroups,
                                                 out, failed, st)));
    return SML_OK;
}

int sml_host_neg_sets(const int64_t* rows, int64_t n, int n_cols, int64_t g0, const int32_t* n_cat, const int32_t* order,
                      const int64_t* h_off, int64_t n_user, const int32_t* h_items, const int32_t* h_since, int neg_num, uint64_t seed,
                      int64_t* out, int32_t* failed) {
    if (!neg_sets_dims_ok(n, n_cols, g0, n_user, neg_num)) return fail(SML_EINVAL, "sml_host_neg_sets", kNegSetsArgs);
    if (!failed || !h_off || (n && (!rows || !n_cat || !order || !out))) return fail(SML_EINVAL, "sml_host_neg_sets", "null argument");
    if (neg_sets_overlap(rows, n, n_cols, n_cat, order, h_off, n_user, h_items, h_since, neg_num, out, failed))
        return fail(SML_EINVAL, "sml_host_neg_sets", "out overlaps an input");
    *failed = (int32_t)sml_neg_sets_host_walk(rows, n, n_cols, g0, n_cat, order, h_off, h_items, h_since, neg_num, seed, out);
    return SML_OK;
}

// ---- training negatives (neg_sampler.hip) ----
static const char* neg_sampler_refusal(const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop, const int64_t* user_ptr,
                                       int64_t n_users, const int64_t* user_items, int pool, const float* w_user, const float* w_item, int d,
                                       int max_workgroups, const int64_t* negs, const int32_t* failed) {
    if (n < 0 || pop <= 0 || n_users < 0 || max_workgroups < 0) return "bad argument (n >= 0, pop > 0, n_users >= 0, max_workgroups >= 0)";
    if (pool < 1 || pool > 64) return "bad argument (1 <= pool <= 64)";
    if (!users || !item_all || !user_ptr || !user_items || !negs || !failed) return "null argument";
    if (pool > 1) {
        if (!w_user || !w_item) return "null argument (pool > 1 scores the candidates: w_user and w_item are needed)";
        if (d != 32 && d != 64) return "bad argument (pool > 1: d must be 32 or 64, fp32 tables)";
        if ((((uintptr_t)w_user) | ((uintptr_t)w_item)) & 15) return "bad argument (the tables must be 16-byte aligned)";
    }
    return nullptr;
}

int sml_sample_negatives_ex(sml_ctx* ctx, const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop, const int64_t* user_ptr,
                            int64_t n_users, const int64_t* user_items, const double* cdf, int pool, const float* w_user,
                            const float* w_item, int d, uint64_t seed, int max_workgroups, int64_t* negs, float* score, int32_t* failed,
                            void* stream) {
    if (!ctx) return fail(SML_EINVAL, "sml_sample_negatives_ex", "null context");
    if (const char* why = neg_sampler_refusal(users, n, item_all, pop, user_ptr, n_users, user_items, pool, w_user, w_item, d, max_workgroups,
                                              negs, failed))
        return fail(SML_EINVAL, "sml_sample_negatives_ex", why);
    DevGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(failed, 0, sizeof(int32_t), st));
    if (n == 0) return SML_OK;
    if (pool == 1 && !cdf && max_workgroups == 0) {
        // the uniform sampler with the grid left to the call: sml_sample_negatives' own kernel, the same bytes -- k_neg_one measured
        // 1.3 % (n = 100,000) and 3.8 % (n = 3,000,000) slower, outside the old kernel's run-to-run spread (profiles/r18_neg_sampler_probe.json)
        PROFILED(PC_MISC, HIPCHK(sml_launch_sample_negatives(users, n, item_all, pop, user_ptr, n_users, user_items, seed, negs, failed, st)));
        return SML_OK;
    }
    PROFILED(PC_MISC, HIPCHK(sml_launch_neg_sampler(users, n, item_all, pop, user_ptr, n_users, user_items, cdf, pool, w_user, w_item, d, seed,
                                                    max_workgroups, negs, pool > 1 ? score : nullptr, failed, st)));
    return SML_OK;
}

int sml_host_sample_negatives_ex(const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop, const int64_t* user_ptr,
                                 int64_t n_users, const int64_t* user_items, const double* cdf, int pool, const float* w_user,
                                 const float* w_item, int d, uint64_t seed, int64_t* negs, float* score, int32_t* failed) {
    if (const char* why = neg_sampler_refusal(users, n, item_all, pop, user_ptr, n_users, user_items, pool, w_user, w_item, d, 0, negs, failed))
        return fail(SML_EINVAL, "sml_host_sample_negatives_ex", why);
    *failed = (int32_t)sml_neg_sampler_host_walk(users, n, item_all, pop, user_ptr, n_users, user_items, cdf, pool, w_user, w_item, d, seed,
                                                 negs, score);
    return SML_OK;
}

// ---- re-ranking (rerank.hip) ----
// what both entries refuse, as the header lists it; nullptr = the call is in order (n == 0 included: nothing is read)
static const char* rerank_refusal(const void* w_item, int elem_bytes, int d, int64_t n_item, const int32_t* pool_items, const float* pool_rel,
                                  int64_t n, int pool_cols, int64_t pool_stride, const float* nrm, float lam, int normalize, int k,
                                  int max_workgroups, const int32_t* items, const int32_t* pos, const float* value, const int32_t* n_sel,
                                  const float* sim_sum) {
    if (!elem_ok(elem_bytes) || !sml_retrieval_supports(d, elem_bytes))
        return "bad argument (d must be 32/64, or 128 for fp16 tables; elem_bytes 4 or 2)";
    if (!size_ok(n_item) || !count_ok(n)) return "bad argument (0 < n_item < 2^31, 0 <= n < 2^31)";
    if (pool_cols < 1 || pool_cols > 128 || pool_stride < pool_cols) return "bad argument (1 <= pool_cols <= 128, pool_stride >= pool_cols)";
    if (k < 1 || k > 128) return "bad argument (1 <= k <= 128)";
    if (!(lam >= 0.0f && lam <= 1.0f)) return "bad argument (lam must lie in [0, 1])";
    if (normalize != 0 && normalize != 1) return "bad argument (normalize must be 0 or 1)";
    if (max_workgroups < 0) return "bad argument (max_workgroups >= 0)";
    if (n == 0) return nullptr;
    if (!w_item || !pool_items || !pool_rel || !items || !pos || !value || !n_sel || !sim_sum) return "null argument";
    if ((uintptr_t)w_item & 15) return "the table must be 16-byte aligned";
    const int64_t pool_bytes = 4 * ((n - 1) * pool_stride + pool_cols), out_bytes = 4 * n * (int64_t)k;
    const Span in[] = {{w_item, n_item * d * elem_bytes}, {pool_items, pool_bytes}, {pool_rel, pool_bytes}, {nrm, 4 * n_item}};
    const Span out[] = {{items, out_bytes}, {pos, out_bytes}, {value, out_bytes}, {n_sel, 4 * n}, {sim_sum, 4 * n}};
    return overlap_refusal(in, out, kOutIn, kOutOut);
}

int sml_rerank_mmr(sml_ctx* ctx, const void* w_item, int elem_bytes, int64_t n_item, const int32_t* pool_items, const float* pool_rel,
                   int64_t n, int pool_cols, int64_t pool_stride, const float* nrm, float lam, int normalize, int k, int max_workgroups,
                   int32_t* items, int32_t* pos, float* value, int32_t* n_sel, float* sim_sum, void* stream) {
    if (!ctx) return fail(SML_EINVAL, "sml_rerank_mmr", "null context");
    if (const char* why = rerank_refusal(w_item, elem_bytes, ctx->d, n_item, pool_items, pool_rel, n, pool_cols, pool_stride, nrm, lam, normalize,
                                         k, max_workgroups, items, pos, value, n_sel, sim_sum))
        return fail(SML_EINVAL, "sml_rerank_mmr", why);
    if (n == 0) return SML_OK;
    DevGuard g(ctx->device); hipStream_t st = (hipStream_t)stream;
    PROFILED(PC_MISC, HIPCHK(sml_launch_rerank_mmr(ctx->d, elem_bytes, w_item, n_item, pool_items, pool_rel, n, pool_cols, pool_stride, nrm, lam,
                                                   normalize, k, max_workgroups, items, pos, value, n_sel, sim_sum, st)));
    return SML_OK;
}

int sml_host_rerank_mmr(const void* w_item, int elem_bytes, int d, int64_t n_item, const int32_t* pool_items, const float* pool_rel, int64_t n,
                        int pool_cols, int64_t pool_stride, const float* nrm, float lam, int normalize, int k, int32_t* items, int32_t* pos,
                        float* value, int32_t* n_sel, float* sim_sum) {
    if (const char* why = rerank_refusal(w_item, elem_bytes, d, n_item, pool_items, pool_rel, n, pool_cols, pool_stride, nrm, lam, normalize, k, 0,
                                         items, pos, value, n_sel, sim_sum))
        return fail(SML_EINVAL, "sml_host_rerank_mmr", why);
    if (n == 0) return SML_OK;
    if (!sml_rerank_host_walk(d, elem_bytes, w_item, n_item, pool_items, pool_rel, n, pool_cols, pool_stride, nrm, lam, normalize, k, items, pos,
                              value, n_sel, sim_sum))
        return fail(SML_EINVAL, "sml_host_rerank_mmr", "no walk for this (d, elem_bytes) pair");
    return SML_OK;
}

int sml_host_resolve_negatives_csr(const int64_t* users, int64_t n, const int64_t* cand, int64_t m,
                                   const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, int64_t* negs,
                                   int64_t* consumed, int64_t* resolved) {
    if (!users || !cand || !user_ptr || !user_items || !negs || !consumed || !resolved || n < 0 || m < 0 || n_users < 0)
        return fail(SML_EINVAL, "sml_host_resolve_negatives_csr", "bad argument");
    int64_t ptr = 0, e = 0;
    for (; e < n; ++e) {
        // (the walk is sequential in the candidate stream; the users are known ahead: their list heads are prefetched)
        if (e + 16 < n) { const int64_t u2 = users[e + 16]; if (u2 >= 0 && u2 < n_users) __builtin_prefetch(user_ptr + u2); }
        if (e + 8 < n) { const int64_t u1 = users[e + 8]; if (u1 >= 0 && u1 < n_users) __builtin_prefetch(user_items + user_ptr[u1]); }
        const int64_t u = users[e];
        int64_t b = 0, t = 0;
        if (u >= 0 && u < n_users) { b = user_ptr[u]; t = user_ptr[u + 1]; }     // the user's own items, ascending
        bool placed = false;
        while (ptr < m) {
            const int64_t c = cand[ptr++];
            bool own = false;
            if (t - b <= 8) { for (int64_t q = b; q < t; ++q) own |= (user_items[q] == c); }
            else {
                int64_t lo = b, hi = t;
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (user_items[mid] < c) lo = mid + 1; else hi = mid; }
                own = lo < t && user_items[lo] == c;
            }
            if (!own) { negs[e] = c; placed = true; break; }
        }
        if (!placed) break;                                    // stream ran out inside element e
    }
    *consumed = ptr;
    *resolved = e;
    return SML_OK;
}

// Host-side gathers of the reference-exact batch supply (data/dataset2.py:172-201, data/dataset.py:41-71): the epoch's
// (user, item) pairs in loader order straight into the [n,3] triple array, and one column of a row-major integer matrix
// into one of its columns.  Plain loops with software prefetch: numpy's fancy indexing builds a temporary and copies it
// through a strided view (1.9 ms per 75,000-row epoch against 0.2 ms here).
int sml_host_gather_pairs(const int64_t* ui, int64_t n_rows, const int64_t* order, int64_t n, int64_t* out3) {
    if (!ui || !order || !out3 || n < 0 || n_rows < 0) return fail(SML_EINVAL, "sml_host_gather_pairs", "bad argument");
    for (int64_t e = 0; e < n; ++e) {
        if (e + 16 < n) __builtin_prefetch(ui + 2 * order[e + 16]);
        const int64_t r = order[e];
        if (r < 0 || r >= n_rows) return fail(SML_EINVAL, "sml_host_gather_pairs", "index outside the data");
        out3[3 * e] = ui[2 * r]; out3[3 * e + 1] = ui[2 * r + 1];
    }
    return SML_OK;
}
int sml_host_gather_column(const void* mat, int64_t n_rows, int64_t row_stride_bytes, int elem_bytes, int64_t col,
                           const int64_t* order, int64_t n, int64_t* out3, int out_col) {
    if (!mat || !order || !out3 || n < 0 || (elem_bytes != 4 && elem_bytes != 8) || out_col < 0 || out_col > 2 || col < 0)
        return fail(SML_EINVAL, "sml_host_gather_column", "bad argument");
    const char* base = reinterpret_cast<const char*>(mat) + col * elem_bytes;
    for (int64_t e = 0; e < n; ++e) {
        if (e + 16 < n) __builtin_prefetch(base + order[e + 16] * row_stride_bytes);
        const int64_t r = order[e];
        if (r < 0 || r >= n_rows) return fail(SML_EINVAL, "sml_host_gather_column", "index outside the data");
        const char* p = base + r * row_stride_bytes;
        out3[3 * e + out_col] = elem_bytes == 8 ? *reinterpret_cast<const int64_t*>(p) : (int64_t)*reinterpret_cast<const int32_t*>(p);
    }
    return SML_OK;
}

}  // extern "C"
