// The SPMF streaming baseline's rank-weighted sampling on gfx950 (reference model/baseline.py:448-503).
//
// Rank weights (SPMF.compute_R_W_P): every training row (u, i) is scored with MFbasemode.forward's chain (mf_dot, the
// bytes of k_mf_forward), ranked by score descending -- rank 1 is the highest score -- and weighted w = exp(rank / N),
// p = w / sum(w): the rows the model already scores low are drawn most.
//
//   k_rw_score    LPR lanes per row: the score, and an order-preserving uint32 key whose ASCENDING order is the score's
//                 DESCENDING order (NaN first as torch.argsort(descending=True) places it, -0.0 == +0.0).
//   radix sort    stable LSD over the key, 8 bits per pass, four passes (radix_sort.h: k_rw_hist, k_rw_tot, k_rw_scan,
//                 k_rw_scatter).  No workgroup waits on another: every dependency is a launch boundary.
//   k_rw_wsum_*   S = sum of w in float64 in a fixed order over rank (w depends on the rank alone, so S depends on N
//                 alone), rounded once to fp32: the same bytes whatever the launch shape.
//   k_rw_finish   order[k-1] = the row of rank k, rank[row] = k, p[row] = expf(k / N) / S.
//
// Weighted epoch (device mode of SPMF.sample_batch): element e draws u from the counter-based stream keyed by (seed, e),
// inverts the rank-order CDF F(k) = (e^(k/N) - 1) / (e - 1) -- exact for w = exp(k/N), so no prefix sum -- and takes
// row order[k-1]; its negative comes from draw_negative, the rejection walk k_sample_negatives uses.
#include <cmath>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "radix_sort.h"
#include "../../include/sml_hip.h"

namespace {

constexpr int RW_WCHUNK = 1024;                   // ranks per float64 partial sum of w

__device__ __forceinline__ uint32_t rank_key(float s) {
    if (s != s) return 0u;                                     // NaN: before +inf (torch's descending order)
    const uint32_t b = __float_as_uint(s == 0.f ? 0.f : s);    // -0.0 -> +0.0
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ~asc;                                               // non-NaN keys are >= 0x00800000 > 0
}

template <int D>
__global__ __launch_bounds__(256) void k_rw_score(const float* __restrict__ wu, const float* __restrict__ wi,
                                                  const int64_t* __restrict__ rows, int64_t n, float* __restrict__ score,
                                                  uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    constexpr int LPR = D / 4;
    const int sub = threadIdx.x % LPR;
    // grid-stride over rows (a row's LPR lanes always share a trip: the stride is a multiple of 256)
    for (int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR; t < n; t += (int64_t)gridDim.x * (256 / LPR)) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(wu + rows[2 * t] * D + sub * 4);
        const f32x4 c = *reinterpret_cast<const f32x4*>(wi + rows[2 * t + 1] * D + sub * 4);
        const float u[4] = {a[0], a[1], a[2], a[3]}, it[4] = {c[0], c[1], c[2], c[3]};
        const float s = mf_dot<LPR>(u, it);
        if (sub == 0) {
            score[t] = s;
            key[t] = rank_key(s);
            val[t] = (uint32_t)t;
        }
    }
}

// partial[t] = sum over ranks k in [t * RW_WCHUNK + 1, (t + 1) * RW_WCHUNK] (and <= n) of expf(k / n), in float64, k ascending
__global__ __launch_bounds__(256) void k_rw_wsum_part(int64_t n, int64_t n_part, double* __restrict__ partial) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_part) return;
    const float fn = (float)n;
    const int64_t k1 = (t + 1) * RW_WCHUNK < n ? (t + 1) * RW_WCHUNK : n;
    double acc = 0.0;
    for (int64_t k = t * RW_WCHUNK + 1; k <= k1; ++k) acc += (double)expf(__fdiv_rn((float)k, fn));
    partial[t] = acc;
}
// S = fp32(sum of the partials): 1024 strided float64 sums, then a fixed tree
__global__ __launch_bounds__(1024) void k_rw_wsum_final(const double* __restrict__ partial, int64_t n_part, float* __restrict__ S) {
    __shared__ double buf[1024];
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < n_part; j += 1024) acc += partial[j];
    buf[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) buf[threadIdx.x] += buf[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) S[0] = (float)buf[0];
}

__global__ __launch_bounds__(256) void k_rw_finish(const uint32_t* __restrict__ sorted_rows, int64_t n, const float* __restrict__ S,
                                                   int32_t* __restrict__ rank, int32_t* __restrict__ order, float* __restrict__ p) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t row = sorted_rows[k];
    order[k] = (int32_t)row;
    rank[row] = (int32_t)(k + 1);
    p[row] = __fdiv_rn(expf(__fdiv_rn((float)(k + 1), (float)n)), S[0]);
}

__global__ __launch_bounds__(256) void k_weighted_epoch(const int64_t* __restrict__ rows, int64_t n, const int32_t* __restrict__ order,
                                                        const int64_t* __restrict__ item_all, int64_t pop,
                                                        const int64_t* __restrict__ user_ptr, int64_t n_users,
                                                        const int64_t* __restrict__ user_items, int64_t n_out, uint64_t seed,
                                                        int64_t* __restrict__ out3, int* __restrict__ failed) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out) return;
    uint64_t st = neg_stream(seed, e);
    const double u = (double)(splitmix64(st) >> 11) * 0x1.0p-53;             // [0, 1)
    int64_t k = (int64_t)ceil((double)n * log1p(u * 1.718281828459045));          // F^-1(u), F(k) = (e^(k/N) - 1) / (e - 1)
    k = k < 1 ? 1 : (k > n ? n : k);
    const int64_t row = order[k - 1];
    const int64_t usr = rows[2 * row];
    out3[3 * e] = usr;
    out3[3 * e + 1] = rows[2 * row + 1];
    out3[3 * e + 2] = draw_negative(st, usr, item_all, pop, user_ptr, n_users, user_items, failed);
}

struct RwScratch {
    uint32_t *key[2], *val[2], *counts, *tot;
    double* partial;
    float* S;
    int64_t n_tiles, n_part, bytes;
};
RwScratch rw_layout(void* base, int64_t n) {
    RwScratch s;
    char* p = (char*)base;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* q = p ? p + off : nullptr; off += (bytes + 255) & ~(int64_t)255; return q; };
    s.n_tiles = (n + RW_TILE - 1) / RW_TILE;
    s.n_part = (n + RW_WCHUNK - 1) / RW_WCHUNK;
    for (int b = 0; b < 2; ++b) {
        s.key[b] = (uint32_t*)take(4 * n);
        s.val[b] = (uint32_t*)take(4 * n);
    }
    s.counts = (uint32_t*)take(4 * 256 * s.n_tiles);
    s.tot = (uint32_t*)take(4 * 256);
    s.partial = (double*)take(8 * s.n_part);
    s.S = (float*)take(4);
    s.bytes = off;
    return s;
}

}  // namespace

int64_t sml_rank_weights_scratch_size(int64_t n) { return n <= 0 ? 0 : rw_layout(nullptr, n).bytes; }

hipError_t sml_launch_rank_weights(int d, const float* wu, const float* wi, const int64_t* rows, int64_t n, void* scratch,
                                   float* score, int32_t* rank, int32_t* order, float* p, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const RwScratch s = rw_layout(scratch, n);
    int64_t nb = (n * (d / 4) + 255) / 256;
    if (nb > 65536) nb = 65536;
    switch (d) {
        case 32: k_rw_score<32><<<dim3((unsigned)nb), dim3(256), 0, st>>>(wu, wi, rows, n, score, s.key[0], s.val[0]); break;
        case 64: k_rw_score<64><<<dim3((unsigned)nb), dim3(256), 0, st>>>(wu, wi, rows, n, score, s.key[0], s.val[0]); break;
        case 128: k_rw_score<128><<<dim3((unsigned)nb), dim3(256), 0, st>>>(wu, wi, rows, n, score, s.key[0], s.val[0]); break;
        default: return hipErrorInvalidValue;
    }
    k_rw_wsum_part<<<dim3((unsigned)((s.n_part + 255) / 256)), dim3(256), 0, st>>>(n, s.n_part, s.partial);
    k_rw_wsum_final<<<dim3(1), dim3(1024), 0, st>>>(s.partial, s.n_part, s.S);
    for (int pass = 0; pass < 4; ++pass) {
        const int src = pass & 1;
        rw_sort_pass(s.key[src], s.val[src], s.key[src ^ 1], s.val[src ^ 1], n, 8 * pass, s.counts, s.tot, st);
    }
    k_rw_finish<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(s.val[0], n, s.S, rank, order, p);
    return hipGetLastError();
}

hipError_t sml_launch_weighted_epoch(const int64_t* rows, int64_t n, const int32_t* order, const int64_t* item_all, int64_t pop,
                                     const int64_t* user_ptr, int64_t n_users, const int64_t* user_items, int64_t n_out,
                                     uint64_t seed, int64_t* out3, int* failed, hipStream_t st) {
    if (n_out <= 0) return hipSuccess;
    k_weighted_epoch<<<dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st>>>(rows, n, order, item_all, pop, user_ptr, n_users,
                                                                                 user_items, n_out, seed, out3, failed);
    return hipGetLastError();
}
