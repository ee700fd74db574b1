// The SPMF streaming baseline's rank-weighted sampling on gfx950 (reference model/baseline.py:448-503).
//
// Rank weights (SPMF.compute_R_W_P): every training row (u, i) is scored with MFbasemode.forward's chain (mf_dot, the
// bytes of k_mf_forward), ranked by score descending -- rank 1 is the highest score -- and weighted w = exp(rank / N),
// p = w / sum(w): the rows the model already scores low are drawn most.
//
//   k_rw_score    LPR lanes per row: the score, and an order-preserving uint32 key whose ASCENDING order is the score's
//                 DESCENDING order (NaN first as torch.argsort(descending=True) places it, -0.0 == +0.0).
//   radix sort    stable LSD over the key, 8 bits per pass, four passes, each three kinds of launch:
//                   k_rw_hist     per-tile digit counts (tile = 4096 rows, LDS atomics: counts are order-free)
//                   k_rw_tot      per-digit totals over the tiles
//                   k_rw_scan     per digit, the exclusive scan of its tile counts plus the totals of the smaller digits
//                   k_rw_scatter  each wave walks its 1024 rows 64 at a time in row order; lanes with the same digit
//                                 find each other with eight ballots, so a row lands after every earlier row of its
//                                 digit: stable, and the same bytes whatever the schedule.
//                 No workgroup waits on another: every dependency is a launch boundary.
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
#include "../../include/sml_hip.h"

namespace {

constexpr int RW_WAVES = 4;                       // waves per workgroup
constexpr int RW_CHUNKS = 16;                     // 64-row chunks per wave
constexpr int RW_TILE = RW_WAVES * RW_CHUNKS * 64;
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

// counts[d * n_tiles + tile] = rows of `tile` whose digit is d
__global__ __launch_bounds__(256) void k_rw_hist(const uint32_t* __restrict__ key, int64_t n, int shift, int64_t n_tiles,
                                                 uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RW_TILE;
    for (int j = threadIdx.x; j < RW_TILE; j += 256) {
        const int64_t r = base + j;
        if (r < n) atomicAdd(&h[(key[r] >> shift) & 255u], 1u);
    }
    __syncthreads();
    counts[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// tot[d] = sum over tiles of counts[d][.]  (one workgroup per digit)
__global__ __launch_bounds__(256) void k_rw_tot(const uint32_t* __restrict__ counts, int64_t n_tiles, uint32_t* __restrict__ tot) {
    __shared__ uint32_t part[256];
    const uint32_t* row = counts + (int64_t)blockIdx.x * n_tiles;
    uint32_t acc = 0;
    for (int64_t b = threadIdx.x; b < n_tiles; b += 256) acc += row[b];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = part[0];
}

// counts[d][b] <- sum(tot[0..d)) + sum(counts[d][0..b)): the first output slot of digit d's rows of tile b
__global__ __launch_bounds__(256) void k_rw_scan(uint32_t* __restrict__ counts, int64_t n_tiles, const uint32_t* __restrict__ tot) {
    __shared__ uint32_t buf[256];
    __shared__ uint32_t carry;
    const int d = blockIdx.x, tid = threadIdx.x;
    buf[tid] = tid < d ? tot[tid] : 0u;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) buf[tid] += buf[tid + w];
        __syncthreads();
    }
    if (tid == 0) carry = buf[0];
    __syncthreads();
    uint32_t* row = counts + (int64_t)d * n_tiles;
    for (int64_t b0 = 0; b0 < n_tiles; b0 += 256) {
        const int64_t b = b0 + tid;
        const uint32_t v = b < n_tiles ? row[b] : 0u;
        buf[tid] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {                // inclusive Hillis-Steele scan
            const uint32_t x = tid >= off ? buf[tid - off] : 0u;
            __syncthreads();
            buf[tid] += x;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (b < n_tiles) row[b] = c + buf[tid] - v;
        __syncthreads();
        if (tid == 255) carry = c + buf[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_rw_scatter(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ val_in,
                                                    uint32_t* __restrict__ key_out, uint32_t* __restrict__ val_out, int64_t n,
                                                    int shift, int64_t n_tiles, const uint32_t* __restrict__ offs) {
    __shared__ uint32_t cnt[RW_WAVES][256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int w = 0; w < RW_WAVES; ++w) cnt[w][tid] = 0;
    __syncthreads();
    const int64_t wbase = (int64_t)blockIdx.x * RW_TILE + (int64_t)wave * RW_CHUNKS * 64;
    for (int c = 0; c < RW_CHUNKS; ++c) {
        const int64_t r = wbase + c * 64 + lane;
        if (r < n) atomicAdd(&cnt[wave][(key_in[r] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {   // digit tid: the slot of the first row of each wave's segment
        uint32_t run = offs[(int64_t)tid * n_tiles + blockIdx.x];
        for (int w = 0; w < RW_WAVES; ++w) { const uint32_t x = cnt[w][tid]; cnt[w][tid] = run; run += x; }
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int c = 0; c < RW_CHUNKS; ++c) {
        const int64_t r = wbase + c * 64 + lane;
        const bool ok = r < n;
        const uint32_t k = ok ? key_in[r] : 0u;
        const uint32_t dg = (k >> shift) & 255u;
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (dg >> bit) & 1u;
            const uint64_t m = __ballot(on);
            peers &= on ? m : ~m;
        }
        uint32_t slot = 0;
        if (ok) slot = cnt[wave][dg] + (uint32_t)__popcll(peers & lt);
        __builtin_amdgcn_wave_barrier();
        if (ok) {
            key_out[slot] = k;
            val_out[slot] = val_in[r];
            if ((peers & lt) == 0) cnt[wave][dg] += (uint32_t)__popcll(peers);   // the digit's lowest lane advances it
        }
        __builtin_amdgcn_wave_barrier();
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
        const int src = pass & 1, shift = 8 * pass;
        k_rw_hist<<<dim3((unsigned)s.n_tiles), dim3(256), 0, st>>>(s.key[src], n, shift, s.n_tiles, s.counts);
        k_rw_tot<<<dim3(256), dim3(256), 0, st>>>(s.counts, s.n_tiles, s.tot);
        k_rw_scan<<<dim3(256), dim3(256), 0, st>>>(s.counts, s.n_tiles, s.tot);
        k_rw_scatter<<<dim3((unsigned)s.n_tiles), dim3(256), 0, st>>>(s.key[src], s.val[src], s.key[src ^ 1], s.val[src ^ 1], n, shift,
                                                                       s.n_tiles, s.counts);
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
