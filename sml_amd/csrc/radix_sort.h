// Stable LSD radix sort on gfx950, 8 bits per pass, over a uint32 key with a uint32 payload (spmf.hip's rank order,
// interaction_set.hip's pair sort).  One pass (rw_sort_pass) is four launches:
//   k_rw_hist     per-tile digit counts (tile = 4096 rows, LDS atomics: counts are order-free)
//   k_rw_tot      per-digit totals over the tiles
//   k_rw_scan     per digit, the exclusive scan of its tile counts plus the totals of the smaller digits
//   k_rw_scatter  each wave walks its 1024 rows 64 at a time in row order; lanes with the same digit find each other with
//                 eight ballots, so a row lands after every earlier row of its digit: stable, and the same bytes whatever
//                 the schedule.
// No workgroup waits on another: every dependency is a launch boundary.  Scratch of a pass: counts uint32 [256 * n_tiles],
// tot uint32 [256], n_tiles = ceil(n / RW_TILE).  Included inside each user's translation unit (internal linkage).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int RW_WAVES = 4;                       // waves per workgroup
constexpr int RW_CHUNKS = 16;                     // 64-row chunks per wave
constexpr int RW_TILE = RW_WAVES * RW_CHUNKS * 64;

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

// rows of (key_in, val_in) -> (key_out, val_out), ordered by the digit at `shift`, equal digits in input order
inline void rw_sort_pass(const uint32_t* key_in, const uint32_t* val_in, uint32_t* key_out, uint32_t* val_out, int64_t n, int shift,
                         uint32_t* counts, uint32_t* tot, hipStream_t st) {
    const int64_t n_tiles = (n + RW_TILE - 1) / RW_TILE;
    k_rw_hist<<<dim3((unsigned)n_tiles), dim3(256), 0, st>>>(key_in, n, shift, n_tiles, counts);
    k_rw_tot<<<dim3(256), dim3(256), 0, st>>>(counts, n_tiles, tot);
    k_rw_scan<<<dim3(256), dim3(256), 0, st>>>(counts, n_tiles, tot);
    k_rw_scatter<<<dim3((unsigned)n_tiles), dim3(256), 0, st>>>(key_in, val_in, key_out, val_out, n, shift, n_tiles, counts);
}

}  // namespace
