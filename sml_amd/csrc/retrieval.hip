// Full-catalogue retrieval for gfx950: the rank of a test row's positive among ALL items, and every user's top-K items,
// without ever writing the [users, items] score matrix.
//
// Score tile: v_mfma_f32_32x32x2_f32 with 32 item rows on the A side and 32 user rows on the B side.  A lane then holds
// one user column (lane & 31) and 16 item scores (rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 0..15), so every
// per-user test is a per-lane compare.  Lane half h carries dims [h D/2, (h+1) D/2) of its row (contiguous 16-byte
// loads); MFMA step s therefore feeds dim s (k0) and then dim s + D/2 (k1), and the score of (u, i) is the fmaf chain
// score_chain() spells out on the VALU -- the positive's score in rank mode is computed that way, bit-identical.  That
// order (dims 0, D/2, 1, D/2 + 1, ..., each fmaf rounded once, subnormals kept) is part of the contract in sml_hip.h;
// tests/test_retrieval_gpu.py compares ranks, lists and score bits with an exact emulation of it.
//
// Grid: (32 * W users) x slices; slice = blockIdx % slices, so with slices a multiple of 8 an XCD walks 1/8 of the
// item table.  Every wave owns 32 users and walks its slice tile by tile (32 items), loading the next tile's item rows
// while the current tile's MFMAs run.  Seen items: a cursor per lane into the user's ascending CSR range yields the
// exclusion bitmap of each 32-item tile in one register word (exact: ids, never scores).
//
//   k_full_rank   counts, per row, items scoring strictly above the positive; per-slice counts land with integer
//                 atomicAdd (exact, order-free).
//   k_topk_slice  keeps a sorted list of the K best (score desc, id asc) per (user, slice) in the wave's LDS; a
//                 register threshold (the K-th entry) filters candidates, so inserts are rare once a list is full.
//   k_topk_merge  places each slice's candidates by counting, with binary searches, the better entries of the other
//                 slices: every surviving candidate has a unique final position.
#include <climits>
#include <cmath>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "../../include/sml_hip.h"

namespace {

constexpr int RT = 32;         // items per score tile = users per wave

// S(u, i) in the k order of tile_scores(): the device-side definition every retrieval kernel agrees with, bit for bit
template <int D>
__device__ __forceinline__ float score_chain(const float* __restrict__ u, const float* __restrict__ x) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        acc = fmaf(x[s], u[s], acc);
        acc = fmaf(x[s + D / 2], u[s + D / 2], acc);
    }
    return acc;
}

template <int D>
__device__ __forceinline__ void load_half(const float* __restrict__ row, int h, f32x4 (&f)[D / 8]) {
    const f32x4* p = reinterpret_cast<const f32x4*>(row + h * (D / 2));
#pragma unroll
    for (int q = 0; q < D / 8; ++q) f[q] = p[q];
}

// 32 items (A) x 32 users (B): acc[r] = S(user lane & 31, item row_of(r, lane >> 5))
template <int D>
__device__ __forceinline__ f32x16 tile_scores(const f32x4 (&a)[D / 8], const f32x4 (&b)[D / 8]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int q = 0; q < D / 8; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][e], b[q][e], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// total order of the top-K lists: score descending, then item id ascending (NaN is never better than anything)
__device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// forward-only cursor over one user's ascending Seen range
struct SeenCursor {
    const int32_t* items;
    int64_t cur, end;
    long long nxt;
    __device__ void init(const int64_t* __restrict__ off, const int32_t* __restrict__ it, int64_t u, long long start) {
        items = it;
        if (!off) { cur = end = 0; nxt = LLONG_MAX; return; }
        int64_t lo = off[u], hi = off[u + 1];
        end = hi;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (it[mid] < start) lo = mid + 1; else hi = mid;
        }
        cur = lo;
        nxt = cur < end ? it[cur] : LLONG_MAX;
    }
    // bit b set <=> item base + b is in Seen; the cursor moves past the tile
    __device__ unsigned word(long long base) {
        unsigned w = 0;
        while (nxt < base + RT) {
            w |= 1u << (unsigned)(nxt - base);
            ++cur;
            nxt = cur < end ? items[cur] : LLONG_MAX;
        }
        return w;
    }
};

template <int D>
__global__ __launch_bounds__(256) void k_full_rank(const float* __restrict__ wu, const float* __restrict__ wi, int64_t n_item,
                                                   const int64_t* __restrict__ rows, int64_t n, int n_cols,
                                                   const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                   int slices, int slice_tiles, int32_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    const int slice = blockIdx.x % slices;
    const int64_t r = ((int64_t)(blockIdx.x / slices) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RT + j;
    const bool valid = r < n;
    const int64_t rr = valid ? r : n - 1;
    const int64_t u = rows[rr * n_cols], p = rows[rr * n_cols + 1];
    const float* urow = wu + u * D;
    f32x4 b[D / 8];
    load_half<D>(urow, h, b);
    const float thr = score_chain<D>(urow, wi + p * D);
    const int64_t n_tiles = (n_item + RT - 1) / RT;
    const int64_t t0 = (int64_t)slice * slice_tiles;
    const int64_t t1 = t0 + slice_tiles < n_tiles ? t0 + slice_tiles : n_tiles;
    if (t0 >= t1) return;
    SeenCursor sc;
    sc.init(seen_off, seen_items, u, t0 * RT);
    f32x4 a[D / 8], an[D / 8];
    int64_t ia = t0 * RT + j;
    load_half<D>(wi + (ia < n_item ? ia : n_item - 1) * D, h, a);
    int cnt = 0;
    for (int64_t t = t0; t < t1; ++t) {
        if (t + 1 < t1) {
            ia = (t + 1) * RT + j;
            load_half<D>(wi + (ia < n_item ? ia : n_item - 1) * D, h, an);
        }
        const f32x16 acc = tile_scores<D>(a, b);
        const int64_t base = t * RT;
        const unsigned w = sc.word(base);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = row_of(q, h);
            cnt += (acc[q] > thr) & !((w >> i) & 1u) & (base + i != p) & (base + i < n_item);
        }
#pragma unroll
        for (int q = 0; q < D / 8; ++q) a[q] = an[q];
    }
    cnt += __shfl_xor(cnt, 32, 64);
    if (h == 0 && valid && cnt) atomicAdd(rank + r, cnt);
}

// insert (s, i) into user j's list (k slots, column j of [k][32] arrays); cnt = live entries
__device__ __forceinline__ void list_insert(float* ls, int* li, int k, int j, int& cnt, float s, int i) {
    int q;
    if (cnt == k) {
        if (!better(s, i, ls[(k - 1) * RT + j], li[(k - 1) * RT + j])) return;
        q = k - 1;
    } else {
        q = cnt++;
    }
    while (q > 0) {
        const float ps = ls[(q - 1) * RT + j];
        const int pi = li[(q - 1) * RT + j];
        if (!better(s, i, ps, pi)) break;
        ls[q * RT + j] = ps;
        li[q * RT + j] = pi;
        --q;
    }
    ls[q * RT + j] = s;
    li[q * RT + j] = i;
}

// candidates of user x, slice s: cand_s / cand_i [(x * slices + s) * k + q], cand_n [x * slices + s]
template <int D>
__global__ __launch_bounds__(256) void k_topk_slice(const float* __restrict__ wu, const float* __restrict__ wi, int64_t n_item,
                                                    const int64_t* __restrict__ users, int64_t n, int k,
                                                    const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                    int slices, int slice_tiles, float* __restrict__ cand_s,
                                                    int32_t* __restrict__ cand_i, int32_t* __restrict__ cand_n) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31, wave = threadIdx.x >> 6;
    float* ls = lds + (size_t)wave * 2 * k * RT;
    int* li = reinterpret_cast<int*>(ls + k * RT);
    const int slice = blockIdx.x % slices;
    const int64_t x = ((int64_t)(blockIdx.x / slices) * (blockDim.x >> 6) + wave) * RT + j;
    const bool valid = x < n;
    const int64_t u = users[valid ? x : n - 1];
    f32x4 b[D / 8];
    load_half<D>(wu + u * D, h, b);
    const int64_t n_tiles = (n_item + RT - 1) / RT;
    const int64_t t0 = (int64_t)slice * slice_tiles;
    const int64_t t1 = t0 + slice_tiles < n_tiles ? t0 + slice_tiles : n_tiles;
    int cnt = 0;                          // live entries of user j's list (both lane halves keep it)
    float thr_s = -INFINITY;              // register copy of the K-th entry: lags the list, never ahead of it
    int thr_i = INT_MAX;
    if (t0 < t1) {
        SeenCursor sc;
        sc.init(seen_off, seen_items, u, t0 * RT);
        f32x4 a[D / 8], an[D / 8];
        int64_t ia = t0 * RT + j;
        load_half<D>(wi + (ia < n_item ? ia : n_item - 1) * D, h, a);
        for (int64_t t = t0; t < t1; ++t) {
            if (t + 1 < t1) {
                ia = (t + 1) * RT + j;
                load_half<D>(wi + (ia < n_item ? ia : n_item - 1) * D, h, an);
            }
            const f32x16 acc = tile_scores<D>(a, b);
            const int64_t base = t * RT;
            const unsigned w = sc.word(base);
            unsigned pass = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = row_of(q, h);
                const bool ok = valid && !((w >> i) & 1u) && base + i < n_item && better(acc[q], (int)(base + i), thr_s, thr_i);
                pass |= (unsigned)ok << q;
            }
            if (__any(pass != 0)) {
                // the two lane halves hold different items of the same users: they insert one after the other
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    if (h == hh) {
#pragma unroll
                        for (int q = 0; q < 16; ++q)
                            if ((pass >> q) & 1u) list_insert(ls, li, k, j, cnt, acc[q], (int)(base + row_of(q, h)));
                    }
                    __builtin_amdgcn_wave_barrier();
                    cnt = __shfl(cnt, j + RT * hh, 64);
                }
                if (cnt == k) {
                    thr_s = ls[(k - 1) * RT + j];
                    thr_i = li[(k - 1) * RT + j];
                }
            }
#pragma unroll
            for (int q = 0; q < D / 8; ++q) a[q] = an[q];
        }
    }
    if (!valid) return;
    const int64_t o = (x * slices + slice) * k;
    for (int q = h; q < k; q += 2) {
        const bool live = q < cnt;
        cand_s[o + q] = live ? ls[q * RT + j] : -INFINITY;
        cand_i[o + q] = live ? li[q * RT + j] : -1;
    }
    if (h == 0) cand_n[x * slices + slice] = cnt;
}

// one thread per (user, slice, slot): the candidate's final position is its slot plus the number of strictly better
// entries in the user's other slices (ids differ across slices, so positions never collide)
__global__ __launch_bounds__(256) void k_topk_merge(const float* __restrict__ cand_s, const int32_t* __restrict__ cand_i,
                                                    const int32_t* __restrict__ cand_n, int64_t n, int k, int slices,
                                                    int32_t* __restrict__ items, float* __restrict__ scores) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * slices * k) return;
    const int q = (int)(idx % k);
    const int s = (int)((idx / k) % slices);
    const int64_t x = idx / ((int64_t)k * slices);
    const int32_t* cn = cand_n + x * slices;
    if (s == 0) {
        int total = 0;
        for (int t = 0; t < slices; ++t) total += cn[t];
        if (q >= total) { items[x * k + q] = -1; scores[x * k + q] = -INFINITY; }
    }
    if (q >= cn[s]) return;
    const int64_t o = (x * slices + s) * k;
    const float cs = cand_s[o + q];
    const int ci = cand_i[o + q];
    int pos = q;
    for (int t = 0; t < slices && pos < k; ++t) {
        if (t == s) continue;
        const int64_t ot = (x * slices + t) * k;
        int lo = 0, hi = cn[t];          // entries [0, lo) of slice t are better than the candidate
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (better(cand_s[ot + mid], cand_i[ot + mid], cs, ci)) lo = mid + 1; else hi = mid;
        }
        pos += lo;
    }
    if (pos < k) { items[x * k + pos] = ci; scores[x * k + pos] = cs; }
}

constexpr int kRankWaves = 4;

// slices (a multiple of 8, one XCD per residue) and tiles per slice for a grid of `groups` workgroup rows
void plan_slices(int64_t groups, int64_t n_item, int64_t target_blocks, int max_mult, int* slices, int* slice_tiles) {
    const int64_t n_tiles = (n_item + RT - 1) / RT;
    int64_t m = (target_blocks + 8 * groups - 1) / (8 * groups);
    if (m < 1) m = 1;
    if (m > max_mult) m = max_mult;
    while (m > 1 && n_tiles / (8 * m) < 16) --m;      // keep at least 16 tiles per slice
    *slices = (int)(8 * m);
    *slice_tiles = (int)((n_tiles + 8 * m - 1) / (8 * m));
}

int topk_waves(int k) {
    const int per_wave = 2 * k * RT * 4;
    int w = 65536 / per_wave;
    return w > 4 ? 4 : w;
}

int topk_slices(int64_t n, int k, int64_t n_item, int* slice_tiles) {
    int s, st;
    const int64_t groups = (n + RT * topk_waves(k) - 1) / (RT * topk_waves(k));
    plan_slices(groups, n_item, 2048, 4, &s, &st);
    if (slice_tiles) *slice_tiles = st;
    return s;
}

}  // namespace

hipError_t sml_launch_full_rank(int d, const float* wu, const float* wi, int64_t n_item, const int64_t* rows, int64_t n, int n_cols,
                                const int64_t* seen_off, const int32_t* seen_items, int32_t* rank, hipStream_t st) {
    hipError_t e = hipMemsetAsync(rank, 0, n * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const int64_t groups = (n + RT * kRankWaves - 1) / (RT * kRankWaves);
    int slices, slice_tiles;
    plan_slices(groups, n_item, 8192, 64, &slices, &slice_tiles);
    const dim3 grid((unsigned)(groups * slices)), block(64 * kRankWaves);
    if (d == 32)
        k_full_rank<32><<<grid, block, 0, st>>>(wu, wi, n_item, rows, n, n_cols, seen_off, seen_items, slices, slice_tiles, rank);
    else
        k_full_rank<64><<<grid, block, 0, st>>>(wu, wi, n_item, rows, n, n_cols, seen_off, seen_items, slices, slice_tiles, rank);
    return hipGetLastError();
}

int64_t sml_topk_scratch_size(int64_t n, int k, int64_t n_item) {
    const int64_t s = topk_slices(n, k, n_item, nullptr);
    return n * s * (int64_t)k * 8 + n * s * 4;
}

hipError_t sml_launch_topk(int d, const float* wu, const float* wi, int64_t n_item, const int64_t* users, int64_t n, int k,
                           const int64_t* seen_off, const int32_t* seen_items, void* scratch, int32_t* items, float* scores,
                           hipStream_t st) {
    int slice_tiles;
    const int slices = topk_slices(n, k, n_item, &slice_tiles);
    const int waves = topk_waves(k);
    const int64_t groups = (n + RT * waves - 1) / (RT * waves);
    float* cs = static_cast<float*>(scratch);
    int32_t* ci = reinterpret_cast<int32_t*>(cs + n * slices * k);
    int32_t* cn = ci + n * slices * k;
    const dim3 grid((unsigned)(groups * slices)), block(64 * waves);
    const size_t lds = (size_t)waves * 2 * k * RT * 4;
    if (d == 32)
        k_topk_slice<32><<<grid, block, lds, st>>>(wu, wi, n_item, users, n, k, seen_off, seen_items, slices, slice_tiles, cs, ci, cn);
    else
        k_topk_slice<64><<<grid, block, lds, st>>>(wu, wi, n_item, users, n, k, seen_off, seen_items, slices, slice_tiles, cs, ci, cn);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t threads = n * slices * k;
    k_topk_merge<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(cs, ci, cn, n, k, slices, items, scores);
    return hipGetLastError();
}
