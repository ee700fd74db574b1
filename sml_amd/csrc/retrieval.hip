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
// Element type: fp32 tables (D = 32 / 64) or fp16 tables (D = 32 / 64 / 128).  A half row travels and stays packed: a
// lane half's D/2 dims are D/16 16-byte loads of eight halves, and the user row, the current and the next item tile sit
// in registers that way (3 D/4 VGPRs instead of 3 D/2).  A half is widened to fp32 (exact: every fp16 value is an fp32
// value) only where it feeds an fmaf or the fp32 MFMA, so S(u, i) on fp16 tables is the same chain on the widened entries
// and equals the fp32 kernels' score of the widened tables bit for bit.  The element type is a parameter of the walk's
// loads (HalfRow).
//
// Every kernel that reads the tables is ONE __global__ template k_x<D, T, F, A>: width, element type (float / _Float16),
// F = an item filter was given, A = per-item score terms were given.  The four share a flat parameter list -- the tables
// and n_item first, allow and adj directly after seen_items -- and an instantiation with F or A false never reads its
// pointer (every use is under `if constexpr`).  with_width() alone turns a catalogue into those four arguments.  (Before
// this, F and the element type were part of the name: k_x_f<D> / k_x_h<D> / k_x_f_h<D>, and k_x_a<D, F> / k_x_a_h<D, F>
// for A; profiles/ and the tables of DESIGN.md recorded under those names keep them.)
//
// Grid: (32 * W users) x slices; slice = blockIdx % slices, so with slices a multiple of 8 an XCD walks 1/8 of the
// item table (plan_grid on the host, lane_pos on the device).  Every wave owns 32 users.
//
// The walk, written once (walk_slice): a wave goes through its slice tile by tile (32 items), loading the next tile's
// item rows while the current tile's MFMAs run; a cursor per lane into the user's ascending Seen range (CSR) yields the
// exclusion bitmap of each tile in one register word (exact: ids, never scores).  Per tile the kernel's callable gets the
// 16 scores of the lane, the tile's first item and a 16-bit mask of the scores that belong to a real, unseen item.  The
// walk holds no workgroup barrier.  What a kernel does with a tile:
//
//   k_full_rank   counts the eligible items scoring strictly above the row's positive; per-slice counts land with
//                 integer atomicAdd (exact, order-free).
//   k_topk_slice  offers them to a sorted list of the K best (score desc, id asc) per (user, slice) in the wave's LDS; a
//                 register threshold (the K-th entry) filters candidates, so inserts are rare once a list is full.
//   k_ur_count    places them in the bins of the user's held-out thresholds (below).
//
//   k_topk_merge  places each slice's candidates by counting, with binary searches, the better entries of the other
//                 slices: every surviving candidate has a unique final position.
//
// Per-user ranking of held-out sets (sml_user_rank, sml_user_metrics):
//   k_ur_thresholds  one thread per held-out entry: its user, its threshold S(u, p) by score_chain, whether p is in Seen(u)
//   k_ur_merge       one pass of a segmented merge sort (run width w -> 2w inside every user's range): each entry's new
//                    place is its place in its run plus a binary-searched count of the smaller keys of the other run.
//                    Key order is `better` with NaN thresholds last, then the entry index: keys are distinct even when
//                    a range repeats an item, so the places form a permutation of the range whatever the input.
//   k_ur_count       every eligible item of the walk that is better than the user's
//                    worst threshold lands in ONE bin: the number of thresholds better than or equal to it (binary search
//                    over the sorted thresholds).  The score-only bound of `above` differs from it only when the item's
//                    score ties a threshold; such items add a -1 / +1 pair to delta bins.  Users with at most kUrWin
//                    non-NaN thresholds keep thresholds and bins in LDS; longer held-out sets are searched and counted
//                    in global memory (L2-resident).  Bin 0 stays in a register.
//   k_ur_finish      one workgroup per user: prefix sums over the bins give pos / above in sorted order, scattered back.
//   k_ur_metrics     one workgroup per user: hit counts and `first` by LDS atomics, then dcg / ap summed by one thread
//                    in ascending pos, read from a bitmap of the hit positions.
//
// Item filter (the sml_*_filtered entry points): a catalogue bitmap, one 32-bit word per tile, bit b of word t <=> item
// 32 t + b may appear.  The filter is per call, not per user, so a tile's word is wave-uniform: the walk reads it with a
// scalar load, ANDs it into the tile's eligibility word, and skips a tile whose word is 0 for the whole wave -- no item
// rows, no MFMAs, no callback; the double buffer prefetches the next NON-EMPTY tile of the slice.  The filtered kernels
// are instantiations of their own (F = true); the unfiltered ones compile to what they were without it.  k_filter_fill /
// k_filter_from_ids build a bitmap from a list of item ids.
//
// Adjusted score (the sml_*_adjusted entry points): A(u, i) = fmaf(S(u, i), scale[i], offset[i]), one more fp32 rounding
// per score, from a padded per-item table adj float [2][n_pad], n_pad = 32 * n_tiles (plane 0 scale, plane 1 offset).  A
// lane's 16 items of a tile are four runs of four consecutive rows (row_of), so the terms of a tile are four 16-byte loads
// per plane, the same for the 32 user lanes of a half; they are requested with the next tile's item rows and applied to
// the 16 accumulators, one explicit fmaf each, before the kernel's callable sees them -- the callables do not change.
// The thresholds (k_full_rank's thr, k_ur_thresholds' key) are the same expression on score_chain.  A skipped
// tile loads no adj; the last tile's loads end at n_pad, whose pad entries belong to items the eligibility word masks.
// The adjusted kernels are instantiations of their own (A = true).  k_adjust_fill / k_adjust_cosine build the table.
//
// Per-user candidate lists (sml_topk_candidates): k_topk_cand<D, T> at the end of the file orders each user's OWN list of item
// ids instead of walking the catalogue -- one wavefront per list, a lane per candidate, the row gathered whole and scored by
// score_chain on the VALU, the K best in the wave's LDS.  It shares score_chain, better, adjusted, offset_plane and
// lower_bound with the kernels above and changes none of them.
//
// Clustered index (sml_ivf_search): k_ivf_search<D, T>, beside k_topk_cand, is that kernel with another source of candidates --
// the members of the lists a user probes, walked as one virtual sequence through cumulative lengths in the wave's LDS -- and
// uses FullRow, score_chain, adjusted, better and cand_insert unchanged; ivf_host_walk is the same definition on the host
// (sml_host_ivf_search).  The centroid update of the index lives in ivf.hip.
//
// Deep lists (sml_topk_deep, 1 <= k <= 1,024): k_deep_count / k_deep_pick / k_deep_collect / k_deep_sort behind it select each
// user's k best by radix over an integer key of the score -- walk_slice callables that keep nothing sorted, so the cost is a
// fixed number of walks whatever k is -- and deep_host_walk is the same definition on the host (sml_host_topk_items).  For
// that walk score_chain, better and adjusted are __host__ __device__: the host and the kernels share the chain's text.
#include <climits>
#include <cmath>
#include <type_traits>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "width_dispatch.h"
#include "topk_list.h"
#include "../../include/sml_hip.h"

namespace {

constexpr int RT = 32;         // items per score tile = users per wave

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// S(u, i) in the k order of tile_scores(): the device-side definition every retrieval kernel agrees with, bit for bit
// (T = _Float16: x[s] and u[s] convert to float, exactly, as fmaf's arguments)
template <int D, class T>
__host__ __device__ __forceinline__ float score_chain(const T* __restrict__ u, const T* __restrict__ x) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        acc = fmaf(x[s], u[s], acc);
        acc = fmaf(x[s + D / 2], u[s + D / 2], acc);
    }
    return acc;
}

// The D/2 dims a lane half owns of one table row, as its 16-byte loads bring them: at(s) = dim h D/2 + s as fp32
template <int D, class T>
struct HalfRow;

template <int D>
struct HalfRow<D, float> {
    f32x4 f[D / 8];
    __device__ __forceinline__ void load(const float* __restrict__ row, int h) {
        const f32x4* p = reinterpret_cast<const f32x4*>(row + h * (D / 2));
#pragma unroll
        for (int q = 0; q < D / 8; ++q) f[q] = p[q];
    }
    __device__ __forceinline__ float at(int s) const { return f[s >> 2][s & 3]; }
    __device__ __forceinline__ void keep_packed() {}
};

// fp16 rows stay packed, eight dims per load and four VGPRs; a value is widened where it is used
template <int D>
struct HalfRow<D, _Float16> {
    f16x8 f[D / 16];
    __device__ __forceinline__ void load(const _Float16* __restrict__ row, int h) {
        const f16x8* p = reinterpret_cast<const f16x8*>(row + h * (D / 2));
#pragma unroll
        for (int q = 0; q < D / 16; ++q) f[q] = p[q];
    }
    __device__ __forceinline__ float at(int s) const { return (float)f[s >> 3][s & 7]; }
    // called on a row that outlives a loop: the widened copy of a loop-invariant row (D/2 more VGPRs) would otherwise be
    // hoisted out of the loop and held beside the packed one
    __device__ __forceinline__ void keep_packed() {
#pragma unroll
        for (int q = 0; q < D / 16; ++q) asm volatile("" : "+v"(f[q]));
    }
};

// 32 items (A) x 32 users (B): acc[r] = S(user lane & 31, item row_of(r, lane >> 5))
template <int D, class T>
__device__ __forceinline__ f32x16 tile_scores(const HalfRow<D, T>& a, const HalfRow<D, T>& b) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.at(s), b.at(s), acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// bit r of the result = bit row_of(r, h) of a tile's 32-item word, r = 0..15
__device__ __forceinline__ unsigned lane_rows(unsigned word, int h) {
    const unsigned x = word >> (4 * h);
    return (x & 0xFu) | ((x >> 4) & 0xF0u) | ((x >> 8) & 0xF00u) | ((x >> 12) & 0xF000u);
}

// (better, lower_bound and cand_insert: topk_list.h, shared with knn.hip)

// forward-only cursor over one user's ascending Seen range
struct SeenCursor {
    const int32_t* items;
    int64_t cur, end;
    long long nxt;
    __device__ void init(const int64_t* __restrict__ off, const int32_t* __restrict__ it, int64_t u, long long start) {
        items = it;
        if (!off) { cur = end = 0; nxt = LLONG_MAX; return; }
        end = off[u + 1];
        cur = lower_bound(off[u], end, [&](int64_t m) { return it[m] < start; });
        nxt = cur < end ? it[cur] : LLONG_MAX;
    }
    // the walk jumped over tiles: drop the Seen items below base (word() assumes that none is left)
    __device__ void skip_to(long long base) {
        if (nxt >= base) return;
        const int32_t* it = items;
        cur = lower_bound(cur + 1, end, [&](int64_t m) { return it[m] < base; });
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

// a lane's place in the grid of (32 * waves users) x slices: lane half h, user column j, the wave, its item slice and its
// row of the n users / test rows (rc: clamped to n - 1, so that lanes past the end read a real row)
struct LanePos {
    int h, j, wave, slice;
    int64_t row, rc;
    bool valid;
};

__device__ __forceinline__ LanePos lane_pos(int slices, int waves, int64_t n) {
    LanePos lp;
    const int lane = threadIdx.x & 63;
    lp.h = lane >> 5;
    lp.j = lane & 31;
    lp.wave = threadIdx.x >> 6;
    lp.slice = blockIdx.x % slices;
    lp.row = ((int64_t)(blockIdx.x / slices) * waves + lp.wave) * RT + lp.j;
    lp.valid = lp.row < n;
    lp.rc = lp.valid ? lp.row : n - 1;
    return lp;
}

// bit i set <=> item 32 t + i exists (< n_item); t < n_tiles, so at least bit 0 is set
__device__ __forceinline__ unsigned tile_items(int64_t t, int64_t n_item) {
    const int64_t left = n_item - t * RT;
    return left < RT ? (1u << left) - 1u : ~0u;
}

// the per-item score terms of the 16 items a lane holds of one tile: rows 8 g + 4 h + {0..3}, g = 0..3, are four floats at a
// 16-byte aligned address of each plane (tiles start at multiples of 32).  A = false: empty, and every use in the walk is
// under `if constexpr (A)`, so that the existing instantiations compile to the instructions they had
template <bool A>
struct TileTerms {};

template <>
struct TileTerms<true> {
    f32x4 sc[4], of[4];
    // base: the tile's first item, a multiple of 32 below n_pad, so every load ends at or before the plane's end
    __device__ __forceinline__ void load(const float* __restrict__ adj, int64_t n_pad, int64_t base, int h) {
        const f32x4* p = reinterpret_cast<const f32x4*>(adj + base + 4 * h);
        const f32x4* q = reinterpret_cast<const f32x4*>(adj + n_pad + base + 4 * h);
#pragma unroll
        for (int g = 0; g < 4; ++g) { sc[g] = p[2 * g]; of[g] = q[2 * g]; }
    }
    // acc[r] = S of item row_of(r, h) -> A: one fmaf each, rounded once, never left to contraction
    __device__ __forceinline__ f32x16 apply(const f32x16& acc) const {
        f32x16 out;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[r] = __builtin_fmaf(acc[r], sc[r >> 2][r & 3], of[r >> 2][r & 3]);
        return out;
    }
};

// plane 1 of adj [2][n_pad]
__device__ __forceinline__ const float* offset_plane(const float* adj, int64_t n_item) { return adj + (n_item + RT - 1) / RT * RT; }

// A(u, p) from s = S(u, p): the expression of TileTerms::apply, for the thresholds (A = false: s itself).  scale / offset:
// the two planes of adj
template <bool A>
__host__ __device__ __forceinline__ float adjusted(float s, const float* __restrict__ scale, const float* __restrict__ offset, int64_t p) {
    if constexpr (!A) return s;
    else return __builtin_fmaf(s, scale[p], offset[p]);
}

// The catalogue walk of one wave: user u's scores against every 32-item tile of the lane's slice, next tile's item rows
// in flight under the current tile's MFMAs.  tile(acc, base, elig) runs once per tile: acc[q] = S(u, base + row_of(q, h)),
// bit q of elig set <=> that item exists (< n_item), is not in Seen(u) and, with a filter, is allowed.  An empty slice
// loads nothing and calls nothing.
// F: `allow` holds one word per tile (bits past n_item are masked off here).  t, the words and the scan are wave-uniform
// (the slice comes from blockIdx), so the words travel through scalar loads and SGPRs.  A tile whose word is 0 is never
// visited: the scan for the next non-empty tile runs before the prefetch, and its first word -- tile t + 1's -- was
// requested one tile earlier, together with that tile's item rows (`pre`).  A slice without a non-empty tile returns at once.
// A: acc[q] is A(u, i) = fmaf(S(u, i), scale[i], offset[i]) instead, the terms read from adj (float [2][32 * n_tiles]).
template <int D, class T, bool F, bool A, class Tile>
__device__ __forceinline__ void walk_slice(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item, int64_t u,
                                           const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                           const uint32_t* __restrict__ allow, const float* __restrict__ adj, const LanePos& lp,
                                           int slice_tiles, Tile&& tile) {
    const int64_t n_tiles = (n_item + RT - 1) / RT;
    const int64_t t0 = (int64_t)lp.slice * slice_tiles;
    const int64_t t1 = t0 + slice_tiles < n_tiles ? t0 + slice_tiles : n_tiles;
    if (t0 >= t1) return;
    int64_t t = t0;
    unsigned w = 0, pre = 0;                             // F: the current tile's word; the raw word of tile t + 1
    if constexpr (F) {
        while (t < t1 && !(w = allow[t] & tile_items(t, n_item))) ++t;
        if (t >= t1) return;
        if (t + 1 < t1) pre = allow[t + 1];
    }
    HalfRow<D, T> b;
    b.load(wu + u * D, lp.h);
    SeenCursor sc;
    sc.init(seen_off, seen_items, u, t * RT);
    HalfRow<D, T> a, an;
    int64_t ia = t * RT + lp.j;
    a.load(wi + (ia < n_item ? ia : n_item - 1) * D, lp.h);
    TileTerms<A> m, mn;
    if constexpr (A) m.load(adj, n_tiles * RT, t * RT, lp.h);
    for (int64_t tn; t < t1; t = tn) {
        tn = t + 1;
        unsigned wn = pre;
        if constexpr (F) {
            while (tn < t1 && !(wn &= tile_items(tn, n_item)))
                if (++tn < t1) wn = allow[tn];
            if (tn + 1 < t1) pre = allow[tn + 1];
        }
        if (tn < t1) {
            ia = tn * RT + lp.j;
            an.load(wi + (ia < n_item ? ia : n_item - 1) * D, lp.h);
            if constexpr (A) mn.load(adj, n_tiles * RT, tn * RT, lp.h);
        }
        b.keep_packed();
        f32x16 acc = tile_scores<D, T>(a, b);
        if constexpr (A) acc = m.apply(acc);
        const int64_t base = t * RT;
        if constexpr (F) sc.skip_to(base);
        // bit i of `real`: item base + i exists, is not in Seen (and is allowed)
        const unsigned real = ~sc.word(base) & (F ? w : tile_items(t, n_item));
        tile(acc, base, lane_rows(real, lp.h));
        a = an;
        if constexpr (A) m = mn;
        w = wn;
    }
}

template <int D, class T, bool F, bool A>
__global__ __launch_bounds__(256) void k_full_rank(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                   const int64_t* __restrict__ rows, int64_t n, int n_cols,
                                                   const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                   const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                   int slice_tiles, int32_t* __restrict__ rank) {
    const LanePos lp = lane_pos(slices, blockDim.x >> 6, n);
    const int64_t u = rows[lp.rc * n_cols], p = rows[lp.rc * n_cols + 1];
    const float thr = adjusted<A>(score_chain<D>(wu + u * D, wi + p * D), adj, A ? offset_plane(adj, n_item) : nullptr, p);
    int cnt = 0;
    walk_slice<D, T, F, A>(wu, wi, n_item, u, seen_off, seen_items, allow, adj, lp, slice_tiles, [&](const f32x16& acc, int64_t base, unsigned elig) {
#pragma unroll
        for (int q = 0; q < 16; ++q) cnt += (acc[q] > thr) & ((elig >> q) & 1u) & (base + row_of(q, lp.h) != p);
    });
    cnt += __shfl_xor(cnt, 32, 64);
    if (lp.h == 0 && lp.valid && cnt) atomicAdd(rank + lp.row, cnt);
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

// k_topk_slice, k_ur_thresholds and k_ur_count keep their code in a __forceinline__ body that the kernel only forwards to.
// Folded into their kernels these three, which store to global memory between their loads, compile to other code
// (k_topk_slice 7 to 31 instructions longer in every instantiation): the body's __restrict__ parameters become alias scopes
// where it is inlined, and those evidently tell the compiler more than the same qualifiers on a __global__ function's
// parameters do.  k_full_rank, whose only write is an atomic, is the same code either way and has no body.

// candidates of user x, slice s: cand_s / cand_i [(x * slices + s) * k + q], cand_n [x * slices + s]
template <int D, class T, bool F, bool A>
__device__ __forceinline__ void topk_slice_body(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                const int64_t* __restrict__ users, int64_t n, int k,
                                                const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                int slice_tiles, float* __restrict__ cand_s, int32_t* __restrict__ cand_i,
                                                int32_t* __restrict__ cand_n) {
    extern __shared__ float lds[];
    const LanePos lp = lane_pos(slices, blockDim.x >> 6, n);
    const int h = lp.h, j = lp.j;
    float* ls = lds + (size_t)lp.wave * 2 * k * RT;
    int* li = reinterpret_cast<int*>(ls + k * RT);
    const int64_t u = users[lp.rc];
    int cnt = 0;                          // live entries of user j's list (both lane halves keep it)
    float thr_s = -INFINITY;              // register copy of the K-th entry: lags the list, never ahead of it
    int thr_i = INT_MAX;
    walk_slice<D, T, F, A>(wu, wi, n_item, u, seen_off, seen_items, allow, adj, lp, slice_tiles, [&](const f32x16& acc, int64_t base, unsigned elig) {
        unsigned pass = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const bool ok = lp.valid && ((elig >> q) & 1u) && better(acc[q], (int)(base + row_of(q, h)), thr_s, thr_i);
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
    });
    if (!lp.valid) return;                // an empty slice still writes its (empty) candidate slots and cand_n
    const int64_t o = (lp.row * slices + lp.slice) * k;
    for (int q = h; q < k; q += 2) {
        const bool live = q < cnt;
        cand_s[o + q] = live ? ls[q * RT + j] : -INFINITY;
        cand_i[o + q] = live ? li[q * RT + j] : -1;
    }
    if (h == 0) cand_n[lp.row * slices + lp.slice] = cnt;
}

template <int D, class T, bool F, bool A>
__global__ __launch_bounds__(256) void k_topk_slice(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                    const int64_t* __restrict__ users, int64_t n, int k,
                                                    const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                    const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                    int slice_tiles, float* __restrict__ cand_s, int32_t* __restrict__ cand_i,
                                                    int32_t* __restrict__ cand_n) {
    topk_slice_body<D, T, F, A>(wu, wi, n_item, users, n, k, seen_off, seen_items, allow, adj, slices, slice_tiles, cand_s, cand_i, cand_n);
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
        // entries [0, lower bound) of slice t are better than the candidate
        pos += lower_bound(0, cn[t], [&](int m) { return better(cand_s[ot + m], cand_i[ot + m], cs, ci); });
    }
    if (pos < k) { items[x * k + pos] = ci; scores[x * k + pos] = cs; }
}

constexpr int kRankWaves = 4;

// the grid of a catalogue walk over n users with `waves` waves per workgroup: `groups` workgroup rows x `slices` item
// slices (a multiple of 8, one XCD per residue, about target_blocks workgroups in all) of slice_tiles tiles each
struct SliceGrid {
    int64_t groups;
    int slices, slice_tiles;
};

SliceGrid plan_grid(int64_t n, int waves, int64_t n_item, int64_t target_blocks, int max_mult) {
    const int64_t groups = (n + RT * waves - 1) / (RT * waves);
    const int64_t n_tiles = (n_item + RT - 1) / RT;
    int64_t m = (target_blocks + 8 * groups - 1) / (8 * groups);
    if (m < 1) m = 1;
    if (m > max_mult) m = max_mult;
    while (m > 1 && n_tiles / (8 * m) < 16) --m;      // keep at least 16 tiles per slice
    return {groups, (int)(8 * m), (int)((n_tiles + 8 * m - 1) / (8 * m))};
}

SliceGrid rank_grid(int64_t n, int waves, int64_t n_item) { return plan_grid(n, waves, n_item, 8192, 64); }

int topk_waves(int k) {
    const int per_wave = 2 * k * RT * 4;
    int w = 65536 / per_wave;
    return w > 4 ? 4 : w;
}

SliceGrid topk_grid(int64_t n, int k, int64_t n_item) { return plan_grid(n, topk_waves(k), n_item, 2048, 4); }

// the one place that turns a catalogue -- embedding width, element type, filter or none, terms or none -- into template
// arguments: f(D, F, A, wu, wi) with D a std::integral_constant, F and A std::bool_constants and the tables typed (fp32:
// d = 32 / 64; fp16, elem_bytes 2: d = 32 / 64 / 128).  A kernel named inside the generic callable depends on D and the
// tables' type, so only the pairs called here are instantiated.  false: a pair the kernels do not exist for, nothing was
// called -- the launchers' refusal, and what sml_retrieval_supports asks
template <class Fn>
bool with_width(const SmlCatalogue& c, Fn&& f) {
    return with_pair<RetrievalPairs>(c.d, c.elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        const T* wu = static_cast<const T*>(c.wu);
        const T* wi = static_cast<const T*>(c.wi);
        if (c.allow && c.adj) f(dd, std::true_type(), std::true_type(), wu, wi);
        else if (c.adj) f(dd, std::false_type(), std::true_type(), wu, wi);
        else if (c.allow) f(dd, std::true_type(), std::false_type(), wu, wi);
        else f(dd, std::false_type(), std::false_type(), wu, wi);
    });
}

// the element type of a typed table pointer, as the kernels' T
template <class P>
using elem_t = std::remove_const_t<std::remove_pointer_t<P>>;

// ---- per-user ranking of held-out sets ------------------------------------------------------------------------------

constexpr int kUrWin = 32;         // non-NaN thresholds per user kept in LDS; longer sets go through global memory
constexpr int kUrWaves = 4;
constexpr int kUrBlock = 256;      // threads of the per-user finishing / metric workgroups

// sort order of a user's held-out entries: `better` on (threshold, id), NaN thresholds last (by id), then the entry
// index x (unique), so that no two entries compare equal
__device__ __forceinline__ bool ur_less(float s, int i, int x, float ts, int ti, int tx) {
    const bool na = s != s, nb = ts != ts;
    if (na != nb) return nb;
    if (i == ti && (na || s == ts)) return x < tx;
    return na ? i < ti : better(s, i, ts, ti);
}

// x with off[x] <= e < off[x + 1] (off non-decreasing, off[0] = 0 <= e < off[n])
__device__ __forceinline__ int64_t ur_segment(const int64_t* __restrict__ off, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// in_seen[e] = 1: the held-out item is not eligible by id -- in Seen(u) or, with a filter (F), not allowed
template <int D, class T, bool F, bool A>
__device__ __forceinline__ void ur_thresholds_body(const T* __restrict__ wu, const T* __restrict__ wi,
                                                   const int64_t* __restrict__ users, int64_t n,
                                                   const int64_t* __restrict__ pos_off, const int32_t* __restrict__ pos_items,
                                                   int64_t n_pos, const int64_t* __restrict__ seen_off,
                                                   const int32_t* __restrict__ seen_items, const uint32_t* __restrict__ allow,
                                                   const float* __restrict__ scale, const float* __restrict__ offset,
                                                   int32_t* __restrict__ seg, float* __restrict__ ks, int32_t* __restrict__ ki,
                                                   int32_t* __restrict__ kx, int32_t* __restrict__ in_seen) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pos) return;
    const int64_t x = ur_segment(pos_off, n, e);
    const int64_t u = users[x];
    const int32_t p = pos_items[e];
    int sn = 0;
    if (seen_off) {
        const int64_t end = seen_off[u + 1];
        const int64_t lo = lower_bound(seen_off[u], end, [&](int64_t m) { return seen_items[m] < p; });
        sn = lo < end && seen_items[lo] == p;
    }
    if constexpr (F) sn |= !((allow[p >> 5] >> (p & 31)) & 1u);
    seg[e] = (int32_t)x;
    ks[e] = adjusted<A>(score_chain<D>(wu + u * D, wi + (int64_t)p * D), scale, offset, p);
    ki[e] = p;
    kx[e] = (int32_t)e;
    in_seen[e] = sn;
}

template <int D, class T, bool F, bool A>
__global__ __launch_bounds__(256) void k_ur_thresholds(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                       const int64_t* __restrict__ users, int64_t n,
                                                       const int64_t* __restrict__ pos_off, const int32_t* __restrict__ pos_items,
                                                       int64_t n_pos, const int64_t* __restrict__ seen_off,
                                                       const int32_t* __restrict__ seen_items, const uint32_t* __restrict__ allow,
                                                       const float* __restrict__ adj, int32_t* __restrict__ seg, float* __restrict__ ks,
                                                       int32_t* __restrict__ ki, int32_t* __restrict__ kx, int32_t* __restrict__ in_seen) {
    ur_thresholds_body<D, T, F, A>(wu, wi, users, n, pos_off, pos_items, n_pos, seen_off, seen_items, allow, adj,
                                   A ? offset_plane(adj, n_item) : nullptr, seg, ks, ki, kx, in_seen);
}

// runs [a0, a0 + w) and [a0 + w, a0 + 2w) of every user's range -> one sorted run
__global__ __launch_bounds__(256) void k_ur_merge(const int64_t* __restrict__ pos_off, const int32_t* __restrict__ seg,
                                                  int64_t n_pos, int64_t w, const float* __restrict__ is,
                                                  const int32_t* __restrict__ ii, const int32_t* __restrict__ ix,
                                                  float* __restrict__ os, int32_t* __restrict__ oi, int32_t* __restrict__ ox) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_pos) return;
    const int64_t x = seg[e];
    const int64_t lo = pos_off[x], hi = pos_off[x + 1];
    const int64_t a0 = lo + (e - lo) / (2 * w) * (2 * w);
    const int64_t mid = a0 + w < hi ? a0 + w : hi;
    const int64_t end = a0 + 2 * w < hi ? a0 + 2 * w : hi;
    const float s = is[e];
    const int32_t i = ii[e], xe = ix[e];
    const auto smaller = [&](int64_t m) { return ur_less(is[m], ii[m], ix[m], s, i, xe); };
    // the entry's place in its own run plus the number of smaller keys of the other run
    const int64_t o = e < mid ? e + (lower_bound(mid, end, smaller) - mid) : a0 + (e - mid) + (lower_bound(a0, mid, smaller) - a0);
    os[o] = s;
    oi[o] = i;
    ox[o] = xe;
}

// place (s, i), an eligible item better than the user's worst threshold, among the mv sorted thresholds ts / ti (stride
// st): k = #{thresholds better than or equal to it} < mv goes to pos bin k.  The above bin is k too unless s ties t_k;
// then it is ka = #{thresholds >= s} > k, recorded as -1 at k and +1 at ka of the delta bins (bd).  Bins 0 stay in the
// registers c0 / d0.
__device__ __forceinline__ void ur_place(const float* ts, const int32_t* ti, int64_t st, int64_t mv, float s, int i, float t0s,
                                         int t0i, int32_t* bp, int32_t* bd, int& c0, int& d0) {
    int64_t k = 0;
    if (!better(s, i, t0s, t0i)) {
        // t_0 is better or equal, t_{mv-1} is not: neither is read
        k = lower_bound<int64_t>(1, mv - 1, [&](int64_t m) { return !better(s, i, ts[m * st], ti[m * st]); });
    }
    const float tk = k ? ts[k * st] : t0s;
    if (k == 0) ++c0; else atomicAdd(bp + k * st, 1);
    if (!(s > tk)) {                       // s == t_k: thresholds k .. ka - 1 tie with s
        const int64_t l = lower_bound(k + 1, mv, [&](int64_t m) { return !(s > ts[m * st]); });
        if (k == 0) --d0; else atomicAdd(bd + k * st, -1);
        if (l < mv) atomicAdd(bd + l * st, 1);
    }
}

// ss / si: every user's thresholds and ids in ur_less order.  At sorted place b of user x, bin_p (zeroed) receives the
// number of eligible items whose pos bound is b, and bin_d (zeroed) what turns those counts into the above bounds'
template <int D, class T, bool F, bool A>
__device__ __forceinline__ void ur_count_body(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                              const int64_t* __restrict__ users, int64_t n,
                                              const int64_t* __restrict__ pos_off,
                                              const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                              const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                              int slice_tiles, const float* __restrict__ ss, const int32_t* __restrict__ si,
                                              int32_t* __restrict__ bin_p, int32_t* __restrict__ bin_d) {
    __shared__ float l_s[kUrWaves][kUrWin * RT];
    __shared__ int32_t l_i[kUrWaves][kUrWin * RT];
    __shared__ int32_t l_p[kUrWaves][kUrWin * RT];
    __shared__ int32_t l_d[kUrWaves][kUrWin * RT];
    const LanePos lp = lane_pos(slices, kUrWaves, n);
    const int h = lp.h, j = lp.j, wave = lp.wave;
    const bool valid = lp.valid;
    const int64_t u = users[lp.rc];
    const int64_t lo = pos_off[lp.rc];
    // non-NaN thresholds (the NaN ones sort last)
    const int64_t mv = lower_bound<int64_t>(0, valid ? pos_off[lp.rc + 1] - lo : 0, [&](int64_t m) { return ss[lo + m] == ss[lo + m]; });
    // users with at most kUrWin thresholds: thresholds and bins in LDS column j; longer sets: the user's global range
    const bool win = mv <= kUrWin;
    for (int k = h; k < kUrWin; k += 2) {
        l_s[wave][k * RT + j] = win && k < mv ? ss[lo + k] : 0.0f;
        l_i[wave][k * RT + j] = win && k < mv ? si[lo + k] : 0;
        l_p[wave][k * RT + j] = 0;
        l_d[wave][k * RT + j] = 0;
    }
    __syncthreads();
    const float t0s = mv ? ss[lo] : 0.0f, tws = mv ? ss[lo + mv - 1] : 0.0f;
    const int t0i = mv ? si[lo] : 0, twi = mv ? si[lo + mv - 1] : 0;
    int c0 = 0, d0 = 0;
    walk_slice<D, T, F, A>(wu, wi, n_item, u, seen_off, seen_items, allow, adj, lp, slice_tiles, [&](const f32x16& acc, int64_t base, unsigned elig) {
        unsigned live = 0;                 // NaN scores fail `better`; an item not better than the worst threshold is in no bin
        if (mv) {
#pragma unroll
            for (int q = 0; q < 16; ++q) live |= (unsigned)better(acc[q], (int)(base + row_of(q, h)), tws, twi) << q;
            live &= elig;
        }
        if (!live) return;
        if (win) {
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((live >> q) & 1u)
                    ur_place(&l_s[wave][j], &l_i[wave][j], RT, mv, acc[q], (int)(base + row_of(q, h)), t0s, t0i, &l_p[wave][j],
                             &l_d[wave][j], c0, d0);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((live >> q) & 1u)
                    ur_place(ss + lo, si + lo, 1, mv, acc[q], (int)(base + row_of(q, h)), t0s, t0i, bin_p + lo, bin_d + lo, c0, d0);
        }
    });
    c0 += __shfl_xor(c0, 32, 64);
    d0 += __shfl_xor(d0, 32, 64);
    if (valid && h == 0) {
        if (c0) atomicAdd(bin_p + lo, c0);
        if (d0) atomicAdd(bin_d + lo, d0);
    }
    __syncthreads();
    if (valid && win) {
        for (int k = 1 + h; k < mv; k += 2) {
            const int32_t vp = l_p[wave][k * RT + j], vd = l_d[wave][k * RT + j];
            if (vp) atomicAdd(bin_p + lo + k, vp);
            if (vd) atomicAdd(bin_d + lo + k, vd);
        }
    }
}

template <int D, class T, bool F, bool A>
__global__ __launch_bounds__(64 * kUrWaves) void k_ur_count(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                            const int64_t* __restrict__ users, int64_t n,
                                                            const int64_t* __restrict__ pos_off,
                                                            const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                            const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                            int slice_tiles, const float* __restrict__ ss, const int32_t* __restrict__ si,
                                                            int32_t* __restrict__ bin_p, int32_t* __restrict__ bin_d) {
    ur_count_body<D, T, F, A>(wu, wi, n_item, users, n, pos_off, seen_off, seen_items, allow, adj, slices, slice_tiles, ss, si, bin_p, bin_d);
}

// ---- adjusted score: the table builders of sml_item_adjust_* ------------------------------------------------------------

// adj [2][n_pad] from optional per-item arrays: NULL scale = 1, NULL offset = +0; the pad entries are written (1, 0)
__global__ __launch_bounds__(256) void k_adjust_fill(const float* __restrict__ scale, const float* __restrict__ offset, int64_t n_item,
                                                     int64_t n_pad, float* __restrict__ adj) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    adj[i] = scale && i < n_item ? scale[i] : 1.0f;
    adj[n_pad + i] = offset && i < n_item ? offset[i] : 0.0f;
}

// plane 0 of adj = 1 / ||x_i||, the squared norm by the score chain with the row on both sides; a zero row (and a row
// whose chain is NaN) gets 0.  sqrtf and the division are the correctly rounded ones (the build has no fast-math flag)
template <int D, class T>
__global__ __launch_bounds__(256) void k_adjust_cosine(const T* __restrict__ wi, int64_t n_item, int64_t n_pad, float* __restrict__ adj) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    float s = 1.0f;
    if (i < n_item) {
        const float n2 = score_chain<D>(wi + i * D, wi + i * D);
        s = n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
    }
    adj[i] = s;
}

// ---- item filter from a list of ids -----------------------------------------------------------------------------------

// every word allows nothing (invert = 0) or every item below n_item (invert = 1: the tail bits of the last word stay 0)
__global__ __launch_bounds__(256) void k_filter_fill(uint32_t* __restrict__ words, int64_t n_words, int64_t n_item, int invert) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_words) words[t] = invert ? tile_items(t, n_item) : 0u;
}

// one thread per id: set (or, inverted, clear) its bit.  Atomic OR / AND commute, so duplicates and order do not matter
__global__ __launch_bounds__(256) void k_filter_from_ids(const int32_t* __restrict__ ids, int64_t n_ids, int invert,
                                                         uint32_t* __restrict__ words) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ids) return;
    const int32_t i = ids[e];
    if (invert) atomicAnd(words + (i >> 5), ~(1u << (i & 31)));
    else atomicOr(words + (i >> 5), 1u << (i & 31));
}

// inclusive prefix sum of v over the workgroup (kUrBlock threads); *total = the sum of all
__device__ __forceinline__ int64_t ur_block_scan(int64_t v, int64_t* sh, int64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kUrBlock / 64; ++q) {
        before += q < wave ? sh[q] : 0;
        all += sh[q];
    }
    __syncthreads();
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(kUrBlock) void k_ur_finish(const int64_t* __restrict__ pos_off, const float* __restrict__ ss,
                                                        const int32_t* __restrict__ sx, const int32_t* __restrict__ in_seen,
                                                        const int32_t* __restrict__ bin_p, const int32_t* __restrict__ bin_d,
                                                        int32_t* __restrict__ above, int32_t* __restrict__ pos) {
    __shared__ int64_t sh[2][kUrBlock / 64];
    const int64_t x = blockIdx.x;
    const int64_t lo = pos_off[x], m = pos_off[x + 1] - lo;
    int64_t cp = 0, ca = 0;
    for (int64_t c = 0; c < m; c += kUrBlock) {
        const int64_t k = c + threadIdx.x;
        const bool in = k < m;
        int64_t tp, ta;
        const int64_t ip = ur_block_scan(in ? bin_p[lo + k] : 0, sh[0], &tp);
        const int64_t ia = ur_block_scan(in ? (int64_t)bin_p[lo + k] + bin_d[lo + k] : 0, sh[1], &ta);
        if (in) {
            const int32_t e = sx[lo + k];
            const bool nan = ss[lo + k] != ss[lo + k];
            above[e] = nan ? 0 : (int32_t)(ca + ia);
            pos[e] = nan || in_seen[e] ? -1 : (int32_t)(cp + ip);
        }
        cp += tp;
        ca += ta;
    }
}

struct UrKs { int k[8]; };

__global__ __launch_bounds__(kUrBlock) void k_ur_metrics(const int32_t* __restrict__ pos, const int64_t* __restrict__ pos_off,
                                                         UrKs ks, int n_k, int32_t* __restrict__ hits, float* __restrict__ dcg,
                                                         float* __restrict__ ap, int32_t* __restrict__ first) {
    constexpr int kWords = 1024;           // bitmap window: 32,768 consecutive positions
    __shared__ unsigned bm[kWords];
    __shared__ int cnt[8];
    __shared__ int fmin;
    const int64_t x = blockIdx.x;
    const int64_t lo = pos_off[x], m = pos_off[x + 1] - lo;
    int kmax = 0;
    for (int q = 0; q < n_k; ++q) kmax = ks.k[q] > kmax ? ks.k[q] : kmax;
    if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) fmin = INT_MAX;
    __syncthreads();
    for (int64_t k = threadIdx.x; k < m; k += kUrBlock) {
        const int p = pos[lo + k];
        if (p < 0) continue;
        atomicMin(&fmin, p);
        for (int q = 0; q < n_k; ++q)
            if (p < ks.k[q]) atomicAdd(&cnt[q], 1);
    }
    __syncthreads();
    int total = 0;                         // hits at the largest K
    for (int q = 0; q < n_k; ++q) total = ks.k[q] == kmax ? cnt[q] : total;
    // thread 0 walks the distinct hit positions in ascending order; the sums at K are recorded when the walk reaches a
    // position >= K, or after it.  With pos values unique in the range (as sml_user_rank writes them) jj reaches total
    // and the walk ends early; a repeated value is one bit of the bitmap and is summed once.
    float sd = 0.0f, sa = 0.0f;
    int jj = 0;
    unsigned done = 0;                     // bit q: dcg / ap at ks.k[q] written
    for (int64_t v0 = 0; v0 < kmax && __syncthreads_or(threadIdx.x == 0 && jj < total); v0 += 32 * kWords) {
        for (int w = threadIdx.x; w < kWords; w += kUrBlock) bm[w] = 0u;
        __syncthreads();
        for (int64_t k = threadIdx.x; k < m; k += kUrBlock) {
            const int64_t p = pos[lo + k];
            if (p >= v0 && p < v0 + 32 * kWords && p < kmax) atomicOr(&bm[(p - v0) >> 5], 1u << ((p - v0) & 31));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 0; w < kWords && jj < total; ++w) {
                unsigned bits = bm[w];
                while (bits) {
                    const int bit = __builtin_ctz(bits);
                    bits &= bits - 1;
                    const int64_t pi = v0 + 32 * w + bit;
                    for (int q = 0; q < n_k; ++q)
                        if (!((done >> q) & 1u) && pi >= ks.k[q]) {
                            dcg[x * n_k + q] = sd;
                            ap[x * n_k + q] = sa;
                            done |= 1u << q;
                        }
                    const float pp = (float)pi;
                    ++jj;
                    sd += 1.0f / log2f(pp + 2.0f);
                    sa += (float)jj / (pp + 1.0f);
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        for (int q = 0; q < n_k; ++q)
            if (!((done >> q) & 1u)) { dcg[x * n_k + q] = sd; ap[x * n_k + q] = sa; }
    }
    if (threadIdx.x < n_k) hits[x * n_k + threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0) first[x] = fmin == INT_MAX ? -1 : fmin;
}

// ---- per-user candidate lists (sml_topk_candidates) ------------------------------------------------------------------------

constexpr int kCandWaves = 4;      // lists per workgroup: one wavefront each
constexpr int kCandRounds = 2;     // rounds of 64 candidates whose rows a lane has in flight at once
constexpr int kCandMaxK = 128;

// one table row in a lane's registers, as its 16-byte loads bring it (fp16: packed, D/2 VGPRs); v is what score_chain reads
template <int D, class T>
struct FullRow {
    alignas(16) T v[D];
    __device__ __forceinline__ void load(const T* __restrict__ row) {
        typedef f32x4 __attribute__((may_alias)) piece;      // 16 bytes of the row, whatever T is
        constexpr int N = D * (int)sizeof(T) / 16;
        const piece* p = reinterpret_cast<const piece*>(row);
        piece* q = reinterpret_cast<piece*>(v);
#pragma unroll
        for (int c = 0; c < N; ++c) q[c] = p[c];
    }
    // the same row by a whole wave, one 16-byte piece per lane (an LDS copy of a wave-uniform row)
    __device__ __forceinline__ void load_by_wave(const T* __restrict__ row, int lane) {
        typedef f32x4 __attribute__((may_alias)) piece;
        constexpr int N = D * (int)sizeof(T) / 16;
        if (lane < N) reinterpret_cast<piece*>(v)[lane] = reinterpret_cast<const piece*>(row)[lane];
    }
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int s = 0; s < D; ++s) v[s] = (T)0;
    }
};

// One wavefront per list, lists walked grid-stride; 64 candidates per round, kCandRounds rounds per step.  A lane reads its
// entry, tests range, filter bit and Seen (a bisection of the user's ascending range) and, if the entry survives, gathers
// the item's whole row with 16-byte loads -- the rows of all rounds of a step are requested before the first is scored.
// The score is score_chain on the VALU against the user row, which is wave-uniform and loaded once per list; with adj one
// explicit fmaf follows (adjusted<true>), without it none.  The K best live in the wave's LDS (cand_insert); a copy of the
// K-th entry is the threshold, only lanes that beat it insert, in lane order, and the survivors are tested again whenever
// the threshold moves.  allow, adj, Seen and the candidates' form and width are wave-uniform branches on the arguments.
// A list of any length is walked by its one wave.
template <int D, class T>
__global__ __launch_bounds__(64 * kCandWaves) void k_topk_cand(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                                const int64_t* __restrict__ users, int64_t n,
                                                                const void* __restrict__ cand, int cand_wide,
                                                                const int64_t* __restrict__ cand_off, int64_t cand_stride,
                                                                int64_t cand_first, int64_t cand_cols, int k,
                                                                const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                                const uint32_t* __restrict__ allow, const float* __restrict__ adj,
                                                                int32_t* __restrict__ items, float* __restrict__ scores,
                                                                int32_t* __restrict__ n_elig) {
    __shared__ float l_s[kCandWaves][kCandMaxK];
    __shared__ int32_t l_i[kCandWaves][kCandMaxK];
    __shared__ FullRow<D, T> l_u[kCandWaves];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const ls = l_s[wave];
    int32_t* const li = l_i[wave];
    const float* const offset = adj ? offset_plane(adj, n_item) : nullptr;
    const int64_t* const c64 = static_cast<const int64_t*>(cand);
    const int32_t* const c32 = static_cast<const int32_t*>(cand);

    for (int64_t x = (int64_t)blockIdx.x * kCandWaves + wave; x < n; x += (int64_t)gridDim.x * kCandWaves) {
        const int64_t u = users[x];
        const int64_t base = cand_off ? cand_off[x] : x * cand_stride + cand_first;
        const int64_t len = cand_off ? cand_off[x + 1] - base : cand_cols;
        l_u[wave].load_by_wave(wu + u * D, lane);
        const int64_t s_lo = seen_off ? seen_off[u] : 0, s_hi = seen_off ? seen_off[u + 1] : 0;
        int cnt = 0, ne = 0;
        float thr_s = -INFINITY;              // the K-th entry once the list is full
        int thr_i = INT_MAX;
        for (int64_t b = 0; b < len; b += 64 * kCandRounds) {
            FullRow<D, T> xr[kCandRounds];
            int ci[kCandRounds];
            bool ok[kCandRounds];
            float sc[kCandRounds], of[kCandRounds];
#pragma unroll
            for (int r = 0; r < kCandRounds; ++r) {
                const int64_t e = b + 64 * r + lane;
                long long c = -1;
                if (e < len) c = cand_wide ? (long long)c64[base + e] : (long long)c32[base + e];
                bool good = c >= 0 && c < n_item;         // anything else is padding: no address is formed from it
                if (good && allow) good = (allow[c >> 5] >> (c & 31)) & 1u;
                if (good && s_lo < s_hi) {
                    const int32_t cc = (int32_t)c;
                    const int64_t at = lower_bound(s_lo, s_hi, [&](int64_t m) { return seen_items[m] < cc; });
                    good = !(at < s_hi && seen_items[at] == cc);
                }
                xr[r].zero();
                sc[r] = 1.0f;
                of[r] = 0.0f;
                if (good) {
                    xr[r].load(wi + c * D);
                    if (adj) { sc[r] = adj[c]; of[r] = offset[c]; }
                }
                ci[r] = good ? (int)c : -1;
                ok[r] = good;
            }
            // the user row is read from LDS where a value feeds its fmaf (every lane the same address: a broadcast); held in
            // registers over the loop it would cost D VGPRs (fp16: the widened copy), more than an item row
            asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < kCandRounds; ++r) {
                float s = score_chain<D, T>(l_u[wave].v, xr[r].v);
                if (adj) s = adjusted<true>(s, &sc[r], &of[r], 0);
                const bool elig = ok[r] && s == s;
                ne += __popcll(__ballot(elig));
                unsigned long long m = __ballot(elig && (cnt < k || better(s, ci[r], thr_s, thr_i)));
                while (m) {
                    const int l = __builtin_ctzll(m);
                    cand_insert(ls, li, k, lane, cnt, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)),
                                __builtin_amdgcn_readlane(ci[r], l));
                    m &= m - 1;
                    if (cnt == k) {
                        thr_s = ls[k - 1];
                        thr_i = li[k - 1];
                        m &= __ballot(elig && better(s, ci[r], thr_s, thr_i));
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < k; q += 64) {
            const bool live = q < cnt;
            items[x * k + q] = live ? li[q] : -1;
            scores[x * k + q] = live ? ls[q] : -INFINITY;
        }
        if (n_elig && lane == 0) n_elig[x] = ne;
        __builtin_amdgcn_wave_barrier();      // the next list's inserts come after these reads
    }
}

// ---- clustered index (sml_ivf_search) ------------------------------------------------------------------------------------

constexpr int kIvfMaxProbe = 128;  // probes per user: two per lane

// inclusive sum over the wave's lanes, in lane order (integers: exact whatever the order)
__device__ __forceinline__ long long wave_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// k_topk_cand with another source of candidates: the members of the lists a user probes, in probe order, as ONE virtual
// sequence -- the lists are short and uneven, and a wave that walked them one by one would run most rounds partly empty.
// Per user: lane l reads probes l and l + 64 (a probe outside [0, n_list) is padding: length 0, no address is formed) and both
// ends of their lists; a wave scan leaves the inclusive cumulative lengths and the list starts in the wave's LDS; then, in
// rounds of 64 (kCandRounds in flight), lane l maps virtual index e to (probe j, e - cum[j - 1]) by a bisection of the
// cumulative lengths (empty lists have no index, so they are stepped over), reads list_items[start[j] + that] and goes on
// exactly as k_topk_cand does with a candidate: range, filter bit, Seen bisection, row gather, chain, optional fmaf, ballot,
// threshold, insert.  A list probed twice is walked twice; cand_insert drops the repeats, n_elig counts them.
template <int D, class T>
__global__ __launch_bounds__(64 * kCandWaves) void k_ivf_search(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                                 const int64_t* __restrict__ users, int64_t n,
                                                                 const int64_t* __restrict__ list_off, const int32_t* __restrict__ list_items,
                                                                 int n_list, const int32_t* __restrict__ probes, int nprobe, int k,
                                                                 const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                                 const uint32_t* __restrict__ allow, const float* __restrict__ adj,
                                                                 int32_t* __restrict__ items, float* __restrict__ scores,
                                                                 int32_t* __restrict__ n_elig) {
    __shared__ float l_s[kCandWaves][kCandMaxK];
    __shared__ int32_t l_i[kCandWaves][kCandMaxK];
    __shared__ FullRow<D, T> l_u[kCandWaves];
    __shared__ long long l_cum[kCandWaves][kIvfMaxProbe];      // inclusive cumulative lengths of the probed lists
    __shared__ int32_t l_start[kCandWaves][kIvfMaxProbe];      // where each probed list starts in list_items (< n_item < 2^31)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* const ls = l_s[wave];
    int32_t* const li = l_i[wave];
    long long* const cum = l_cum[wave];
    int32_t* const start = l_start[wave];
    const float* const offset = adj ? offset_plane(adj, n_item) : nullptr;

    for (int64_t x = (int64_t)blockIdx.x * kCandWaves + wave; x < n; x += (int64_t)gridDim.x * kCandWaves) {
        const int64_t u = users[x];
        l_u[wave].load_by_wave(wu + u * D, lane);
        long long len0 = 0, len1 = 0;
        int st0 = 0, st1 = 0;
        if (lane < nprobe) {
            const int p = probes[x * nprobe + lane];
            if (p >= 0 && p < n_list) {
                const int64_t lo = list_off[p], hi = list_off[p + 1];
                if (hi > lo) { len0 = hi - lo; st0 = (int)lo; }
            }
        }
        if (lane + 64 < nprobe) {
            const int p = probes[x * nprobe + lane + 64];
            if (p >= 0 && p < n_list) {
                const int64_t lo = list_off[p], hi = list_off[p + 1];
                if (hi > lo) { len1 = hi - lo; st1 = (int)lo; }
            }
        }
        const long long c0 = wave_scan(len0, lane);
        const long long half = __shfl(c0, 63);
        const long long c1 = half + wave_scan(len1, lane);
        const long long len = __shfl(c1, 63);
        cum[lane] = c0;
        cum[lane + 64] = c1;
        start[lane] = st0;
        start[lane + 64] = st1;
        __builtin_amdgcn_wave_barrier();
        const int64_t s_lo = seen_off ? seen_off[u] : 0, s_hi = seen_off ? seen_off[u + 1] : 0;
        int cnt = 0, ne = 0;
        float thr_s = -INFINITY;              // the K-th entry once the list is full
        int thr_i = INT_MAX;
        for (long long b = 0; b < len; b += 64 * kCandRounds) {
            FullRow<D, T> xr[kCandRounds];
            int ci[kCandRounds];
            bool ok[kCandRounds];
            float sc[kCandRounds], of[kCandRounds];
            asm volatile("" ::: "memory");    // cum / start are read below what other lanes wrote above
#pragma unroll
            for (int r = 0; r < kCandRounds; ++r) {
                const long long e = b + 64 * r + lane;
                long long c = -1;
                if (e < len) {
                    // the first probe whose cumulative length exceeds e: e < len = cum[nprobe - 1], so j < nprobe
                    const int j = lower_bound(0, nprobe, [&](int m) { return cum[m] <= e; });
                    c = list_items[start[j] + (e - (j ? cum[j - 1] : 0))];
                }
                bool good = c >= 0 && c < n_item;         // (a list is trusted to hold item ids; anything else forms no address)
                if (good && allow) good = (allow[c >> 5] >> (c & 31)) & 1u;
                if (good && s_lo < s_hi) {
                    const int32_t cc = (int32_t)c;
                    const int64_t at = lower_bound(s_lo, s_hi, [&](int64_t m) { return seen_items[m] < cc; });
                    good = !(at < s_hi && seen_items[at] == cc);
                }
                xr[r].zero();
                sc[r] = 1.0f;
                of[r] = 0.0f;
                if (good) {
                    xr[r].load(wi + c * D);
                    if (adj) { sc[r] = adj[c]; of[r] = offset[c]; }
                }
                ci[r] = good ? (int)c : -1;
                ok[r] = good;
            }
            asm volatile("" ::: "memory");    // (the user row is read from LDS where a value feeds its fmaf, as in k_topk_cand)
#pragma unroll
            for (int r = 0; r < kCandRounds; ++r) {
                float s = score_chain<D, T>(l_u[wave].v, xr[r].v);
                if (adj) s = adjusted<true>(s, &sc[r], &of[r], 0);
                const bool elig = ok[r] && s == s;
                ne += __popcll(__ballot(elig));
                unsigned long long m = __ballot(elig && (cnt < k || better(s, ci[r], thr_s, thr_i)));
                while (m) {
                    const int l = __builtin_ctzll(m);
                    cand_insert(ls, li, k, lane, cnt, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)),
                                __builtin_amdgcn_readlane(ci[r], l));
                    m &= m - 1;
                    if (cnt == k) {
                        thr_s = ls[k - 1];
                        thr_i = li[k - 1];
                        m &= __ballot(elig && better(s, ci[r], thr_s, thr_i));
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < k; q += 64) {
            const bool live = q < cnt;
            items[x * k + q] = live ? li[q] : -1;
            scores[x * k + q] = live ? ls[q] : -INFINITY;
        }
        if (n_elig && lane == 0) n_elig[x] = ne;
        __builtin_amdgcn_wave_barrier();      // the next user's scan and inserts come after these reads
    }
}

// ---- deep lists (sml_topk_deep): top-K up to 1,024 by radix select -----------------------------------------------------------
//
// The cost of a list must not grow with k, so nothing is kept sorted during the walks.  Per user: the key of the k-th best
// eligible score is found by an MSB-first radix select over an order-preserving integer key of the score (four passes of 8
// bits, each one catalogue walk that counts into 256 bins), one more walk collects everything above that key (and the ties
// with it that belong to the list), and a bitonic sort per user puts the at most k collected pairs in the top-K order.  The
// number of launches and walks is fixed by the arguments, never by the data.
//
//   k_deep_count    a walk_slice callable: an eligible score whose key agrees with the user's prefix so far adds 1 to bin
//                   (key >> shift) & 255 of the wave's LDS histogram [256][32] (column = user lane: the 32 lanes of a half hit
//                   32 banks; the two halves hold other items of the same users and meet only on equal digits, which the LDS
//                   atomic serialises).  The wave then adds its non-zero bins to the global histogram of its 32 users, layout
//                   [user group][256][32] so that a wave's adds and the pick's reads are contiguous -- integer atomicAdd.
//   k_deep_pick     one thread per user: bins from the top, the digit that holds the k-th best extends the prefix, need -=
//                   the population above it; every bin read is written back 0 for the next pass.  Pass 0's total is n_elig; a
//                   user with fewer than k eligible items takes them all (need 0, key 0: no eligible key is 0).  After the
//                   last pass the prefix is K*, the key of the k-th entry, need = k - #{key > K*} and ties = #{key == K*}.
//   k_deep_collect  phase 0: entries with key > K*, and those with key == K* when ties == need, go to slots of the user's row
//                   of items / scores handed out by an integer atomic counter (any order: the sort fixes it); the ties a wave
//                   met in its slice are written per (user, slice).  Phase 1 serves the users with ties > need, who take the
//                   `need` smallest ids among the ties: slices are ascending id ranges, so a tie's place is the ties of the
//                   earlier slices plus those earlier in the walk plus a popcount over the tile's tie word (both lane halves'
//                   rows, ascending); a tie whose place is below need goes to slot k - need + place.  A wave without such
//                   a user returns before it loads anything.
//   k_deep_sort     one workgroup per user: the collected pairs, padded to a power of two with (-inf, INT_MAX), sorted in
//                   LDS under `better` and written over the row with the (-1, -inf) padding.  Ids are distinct, so the order
//                   is total and the bytes do not depend on the slots the atomics gave.

constexpr int kDeepWaves = 2;              // 32 KB of histogram per wave: 64 KB of dynamic LDS per workgroup
constexpr int kDeepBins = 256;
constexpr int kDeepPasses = 4;

// the usual order-preserving integer of an fp32 with the two zeros merged (the order compares floats: -0 == +0, the id decides).
// No non-NaN score has key 0
__host__ __device__ __forceinline__ uint32_t deep_key(float a) {
    const uint32_t b = a == 0.0f ? 0u : __builtin_bit_cast(uint32_t, a);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// bit q: acc[q] belongs to an eligible item (elig) and is not NaN
__device__ __forceinline__ unsigned deep_live(const f32x16& acc, unsigned elig) {
    unsigned ok = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) ok |= (unsigned)(acc[q] == acc[q]) << q;
    return ok & elig;
}

// per-user state of a call, int32 [kDeepState][n_pad] behind the histogram
enum { DS_CNT = 0, DS_PREFIX, DS_NEED, DS_TOTAL, DS_TIES, kDeepState };

template <int D, class T, bool F, bool A>
__device__ __forceinline__ void deep_count_body(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                const int64_t* __restrict__ users, int64_t n,
                                                const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                int slice_tiles, int shift, const int32_t* __restrict__ prefix,
                                                int32_t* __restrict__ hist) {
    extern __shared__ float lds[];
    const LanePos lp = lane_pos(slices, kDeepWaves, n);
    const int lane = threadIdx.x & 63;
    unsigned* lh = reinterpret_cast<unsigned*>(lds) + (size_t)lp.wave * kDeepBins * RT;
    for (int e = lane; e < kDeepBins * RT; e += 64) lh[e] = 0u;
    __builtin_amdgcn_wave_barrier();
    const int64_t u = users[lp.rc];
    // pass 0 (shift 24) has no prefix yet: every key agrees
    const unsigned pfx = shift < 24 ? (unsigned)prefix[lp.rc] : 0u;
    const unsigned high = shift < 24 ? ~0u << (shift + 8) : 0u;
    walk_slice<D, T, F, A>(wu, wi, n_item, u, seen_off, seen_items, allow, adj, lp, slice_tiles, [&](const f32x16& acc, int64_t, unsigned elig) {
        const unsigned ok = lp.valid ? deep_live(acc, elig) : 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const unsigned key = deep_key(acc[q]);
            if (((ok >> q) & 1u) && ((key ^ pfx) & high) == 0u) atomicAdd(&lh[((key >> shift) & 255u) * RT + lp.j], 1u);
        }
    });
    __builtin_amdgcn_wave_barrier();
    // the wave's 32 users are one aligned group of the global histogram: [group][256][32], the LDS image's own layout
    const int64_t group = (lp.row - lp.j) / RT;
    if (group * RT < n) {
        int32_t* gh = hist + group * (kDeepBins * RT);
        for (int e = lane; e < kDeepBins * RT; e += 64) {
            const unsigned v = lh[e];
            if (v) atomicAdd(gh + e, (int32_t)v);
        }
    }
}

template <int D, class T, bool F, bool A>
__global__ __launch_bounds__(64 * kDeepWaves) void k_deep_count(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                                const int64_t* __restrict__ users, int64_t n,
                                                                const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                                const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                                int slice_tiles, int shift, const int32_t* __restrict__ prefix,
                                                                int32_t* __restrict__ hist) {
    deep_count_body<D, T, F, A>(wu, wi, n_item, users, n, seen_off, seen_items, allow, adj, slices, slice_tiles, shift, prefix, hist);
}

// state: [kDeepState][n_pad]
__global__ __launch_bounds__(256) void k_deep_pick(int32_t* __restrict__ hist, int32_t* __restrict__ state, int64_t n, int64_t n_pad,
                                                   int k, int shift, int32_t* __restrict__ n_elig) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    int32_t* bins = hist + (x / RT) * (kDeepBins * RT) + (x % RT);
    const bool first = shift == 24;
    int need = first ? k : state[DS_NEED * n_pad + x];
    int cum = 0, chosen = -1, above = 0, pop = 0;
    for (int dgt = kDeepBins - 1; dgt >= 0; --dgt) {
        const int c = bins[dgt * RT];
        bins[dgt * RT] = 0;
        if (chosen < 0 && need > 0 && cum + c >= need) { chosen = dgt; above = cum; pop = c; }
        cum += c;
    }
    unsigned pfx = first ? 0u : (unsigned)state[DS_PREFIX * n_pad + x];
    if (first) {
        state[DS_TOTAL * n_pad + x] = cum;
        if (n_elig) n_elig[x] = cum;
    }
    if (chosen < 0) {                      // fewer than k eligible items (pass 0), or already so: everything is taken
        pfx = 0u;
        need = 0;
        pop = 0;
    } else {
        pfx |= (unsigned)chosen << shift;
        need -= above;
    }
    state[DS_PREFIX * n_pad + x] = (int32_t)pfx;
    state[DS_NEED * n_pad + x] = need;
    state[DS_TIES * n_pad + x] = pop;      // (the last pass's is the population of K*)
}

template <int D, class T, bool F, bool A>
__device__ __forceinline__ void deep_collect_body(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                  const int64_t* __restrict__ users, int64_t n, int k,
                                                  const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                  const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                  int slice_tiles, int phase, int32_t* __restrict__ state, int64_t n_pad,
                                                  int32_t* __restrict__ tie_cnt, int32_t* __restrict__ items, float* __restrict__ scores) {
    const LanePos lp = lane_pos(slices, kDeepWaves, n);
    const int h = lp.h;
    const unsigned kstar = (unsigned)state[DS_PREFIX * n_pad + lp.rc];
    const int need = state[DS_NEED * n_pad + lp.rc];
    const int ties = state[DS_TIES * n_pad + lp.rc];
    const bool by_place = lp.valid && ties != need;        // this user takes the `need` smallest ids among the ties
    int before = 0;                                        // ties of the earlier slices (phase 1), then of the walk so far
    if (phase == 1) {
        bool mine = by_place;
        if (mine) {
            for (int s = 0; s < lp.slice && before < need; ++s) before += tie_cnt[lp.row * slices + s];
            mine = before < need;
        }
        if (!__any(mine)) return;
    }
    const int64_t u = users[lp.rc];
    int32_t* const cnt = state + DS_CNT * n_pad + lp.row;
    const int64_t o = lp.row * k;
    walk_slice<D, T, F, A>(wu, wi, n_item, u, seen_off, seen_items, allow, adj, lp, slice_tiles, [&](const f32x16& acc, int64_t base, unsigned elig) {
        const unsigned ok = lp.valid ? deep_live(acc, elig) : 0u;
        unsigned take = 0, tie = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const unsigned key = deep_key(acc[q]);
            take |= (unsigned)(key > kstar) << q;
            tie |= (unsigned)(key == kstar) << q;
        }
        take &= ok;
        tie &= ok;
        if (phase == 0) {
            if (!by_place) take |= tie;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if ((take >> q) & 1u) {
                    const int slot = atomicAdd(cnt, 1);
                    if (slot < k) {
                        items[o + slot] = (int32_t)(base + row_of(q, h));
                        scores[o + slot] = acc[q];
                    }
                }
            }
        }
        if (!__any(by_place && tie != 0)) return;
        // the tile's tie word over its 32 rows, both lane halves' bits: a tie's place is the number of ties below it
        unsigned word = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) word |= ((tie >> q) & 1u) << row_of(q, h);
        word |= (unsigned)__shfl_xor((int)word, 32, 64);
        if (phase == 1 && by_place) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if ((tie >> q) & 1u) {
                    const int r = row_of(q, h);
                    const int place = before + __popc(word & ((1u << r) - 1u));
                    if (place < need) {
                        const int slot = k - need + place;
                        if (slot >= 0 && slot < k) {
                            items[o + slot] = (int32_t)(base + r);
                            scores[o + slot] = acc[q];
                        }
                    }
                }
            }
        }
        if (by_place) before += __popc(word);
    });
    // phase 0: an empty slice still writes its count
    if (phase == 0 && lp.valid && h == 0) tie_cnt[lp.row * slices + lp.slice] = by_place ? before : 0;
}

template <int D, class T, bool F, bool A>
__global__ __launch_bounds__(64 * kDeepWaves) void k_deep_collect(const T* __restrict__ wu, const T* __restrict__ wi, int64_t n_item,
                                                                  const int64_t* __restrict__ users, int64_t n, int k,
                                                                  const int64_t* __restrict__ seen_off, const int32_t* __restrict__ seen_items,
                                                                  const uint32_t* __restrict__ allow, const float* __restrict__ adj, int slices,
                                                                  int slice_tiles, int phase, int32_t* __restrict__ state, int64_t n_pad,
                                                                  int32_t* __restrict__ tie_cnt, int32_t* __restrict__ items,
                                                                  float* __restrict__ scores) {
    deep_collect_body<D, T, F, A>(wu, wi, n_item, users, n, k, seen_off, seen_items, allow, adj, slices, slice_tiles, phase, state, n_pad, tie_cnt,
                                  items, scores);
}

// one workgroup per user, P = the power of two >= k (<= 1024) pairs in LDS, P / 2 compare-exchanges per step
__global__ __launch_bounds__(256) void k_deep_sort(const int32_t* __restrict__ state, int64_t n_pad, int k, int P,
                                                   int32_t* __restrict__ items, float* __restrict__ scores) {
    __shared__ float l_s[SML_TOPK_DEEP_MAX];
    __shared__ int32_t l_i[SML_TOPK_DEEP_MAX];
    const int64_t x = blockIdx.x;
    const int total = state[DS_TOTAL * n_pad + x];
    const int m = total < k ? total : k;
    for (int q = threadIdx.x; q < P; q += blockDim.x) {
        const bool live = q < m;
        l_s[q] = live ? scores[x * k + q] : -INFINITY;
        l_i[q] = live ? items[x * k + q] : INT_MAX;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += blockDim.x) {
                const int a = 2 * t - (t & (stride - 1)), b = a + stride;
                const float sa = l_s[a], sb = l_s[b];
                const int ia = l_i[a], ib = l_i[b];
                // blocks of `size` alternate direction; the last step (size == P) runs best-first throughout
                const bool swap = (a & size) == 0 ? better(sb, ib, sa, ia) : better(sa, ia, sb, ib);
                if (swap) { l_s[a] = sb; l_i[a] = ib; l_s[b] = sa; l_i[b] = ia; }
            }
            __syncthreads();
        }
    }
    for (int q = threadIdx.x; q < k; q += blockDim.x) {
        const bool live = q < m;
        items[x * k + q] = live ? l_i[q] : -1;
        scores[x * k + q] = live ? l_s[q] : -INFINITY;
    }
}

// the grid of a deep call: slices forced (1 .. 256) or left to the planner (0)
SliceGrid deep_grid(int64_t n, int64_t n_item, int slices) {
    if (slices <= 0) return plan_grid(n, kDeepWaves, n_item, 2048, 8);
    const int64_t n_tiles = (n_item + RT - 1) / RT;
    return {(n + RT * kDeepWaves - 1) / (RT * kDeepWaves), slices, (int)((n_tiles + slices - 1) / slices)};
}

int64_t deep_pad(int64_t n) { return (n + RT - 1) / RT * RT; }

// The definition as a single-threaded walk over host memory: every item's score by score_chain (and adjusted), the eligible
// ones kept as the k best so far in a binary heap under `better` (worst on top), then written best first.
template <int D, class T>
void deep_host_walk(const T* wu, const T* wi, int64_t n_item, const int64_t* users, int64_t n, int k, const int64_t* seen_off,
                    const int32_t* seen_items, const uint32_t* allow, const float* adj, int32_t* items, float* scores, int32_t* n_elig) {
    const float* offset = adj ? adj + (n_item + RT - 1) / RT * RT : nullptr;
    float hs[SML_TOPK_DEEP_MAX];
    int32_t hi[SML_TOPK_DEEP_MAX];
    // worse(a, b): entry a orders after entry b
    const auto worse = [&](int a, int b) { return better(hs[b], hi[b], hs[a], hi[a]); };
    for (int64_t x = 0; x < n; ++x) {
        const int64_t u = users[x];
        int64_t sp = seen_off ? seen_off[u] : 0;
        const int64_t se = seen_off ? seen_off[u + 1] : 0;
        int m = 0, ne = 0;
        for (int64_t i = 0; i < n_item; ++i) {
            while (sp < se && seen_items[sp] < i) ++sp;
            if (sp < se && seen_items[sp] == i) continue;
            if (allow && !((allow[i >> 5] >> (i & 31)) & 1u)) continue;
            float s = score_chain<D, T>(wu + u * D, wi + i * D);
            if (adj) s = adjusted<true>(s, adj, offset, i);
            if (s != s) continue;
            ++ne;
            if (m == k) {
                if (!better(s, (int)i, hs[0], hi[0])) continue;
                // replace the worst entry and sift down
                int p = 0;
                for (;;) {
                    int c = 2 * p + 1;
                    if (c >= m) break;
                    if (c + 1 < m && worse(c + 1, c)) ++c;
                    if (!better(s, (int)i, hs[c], hi[c])) break;
                    hs[p] = hs[c];
                    hi[p] = hi[c];
                    p = c;
                }
                hs[p] = s;
                hi[p] = (int32_t)i;
            } else {
                int p = m++;
                while (p > 0) {
                    const int q = (p - 1) / 2;
                    if (!better(hs[q], hi[q], s, (int)i)) break;      // the parent is already worse
                    hs[p] = hs[q];
                    hi[p] = hi[q];
                    p = q;
                }
                hs[p] = s;
                hi[p] = (int32_t)i;
            }
        }
        for (int q = m; q < k; ++q) { items[x * k + q] = -1; scores[x * k + q] = -INFINITY; }
        // pop the worst into the last live slot
        for (int live = m; live > 0; --live) {
            items[x * k + live - 1] = hi[0];
            scores[x * k + live - 1] = hs[0];
            const float s = hs[live - 1];
            const int32_t i = hi[live - 1];
            int p = 0;
            for (;;) {
                int c = 2 * p + 1;
                if (c >= live - 1) break;
                if (c + 1 < live - 1 && worse(c + 1, c)) ++c;
                if (!better(s, i, hs[c], hi[c])) break;
                hs[p] = hs[c];
                hi[p] = hi[c];
                p = c;
            }
            hs[p] = s;
            hi[p] = i;
        }
        if (n_elig) n_elig[x] = ne;
    }
}

// sml_ivf_search as a single-threaded walk over host memory: the probed lists in probe order, every member tested and scored as
// k_ivf_search does (score_chain, adjusted), the distinct eligible ones kept as a sorted list of at most k under `better`.
template <int D, class T>
void ivf_host_walk(const T* wu, const T* wi, int64_t n_item, const int64_t* users, int64_t n, const int64_t* list_off,
                   const int32_t* list_items, int n_list, const int32_t* probes, int nprobe, int k, const int64_t* seen_off,
                   const int32_t* seen_items, const uint32_t* allow, const float* adj, int32_t* items, float* scores, int32_t* n_elig) {
    const float* offset = adj ? adj + (n_item + RT - 1) / RT * RT : nullptr;
    float ls[kCandMaxK];
    int32_t li[kCandMaxK];
    for (int64_t x = 0; x < n; ++x) {
        const int64_t u = users[x];
        const int64_t s_lo = seen_off ? seen_off[u] : 0, s_hi = seen_off ? seen_off[u + 1] : 0;
        int cnt = 0, ne = 0;
        for (int j = 0; j < nprobe; ++j) {
            const int p = probes[x * nprobe + j];
            if (p < 0 || p >= n_list) continue;
            for (int64_t m = list_off[p]; m < list_off[p + 1]; ++m) {
                const int64_t c = list_items[m];
                if (c < 0 || c >= n_item) continue;
                if (allow && !((allow[c >> 5] >> (c & 31)) & 1u)) continue;
                int64_t lo = s_lo, hi = s_hi;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (seen_items[mid] < c) lo = mid + 1; else hi = mid;
                }
                if (lo < s_hi && seen_items[lo] == c) continue;
                float s = score_chain<D, T>(wu + u * D, wi + c * D);
                if (adj) s = adjusted<true>(s, adj, offset, c);
                if (s != s) continue;
                ++ne;
                int pos = 0;
                bool repeat = false;
                for (int q = 0; q < cnt; ++q) {
                    repeat |= ls[q] == s && li[q] == (int32_t)c;
                    pos += better(ls[q], li[q], s, (int)c);
                }
                if (repeat || pos >= k) continue;
                if (cnt < k) ++cnt;
                for (int q = cnt - 1; q > pos; --q) { ls[q] = ls[q - 1]; li[q] = li[q - 1]; }
                ls[pos] = s;
                li[pos] = (int32_t)c;
            }
        }
        for (int q = 0; q < k; ++q) {
            items[x * k + q] = q < cnt ? li[q] : -1;
            scores[x * k + q] = q < cnt ? ls[q] : -INFINITY;
        }
        if (n_elig) n_elig[x] = ne;
    }
}

}  // namespace

bool sml_retrieval_supports(int d, int elem_bytes) {
    SmlCatalogue c = {};
    c.d = d;
    c.elem_bytes = elem_bytes;
    return with_width(c, [](auto, auto, auto, auto*, auto*) {});
}

hipError_t sml_launch_full_rank(const SmlCatalogue& c, const int64_t* rows, int64_t n, int n_cols, int32_t* rank, hipStream_t st) {
    hipError_t e = hipMemsetAsync(rank, 0, n * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const SliceGrid g = rank_grid(n, kRankWaves, c.n_item);
    const dim3 grid((unsigned)(g.groups * g.slices)), block(64 * kRankWaves);
    if (!with_width(c, [&](auto dd, auto ff, auto aa, auto* tu, auto* ti) {
        k_full_rank<dd(), elem_t<decltype(tu)>, ff(), aa()><<<grid, block, 0, st>>>(
            tu, ti, c.n_item, rows, n, n_cols, c.seen_off, c.seen_items, c.allow, c.adj, g.slices, g.slice_tiles, rank);
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

int64_t sml_topk_scratch_size(int64_t n, int k, int64_t n_item) {
    const int64_t s = topk_grid(n, k, n_item).slices;
    return n * s * (int64_t)k * 8 + n * s * 4;
}

hipError_t sml_launch_topk(const SmlCatalogue& c, const int64_t* users, int64_t n, int k, void* scratch, int32_t* items, float* scores,
                           hipStream_t st) {
    const SliceGrid g = topk_grid(n, k, c.n_item);
    const int slices = g.slices, waves = topk_waves(k);
    float* cs = static_cast<float*>(scratch);
    int32_t* ci = reinterpret_cast<int32_t*>(cs + n * slices * k);
    int32_t* cn = ci + n * slices * k;
    const dim3 grid((unsigned)(g.groups * slices)), block(64 * waves);
    const size_t lds = (size_t)waves * 2 * k * RT * 4;
    if (!with_width(c, [&](auto dd, auto ff, auto aa, auto* tu, auto* ti) {
        k_topk_slice<dd(), elem_t<decltype(tu)>, ff(), aa()><<<grid, block, lds, st>>>(
            tu, ti, c.n_item, users, n, k, c.seen_off, c.seen_items, c.allow, c.adj, slices, g.slice_tiles, cs, ci, cn);
    }))
        return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t threads = n * slices * k;
    k_topk_merge<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(cs, ci, cn, n, k, slices, items, scores);
    return hipGetLastError();
}

// scratch of sml_user_rank, 256-byte aligned pieces: seg, in_seen, 2 x (key score, key id, entry), bin_p, bin_d
static int64_t ur_piece(int64_t n_pos) { return (n_pos * 4 + 255) / 256 * 256; }

int64_t sml_user_rank_scratch_size(int64_t n_pos) { return 10 * ur_piece(n_pos); }

hipError_t sml_launch_user_rank(const SmlCatalogue& c, const int64_t* users, int64_t n, const int64_t* pos_off, const int32_t* pos_items,
                                int64_t n_pos, void* scratch, int32_t* above, int32_t* pos, hipStream_t st) {
    char* base = static_cast<char*>(scratch);
    const int64_t pc = ur_piece(n_pos);
    int32_t* seg = reinterpret_cast<int32_t*>(base);
    int32_t* in_seen = reinterpret_cast<int32_t*>(base + pc);
    float* ks[2] = {reinterpret_cast<float*>(base + 2 * pc), reinterpret_cast<float*>(base + 5 * pc)};
    int32_t* ki[2] = {reinterpret_cast<int32_t*>(base + 3 * pc), reinterpret_cast<int32_t*>(base + 6 * pc)};
    int32_t* kx[2] = {reinterpret_cast<int32_t*>(base + 4 * pc), reinterpret_cast<int32_t*>(base + 7 * pc)};
    int32_t* bin_p = reinterpret_cast<int32_t*>(base + 8 * pc);
    int32_t* bin_d = reinterpret_cast<int32_t*>(base + 9 * pc);
    hipError_t e = hipMemsetAsync(bin_p, 0, 2 * pc, st);
    if (e != hipSuccess) return e;
    const dim3 eg((unsigned)((n_pos + 255) / 256)), eb(256);
    if (!with_width(c, [&](auto dd, auto ff, auto aa, auto* tu, auto* ti) {
        k_ur_thresholds<dd(), elem_t<decltype(tu)>, ff(), aa()><<<eg, eb, 0, st>>>(
            tu, ti, c.n_item, users, n, pos_off, pos_items, n_pos, c.seen_off, c.seen_items, c.allow, c.adj, seg, ks[0], ki[0], kx[0], in_seen);
    }))
        return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // a user's range is at most n_pos long: ceil(log2 n_pos) merge passes sort every range
    int cur = 0;
    for (int64_t w = 1; w < n_pos; w *= 2, cur ^= 1) {
        k_ur_merge<<<eg, eb, 0, st>>>(pos_off, seg, n_pos, w, ks[cur], ki[cur], kx[cur], ks[cur ^ 1], ki[cur ^ 1], kx[cur ^ 1]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const SliceGrid g = rank_grid(n, kUrWaves, c.n_item);
    const dim3 grid((unsigned)(g.groups * g.slices)), block(64 * kUrWaves);
    if (!with_width(c, [&](auto dd, auto ff, auto aa, auto* tu, auto* ti) {
        k_ur_count<dd(), elem_t<decltype(tu)>, ff(), aa()><<<grid, block, 0, st>>>(
            tu, ti, c.n_item, users, n, pos_off, c.seen_off, c.seen_items, c.allow, c.adj, g.slices, g.slice_tiles, ks[cur], ki[cur], bin_p, bin_d);
    }))
        return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    k_ur_finish<<<dim3((unsigned)n), dim3(kUrBlock), 0, st>>>(pos_off, ks[cur], kx[cur], in_seen, bin_p, bin_d, above, pos);
    return hipGetLastError();
}

hipError_t sml_launch_user_metrics(const int32_t* pos, const int64_t* pos_off, int64_t n, const int32_t* ks, int n_k,
                                   int32_t* hits, float* dcg, float* ap, int32_t* first, hipStream_t st) {
    UrKs k = {};
    for (int q = 0; q < n_k; ++q) k.k[q] = ks[q];
    k_ur_metrics<<<dim3((unsigned)n), dim3(kUrBlock), 0, st>>>(pos, pos_off, k, n_k, hits, dcg, ap, first);
    return hipGetLastError();
}

hipError_t sml_launch_topk_candidates(const SmlCatalogue& c, const int64_t* users, int64_t n, const SmlCandidates& l, int k,
                                      int max_workgroups, int32_t* items, float* scores, int32_t* n_elig, hipStream_t st) {
    int64_t blocks = (n + kCandWaves - 1) / kCandWaves;
    if (blocks > 65536) blocks = 65536;                  // beyond this the lists are walked grid-stride
    if (max_workgroups > 0 && blocks > max_workgroups) blocks = max_workgroups;
    const dim3 grid((unsigned)blocks), block(64 * kCandWaves);
    if (!with_width(c, [&](auto dd, auto, auto, auto* tu, auto* ti) {
        k_topk_cand<dd(), elem_t<decltype(tu)>><<<grid, block, 0, st>>>(
            tu, ti, c.n_item, users, n, l.cand, l.elem_bytes == 8, l.off, l.stride, l.first, l.cols, k, c.seen_off, c.seen_items, c.allow, c.adj,
            items, scores, n_elig);
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t sml_launch_ivf_search(const SmlCatalogue& c, const int64_t* users, int64_t n, const SmlIvfLists& l, int k, int max_workgroups,
                                 int32_t* items, float* scores, int32_t* n_elig, hipStream_t st) {
    int64_t blocks = (n + kCandWaves - 1) / kCandWaves;
    if (blocks > 65536) blocks = 65536;                  // beyond this the users are walked grid-stride
    if (max_workgroups > 0 && blocks > max_workgroups) blocks = max_workgroups;
    const dim3 grid((unsigned)blocks), block(64 * kCandWaves);
    if (!with_width(c, [&](auto dd, auto, auto, auto* tu, auto* ti) {
        k_ivf_search<dd(), elem_t<decltype(tu)>><<<grid, block, 0, st>>>(
            tu, ti, c.n_item, users, n, l.off, l.items, l.n_list, l.probes, l.nprobe, k, c.seen_off, c.seen_items, c.allow, c.adj, items, scores,
            n_elig);
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

bool sml_ivf_host_walk(const SmlCatalogue& c, const int64_t* users, int64_t n, const SmlIvfLists& l, int k, int32_t* items, float* scores,
                       int32_t* n_elig) {
    return with_width(c, [&](auto dd, auto, auto, auto* tu, auto* ti) {
        ivf_host_walk<dd(), elem_t<decltype(tu)>>(tu, ti, c.n_item, users, n, l.off, l.items, l.n_list, l.probes, l.nprobe, k, c.seen_off,
                                                  c.seen_items, c.allow, c.adj, items, scores, n_elig);
    });
}

hipError_t sml_launch_item_filter(const int32_t* ids, int64_t n_ids, int64_t n_item, int invert, uint32_t* words, hipStream_t st) {
    const int64_t n_words = (n_item + RT - 1) / RT;
    k_filter_fill<<<dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st>>>(words, n_words, n_item, invert);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_ids == 0) return e;
    k_filter_from_ids<<<dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, st>>>(ids, n_ids, invert, words);
    return hipGetLastError();
}

int64_t sml_item_adjust_pad(int64_t n_item) { return (n_item + RT - 1) / RT * RT; }

hipError_t sml_launch_item_adjust_fill(const float* scale, const float* offset, int64_t n_item, float* adj, hipStream_t st) {
    const int64_t n_pad = sml_item_adjust_pad(n_item);
    k_adjust_fill<<<dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st>>>(scale, offset, n_item, n_pad, adj);
    return hipGetLastError();
}

hipError_t sml_launch_item_adjust_cosine(int d, int elem_bytes, const void* wi, int64_t n_item, float* adj, hipStream_t st) {
    const int64_t n_pad = sml_item_adjust_pad(n_item);
    const dim3 grid((unsigned)((n_pad + 255) / 256)), block(256);
    SmlCatalogue c = {};
    c.d = d;
    c.elem_bytes = elem_bytes;
    c.wi = wi;
    if (!with_width(c, [&](auto dd, auto, auto, auto*, auto* ti) {
        k_adjust_cosine<dd(), elem_t<decltype(ti)>><<<grid, block, 0, st>>>(ti, n_item, n_pad, adj);
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// scratch of sml_topk_deep: the histogram int32 [n_pad / 32][256][32], the per-user state int32 [kDeepState][n_pad] (both zeroed
// by the call), the ties per (user, slice) int32 [n][slices]
int64_t sml_topk_deep_scratch_size(int64_t n, int64_t n_item, int slices) {
    const int64_t n_pad = deep_pad(n);
    const int64_t bytes = n_pad * (kDeepBins + kDeepState) * 4 + n * deep_grid(n, n_item, slices).slices * 4;
    return (bytes + 255) / 256 * 256;
}

hipError_t sml_launch_topk_deep(const SmlCatalogue& c, const int64_t* users, int64_t n, int k, int slices, void* scratch, int32_t* items,
                                float* scores, int32_t* n_elig, hipStream_t st) {
    const SliceGrid g = deep_grid(n, c.n_item, slices);
    const int64_t n_pad = deep_pad(n);
    int32_t* hist = static_cast<int32_t*>(scratch);
    int32_t* state = hist + n_pad * kDeepBins;
    int32_t* tie_cnt = state + n_pad * kDeepState;
    hipError_t e = hipMemsetAsync(hist, 0, n_pad * (kDeepBins + kDeepState) * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(g.groups * g.slices)), block(64 * kDeepWaves);
    const size_t lds = (size_t)kDeepWaves * kDeepBins * RT * 4;
    const dim3 ugrid((unsigned)((n + 255) / 256)), ublock(256);
    for (int pass = 0; pass < kDeepPasses; ++pass) {
        const int shift = 24 - 8 * pass;
        if (!with_width(c, [&](auto dd, auto ff, auto aa, auto* tu, auto* ti) {
            k_deep_count<dd(), elem_t<decltype(tu)>, ff(), aa()><<<grid, block, lds, st>>>(
                tu, ti, c.n_item, users, n, c.seen_off, c.seen_items, c.allow, c.adj, g.slices, g.slice_tiles, shift, state + DS_PREFIX * n_pad, hist);
        }))
            return hipErrorInvalidValue;
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_deep_pick<<<ugrid, ublock, 0, st>>>(hist, state, n, n_pad, k, shift, n_elig);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int phase = 0; phase < 2; ++phase) {
        if (!with_width(c, [&](auto dd, auto ff, auto aa, auto* tu, auto* ti) {
            k_deep_collect<dd(), elem_t<decltype(tu)>, ff(), aa()><<<grid, block, 0, st>>>(
                tu, ti, c.n_item, users, n, k, c.seen_off, c.seen_items, c.allow, c.adj, g.slices, g.slice_tiles, phase, state, n_pad, tie_cnt, items,
                scores);
        }))
            return hipErrorInvalidValue;
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    int P = 1;
    while (P < k) P <<= 1;
    const int threads = P / 2 < 64 ? 64 : (P / 2 > 256 ? 256 : P / 2);
    k_deep_sort<<<dim3((unsigned)n), dim3(threads), 0, st>>>(state, n_pad, k, P, items, scores);
    return hipGetLastError();
}

bool sml_topk_host_walk(const SmlCatalogue& c, const int64_t* users, int64_t n, int k, int32_t* items, float* scores, int32_t* n_elig) {
    return with_width(c, [&](auto dd, auto, auto, auto* tu, auto* ti) {
        deep_host_walk<dd(), elem_t<decltype(tu)>>(tu, ti, c.n_item, users, n, k, c.seen_off, c.seen_items, c.allow, c.adj, items, scores, n_elig);
    });
}
