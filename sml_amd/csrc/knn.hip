// Neighbourhood model on gfx950 (include/sml_hip.h, "NEIGHBOURS"): for a row x, accumulate over the lists of x's members and keep
// the K best -- out(x) = top-K over j of sum_{m in R(x)} W[m, j].  sml_cooc_topk is this with R(x) the users of item x and W[m, .]
// the items of user m with unit weights; sml_knn_topk with R(x) a history and W[m, .] item m's neighbour list with its similarities
// in fixed point; sml_cooc_topk_weighted is sml_cooc_topk with user m's unit replaced by its weight in fixed point.  The only
// atomics are integer (exact, order-free), so the bytes depend on no launch geometry.
//
// One wavefront per row, rows walked grid-stride, kKnnWaves rows per workgroup in flight.  Two paths, chosen per row from the
// row's total list length (known before the walk, and a bound on its distinct ids):
//   LDS path    total <= kKnnLdsLimit: an open-addressing table of kKnnTabSlots = 2 * kKnnLdsLimit slots per wave in LDS (key by
//               ds compare-and-swap, sum by ds add).  The table can never fill, and the probe loop is bounded by its size anyway.
//               The candidates are then read off the table's slots, which are reset as they are read.
//   dense path  a dense accumulator over [0, n_item) per wave in scratch (int32 counts; int64 weighted counts; int64 sums + a
//               touched bitmap).  Pass 1 adds with no-return global atomics; pass 2 walks the same lists again and the lane that
//               claims a candidate (counts, weighted or not: the exchange that returns a non-zero value -- every contribution is
//               >= 1; sums: the atomic AND that clears its touched bit) takes the sum with an exchange that resets the slot to
//               zero, so the scratch is zero again when the row is done.  A history with more slots than the catalogue has items
//               skips the second walk: its candidates are claimed from the bitmap's words.
// Either way the claimed (id, sum) pairs go through the same eligibility and score text and into the wave's sorted LDS list
// (cand_insert, topk_list.h); the sums are integers and the order is total, so who claims what never shows in the output.
// The kernels and the single-threaded host walks share the score functions.  Contraction is OFF in the whole file.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "topk_list.h"
#include "../../include/sml_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kKnnWaves = 4;                       // rows in flight per workgroup: one wavefront each
constexpr int kKnnMaxK = 128;
static_assert(kKnnMaxK <= 128, "cand_insert: a lane holds two slots of the list");
constexpr int kKnnTabBits = 10;
constexpr int kKnnTabSlots = 1 << kKnnTabBits;     // per wave: 4 KB of keys + 8 KB of sums; 56 KB per workgroup with the lists
constexpr int kKnnLdsLimit = kKnnTabSlots / 2;     // rows whose total list length is at most this take the LDS path
constexpr int kKnnGrid = 256;                      // workgroups when max_workgroups == 0: one per CU
static_assert(kKnnTabSlots >= 2 * kKnnLdsLimit, "the table holds at least twice the admitted entries: it can never fill");

// ---- the scores: the text the header names, shared by the kernels and the host walks ------------------------------------------
// numerator -> similarity: den = a[i] * b[j] (one fp64 rounding); den = den + shrink; s64 = num / den (correctly rounded); (float)s64
__host__ __device__ __forceinline__ float cooc_ratio(double num, const double* __restrict__ na, const double* __restrict__ nb, int64_t i, int64_t j,
                                                     double shrink) {
    double den = na[i] * nb[j];
    den = den + shrink;
    const double s64 = num / den;
    return (float)s64;
}
// count -> similarity
__host__ __device__ __forceinline__ float cooc_score(int c, const double* __restrict__ na, const double* __restrict__ nb, int64_t i, int64_t j,
                                                     double shrink) {
    if (!na) return (float)c;
    return cooc_ratio((double)c, na, nb, i, j, shrink);
}
// similarity -> fixed point: q = rint(ldexp((double)sim, F)), to nearest even; false: the slot contributes nothing
__host__ __device__ __forceinline__ bool knn_quant(float sim, int F, long long* q) {
    if (!(fabsf(sim) <= 3.402823466e+38f)) return false;             // NaN and +-inf
    const double r = rint(ldexp((double)sim, F));
    if (fabs(r) > 4294967296.0) return false;
    *q = (long long)r;
    return true;
}
// fixed point -> score: (float)ldexp((double)acc, -F), both conversions to nearest even
__host__ __device__ __forceinline__ float knn_score(long long acc, int F) { return (float)ldexp((double)acc, -F); }

// weighted count -> similarity: num = ldexp((double)cw, -F), the conversion to nearest even; then the text of the count
__host__ __device__ __forceinline__ float cooc_score_weighted(long long cw, int F, const double* __restrict__ na, const double* __restrict__ nb,
                                                              int64_t i, int64_t j, double shrink) {
    const double num = ldexp((double)cw, -F);
    if (!na) return (float)num;
    return cooc_ratio(num, na, nb, i, j, shrink);
}
// a user's weight in fixed point (knn_quant's text); false: the user contributes nothing
__host__ __device__ __forceinline__ bool cooc_user_quant(const float* __restrict__ user_w, int64_t u, int F, long long* q) {
    return knn_quant(user_w[u], F, q) && *q > 0;
}

__host__ __device__ __forceinline__ bool knn_allowed(const uint32_t* __restrict__ allow, int j) {
    return !allow || ((allow[j >> 5] >> (j & 31)) & 1u);
}

__host__ __device__ constexpr int64_t knn_pad256(int64_t b) { return (b + 255) / 256 * 256; }
// one wave's slot of the scratch: kind 0 (counts) int32 [n_item]; kind 1 (sums) int64 [n_item], then the touched bitmap; the
// weighted counts: int64 [n_item] (knn_acc_bytes(n_item, 1)) and no bitmap
__host__ __device__ constexpr int64_t knn_acc_bytes(int64_t n_item, int kind) { return knn_pad256(n_item * (kind ? 8 : 4)); }
__host__ __device__ constexpr int64_t knn_slot_bytes(int64_t n_item, int kind) {
    return knn_acc_bytes(n_item, kind) + (kind ? knn_pad256((n_item + 31) / 32 * 4) : 0);
}

#ifdef __HIP_DEVICE_COMPILE__
__device__ __forceinline__ long long knn_readlane64(long long v, int src) {
    const int lo = __builtin_amdgcn_readlane((int)(unsigned long long)v, src);
    const int hi = __builtin_amdgcn_readlane((int)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// inclusive scan over the wave
__device__ __forceinline__ long long knn_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ long long knn_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the wave's sorted list (cand_insert) with a copy of its K-th entry as the threshold, as k_topk_cand keeps it
struct KnnList {
    float* ls;
    int32_t* li;
    int k, cnt, ne;
    float thr_s;
    int thr_i;
    __device__ __forceinline__ void reset() { cnt = 0; ne = 0; thr_s = -INFINITY; thr_i = INT_MAX; }
    // every lane calls this; elig lanes offer (s, id): lanes that beat the threshold insert, in lane order
    __device__ __forceinline__ void offer(int lane, bool elig, float s, int id) {
        ne += __popcll(__ballot(elig));
        unsigned long long m = __ballot(elig && (cnt < k || better(s, id, thr_s, thr_i)));
        while (m) {
            const int l = __builtin_ctzll(m);
            cand_insert(ls, li, k, lane, cnt, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)),
                        __builtin_amdgcn_readlane(id, l));
            m &= m - 1;
            if (cnt == k) {
                thr_s = ls[k - 1];
                thr_i = li[k - 1];
                m &= __ballot(elig && better(s, id, thr_s, thr_i));
            }
        }
    }
    __device__ __forceinline__ void write(int lane, int64_t x, int32_t* __restrict__ items, float* __restrict__ scores,
                                          int32_t* __restrict__ n_elig) {
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < k; q += 64) {
            const bool live = q < cnt;
            items[x * k + q] = live ? li[q] : -1;
            scores[x * k + q] = live ? ls[q] : -INFINITY;
        }
        if (n_elig && lane == 0) n_elig[x] = ne;
        __builtin_amdgcn_wave_barrier();      // the next row's inserts come after these reads
    }
};

// sum += q under key j in the wave's open-addressing table.  At most kKnnLdsLimit distinct keys ever live in kKnnTabSlots slots,
// so a free or matching slot is always found; the loop is bounded by the table's size regardless.
template <class V>
__device__ __forceinline__ void knn_tab_add(int32_t* keys, V* vals, int j, V q) {
    unsigned h = ((unsigned)j * 2654435761u) >> (32 - kKnnTabBits);
    for (int p = 0; p < kKnnTabSlots; ++p) {
        const int old = atomicCAS(&keys[h], -1, j);
        if (old == -1 || old == j) {
            __hip_atomic_fetch_add(&vals[h], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
        h = (h + 1) & (kKnnTabSlots - 1);
    }
}

// the wave's LDS operations so far are done before the next ones start
__device__ __forceinline__ void knn_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Walk of a co-occurrence row: f(valid, j) for every entry j of the item lists of users[lo .. hi), called by all 64 lanes together
// (valid: this lane holds an entry).  64 users at a time: their ranges are scanned into the wave's LDS and the entries are dealt
// to the lanes 64 at a time whatever the lists' lengths, each lane finding its list by a bisection of the scanned starts.
template <class F>
__device__ __forceinline__ void cooc_walk(const int64_t* __restrict__ user_off, const int32_t* __restrict__ user_items,
                                          const int32_t* __restrict__ users, int64_t lo, int64_t hi, int lane, long long* w_end,
                                          long long* w_base, F&& f) {
    for (int64_t b = lo; b < hi; b += 64) {
        long long l0 = 0, len = 0;
        if (b + lane < hi) {
            const int64_t u = users[b + lane];
            l0 = user_off[u];
            len = user_off[u + 1] - l0;
        }
        const long long end = knn_scan(len, lane);        // entries of the batch up to and including this lane's list
        knn_lds_order();
        w_end[lane] = end;
        w_base[lane] = l0 - (end - len);                  // entry t of the batch, if in this list, is user_items[w_base + t]
        knn_lds_order();
        const long long total = knn_readlane64(end, 63);
        for (long long t0 = 0; t0 < total; t0 += 64) {
            const long long t = t0 + lane;
            const bool valid = t < total;
            int j = -1;
            if (valid) {
                const int q = lower_bound(0, 63, [&](int m) { return w_end[m] <= t; });
                j = user_items[w_base[q] + t];
            }
            f(valid, j);
        }
    }
}

// The weighted walk: f(valid, j, q) -- the walk above in which each entry comes with its user's weight in fixed point (the batch's
// 64 values lie in w_q beside the starts) and a user that contributes nothing has a list of length 0: it deals no entry.  (A
// sibling and not a parameter of cooc_walk, whose text stays what k_cooc_topk was compiled from.)
template <class F>
__device__ __forceinline__ void cooc_walk_weighted(const int64_t* __restrict__ user_off, const int32_t* __restrict__ user_items,
                                                   const int32_t* __restrict__ users, int64_t lo, int64_t hi, int lane, long long* w_end,
                                                   long long* w_base, const float* __restrict__ user_w, int frac_bits, long long* w_q,
                                                   F&& f) {
    for (int64_t b = lo; b < hi; b += 64) {
        long long l0 = 0, len = 0, uq = 0;
        if (b + lane < hi) {
            const int64_t u = users[b + lane];
            if (cooc_user_quant(user_w, u, frac_bits, &uq)) {
                l0 = user_off[u];
                len = user_off[u + 1] - l0;
            }
        }
        const long long end = knn_scan(len, lane);        // entries of the batch up to and including this lane's list
        knn_lds_order();
        w_end[lane] = end;
        w_base[lane] = l0 - (end - len);                  // entry t of the batch, if in this list, is user_items[w_base + t]
        w_q[lane] = uq;
        knn_lds_order();
        const long long total = knn_readlane64(end, 63);
        for (long long t0 = 0; t0 < total; t0 += 64) {
            const long long t = t0 + lane;
            const bool valid = t < total;
            int j = -1;
            long long q = 0;
            if (valid) {
                const int m = lower_bound(0, 63, [&](int c) { return w_end[c] <= t; });
                j = user_items[w_base[m] + t];
                q = w_q[m];
            }
            f(valid, j, q);
        }
    }
}

#endif

// ---- neighbours of items ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kKnnWaves) void k_cooc_topk(SmlCooc a, int path, char* __restrict__ scratch, int32_t* __restrict__ items,
                                                               float* __restrict__ sims, int32_t* __restrict__ n_elig) {
#ifdef __HIP_DEVICE_COMPILE__
    __shared__ float l_s[kKnnWaves][kKnnMaxK];
    __shared__ int32_t l_i[kKnnWaves][kKnnMaxK];
    __shared__ int32_t t_key[kKnnWaves][kKnnTabSlots];
    __shared__ int32_t t_val[kKnnWaves][kKnnTabSlots];
    __shared__ long long w_end[kKnnWaves][64];
    __shared__ long long w_base[kKnnWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int32_t* const keys = t_key[wave];
    int32_t* const vals = t_val[wave];
    for (int s = lane; s < kKnnTabSlots; s += 64) { keys[s] = -1; vals[s] = 0; }
    knn_lds_order();
    int32_t* const acc = reinterpret_cast<int32_t*>(scratch + ((int64_t)blockIdx.x * kKnnWaves + wave) * knn_slot_bytes(a.n_item, 0));
    KnnList top;
    top.ls = l_s[wave];
    top.li = l_i[wave];
    top.k = a.k;

    for (int64_t x = (int64_t)blockIdx.x * kKnnWaves + wave; x < a.n; x += (int64_t)gridDim.x * kKnnWaves) {
        const int64_t i = a.rows ? a.rows[x] : x;
        const int64_t lo = a.item_off ? a.item_off[i] : 0, hi = a.item_off ? a.item_off[i + 1] : 0;
        top.reset();
        // the row's total list length, as far as the path needs it: every user of the row holds at least the row's item
        bool lds = path != 1 && hi - lo <= kKnnLdsLimit;
        if (lds) {
            long long mine = 0;
            for (int64_t e = lo + lane; e < hi; e += 64) {
                const int64_t u = a.item_users[e];
                mine += a.user_off[u + 1] - a.user_off[u];
            }
            lds = knn_wave_sum(mine) <= kKnnLdsLimit;
        }
        const auto consume = [&](bool have, int j, int c) {
            bool elig = have && j != (int)i && c >= a.min_co && knn_allowed(a.allow, j);
            float s = 0.0f;
            if (elig) {
                s = cooc_score(c, a.norm_a, a.norm_b, i, j, a.shrink);
                elig = s == s;
            }
            top.offer(lane, elig, s, j);
        };
        if (lds) {
            cooc_walk(a.user_off, a.user_items, a.item_users, lo, hi, lane, w_end[wave], w_base[wave], [&](bool valid, int j) {
                if (valid) knn_tab_add<int32_t>(keys, vals, j, 1);
            });
            knn_lds_order();
            for (int s0 = 0; s0 < kKnnTabSlots; s0 += 64) {
                const int j = keys[s0 + lane], c = vals[s0 + lane];
                if (__ballot(j != -1) == 0) continue;
                if (j != -1) { keys[s0 + lane] = -1; vals[s0 + lane] = 0; }
                consume(j != -1, j, c);
            }
            knn_lds_order();
        } else {
            cooc_walk(a.user_off, a.user_items, a.item_users, lo, hi, lane, w_end[wave], w_base[wave], [&](bool valid, int j) {
                if (valid) __hip_atomic_fetch_add(&acc[j], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            });
            __threadfence();                  // this wave's adds have landed before anything is claimed
            cooc_walk(a.user_off, a.user_items, a.item_users, lo, hi, lane, w_end[wave], w_base[wave], [&](bool valid, int j) {
                int c = 0;
                if (valid) c = __hip_atomic_exchange(&acc[j], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                consume(c != 0, j, c);        // a non-zero count: this lane is the one that claimed j
            });
        }
        top.write(lane, x, items, sims, n_elig);
    }
#endif
}

// ---- weighted neighbours of items: the kernel above with each user's unit replaced by its weight in fixed point ---------------
// (a sibling and not a template parameter of k_cooc_topk, whose instructions stay as they are).  Static LDS: the two lists 2 KB
// each, 16 KB of keys, 32 KB of sums, three per-wave arrays of 2 KB: 58 KB.
__global__ __launch_bounds__(64 * kKnnWaves) void k_cooc_topk_weighted(SmlCoocWeighted a, int path, char* __restrict__ scratch,
                                                                        int32_t* __restrict__ items, float* __restrict__ sims,
                                                                        int32_t* __restrict__ n_elig) {
#ifdef __HIP_DEVICE_COMPILE__
    __shared__ float l_s[kKnnWaves][kKnnMaxK];
    __shared__ int32_t l_i[kKnnWaves][kKnnMaxK];
    __shared__ int32_t t_key[kKnnWaves][kKnnTabSlots];
    __shared__ long long t_val[kKnnWaves][kKnnTabSlots];
    __shared__ long long w_end[kKnnWaves][64];
    __shared__ long long w_base[kKnnWaves][64];
    __shared__ long long w_q[kKnnWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int32_t* const keys = t_key[wave];
    long long* const vals = t_val[wave];
    for (int s = lane; s < kKnnTabSlots; s += 64) { keys[s] = -1; vals[s] = 0; }
    knn_lds_order();
    long long* const acc = reinterpret_cast<long long*>(scratch + ((int64_t)blockIdx.x * kKnnWaves + wave) * knn_acc_bytes(a.n_item, 1));
    KnnList top;
    top.ls = l_s[wave];
    top.li = l_i[wave];
    top.k = a.k;

    for (int64_t x = (int64_t)blockIdx.x * kKnnWaves + wave; x < a.n; x += (int64_t)gridDim.x * kKnnWaves) {
        const int64_t i = a.rows ? a.rows[x] : x;
        const int64_t lo = a.item_off ? a.item_off[i] : 0, hi = a.item_off ? a.item_off[i + 1] : 0;
        top.reset();
        // the row's total list length over all its users, contributing or not: a bound on what the walk deals
        bool lds = path != 1 && hi - lo <= kKnnLdsLimit;
        if (lds) {
            long long mine = 0;
            for (int64_t e = lo + lane; e < hi; e += 64) {
                const int64_t u = a.item_users[e];
                mine += a.user_off[u + 1] - a.user_off[u];
            }
            lds = knn_wave_sum(mine) <= kKnnLdsLimit;
        }
        const auto consume = [&](bool have, int j, long long cw) {
            bool elig = have && j != (int)i && knn_allowed(a.allow, j);
            float s = 0.0f;
            if (elig) {
                s = cooc_score_weighted(cw, a.frac_bits, a.norm_a, a.norm_b, i, j, a.shrink);
                elig = s == s;
            }
            top.offer(lane, elig, s, j);
        };
        const auto walk = [&](auto&& f) {
            cooc_walk_weighted(a.user_off, a.user_items, a.item_users, lo, hi, lane, w_end[wave], w_base[wave], a.user_w, a.frac_bits,
                               w_q[wave], f);
        };
        if (lds) {
            walk([&](bool valid, int j, long long q) {
                if (valid) knn_tab_add<long long>(keys, vals, j, q);
            });
            knn_lds_order();
            for (int s0 = 0; s0 < kKnnTabSlots; s0 += 64) {
                const int j = keys[s0 + lane];
                const long long cw = vals[s0 + lane];
                if (__ballot(j != -1) == 0) continue;
                if (j != -1) { keys[s0 + lane] = -1; vals[s0 + lane] = 0; }
                consume(j != -1, j, cw);
            }
            knn_lds_order();
        } else {
            walk([&](bool valid, int j, long long q) {
                if (valid) __hip_atomic_fetch_add(&acc[j], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            });
            __threadfence();                  // this wave's adds have landed before anything is claimed
            walk([&](bool valid, int j, long long) {
                long long cw = 0;
                if (valid) cw = __hip_atomic_exchange(&acc[j], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                consume(cw != 0, j, cw);      // every contribution is >= 1: a non-zero sum says this lane claimed j
            });
        }
        top.write(lane, x, items, sims, n_elig);
    }
#endif
}

// ---- the list of a history ----------------------------------------------------------------------------------------------------
#ifdef __HIP_DEVICE_COMPILE__
// Walk of a history: f(valid, j, q) for every contributing slot of the neighbour lists of hist[lo .. hi), called by all 64 lanes
// together.  A round covers 64 / k_nbr members (k_nbr <= 64) or half a member (k_nbr > 64).
template <class F>
__device__ __forceinline__ void knn_walk(const SmlKnn& a, int64_t lo, int64_t hi, int lane, F&& f) {
    const int group = a.k_nbr <= 64 ? 64 / a.k_nbr : 1;          // members per round
    const int rounds = (a.k_nbr + 63) / 64;
    for (int64_t mb = lo; mb < hi; mb += group)
        for (int r = 0; r < rounds; ++r) {
            const int t = lane + 64 * r;
            const int g = t / a.k_nbr, slot = t - g * a.k_nbr;
            bool valid = g < group && mb + g < hi;
            int j = -1;
            long long q = 0;
            if (valid) {
                const int64_t m = a.hist_items[mb + g];
                valid = m >= 0 && m < a.n_rows_nbr;              // (no address is formed from a member out of range)
                if (valid) {
                    j = a.nbr_items[m * a.k_nbr + slot];
                    valid = j >= 0 && j < a.n_item && knn_quant(a.nbr_sims[m * a.k_nbr + slot], a.frac_bits, &q);
                }
            }
            f(valid, j, q);
        }
}
#endif

__global__ __launch_bounds__(64 * kKnnWaves) void k_knn_topk(SmlKnn a, int path, char* __restrict__ scratch, int32_t* __restrict__ items,
                                                              float* __restrict__ scores, int32_t* __restrict__ n_elig) {
#ifdef __HIP_DEVICE_COMPILE__
    __shared__ float l_s[kKnnWaves][kKnnMaxK];
    __shared__ int32_t l_i[kKnnWaves][kKnnMaxK];
    __shared__ int32_t t_key[kKnnWaves][kKnnTabSlots];
    __shared__ long long t_val[kKnnWaves][kKnnTabSlots];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int32_t* const keys = t_key[wave];
    long long* const vals = t_val[wave];
    for (int s = lane; s < kKnnTabSlots; s += 64) { keys[s] = -1; vals[s] = 0; }
    knn_lds_order();
    char* const slot = scratch + ((int64_t)blockIdx.x * kKnnWaves + wave) * knn_slot_bytes(a.n_item, 1);
    long long* const acc = reinterpret_cast<long long*>(slot);
    uint32_t* const touched = reinterpret_cast<uint32_t*>(slot + knn_acc_bytes(a.n_item, 1));
    KnnList top;
    top.ls = l_s[wave];
    top.li = l_i[wave];
    top.k = a.k;

    for (int64_t x = (int64_t)blockIdx.x * kKnnWaves + wave; x < a.n; x += (int64_t)gridDim.x * kKnnWaves) {
        const int64_t u = a.users ? a.users[x] : x;
        const int64_t lo = a.hist_off ? a.hist_off[u] : 0, hi = a.hist_off ? a.hist_off[u + 1] : 0;
        const int64_t s_lo = a.seen_off ? a.seen_off[u] : 0, s_hi = a.seen_off ? a.seen_off[u + 1] : 0;
        top.reset();
        const bool lds = path != 1 && (hi - lo) * a.k_nbr <= kKnnLdsLimit;
        const auto consume = [&](bool have, int j, long long sum) {
            bool elig = have && knn_allowed(a.allow, j);
            if (elig && s_lo < s_hi) {
                const int64_t at = lower_bound(s_lo, s_hi, [&](int64_t m) { return a.seen_items[m] < j; });
                elig = !(at < s_hi && a.seen_items[at] == j);
            }
            top.offer(lane, elig, knn_score(sum, a.frac_bits), j);
        };
        if (lds) {
            knn_walk(a, lo, hi, lane, [&](bool valid, int j, long long q) {
                if (valid) knn_tab_add<long long>(keys, vals, j, q);
            });
            knn_lds_order();
            for (int s0 = 0; s0 < kKnnTabSlots; s0 += 64) {
                const int j = keys[s0 + lane];
                const long long sum = vals[s0 + lane];
                if (__ballot(j != -1) == 0) continue;
                if (j != -1) { keys[s0 + lane] = -1; vals[s0 + lane] = 0; }
                consume(j != -1, j, sum);
            }
            knn_lds_order();
        } else {
            knn_walk(a, lo, hi, lane, [&](bool valid, int j, long long q) {
                if (valid) {
                    __hip_atomic_fetch_add(&acc[j], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_or(&touched[j >> 5], 1u << (j & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            });
            __threadfence();                  // this wave's adds have landed before anything is claimed
            if ((hi - lo) * a.k_nbr > a.n_item) {
                // more slots than items: the candidates are claimed from the bitmap itself, a word per lane (taken and cleared by
                // one exchange), then bit by bit -- at most n_item / 64 rounds, where a second walk would take slots / 64
                const int64_t n_words = (a.n_item + 31) / 32;
                for (int64_t w0 = 0; w0 < n_words; w0 += 64) {
                    const int64_t w = w0 + lane;
                    uint32_t word = 0;
                    if (w < n_words) word = __hip_atomic_exchange(&touched[w], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (__ballot(word != 0) == 0) continue;
                    for (int b = 0; b < 32; ++b) {
                        const bool mine = (word >> b) & 1u;
                        if (__ballot(mine) == 0) continue;
                        const int j = (int)(w * 32 + b);
                        long long sum = 0;
                        if (mine) sum = __hip_atomic_exchange(&acc[j], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        consume(mine, j, sum);
                    }
                }
            } else {
                knn_walk(a, lo, hi, lane, [&](bool valid, int j, long long) {
                    bool mine = false;
                    long long sum = 0;
                    if (valid) {
                        const uint32_t bit = 1u << (j & 31);
                        mine = __hip_atomic_fetch_and(&touched[j >> 5], ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit;
                        if (mine) sum = __hip_atomic_exchange(&acc[j], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    consume(mine, j, sum);    // a sum that cancelled to 0 is still a candidate: the bit says so, not the sum
                });
            }
        }
        top.write(lane, x, items, scores, n_elig);
    }
#endif
}

int64_t knn_blocks(int64_t n, int max_workgroups) {
    const int64_t cap = max_workgroups > 0 ? max_workgroups : kKnnGrid;
    const int64_t blocks = (n + kKnnWaves - 1) / kKnnWaves;
    return blocks < cap ? blocks : cap;
}

// the K best of cand (a full sort by `better`), then (-1, -inf)
void knn_host_emit(std::vector<std::pair<float, int32_t>>& cand, int k, int32_t* items, float* scores, int32_t* n_elig) {
    std::sort(cand.begin(), cand.end(), [](const std::pair<float, int32_t>& p, const std::pair<float, int32_t>& q) {
        return better(p.first, p.second, q.first, q.second);
    });
    for (int q = 0; q < k; ++q) {
        const bool live = q < (int)cand.size();
        items[q] = live ? cand[q].second : -1;
        scores[q] = live ? cand[q].first : -INFINITY;
    }
    if (n_elig) *n_elig = (int32_t)cand.size();
}

}  // namespace

int sml_knn_lds_entries(void) { return kKnnLdsLimit; }

int64_t sml_knn_scratch_size(int64_t n_item, int max_workgroups, int kind) {
    return (max_workgroups > 0 ? (int64_t)max_workgroups : (int64_t)kKnnGrid) * kKnnWaves * knn_slot_bytes(n_item, kind);
}

hipError_t sml_launch_cooc_topk(const SmlCooc& a, int max_workgroups, int path, void* scratch, int32_t* items, float* sims, int32_t* n_elig,
                                hipStream_t st) {
    const int64_t blocks = knn_blocks(a.n, max_workgroups);
    const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)(blocks * kKnnWaves * knn_slot_bytes(a.n_item, 0)), st);
    if (e != hipSuccess) return e;
    k_cooc_topk<<<dim3((unsigned)blocks), dim3(64 * kKnnWaves), 0, st>>>(a, path, static_cast<char*>(scratch), items, sims, n_elig);
    return hipGetLastError();
}

int64_t sml_cooc_weighted_scratch_size(int64_t n_item, int max_workgroups) {
    return (max_workgroups > 0 ? (int64_t)max_workgroups : (int64_t)kKnnGrid) * kKnnWaves * knn_acc_bytes(n_item, 1);
}

hipError_t sml_launch_cooc_topk_weighted(const SmlCoocWeighted& a, int max_workgroups, int path, void* scratch, int32_t* items, float* sims,
                                         int32_t* n_elig, hipStream_t st) {
    const int64_t blocks = knn_blocks(a.n, max_workgroups);
    const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)(blocks * kKnnWaves * knn_acc_bytes(a.n_item, 1)), st);
    if (e != hipSuccess) return e;
    k_cooc_topk_weighted<<<dim3((unsigned)blocks), dim3(64 * kKnnWaves), 0, st>>>(a, path, static_cast<char*>(scratch), items, sims, n_elig);
    return hipGetLastError();
}

hipError_t sml_launch_knn_topk(const SmlKnn& a, int max_workgroups, int path, void* scratch, int32_t* items, float* scores, int32_t* n_elig,
                               hipStream_t st) {
    const int64_t blocks = knn_blocks(a.n, max_workgroups);
    const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)(blocks * kKnnWaves * knn_slot_bytes(a.n_item, 1)), st);
    if (e != hipSuccess) return e;
    k_knn_topk<<<dim3((unsigned)blocks), dim3(64 * kKnnWaves), 0, st>>>(a, path, static_cast<char*>(scratch), items, scores, n_elig);
    return hipGetLastError();
}

// the definitions as the header writes them: a plain dense array, then a full sort
void sml_cooc_host_walk(const SmlCooc& a, int32_t* items, float* sims, int32_t* n_elig) {
    std::vector<int32_t> count((size_t)a.n_item, 0);
    std::vector<int32_t> seen_ids;
    std::vector<std::pair<float, int32_t>> cand;
    for (int64_t x = 0; x < a.n; ++x) {
        const int64_t i = a.rows ? a.rows[x] : x;
        const int64_t lo = a.item_off ? a.item_off[i] : 0, hi = a.item_off ? a.item_off[i + 1] : 0;
        seen_ids.clear();
        cand.clear();
        for (int64_t e = lo; e < hi; ++e) {
            const int64_t u = a.item_users[e];
            for (int64_t p = a.user_off[u]; p < a.user_off[u + 1]; ++p) {
                const int32_t j = a.user_items[p];
                if (count[j]++ == 0) seen_ids.push_back(j);
            }
        }
        for (const int32_t j : seen_ids) {
            const int c = count[j];
            count[j] = 0;
            if (j == (int32_t)i || c < a.min_co || !knn_allowed(a.allow, j)) continue;
            const float s = cooc_score(c, a.norm_a, a.norm_b, i, j, a.shrink);
            if (s == s) cand.emplace_back(s, j);
        }
        knn_host_emit(cand, a.k, items + x * a.k, sims + x * a.k, n_elig ? n_elig + x : nullptr);
    }
}

void sml_cooc_weighted_host_walk(const SmlCoocWeighted& a, int32_t* items, float* sims, int32_t* n_elig) {
    std::vector<long long> cw((size_t)a.n_item, 0);
    std::vector<int32_t> seen_ids;
    std::vector<std::pair<float, int32_t>> cand;
    for (int64_t x = 0; x < a.n; ++x) {
        const int64_t i = a.rows ? a.rows[x] : x;
        const int64_t lo = a.item_off ? a.item_off[i] : 0, hi = a.item_off ? a.item_off[i + 1] : 0;
        seen_ids.clear();
        cand.clear();
        for (int64_t e = lo; e < hi; ++e) {
            const int64_t u = a.item_users[e];
            long long q;
            if (!cooc_user_quant(a.user_w, u, a.frac_bits, &q)) continue;
            for (int64_t p = a.user_off[u]; p < a.user_off[u + 1]; ++p) {
                const int32_t j = a.user_items[p];
                if (cw[j] == 0) seen_ids.push_back(j);        // every q is >= 1: touched <=> non-zero
                cw[j] += q;
            }
        }
        for (const int32_t j : seen_ids) {
            const long long sum = cw[j];
            cw[j] = 0;
            if (j == (int32_t)i || !knn_allowed(a.allow, j)) continue;
            const float s = cooc_score_weighted(sum, a.frac_bits, a.norm_a, a.norm_b, i, j, a.shrink);
            if (s == s) cand.emplace_back(s, j);
        }
        knn_host_emit(cand, a.k, items + x * a.k, sims + x * a.k, n_elig ? n_elig + x : nullptr);
    }
}

void sml_knn_host_walk(const SmlKnn& a, int32_t* items, float* scores, int32_t* n_elig) {
    std::vector<long long> acc((size_t)a.n_item, 0);
    std::vector<char> touched((size_t)a.n_item, 0);
    std::vector<int32_t> ids;
    std::vector<std::pair<float, int32_t>> cand;
    for (int64_t x = 0; x < a.n; ++x) {
        const int64_t u = a.users ? a.users[x] : x;
        const int64_t lo = a.hist_off ? a.hist_off[u] : 0, hi = a.hist_off ? a.hist_off[u + 1] : 0;
        const int64_t s_lo = a.seen_off ? a.seen_off[u] : 0, s_hi = a.seen_off ? a.seen_off[u + 1] : 0;
        ids.clear();
        cand.clear();
        for (int64_t e = lo; e < hi; ++e) {
            const int64_t m = a.hist_items[e];
            if (m < 0 || m >= a.n_rows_nbr) continue;
            for (int s = 0; s < a.k_nbr; ++s) {
                const int32_t j = a.nbr_items[m * a.k_nbr + s];
                long long q;
                if (j < 0 || j >= a.n_item || !knn_quant(a.nbr_sims[m * a.k_nbr + s], a.frac_bits, &q)) continue;
                acc[j] += q;
                if (!touched[j]) { touched[j] = 1; ids.push_back(j); }
            }
        }
        for (const int32_t j : ids) {
            const long long sum = acc[j];
            acc[j] = 0;
            touched[j] = 0;
            if (!knn_allowed(a.allow, j)) continue;
            if (s_lo < s_hi && std::binary_search(a.seen_items + s_lo, a.seen_items + s_hi, j)) continue;
            cand.emplace_back(knn_score(sum, a.frac_bits), j);
        }
        knn_host_emit(cand, a.k, items + x * a.k, scores + x * a.k, n_elig ? n_elig + x : nullptr);
    }
}
