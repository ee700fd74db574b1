// Training negatives on gfx950 (include/sml_hip.h, "training negatives"): one negative per element, drawn uniformly or by a
// popularity cdf over item_all, never one of the user's own items, and -- with a pool of M > 1 -- the one of the first M
// admissible candidates that the current model scores highest (dynamic negative sampling).
//
// k_neg_one     M == 1: one lane per element, elements walked grid-stride; draw_negative's walk with the draws addressed by
//               their number, so with cdf == NULL the bytes are k_sample_negatives'.  No table is read.  (The entry point
//               launches k_sample_negatives itself for cdf == NULL with the grid left to the call: this kernel measured
//               1.3 - 3.8 % slower there, profiles/r18_neg_sampler_probe.json; it serves the cdf and a capped grid.)
// k_neg_pool<D> M > 1: G = the smallest power of two >= M lanes per element, 64 / G elements per wavefront, walked
//               grid-stride.  In round r lane j of a group examines candidate number c = r * G + j: the draw, the position in
//               item_all (uniform or a bisection of the cdf), the bisection of the user's range.  The group's slice of the
//               ballot gives every admissible lane its slot -- the group's running count plus the admissible lanes below it --
//               and lanes with a slot < M gather their candidate's row with 16-byte loads and run the fmaf chain of the
//               retrieval kernels (score_chain, restated below as ns_chain) on the VALU.  A lane keeps the best of its own
//               candidates over the rounds; rounds go on while the group has fewer than M and c < 4096.  Then a G-wide xor
//               butterfly reduces by (NaN last, score descending, c ascending): a total order on the lanes' entries, so the
//               butterfly's order cannot change the result, and the lane that owns the winning c stores it.
// The pool is therefore the first M admissible candidates in order of c whatever G, the grid or the schedule are: the bytes
// are those of sml_neg_sampler_host_walk below, the plain sequential walk of the definition.
// Stores are plain vector stores; the only global atomic is the failure counter.  No LDS, no scratch, no spills
// (tests/test_neg_sampler_host.py reads the compiler's resource report).
//
// Per element with a pool: M * D * 4 bytes of item rows and D * 4 of the user row (every lane of the group holds it: one
// fetch, G - 1 cache hits), M draws of 8 bytes out of item_all, and log2 |range| dependent 8-byte loads per candidate.
#include <cmath>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "../../include/sml_hip.h"

namespace {

constexpr uint32_t NS_NONE = 0xffffffffu;                       // "no candidate yet": loses to every real entry

// S(u, i): retrieval.hip's score_chain, the same fmaf order (dims 0, D/2, 1, D/2 + 1, ...), on rows held by value
template <int D>
__host__ __device__ __forceinline__ float ns_chain(const float (&u)[D], const float (&x)[D]) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        acc = fmaf(x[s], u[s], acc);
        acc = fmaf(x[s + D / 2], u[s + D / 2], acc);
    }
    return acc;
}
template <int D>
__device__ __forceinline__ void ns_load_row(float (&r)[D], const float* __restrict__ row) {
    const f32x4* p = reinterpret_cast<const f32x4*>(row);
#pragma unroll
    for (int q = 0; q < D / 4; ++q) {
        const f32x4 v = p[q];
        r[4 * q] = v[0]; r[4 * q + 1] = v[1]; r[4 * q + 2] = v[2]; r[4 * q + 3] = v[3];
    }
}
// does entry a = (score sa, number ca) come before entry b?  NaN after every number; then the greater score; then the smaller c
__host__ __device__ __forceinline__ bool ns_before(float sa, uint32_t ca, float sb, uint32_t cb) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return sa > sb;
    return ca < cb;
}

__global__ __launch_bounds__(256) void k_neg_one(const int64_t* __restrict__ users, int64_t n, const int64_t* __restrict__ item_all,
                                                 int64_t pop, const int64_t* __restrict__ user_ptr, int64_t n_users,
                                                 const int64_t* __restrict__ user_items, const double* __restrict__ cdf, uint64_t seed,
                                                 int64_t* __restrict__ negs, int* __restrict__ failed) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t u = users[e];
        int64_t b = 0, t = 0;
        if (u >= 0 && u < n_users) { b = user_ptr[u]; t = user_ptr[u + 1]; }
        const uint64_t s0 = neg_stream(seed, e);
        int64_t cand = item_all[0];
        bool found = false;
        for (uint32_t c = 0; c < (uint32_t)SML_NEG_DRAW_CAP; ++c) {
            cand = item_all[neg_candidate_pos(neg_draw(s0, c), pop, cdf)];
            if (!neg_is_own(user_items, b, t, cand)) { found = true; break; }
        }
        if (!found) atomicAdd(failed, 1);
        negs[e] = cand;
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_neg_pool(const int64_t* __restrict__ users, int64_t n, const int64_t* __restrict__ item_all,
                                                  int64_t pop, const int64_t* __restrict__ user_ptr, int64_t n_users,
                                                  const int64_t* __restrict__ user_items, const double* __restrict__ cdf, int M, int G,
                                                  const float* __restrict__ wu, const float* __restrict__ wi, uint64_t seed,
                                                  int64_t* __restrict__ negs, float* __restrict__ score, int* __restrict__ failed) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & (G - 1), gbase = lane & ~(G - 1);         // my place in the group, the group's first lane
    const int epw = 64 / G;                                         // elements per wavefront
    const uint64_t gmask = G == 64 ? ~0ull : (1ull << G) - 1ull;
    const uint64_t below = (1ull << j) - 1ull;
    const float nan = __builtin_nanf("");

    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * epw; base < n; base += (int64_t)gridDim.x * 4 * epw) {   // (wave-uniform)
        const int64_t e = base + (lane / G);
        const bool valid = e < n;
        int64_t u = 0, b = 0, t = 0;
        float ur[D];
#pragma unroll
        for (int q = 0; q < D; ++q) ur[q] = 0.f;
        if (valid) {
            u = users[e];
            if (u >= 0 && u < n_users) { b = user_ptr[u]; t = user_ptr[u + 1]; }
            ns_load_row<D>(ur, wu + u * D);
        }
        const uint64_t s0 = neg_stream(seed, e);
        int have = 0;                                               // admissible candidates of the group so far (group-uniform)
        float best_s = nan;
        uint32_t best_c = NS_NONE;
        int64_t best_item = 0, cand = 0;
        for (uint32_t c0 = 0; c0 < (uint32_t)SML_NEG_DRAW_CAP; c0 += (uint32_t)G) {
            const bool active = valid && have < M;
            if (__ballot(active) == 0ull) break;                    // every group of the wavefront has its pool
            const uint32_t c = c0 + (uint32_t)j;
            bool ok = false;
            if (active) {
                cand = item_all[neg_candidate_pos(neg_draw(s0, c), pop, cdf)];
                ok = !neg_is_own(user_items, b, t, cand);
            }
            const uint64_t slice = (__ballot(ok) >> gbase) & gmask;
            const int slot = have + __popcll(slice & below);
            if (ok && slot < M) {
                float xr[D];
                ns_load_row<D>(xr, wi + cand * D);
                const float s = ns_chain<D>(ur, xr);
                if (ns_before(s, c, best_s, best_c)) { best_s = s; best_c = c; best_item = cand; }
            }
            have += __popcll(slice);
        }
        const uint32_t mine = best_c;
        for (int off = G >> 1; off >= 1; off >>= 1) {               // (G is wave-uniform: every lane takes every step)
            const float os = __shfl_xor(best_s, off, 64);
            const uint32_t oc = (uint32_t)__shfl_xor((int)best_c, off, 64);
            if (ns_before(os, oc, best_s, best_c)) { best_s = os; best_c = oc; }
        }
        if (valid) {
            if (best_c != NS_NONE) {
                if (mine == best_c) {
                    negs[e] = best_item;
                    if (score) score[e] = best_s;
                }
            } else if (j == G - 1) {
                // nothing admissible below the cap: the group went through every round, and this lane's last candidate is
                // number 4095 (4096 is a multiple of G)
                negs[e] = cand;
                if (score) {
                    float xr[D];
                    ns_load_row<D>(xr, wi + cand * D);
                    score[e] = ns_chain<D>(ur, xr);
                }
                atomicAdd(failed, 1);
            }
        }
    }
}

template <int D>
float host_score(const float* wu, const float* wi, int64_t u, int64_t item) {
    float a[D], x[D];
    for (int q = 0; q < D; ++q) { a[q] = wu[u * D + q]; x[q] = wi[item * D + q]; }
    return ns_chain<D>(a, x);
}

}  // namespace

hipError_t sml_launch_neg_sampler(const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop, const int64_t* user_ptr,
                                  int64_t n_users, const int64_t* user_items, const double* cdf, int pool, const float* wu, const float* wi,
                                  int d, uint64_t seed, int max_workgroups, int64_t* negs, float* score, int* failed, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (pool == 1) {
        int64_t grid = (n + 255) / 256;                            // the kernel's own choice: one pass, as k_sample_negatives
        const int64_t cap = max_workgroups > 0 ? max_workgroups : ((int64_t)1 << 22);
        if (grid > cap) grid = cap;
        k_neg_one<<<dim3((unsigned)grid), dim3(256), 0, st>>>(users, n, item_all, pop, user_ptr, n_users, user_items, cdf, seed, negs, failed);
        return hipGetLastError();
    }
    int G = 2;
    while (G < pool) G <<= 1;
    const int64_t per_block = 4 * (64 / G);
    int64_t grid = (n + per_block - 1) / per_block;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : 16384;   // the kernel's own choice: 64 workgroups per CU of 256
    if (grid > cap) grid = cap;
    switch (d) {
        case 32:
            k_neg_pool<32><<<dim3((unsigned)grid), dim3(256), 0, st>>>(users, n, item_all, pop, user_ptr, n_users, user_items, cdf, pool, G, wu,
                                                                      wi, seed, negs, score, failed);
            break;
        case 64:
            k_neg_pool<64><<<dim3((unsigned)grid), dim3(256), 0, st>>>(users, n, item_all, pop, user_ptr, n_users, user_items, cdf, pool, G, wu,
                                                                      wi, seed, negs, score, failed);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The definition as a plain single-threaded walk over host memory (sml_host_sample_negatives_ex): candidates in order of c,
// one at a time, the best so far replaced only by an entry that comes before it.
int64_t sml_neg_sampler_host_walk(const int64_t* users, int64_t n, const int64_t* item_all, int64_t pop, const int64_t* user_ptr,
                                  int64_t n_users, const int64_t* user_items, const double* cdf, int pool, const float* wu, const float* wi,
                                  int d, uint64_t seed, int64_t* negs, float* score) {
    int64_t failed = 0;
    for (int64_t e = 0; e < n; ++e) {
        const int64_t u = users[e];
        int64_t b = 0, t = 0;
        if (u >= 0 && u < n_users) { b = user_ptr[u]; t = user_ptr[u + 1]; }
        const uint64_t s0 = neg_stream(seed, e);
        int have = 0;
        float best_s = std::nanf("");
        uint32_t best_c = NS_NONE;
        int64_t best_item = 0, cand = item_all[0];
        for (uint32_t c = 0; c < (uint32_t)SML_NEG_DRAW_CAP && have < pool; ++c) {
            cand = item_all[neg_candidate_pos(neg_draw(s0, c), pop, cdf)];
            if (neg_is_own(user_items, b, t, cand)) continue;
            ++have;
            if (pool == 1) { best_c = c; best_item = cand; break; }
            const float s = d == 32 ? host_score<32>(wu, wi, u, cand) : host_score<64>(wu, wi, u, cand);
            if (ns_before(s, c, best_s, best_c)) { best_s = s; best_c = c; best_item = cand; }
        }
        if (have == 0) {
            ++failed;
            best_item = cand;                                       // candidate number 4095
            if (pool > 1) best_s = d == 32 ? host_score<32>(wu, wi, u, cand) : host_score<64>(wu, wi, u, cand);
        }
        negs[e] = best_item;
        if (score && pool > 1) score[e] = best_s;
    }
    return failed;
}
