// Greedy MMR re-ranking on gfx950 (include/sml_hip.h, "RE-RANKING"): from each list's pool of at most 128 (item, relevance)
// entries pick up to k, one at a time, each pick the unpicked entry with the greatest
//     v = lam * r - (1 - lam) * max over the picks so far of sim(entry, pick),
// and report the sum of the pairwise similarities of the picks.  The header states every rounding; this file has the kernel
// and the single-threaded host walk of the same definition, built from the same __host__ __device__ pieces.
//
// k_rerank_mmr<D, T>  one wavefront per list, lists walked grid-stride, kRrWaves lists per workgroup.  Lane l owns pool slots l
//               and l + 64.  Setting a list up: the entries' ids go into the wave's LDS (-1 for padding and NaN relevance),
//               every lane tests its slots against the lower positions (first occurrence wins), gathers its (up to two)
//               item rows whole with 16-byte loads and KEEPS them in registers (fp16 packed: at most 2 x 64 VGPRs of rows at
//               fp32 d = 64 and at fp16 d = 128), and the list's lo / hi come by a wave min / max over an order-preserving
//               integer key (exact, order-free, -0 below +0).
//               Each step: every lane forms v for its slots; a 64-wide xor butterfly over (NaN last, v descending, position
//               ascending) elects the pick -- a total order, so the butterfly's shape cannot change the result; the owner
//               copies its row to the wave's LDS slot; every lane runs the fmaf chain of its slots against that row on the
//               VALU (the LDS reads are broadcasts) and updates pen and sum; the pick's sum, read from its owner, goes into
//               total.  Registers were built, not LDS rows: the report shows no spill and no scratch at any width
//               (tests/test_rerank_host.py reads it), and LDS rows would cost 32 KB per wave at C = 128.
// No global atomics, no scratch; stores are plain vector stores.  The wave's LDS state (ids, the pick's row) is rewritten for
// every list before it is read.
//
// Contraction is OFF in the whole file: every multiply, add and subtract the header names is one rounding, on the device and
// in the host walk alike; the only fused operations are the fmaf calls spelled out below.
#include <cmath>
#include <cstring>
#include <type_traits>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "width_dispatch.h"
#include "../../include/sml_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRrWaves = 4;                                     // lists per workgroup: one wavefront each
constexpr int kRrMax = 128;                                     // pool entries and picks per list
constexpr uint32_t RR_NONE = 0xffffffffu;                       // "no entry": loses to every real entry

typedef _Float16 rr_f16x8 __attribute__((ext_vector_type(8)));

// one table row as its 16-byte pieces bring it (fp16: packed, D/2 registers); at(s) = dim s as fp32, widened exactly
template <int D, class T>
struct RrRow {
    static constexpr int N = D * (int)sizeof(T) / 16;
    f32x4 p[N];
    __host__ __device__ __forceinline__ float at(int s) const {
        if constexpr (sizeof(T) == 4) return p[s >> 2][s & 3];
        else return (float)__builtin_bit_cast(rr_f16x8, p[s >> 3])[s & 7];
    }
    __host__ __device__ __forceinline__ void zero() {
#pragma unroll
        for (int c = 0; c < N; ++c) p[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void load(const T* __restrict__ row) {
        const f32x4* q = reinterpret_cast<const f32x4*>(row);
#pragma unroll
        for (int c = 0; c < N; ++c) p[c] = q[c];
    }
    // called inside the loop a row outlives: the widened copy of a loop-invariant fp16 row (D/2 more VGPRs) would otherwise
    // be hoisted out of the loop and held beside the packed one (no instruction is emitted)
    __device__ __forceinline__ void keep_packed() {
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int c = 0; c < N; ++c) asm volatile("" : "+v"(p[c]));
        }
    }
};

// S with x_s (the pick) on the user side and x_c (the candidate) on the item side: retrieval.hip's score_chain, the same
// fmaf order (dims 0, D/2, 1, D/2 + 1, ...)
template <int D, class T>
__host__ __device__ __forceinline__ float rr_chain(const RrRow<D, T>& u, const RrRow<D, T>& x) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        acc = fmaf(x.at(s), u.at(s), acc);
        acc = fmaf(x.at(s + D / 2), u.at(s + D / 2), acc);
    }
    return acc;
}
// the same chain for both of a lane's slots at once: each value of the pick's row is read (and, fp16, widened) once
template <int D, class T>
__device__ __forceinline__ void rr_chain2(const RrRow<D, T>& u, const RrRow<D, T>& x0, const RrRow<D, T>& x1, float& s0, float& s1) {
    float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        const float ul = u.at(s), uh = u.at(s + D / 2);
        a0 = fmaf(x0.at(s), ul, a0);
        a1 = fmaf(x1.at(s), ul, a1);
        a0 = fmaf(x0.at(s + D / 2), uh, a0);
        a1 = fmaf(x1.at(s + D / 2), uh, a1);
    }
    s0 = a0;
    s1 = a1;
}
// does entry a = (value va, position ea) come before entry b?  NaN after every number; then the greater value; then the
// smaller position (ns_before's shape)
__host__ __device__ __forceinline__ bool rr_before(float va, uint32_t ea, float vb, uint32_t eb) {
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return nb;
    if (!na && va != vb) return va > vb;
    return ea < eb;
}
// an integer key with the order of the non-NaN floats, -0 below +0: the list's lo / hi are the min / max key
__host__ __device__ __forceinline__ uint32_t rr_key(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float rr_unkey(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__host__ __device__ __forceinline__ float rr_relevance(float rel, float lo, float span, int normalize) {
    if (!normalize) return rel;
    if (!(span > 0.0f)) return 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(rel - lo, span);
#else
    return (rel - lo) / span;
#endif
}
__host__ __device__ __forceinline__ float rr_value(float lam, float oml, float r, float pen, bool first) {
    const float q = first ? 0.0f : -(oml * pen);
    return fmaf(lam, r, q);
}
// the candidate's norm first
__host__ __device__ __forceinline__ float rr_sim(float S, float nc, float ns, bool cosine) { return cosine ? (S * nc) * ns : S; }

__device__ __forceinline__ uint32_t rr_wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t rr_wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <int D, class T>
__global__ __launch_bounds__(64 * kRrWaves) void k_rerank_mmr(const T* __restrict__ wi, int64_t n_item,
                                                              const int32_t* __restrict__ pool_items,
                                                              const float* __restrict__ pool_rel, int64_t n, int pool_cols,
                                                              int64_t pool_stride, const float* __restrict__ nrm, float lam,
                                                              float oml, int normalize, int k, int32_t* __restrict__ items,
                                                              int32_t* __restrict__ pos, float* __restrict__ value,
                                                              int32_t* __restrict__ n_sel, float* __restrict__ sim_sum) {
    __shared__ int32_t l_key[kRrWaves][kRrMax];                  // the id of a valid entry (in range, rel not NaN), else -1
    __shared__ RrRow<D, T> l_row[kRrWaves];                      // the pick's row
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int32_t* const lk = l_key[wave];
    const bool cosine = nrm != nullptr;
    const bool two = pool_cols > 64;                             // (wave-uniform) slots 64.. exist

    for (int64_t x = (int64_t)blockIdx.x * kRrWaves + wave; x < n; x += (int64_t)gridDim.x * kRrWaves) {
        const int64_t base = x * pool_stride;
        int id0 = -1, id1 = -1;
        float rel0 = 0.0f, rel1 = 0.0f;
        if (lane < pool_cols) { id0 = pool_items[base + lane]; rel0 = pool_rel[base + lane]; }
        if (lane + 64 < pool_cols) { id1 = pool_items[base + lane + 64]; rel1 = pool_rel[base + lane + 64]; }
        bool el0 = id0 >= 0 && id0 < n_item && rel0 == rel0;     // anything else is padding: no address is formed from it
        bool el1 = id1 >= 0 && id1 < n_item && rel1 == rel1;
        lk[lane] = el0 ? id0 : -1;
        lk[lane + 64] = el1 ? id1 : -1;
        __builtin_amdgcn_wave_barrier();
        for (int e = 0; e < pool_cols - 1; ++e) {               // the first occurrence wins (a broadcast read per position)
            const int32_t c = lk[e];
            el0 = el0 && !(e < lane && c == id0);
            el1 = el1 && !(e < lane + 64 && c == id1);
        }
        RrRow<D, T> r0, r1;
        r0.zero();
        r1.zero();
        float n0 = 0.0f, n1 = 0.0f;
        if (el0) {
            r0.load(wi + (int64_t)id0 * D);
            if (cosine) n0 = nrm[id0];
        }
        if (el1) {
            r1.load(wi + (int64_t)id1 * D);
            if (cosine) n1 = nrm[id1];
        }
        const int m = __popcll(__ballot(el0)) + __popcll(__ballot(el1));
        const int nsel = m < k ? m : k;
        uint32_t klo = 0xffffffffu, khi = 0u;
        if (el0) klo = khi = rr_key(rel0);
        if (el1) {
            const uint32_t q = rr_key(rel1);
            klo = q < klo ? q : klo;
            khi = q > khi ? q : khi;
        }
        float rl0 = rel0, rl1 = rel1;
        if (normalize && m > 0) {
            const float lo = rr_unkey(rr_wave_min(klo)), hi = rr_unkey(rr_wave_max(khi));
            const float span = hi - lo;
            rl0 = rr_relevance(rel0, lo, span, 1);
            rl1 = rr_relevance(rel1, lo, span, 1);
        }
        float pen0 = -INFINITY, pen1 = -INFINITY, sum0 = 0.0f, sum1 = 0.0f, total = 0.0f;
        bool live0 = el0, live1 = el1;
        int oi0 = -1, oi1 = -1, op0 = -1, op1 = -1;              // lane l keeps the outputs of picks l and l + 64
        float ov0 = -INFINITY, ov1 = -INFINITY;

        for (int t = 0; t < nsel; ++t) {
            r0.keep_packed();
            r1.keep_packed();
            const float v0 = rr_value(lam, oml, rl0, pen0, t == 0), v1 = rr_value(lam, oml, rl1, pen1, t == 0);
            float bv = __builtin_nanf("");
            uint32_t bp = RR_NONE;
            if (live0) { bv = v0; bp = (uint32_t)lane; }
            if (live1 && rr_before(v1, (uint32_t)lane + 64u, bv, bp)) { bv = v1; bp = (uint32_t)lane + 64u; }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off, 64);
                const uint32_t oe = (uint32_t)__shfl_xor((int)bp, off, 64);
                if (rr_before(ov, oe, bv, bp)) { bv = ov; bp = oe; }
            }
            // every lane holds the pick now (t < nsel: an eligible entry is unpicked, so bp is a position)
            const int e = __builtin_amdgcn_readfirstlane((int)bp);
            const float v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bv)));
            const int ol = e & 63;
            const bool hi_slot = e >= 64;
            const int pid = lk[e];
            if (lane == (t & 63)) {
                if (t < 64) { oi0 = pid; op0 = e; ov0 = v; }
                else { oi1 = pid; op1 = e; ov1 = v; }
            }
            const float psum = __shfl(hi_slot ? sum1 : sum0, ol, 64);
            const float pn = __shfl(hi_slot ? n1 : n0, ol, 64);
            total = total + psum;
            if (t + 1 == nsel) break;                            // nothing reads pen or sum after the last pick
            if (hi_slot) {
                if (lane == ol) { l_row[wave] = r1; live1 = false; }
            } else {
                if (lane == ol) { l_row[wave] = r0; live0 = false; }
            }
            __builtin_amdgcn_wave_barrier();
            float c0, c1 = 0.0f;
            if (two) rr_chain2<D, T>(l_row[wave], r0, r1, c0, c1);
            else c0 = rr_chain<D, T>(l_row[wave], r0);
            const float s0 = rr_sim(c0, n0, pn, cosine), s1 = rr_sim(c1, n1, pn, cosine);
            if (live0) {
                pen0 = s0 > pen0 ? s0 : pen0;                    // (a NaN sim never replaces pen)
                sum0 = sum0 + s0;
            }
            if (live1) {
                pen1 = s1 > pen1 ? s1 : pen1;
                sum1 = sum1 + s1;
            }
            __builtin_amdgcn_wave_barrier();                     // the next pick's row is written after these reads
        }
        if (lane < k) {
            items[x * k + lane] = oi0;
            pos[x * k + lane] = op0;
            value[x * k + lane] = ov0;
        }
        if (lane + 64 < k) {
            items[x * k + lane + 64] = oi1;
            pos[x * k + lane + 64] = op1;
            value[x * k + lane + 64] = ov1;
        }
        if (lane == 0) {
            n_sel[x] = nsel;
            sim_sum[x] = total;
        }
        __builtin_amdgcn_wave_barrier();                         // the next list's ids are written after this list's reads
    }
}

// The definition as a plain single-threaded walk over host memory (sml_host_rerank_mmr): one entry at a time, the best so
// far replaced only by an entry that comes before it.
template <int D, class T>
void rr_host_walk(const T* wi, int64_t n_item, const int32_t* pool_items, const float* pool_rel, int64_t n, int pool_cols,
                  int64_t pool_stride, const float* nrm, float lam, int normalize, int k, int32_t* items, int32_t* pos, float* value,
                  int32_t* n_sel, float* sim_sum) {
    const float oml = 1.0f - lam;
    const bool cosine = nrm != nullptr;
    static thread_local RrRow<D, T> row[kRrMax];
    for (int64_t x = 0; x < n; ++x) {
        const int32_t* id = pool_items + x * pool_stride;
        const float* rel = pool_rel + x * pool_stride;
        bool live[kRrMax];
        float r[kRrMax], pen[kRrMax], sum[kRrMax], nr[kRrMax];
        int m = 0;
        uint32_t klo = 0xffffffffu, khi = 0u;
        for (int e = 0; e < pool_cols; ++e) {
            bool ok = id[e] >= 0 && id[e] < n_item && rel[e] == rel[e];
            for (int f = 0; ok && f < e; ++f) ok = !(id[f] == id[e] && rel[f] == rel[f]);
            live[e] = ok;
            pen[e] = -INFINITY;
            sum[e] = 0.0f;
            nr[e] = 0.0f;
            if (!ok) continue;
            ++m;
            std::memcpy(&row[e], wi + (int64_t)id[e] * D, sizeof(row[e]));
            if (cosine) nr[e] = nrm[id[e]];
            const uint32_t q = rr_key(rel[e]);
            klo = q < klo ? q : klo;
            khi = q > khi ? q : khi;
        }
        if (m > 0) {
            const float lo = rr_unkey(klo), hi = rr_unkey(khi);
            const float span = hi - lo;
            for (int e = 0; e < pool_cols; ++e)
                if (live[e]) r[e] = rr_relevance(rel[e], lo, span, normalize);
        }
        const int nsel = m < k ? m : k;
        float total = 0.0f;
        for (int t = 0; t < nsel; ++t) {
            float bv = std::nanf("");
            uint32_t bp = RR_NONE;
            for (int e = 0; e < pool_cols; ++e) {
                if (!live[e]) continue;
                const float v = rr_value(lam, oml, r[e], pen[e], t == 0);
                if (rr_before(v, (uint32_t)e, bv, bp)) { bv = v; bp = (uint32_t)e; }
            }
            const int s = (int)bp;
            items[x * k + t] = id[s];
            pos[x * k + t] = s;
            value[x * k + t] = bv;
            total = total + sum[s];
            live[s] = false;
            for (int e = 0; e < pool_cols; ++e) {
                if (!live[e]) continue;
                const float sim = rr_sim(rr_chain<D, T>(row[s], row[e]), nr[e], nr[s], cosine);
                pen[e] = sim > pen[e] ? sim : pen[e];
                sum[e] = sum[e] + sim;
            }
        }
        for (int t = nsel; t < k; ++t) {
            items[x * k + t] = -1;
            pos[x * k + t] = -1;
            value[x * k + t] = -INFINITY;
        }
        n_sel[x] = nsel;
        sim_sum[x] = total;
    }
}

}  // namespace

hipError_t sml_launch_rerank_mmr(int d, int elem_bytes, const void* wi, int64_t n_item, const int32_t* pool_items, const float* pool_rel,
                                 int64_t n, int pool_cols, int64_t pool_stride, const float* nrm, float lam, int normalize, int k,
                                 int max_workgroups, int32_t* items, int32_t* pos, float* value, int32_t* n_sel, float* sim_sum,
                                 hipStream_t st) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + kRrWaves - 1) / kRrWaves;
    if (blocks > 65536) blocks = 65536;                          // beyond this the lists are walked grid-stride
    if (max_workgroups > 0 && blocks > max_workgroups) blocks = max_workgroups;
    const dim3 grid((unsigned)blocks), block(64 * kRrWaves);
    const float oml = 1.0f - lam;
    if (!with_pair<RetrievalPairs>(d, elem_bytes, [&](auto dd, auto* t) {
            using T = std::remove_pointer_t<decltype(t)>;
            k_rerank_mmr<dd(), T><<<grid, block, 0, st>>>(static_cast<const T*>(wi), n_item, pool_items, pool_rel, n, pool_cols, pool_stride, nrm,
                                                          lam, oml, normalize, k, items, pos, value, n_sel, sim_sum);
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

bool sml_rerank_host_walk(int d, int elem_bytes, const void* wi, int64_t n_item, const int32_t* pool_items, const float* pool_rel, int64_t n,
                          int pool_cols, int64_t pool_stride, const float* nrm, float lam, int normalize, int k, int32_t* items,
                          int32_t* pos, float* value, int32_t* n_sel, float* sim_sum) {
    return with_pair<RetrievalPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        rr_host_walk<dd(), T>(static_cast<const T*>(wi), n_item, pool_items, pool_rel, n, pool_cols, pool_stride, nrm, lam, normalize, k, items,
                              pos, value, n_sel, sim_sum);
    });
}
