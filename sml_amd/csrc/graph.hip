// Graph propagation on gfx950 (include/sml_hip.h, "PROPAGATION"): out[x] = a[row] * sum over the row's members m of b[m] * src[m],
// the sparse-times-dense product behind a LightGCN layer, as a pure random-row gather.  The order of every fp32 operation is named
// by the header -- eight strands of fmaf per segment of SML_PROP_SEG members, a fixed tree of adds, the segments added in order --
// so the bytes depend on no launch geometry; there are no floating-point atomics and no matrix instructions.
//
// Lanes.  A member row of D elements is loaded by G = D / 4 lanes, four consecutive elements each (16 B of fp32, 8 B of fp16), so a
//               wavefront holds NG = 64 / G groups (8 / 4 / 2 at d = 32 / 64 / 128).  Group g owns the strands j with j % NG == g
//               -- 1 / 2 / 4 chains of four accumulators per lane -- and the tree's adds between strands of one group are in-lane,
//               the others one cross-lane exchange each (lane distance 32, 16, 8).  A wave therefore has 8 member rows in flight
//               per step and issues two steps before it adds the first.  The ids and their b values are loaded 64 at a time, one
//               per lane, and handed to the groups by ds_bpermute.
// k_prop_rows   one wavefront per output row, rows walked grid-stride.  A row that is not split is summed here, segment after
//               segment, and written.  A split row reserves its segments' slots in scratch (one integer atomic on the header: the
//               slot numbers depend on arrival, the bytes do not) and names itself in every slot.
// k_prop_segs   one wavefront per reserved slot, grid-stride: the segment's value goes to part[slot].
// k_prop_sum    G threads per split row: tot = +0, tot += part in segment order, out = a * tot.
// The kernels and the single-threaded host walk share the prop_* step functions.  Contraction is OFF in the whole file: every fused
// step is an explicit fmaf().
#include <cmath>
#include <type_traits>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "width_dispatch.h"
#include "../../include/sml_hip.h"

#pragma clang fp contract(off)

#ifndef SML_GRAPH_SPLIT_FROM
#define SML_GRAPH_SPLIT_FROM 2      // segments from which a row is split: the value tools/graph_probe.py measured
#endif

namespace {

constexpr int kSeg = SML_PROP_SEG;           // members per segment: a constant of the definition
constexpr int kStrands = SML_PROP_STRANDS;   // independent chains per segment: a constant of the definition
constexpr int kPropWaves = 4;                // wavefronts per workgroup
constexpr int kPropGrid = 2048;              // workgroups when max_workgroups == 0: 8 per CU of 256
constexpr int kSumBatch = 8;                 // k_prop_sum: partial sums in flight per thread
constexpr int kHeaderBytes = 256;          // scratch: the slot counter, alone in its line
static_assert(kStrands == 8 && kSeg % 64 == 0, "the lane plan below is written for 8 strands and whole 64-member loads");

// acc + b * v, one rounding
__host__ __device__ __forceinline__ float prop_mac(float acc, float b, float v) { return fmaf(b, v, acc); }
// one fp32 add of the tree or of the segment sum
__host__ __device__ __forceinline__ float prop_add(float x, float y) { return x + y; }
// a[row] * tot, one rounding
__host__ __device__ __forceinline__ float prop_out(float a, float tot) { return a * tot; }
// the number of segments of a set of len members
__host__ __device__ __forceinline__ int64_t prop_segs(int64_t len) { return (len + kSeg - 1) / kSeg; }
// whether a row of n_seg segments is split under `path` (0 auto, 1 never, 2 every row of more than one segment)
__host__ __device__ __forceinline__ bool prop_split(int64_t n_seg, int path) {
    return path == 1 ? false : path == 2 ? n_seg > 1 : n_seg >= SML_GRAPH_SPLIT_FROM && n_seg > 0;
}

struct PropArgs {
    const void* src;
    const int64_t* set_off; const int32_t* set_items;
    const int64_t* rows; int64_t n;
    const float* a; const float* b;
    float* out;
    int path;
};

#ifdef __HIP_DEVICE_COMPILE__
template <class T> struct PropVec;
template <> struct PropVec<float> {
    __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};
template <> struct PropVec<_Float16> {
    __device__ static __forceinline__ void load(const _Float16* p, float (&v)[4]) {
        typedef _Float16 half4 __attribute__((ext_vector_type(4)));
        const half4 q = *reinterpret_cast<const half4*>(p);
        v[0] = (float)q[0]; v[1] = (float)q[1]; v[2] = (float)q[2]; v[3] = (float)q[3];
    }
};

__device__ __forceinline__ float prop_xor(float v, int mask) { return __shfl_xor(v, mask, 64); }

// The value of one segment -- members items[0 .. cnt), 0 < cnt <= kSeg -- for elements 4 t .. 4 t + 3 (t = lane % G): valid in the
// lanes of group 0.  Every lane of the wave calls it.
template <int D, class T>
__device__ __forceinline__ void prop_segment(const T* __restrict__ src, const float* __restrict__ b, const int32_t* __restrict__ items, int cnt,
                                             int lane, float (&seg)[4]) {
    constexpr int G = D / 4, NG = 64 / G, SPG = kStrands / NG;
    const int grp = lane / G, t = lane % G;
    float acc[SPG][4];
#pragma unroll
    for (int k = 0; k < SPG; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.0f;
    for (int p0 = 0; p0 < cnt; p0 += 64) {
        // 64 ids and their b values, one per lane (a lane past the end holds id 0 and is never asked)
        const int mine = p0 + lane < cnt ? items[p0 + lane] : 0;
        const float bmine = b && p0 + lane < cnt ? b[mine] : 1.0f;
        const int left = cnt - p0 < 64 ? cnt - p0 : 64;
        for (int q = 0; q < left; q += 2 * kStrands) {
            // two steps of 8 positions: position q + 8 s + j belongs to strand j, strand j = grp + NG k to this lane
            float v[2][SPG][4], bb[2][SPG];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int k = 0; k < SPG; ++k) {
                    const int p = q + kStrands * s + grp + NG * k;
                    const int m = __shfl(mine, p & 63, 64);
                    bb[s][k] = __shfl(bmine, p & 63, 64);
                    if (p < left) PropVec<T>::load(src + (int64_t)m * D + 4 * t, v[s][k]);
                }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int k = 0; k < SPG; ++k) {
                    const int p = q + kStrands * s + grp + NG * k;
                    if (p < left) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[k][e] = prop_mac(acc[k][e], bb[s][k], v[s][k][e]);
                    }
                }
        }
    }
    // the tree: u_j = acc_j + acc_{j+4}, v_j = u_j + u_{j+2}, seg = v_0 + v_1.  Strand j lives in group j % NG, chain j / NG; the
    // partner of an exchange holds the other operand, and the lanes of group 0 add in the header's operand order
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (NG == 8) {
            const float u = prop_add(acc[0][e], prop_xor(acc[0][e], 4 * G));
            const float w = prop_add(u, prop_xor(u, 2 * G));
            seg[e] = prop_add(w, prop_xor(w, G));
        } else if constexpr (NG == 4) {
            const float u = prop_add(acc[0][e], acc[1][e]);
            const float w = prop_add(u, prop_xor(u, 2 * G));
            seg[e] = prop_add(w, prop_xor(w, G));
        } else {
            const float u0 = prop_add(acc[0][e], acc[2][e]), u2 = prop_add(acc[1][e], acc[3][e]);
            const float w = prop_add(u0, u2);
            seg[e] = prop_add(w, prop_xor(w, G));
        }
    }
}
#endif

// scratch: the header, base[n], then one record per slot -- the row it belongs to (16 bytes) and its D partial sums -- so that where
// a record lies depends on n and d alone; nnz only bounds how many there can be
struct PropScratch {
    unsigned long long* n_slots;     // header: slots reserved by this call
    int64_t* base;                   // [n]: the first slot of row x, -1: not split
    char* slots;                     // [max_slots] records of prop_stride(D) bytes
};

__host__ __device__ __forceinline__ int64_t prop_align(int64_t v) { return (v + 255) & ~(int64_t)255; }
__host__ __device__ __forceinline__ int64_t prop_stride(int d) { return 16 + 4 * (int64_t)d; }
__host__ __device__ __forceinline__ int32_t* prop_slot_x(char* slots, int d, int64_t s) { return reinterpret_cast<int32_t*>(slots + s * prop_stride(d)); }
__host__ __device__ __forceinline__ float* prop_slot_part(char* slots, int d, int64_t s) {
    return reinterpret_cast<float*>(slots + s * prop_stride(d) + 16);
}
// every named row has at most len / kSeg + 1 segments
int64_t prop_max_slots(int64_t n, int64_t nnz) { return nnz / kSeg + n; }
PropScratch prop_carve(void* scratch, int64_t n) {
    char* p = static_cast<char*>(scratch);
    return PropScratch{reinterpret_cast<unsigned long long*>(p), reinterpret_cast<int64_t*>(p + kHeaderBytes), p + kHeaderBytes + prop_align(8 * n)};
}

template <int D, class T>
__global__ __launch_bounds__(64 * kPropWaves) void k_prop_rows(PropArgs a, unsigned long long* __restrict__ n_slots, int64_t* __restrict__ base,
                                                                char* __restrict__ slots) {
#ifdef __HIP_DEVICE_COMPILE__
    constexpr int G = D / 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const T* src = static_cast<const T*>(a.src);
    for (int64_t x = (int64_t)blockIdx.x * kPropWaves + wv; x < a.n; x += (int64_t)gridDim.x * kPropWaves) {
        const int64_t row = a.rows ? a.rows[x] : x;
        const int64_t lo = a.set_off ? a.set_off[row] : 0, hi = a.set_off ? a.set_off[row + 1] : 0;
        const int64_t n_seg = prop_segs(hi - lo);
        if (base && prop_split(n_seg, a.path)) {
            unsigned long long first = 0;
            if (lane == 0) {
                first = atomicAdd(n_slots, (unsigned long long)n_seg);
                base[x] = (int64_t)first;
            }
            first = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) |
                    (unsigned)__builtin_amdgcn_readfirstlane((int)first);
            for (int64_t c = lane; c < n_seg; c += 64) *prop_slot_x(slots, D, (int64_t)first + c) = (int32_t)x;
            continue;
        }
        if (base && lane == 0) base[x] = -1;
        float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t c = 0; c < n_seg; ++c) {
            const int64_t s0 = lo + c * kSeg;
            float seg[4];
            prop_segment<D, T>(src, a.b, a.set_items + s0, (int)(hi - s0 < kSeg ? hi - s0 : kSeg), lane, seg);
#pragma unroll
            for (int e = 0; e < 4; ++e) tot[e] = prop_add(tot[e], seg[e]);
        }
        if (lane < G) {
            const float ar = a.a ? a.a[row] : 1.0f;
            float4 o;
            o.x = prop_out(ar, tot[0]); o.y = prop_out(ar, tot[1]); o.z = prop_out(ar, tot[2]); o.w = prop_out(ar, tot[3]);
            *reinterpret_cast<float4*>(a.out + x * D + 4 * lane) = o;
        }
    }
#endif
}

template <int D, class T>
__global__ __launch_bounds__(64 * kPropWaves) void k_prop_segs(PropArgs a, const unsigned long long* __restrict__ n_slots,
                                                                const int64_t* __restrict__ base, char* __restrict__ slots) {
#ifdef __HIP_DEVICE_COMPILE__
    constexpr int G = D / 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const T* src = static_cast<const T*>(a.src);
    const int64_t n_used = (int64_t)*n_slots;
    for (int64_t s = (int64_t)blockIdx.x * kPropWaves + wv; s < n_used; s += (int64_t)gridDim.x * kPropWaves) {
        const int64_t x = *prop_slot_x(slots, D, s);
        const int64_t c = s - base[x];
        const int64_t row = a.rows ? a.rows[x] : x;
        const int64_t s0 = a.set_off[row] + c * kSeg, hi = a.set_off[row + 1];
        float seg[4];
        prop_segment<D, T>(src, a.b, a.set_items + s0, (int)(hi - s0 < kSeg ? hi - s0 : kSeg), lane, seg);
        if (lane < G) *reinterpret_cast<float4*>(prop_slot_part(slots, D, s) + 4 * lane) = make_float4(seg[0], seg[1], seg[2], seg[3]);
    }
#endif
}

template <int D>
__global__ __launch_bounds__(256) void k_prop_sum(PropArgs a, const int64_t* __restrict__ base, char* __restrict__ slots) {
    constexpr int G = D / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n * G; i += (int64_t)gridDim.x * 256) {
        const int64_t x = i / G;
        const int t = (int)(i % G);
        const int64_t first = base[x];
        if (first < 0) continue;
        const int64_t row = a.rows ? a.rows[x] : x;
        const int64_t n_seg = prop_segs(a.set_off[row + 1] - a.set_off[row]);
        float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t c0 = 0; c0 < n_seg; c0 += kSumBatch) {            // kSumBatch partials requested before the first is added
            float4 q[kSumBatch];
#pragma unroll
            for (int k = 0; k < kSumBatch; ++k)
                if (c0 + k < n_seg) q[k] = *reinterpret_cast<const float4*>(prop_slot_part(slots, D, first + c0 + k) + 4 * t);
#pragma unroll
            for (int k = 0; k < kSumBatch; ++k)
                if (c0 + k < n_seg) {
                    tot[0] = prop_add(tot[0], q[k].x); tot[1] = prop_add(tot[1], q[k].y);
                    tot[2] = prop_add(tot[2], q[k].z); tot[3] = prop_add(tot[3], q[k].w);
                }
        }
        const float ar = a.a ? a.a[row] : 1.0f;
        *reinterpret_cast<float4*>(a.out + x * D + 4 * t) =
            make_float4(prop_out(ar, tot[0]), prop_out(ar, tot[1]), prop_out(ar, tot[2]), prop_out(ar, tot[3]));
    }
}

// the definition as the header writes it, one row and one element at a time
template <int D, class T>
void prop_row_host(const T* src, const float* b, const int32_t* mem, int64_t len, float ar, float* out) {
    for (int s = 0; s < D; ++s) {
        float tot = 0.0f;
        for (int64_t c0 = 0; c0 < len; c0 += kSeg) {
            const int64_t c1 = c0 + kSeg < len ? c0 + kSeg : len;
            float acc[kStrands];
            for (int j = 0; j < kStrands; ++j) acc[j] = 0.0f;
            for (int64_t p = c0; p < c1; ++p) {
                const int j = (int)(p % kStrands);
                acc[j] = prop_mac(acc[j], b ? b[mem[p]] : 1.0f, (float)src[(int64_t)mem[p] * D + s]);
            }
            float u[4], v[2];
            for (int j = 0; j < 4; ++j) u[j] = prop_add(acc[j], acc[j + 4]);
            for (int j = 0; j < 2; ++j) v[j] = prop_add(u[j], u[j + 2]);
            tot = prop_add(tot, prop_add(v[0], v[1]));
        }
        out[s] = prop_out(ar, tot);
    }
}

}  // namespace

bool sml_graph_supports(int d, int elem_bytes) {
    return with_pair<PropagationPairs>(d, elem_bytes, [](auto, auto*) {});
}

int sml_graph_split_segments(void) { return SML_GRAPH_SPLIT_FROM; }

int64_t sml_graph_scratch_size(int d, int64_t n, int64_t nnz) {
    return kHeaderBytes + prop_align(8 * n) + prop_align(prop_max_slots(n, nnz) * prop_stride(d));
}

hipError_t sml_launch_graph_propagate(int d, int elem_bytes, const void* src, const int64_t* set_off, const int32_t* set_items,
                                      const int64_t* rows, int64_t n, const float* a, const float* b, int max_workgroups, int path,
                                      void* scratch, float* out, hipStream_t st) {
    const PropArgs args = {src, set_off, set_items, rows, n, a, b, out, path};
    const int64_t cap = max_workgroups > 0 ? max_workgroups : kPropGrid;
    int64_t blocks = (n + kPropWaves - 1) / kPropWaves;
    if (blocks > cap) blocks = cap;
    const bool may_split = path != 1 && set_off && scratch;
    const PropScratch s = may_split ? prop_carve(scratch, n) : PropScratch{nullptr, nullptr, nullptr};
    if (may_split) {
        const hipError_t e = hipMemsetAsync(s.n_slots, 0, sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
    }
    const dim3 block(64 * kPropWaves);
    if (!with_pair<PropagationPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        constexpr int D = dd();
        k_prop_rows<D, T><<<dim3((unsigned)blocks), block, 0, st>>>(args, s.n_slots, s.base, s.slots);
        if (may_split) {
            // the slots are counted on the device: both passes take the call's grid and walk what they find
            k_prop_segs<D, T><<<dim3((unsigned)cap), block, 0, st>>>(args, s.n_slots, s.base, s.slots);
            int64_t sum_blocks = (n * (D / 4) + 255) / 256;
            if (sum_blocks > cap) sum_blocks = cap;
            k_prop_sum<D><<<dim3((unsigned)sum_blocks), dim3(256), 0, st>>>(args, s.base, s.slots);
        }
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

bool sml_graph_host_walk(int d, int elem_bytes, const void* src, const int64_t* set_off, const int32_t* set_items, const int64_t* rows,
                         int64_t n, const float* a, const float* b, float* out) {
    return with_pair<PropagationPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        constexpr int D = dd();
        for (int64_t x = 0; x < n; ++x) {
            const int64_t row = rows ? rows[x] : x;
            const int64_t lo = set_off ? set_off[row] : 0, hi = set_off ? set_off[row + 1] : 0;
            prop_row_host<D, T>(static_cast<const T*>(src), b, set_items ? set_items + lo : nullptr, hi - lo, a ? a[row] : 1.0f, out + x * D);
        }
    });
}
