// The centroid update of the clustered item index on gfx950 (include/sml_hip.h, "CLUSTERED INDEX"): centroid c becomes the mean
// of the item rows of list c,
//     acc = 0.0 (double); acc += (double)x[m_j][s] for the members m_0 < m_1 < ... in that order; out[c][s] = (T)(float)(acc / len),
// and an empty list keeps centroids_in[c].  The order of the additions is part of the definition, so the bytes depend on no
// launch geometry; there are no atomics.  The search that reads the lists is k_ivf_search in retrieval.hip.
//
// k_ivf_centroids<D, T>  one wavefront per list, kCenWaves lists per workgroup, lanes over the dims (d = 128: dims l and l + 64
//               per lane; d = 32: the upper half of the wave idles).  The member ids are wave-uniform; kCenBatch members' values
//               are requested before the first is added, and the fp64 adds then run in member order.  It runs once per build
//               iteration over n_item rows in all and is not a hot path.
// The kernel and the single-threaded host walk share cen_add / cen_finish.  Contraction is OFF in the whole file (there is no
// multiply to fuse; the pragma states the intent): nothing is contracted or reassociated on either side.
#include <cmath>
#include <type_traits>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "width_dispatch.h"
#include "../../include/sml_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kCenWaves = 4;       // lists per workgroup: one wavefront each
constexpr int kCenBatch = 8;       // members whose values a lane has in flight before the serial adds

// widening to double is exact for fp32 and fp16 alike
template <class T>
__host__ __device__ __forceinline__ void cen_add(double& acc, T x) { acc += (double)x; }

// correctly rounded fp64 division, then double -> float -> T, each to nearest even
template <class T>
__host__ __device__ __forceinline__ T cen_finish(double acc, int64_t len) { return (T)(float)(acc / (double)len); }

// cin and cout may be the same array: a wave reads row c of cin (empty list only) and writes row c of cout, nothing else
template <int D, class T>
__global__ __launch_bounds__(64 * kCenWaves) void k_ivf_centroids(const T* __restrict__ wi, const int64_t* __restrict__ list_off,
                                                                   const int32_t* __restrict__ list_items, int n_list, const T* cin,
                                                                   T* cout) {
    constexpr int P = D > 64 ? D / 64 : 1;      // dims per lane
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.x * kCenWaves + (int)(threadIdx.x >> 6);
    if (c >= n_list || lane >= D) return;
    const int64_t lo = list_off[c], hi = list_off[c + 1];
    if (hi <= lo) {
#pragma unroll
        for (int p = 0; p < P; ++p) cout[(int64_t)c * D + lane + 64 * p] = cin[(int64_t)c * D + lane + 64 * p];
        return;
    }
    double acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.0;
    for (int64_t m = lo; m < hi; m += kCenBatch) {
        T v[kCenBatch][P];
#pragma unroll
        for (int q = 0; q < kCenBatch; ++q) {
            if (m + q < hi) {
                const int64_t id = list_items[m + q];
#pragma unroll
                for (int p = 0; p < P; ++p) v[q][p] = wi[id * D + lane + 64 * p];
            }
        }
#pragma unroll
        for (int q = 0; q < kCenBatch; ++q) {
            if (m + q < hi) {
#pragma unroll
                for (int p = 0; p < P; ++p) cen_add(acc[p], v[q][p]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) cout[(int64_t)c * D + lane + 64 * p] = cen_finish<T>(acc[p], hi - lo);
}

template <int D, class T>
void centroids_host_walk(const T* wi, const int64_t* list_off, const int32_t* list_items, int n_list, const T* cin, T* cout) {
    for (int c = 0; c < n_list; ++c) {
        const int64_t lo = list_off[c], hi = list_off[c + 1];
        for (int s = 0; s < D; ++s) {
            if (hi <= lo) { cout[(int64_t)c * D + s] = cin[(int64_t)c * D + s]; continue; }
            double acc = 0.0;
            for (int64_t m = lo; m < hi; ++m) cen_add(acc, wi[(int64_t)list_items[m] * D + s]);
            cout[(int64_t)c * D + s] = cen_finish<T>(acc, hi - lo);
        }
    }
}

}  // namespace

hipError_t sml_launch_ivf_centroids(int d, int elem_bytes, const void* wi, const int64_t* list_off, const int32_t* list_items, int n_list,
                                    const void* cin, void* cout, hipStream_t st) {
    const dim3 grid((unsigned)((n_list + kCenWaves - 1) / kCenWaves)), block(64 * kCenWaves);
    if (!with_pair<RetrievalPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        k_ivf_centroids<dd(), T><<<grid, block, 0, st>>>(static_cast<const T*>(wi), list_off, list_items, n_list, static_cast<const T*>(cin),
                                                         static_cast<T*>(cout));
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

bool sml_ivf_centroids_host_walk(int d, int elem_bytes, const void* wi, const int64_t* list_off, const int32_t* list_items, int n_list,
                                 const void* cin, void* cout) {
    return with_pair<RetrievalPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        centroids_host_walk<dd(), T>(static_cast<const T*>(wi), list_off, list_items, n_list, static_cast<const T*>(cin), static_cast<T*>(cout));
    });
}
