// The top-K family's order and the wave's sorted LDS list, shared by retrieval.hip (sml_topk_candidates, sml_ivf_search) and
// knn.hip (sml_cooc_topk, sml_knn_topk): moved here verbatim from retrieval.hip, whose kernels compile to the same instructions
// (profiles/r23_knn_isa_diff.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// total order of the top-K lists: score descending, then item id ascending (NaN is never better than anything)
__host__ __device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// first index of [lo, hi) at which pred is false, hi if there is none (pred holds on a prefix of the range)
template <class I, class P>
__device__ __forceinline__ I lower_bound(I lo, I hi, P pred) {
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (pred(mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The whole wave inserts the wave-uniform (s, i) into its sorted list ls / li (cnt live entries of k slots, `better` order);
// lane l holds slots l and l + 64.  An entry equal to it in score and id is a repeat: nothing changes.  Otherwise its place
// is the number of better entries (the list is sorted, so those are a prefix), every entry behind moves one slot down (the
// one in slot k - 1 leaves) and lane 0 writes the new one.  Reads come before writes in program order and a wave's LDS
// operations are served in order, so the two need no more than the compiler keeping that order.
__device__ __forceinline__ void cand_insert(float* ls, int32_t* li, int k, int lane, int& cnt, float s, int i) {
    const bool h0 = lane < cnt, h1 = lane + 64 < cnt;
    const float s0 = h0 ? ls[lane] : 0.0f, s1 = h1 ? ls[lane + 64] : 0.0f;
    const int i0 = h0 ? li[lane] : -1, i1 = h1 ? li[lane + 64] : -1;
    if (__any((h0 && s0 == s && i0 == i) || (h1 && s1 == s && i1 == i))) return;
    const bool b0 = h0 && better(s0, i0, s, i), b1 = h1 && better(s1, i1, s, i);
    const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));
    __builtin_amdgcn_wave_barrier();
    if (h0 && !b0 && lane + 1 < k) { ls[lane + 1] = s0; li[lane + 1] = i0; }
    if (h1 && !b1 && lane + 65 < k) { ls[lane + 65] = s1; li[lane + 65] = i1; }
    if (lane == 0 && pos < k) { ls[pos] = s; li[pos] = i; }
    __builtin_amdgcn_wave_barrier();
    if (cnt < k) ++cnt;
}
