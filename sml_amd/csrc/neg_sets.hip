// Test-set negatives on gfx950: every row of a test period gets neg_num distinct items of the catalogue as of that row that
// its user has not interacted with as of that row (include/sml_hip.h, "test-set negatives"; the device form of the reference's
// data/dataset2.py select_neg_forinteraction, as a distribution).
//
// k_neg_sets: ONE WAVEFRONT PER ROW, rows walked grid-stride.  For the row at global position g = g0 + r with user u:
//   history size   the lanes stride over u's range of h_since and count the entries <= g (a butterfly sum): |H(g)|.
//                  n_cat - |H(g)| < neg_num: the row cannot be served -- every slot gets -1, *failed += 1, no draw is made.
//   rounds         64 candidates per round, lane l takes candidate number c = 64 * round + l (neg_set_index, sml_dev.h:
//                  addressed by c, no state to walk).  A lane rejects its candidate when
//                    - it is in H(g): a bisection of u's ascending h_items, then h_since <= g;
//                    - a LOWER lane of this round drew the same item (64 v_readlane compares): whatever became of that lane
//                      -- accepted, in H(g), or a repeat of an earlier accept -- this one is a repeat or shares its fate;
//                    - it was accepted in an earlier round: a probe of the wave's LDS hash set.
//                  The accepted lanes take the slots accepted_so_far + popcount(ballot below me), in candidate order; slots
//                  >= neg_num are dropped.  Then the accepted lanes enter the hash set.
//   hash set       per wave, int32 item ids, a power of two >= 2 * neg_num slots (load <= 1/2), linear probing.  A slot is
//                  claimed with an LDS compare-and-swap on the ITEM ID against "empty": which lane gets which slot depends on
//                  the hardware's order, membership does not, and membership is all that is ever read.
// The output therefore depends on neither the round width, the grid nor the schedule: it is the sequential walk of the
// definition, which sml_neg_sets_host_walk below restates in plain C++ for the host entry.
// Stores are plain vector stores; the only global atomic is the failure counter.  No scratch, no spills
// (tests/test_neg_sets_host.py reads the compiler's resource report).
//
// Per row at the Yelp shape (n_cat ~ 1e5, neg_num 999, |H| small): ~1,010 candidates in 16-17 rounds; per candidate one
// 4-byte gather of `order`, a bisection of the user's range (log2 |range| dependent 4-byte loads, L2 hits after the first
// round), 64 compares and one LDS probe; per row 8,008 bytes written.  The writes are the traffic that matters.
#include "sml_dev.h"
#include "sml_kernels.h"
#include "../../include/sml_hip.h"

#include <vector>

namespace {

constexpr int32_t NS_EMPTY = -1;

__device__ __forceinline__ uint32_t ns_hash(int32_t x) { return (uint32_t)x * 0x9e3779b1u; }

__global__ __launch_bounds__(256) void k_neg_sets(const int64_t* __restrict__ rows, int64_t n, int n_cols, int64_t g0,
                                                  const int32_t* __restrict__ n_cat, const int32_t* __restrict__ order,
                                                  const int64_t* __restrict__ h_off, const int32_t* __restrict__ h_items,
                                                  const int32_t* __restrict__ h_since, int neg_num, uint64_t seed, int slots,
                                                  int64_t* __restrict__ out, int32_t* __restrict__ failed) {
    extern __shared__ int32_t ns_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int32_t* const tab = ns_lds + (size_t)wave * slots;
    const uint32_t mask = (uint32_t)slots - 1u;
    const uint64_t below = (1ull << lane) - 1ull;
    const int64_t width = 2 + (int64_t)neg_num;

    for (int64_t r = (int64_t)blockIdx.x * waves + wave; r < n; r += (int64_t)gridDim.x * waves) {
        const int64_t g = g0 + r;
        const int32_t gi = (int32_t)g;
        const int64_t u = rows[r * n_cols];
        int64_t* const o = out + r * width;
        if (lane < 2) o[lane] = rows[r * n_cols + lane];
        int64_t* const neg = o + 2;
        const int64_t b = h_off[u], t = h_off[u + 1];
        const int32_t nc = n_cat[r];

        int mine = 0;                                                 // |H(g)|: every lane counts its own stride of the range
#pragma unroll 8                                                      // (independent loads: eight in flight per lane)
        for (int64_t q = b + lane; q < t; q += 64) mine += h_since[q] <= gi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
        const int64_t hist = __builtin_amdgcn_readfirstlane(mine);
        int acc = 0;
        if ((int64_t)nc - hist >= (int64_t)neg_num) {
            for (int s = lane; s < slots; s += 64) tab[s] = NS_EMPTY;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint64_t s0 = neg_stream(seed, g);
            for (uint32_t c0 = 0; c0 < (uint32_t)SML_NEG_SET_CAP && acc < neg_num; c0 += 64) {
                const int32_t cand = order[neg_set_index(s0, (uint64_t)(c0 + lane), (uint32_t)nc)];
                // in H(g)?
                int64_t lo = b, hi = t;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (h_items[mid] < cand) lo = mid + 1; else hi = mid;
                }
                bool reject = lo < t && h_items[lo] == cand && h_since[lo] <= gi;
                // drawn by a lower lane of this round?
#pragma nounroll                                               // (unrolled, the 63 lane values are hoisted into SGPRs: 99 spilled)
                for (int j = 0; j < 63; ++j) reject |= (j < lane) & (__builtin_amdgcn_readlane(cand, j) == cand);
                // accepted in an earlier round?
                if (!reject) {
                    uint32_t p = ns_hash(cand) & mask;
                    for (;;) {
                        const int32_t x = __hip_atomic_load(tab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        if (x == NS_EMPTY) break;
                        if (x == cand) { reject = true; break; }
                        p = (p + 1u) & mask;
                    }
                }
                const uint64_t ok = __ballot(!reject);
                const int slot = acc + __popcll(ok & below);
                if (!reject && slot < neg_num) {
                    neg[slot] = (int64_t)cand;
                    uint32_t p = ns_hash(cand) & mask;                // (at most neg_num entries in >= 2 * neg_num slots: it ends)
                    while (atomicCAS(tab + p, NS_EMPTY, cand) != NS_EMPTY)
                        p = (p + 1u) & mask;
                }
                acc += __popcll(ok);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (acc > neg_num) acc = neg_num;
        }
        if (acc < neg_num) {                                          // not eligible, or the cap: the unfilled slots hold -1
            for (int s = acc + lane; s < neg_num; s += 64) neg[s] = -1;
            if (lane == 0) atomicAdd(failed, 1);
        }
    }
}

inline int slots_for(int neg_num) {
    int s = 128;
    while (s < 2 * neg_num) s <<= 1;
    return s;
}

}  // namespace

hipError_t sml_launch_neg_sets(const int64_t* rows, int64_t n, int n_cols, int64_t g0, const int32_t* n_cat, const int32_t* order,
                               const int64_t* h_off, const int32_t* h_items, const int32_t* h_since, int neg_num, uint64_t seed,
                               int max_workgroups, int64_t* out, int32_t* failed, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int slots = slots_for(neg_num);                             // 128 .. 8192 slots: 512 B .. 32 KB per wave
    int waves = 32768 / (slots * 4);                                  // at most 32 KB of LDS per workgroup
    waves = waves < 1 ? 1 : waves > 4 ? 4 : waves;
    int64_t grid = (n + waves - 1) / waves;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : 8192;   // the kernel's own choice: 32 workgroups per CU of 256
    if (grid > cap) grid = cap;
    k_neg_sets<<<dim3((unsigned)grid), dim3(64 * waves), (size_t)waves * slots * 4, st>>>(rows, n, n_cols, g0, n_cat, order, h_off, h_items,
                                                                                        h_since, neg_num, seed, slots, out, failed);
    return hipGetLastError();
}

// The definition as a plain single-threaded walk over host memory (sml_host_neg_sets): candidates in order of c, one at a
// time.  The accepted set is a stamp per catalogue POSITION (order holds every item once, so equal positions are equal items).
int64_t sml_neg_sets_host_walk(const int64_t* rows, int64_t n, int n_cols, int64_t g0, const int32_t* n_cat, const int32_t* order,
                               const int64_t* h_off, const int32_t* h_items, const int32_t* h_since, int neg_num, uint64_t seed,
                               int64_t* out) {
    int32_t top = 0;
    for (int64_t r = 0; r < n; ++r) top = n_cat[r] > top ? n_cat[r] : top;
    std::vector<int64_t> stamp((size_t)top, (int64_t)-1);             // stamp[k] = the last row that accepted order[k]
    const int64_t width = 2 + (int64_t)neg_num;
    int64_t failed = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t g = g0 + r, u = rows[r * n_cols];
        int64_t* const o = out + r * width;
        o[0] = u; o[1] = rows[r * n_cols + 1];
        const int64_t b = h_off[u], t = h_off[u + 1];
        const int32_t nc = n_cat[r];
        int64_t hist = 0;
        for (int64_t q = b; q < t; ++q) hist += h_since[q] <= g;
        int acc = 0;
        if ((int64_t)nc - hist >= (int64_t)neg_num) {
            const uint64_t s0 = neg_stream(seed, g);
            for (uint64_t c = 0; c < (uint64_t)SML_NEG_SET_CAP && acc < neg_num; ++c) {
                const uint32_t k = neg_set_index(s0, c, (uint32_t)nc);
                const int32_t cand = order[k];
                int64_t lo = b, hi = t;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (h_items[mid] < cand) lo = mid + 1; else hi = mid;
                }
                if (lo < t && h_items[lo] == cand && h_since[lo] <= g) continue;
                if (stamp[k] == r) continue;
                stamp[k] = r;
                o[2 + acc++] = (int64_t)cand;
            }
        }
        if (acc < neg_num) {
            for (int s = acc; s < neg_num; ++s) o[2 + s] = -1;
            ++failed;
        }
    }
    return failed;
}
