// Interaction sets on gfx950: build, union and membership of the Seen CSR (include/sml_hip.h, "interaction sets").
//
// A set over (n_user, n_item) is off int64 [n_user + 1] (off[0] = 0) and items int32 [nnz], ascending and unique inside
// each user's range -- what sml_full_rank / sml_topk_items / sml_user_rank take as Seen or held-out sets.
//
// build (rows int64 [m, n_cols] -> set):
//   k_is_split      column 0 -> user[r], column 1 -> item[r] as uint32
//   radix sort      stable LSD, 8 bits per pass (radix_sort.h, the sort of spmf.hip: tiles of 4096, ballots for
//                   stability): first by item over the passes that cover n_item - 1, then by user over the passes that
//                   cover n_user - 1.  The composite key u * n_item + i is never formed (7.4e9 at 60,000 x 123,000), and a
//                   small catalogue pays for its own bits only.
//   k_is_heads      head[r] = 1 when sorted pair r differs from pair r - 1
//   scan            pos = exclusive scan of head, pos[m] = nnz (three launches, see below)
//   k_is_emit       items[pos[r]] = item[r] for every head r
//   k_is_build_off  off[u] = pos[first sorted r with user[r] >= u]: one bisection of the sorted users per user, so a user
//                   range without pairs costs its own threads only and no lane walks a gap.
//
// union (a, b -> out), element-parallel; no lane walks a user's range:
//   k_is_probe      every b element finds its user (bisection of b_off) and bisects that user's a range: rank[j] = the
//                   first a element >= it, fresh[j] = 1 when a does not hold it
//   scan            npos = exclusive scan of fresh over nnz_b
//   k_is_merge      a element k goes to slot k + npos[first b element of its user >= it]; a fresh b element j to slot
//                   rank[j] + npos[j]; out_off[u] = a_off[u] + npos[b_off[u]].  Every slot is computed, none is counted.
//   The cost of one union is O((nnz_a + nnz_b) log) reads and nnz_a + nnz_b writes: the history is copied once per add.
//
// contains: one lane per row bisects its user's range.
//
// scan (uint32, n + 1 outputs, in place): k_is_tile_sum (per 4096), k_is_scan_sums (one workgroup walks the tile sums and
// writes the total to x[n]), k_is_tile_scan.  Integer work only; the only atomics are the LDS digit counters of the sort
// (order-free counts).  No workgroup waits on another: every dependency is a launch boundary.  The same bytes whatever the
// schedule.
#include "sml_dev.h"
#include "sml_kernels.h"
#include "radix_sort.h"
#include "../../include/sml_hip.h"

namespace {

constexpr int IS_TILE = RW_TILE;                  // 4096: rows per scan tile, as per sort tile
constexpr int IS_PER = IS_TILE / 256;             // scan: consecutive entries per lane

__global__ __launch_bounds__(256) void k_is_split(const int64_t* __restrict__ rows, int64_t m, int n_cols, uint32_t* __restrict__ user,
                                                  uint32_t* __restrict__ item) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    user[r] = (uint32_t)rows[r * n_cols];
    item[r] = (uint32_t)rows[r * n_cols + 1];
}

// the workgroup's inclusive scan of one value per lane (Hillis-Steele over LDS); buf holds the result
__device__ __forceinline__ void block_scan_256(uint32_t* buf, int tid, uint32_t v) {
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t x = tid >= off ? buf[tid - off] : 0u;
        __syncthreads();
        buf[tid] += x;
        __syncthreads();
    }
}

// ---- exclusive scan of x[0 .. n) in place, x[n] = total ----
__global__ __launch_bounds__(256) void k_is_tile_sum(const uint32_t* __restrict__ x, int64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t part[256];
    const int64_t base = (int64_t)blockIdx.x * IS_TILE;
    uint32_t acc = 0;
    for (int j = threadIdx.x; j < IS_TILE; j += 256) {
        const int64_t r = base + j;
        if (r < n) acc += x[r];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}

// sums[b] <- sum(sums[0..b)), x[n] = the total; one workgroup (n_tiles = 0: x[0] = 0)
__global__ __launch_bounds__(256) void k_is_scan_sums(uint32_t* __restrict__ sums, int64_t n_tiles, uint32_t* __restrict__ x, int64_t n) {
    __shared__ uint32_t buf[256];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0u;
    __syncthreads();
    for (int64_t b0 = 0; b0 < n_tiles; b0 += 256) {
        const int64_t b = b0 + tid;
        const uint32_t v = b < n_tiles ? sums[b] : 0u;
        block_scan_256(buf, tid, v);
        const uint32_t c = carry;
        if (b < n_tiles) sums[b] = c + buf[tid] - v;
        __syncthreads();
        if (tid == 255) carry = c + buf[255];
        __syncthreads();
    }
    if (tid == 0) x[n] = carry;
}

__global__ __launch_bounds__(256) void k_is_tile_scan(uint32_t* __restrict__ x, int64_t n, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t buf[256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * IS_TILE + (int64_t)tid * IS_PER;
    uint32_t v[IS_PER];
    uint32_t acc = 0;
#pragma unroll
    for (int j = 0; j < IS_PER; ++j) {
        v[j] = base + j < n ? x[base + j] : 0u;
        acc += v[j];
    }
    block_scan_256(buf, tid, acc);
    uint32_t run = sums[blockIdx.x] + buf[tid] - acc;
#pragma unroll
    for (int j = 0; j < IS_PER; ++j) {
        if (base + j < n) x[base + j] = run;
        run += v[j];
    }
}

// ---- bisections ----
// first index in [lo, hi) with a[index] >= x (hi when none)
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int32_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the user whose range holds element e: the last u in [0, n_user) with off[u] <= e  (e < off[n_user])
__device__ __forceinline__ int64_t owner_of(const int64_t* __restrict__ off, int64_t n_user, int64_t e) {
    int64_t lo = 0, hi = n_user;                  // invariant: off[lo] <= e < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- build ----
__global__ __launch_bounds__(256) void k_is_heads(const uint32_t* __restrict__ user, const uint32_t* __restrict__ item, int64_t m,
                                                  uint32_t* __restrict__ head) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    head[r] = (r == 0 || user[r] != user[r - 1] || item[r] != item[r - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_is_emit(const uint32_t* __restrict__ item, const uint32_t* __restrict__ pos, int64_t m,
                                                 int32_t* __restrict__ items) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const uint32_t p = pos[r];
    if (pos[r + 1] != p) items[p] = (int32_t)item[r];
}

// off[u] = pos[first r with user[r] >= u], u in [0, n_user]  (pos[m] = nnz; m = 0: pos[0] = 0)
__global__ __launch_bounds__(256) void k_is_build_off(const uint32_t* __restrict__ user, const uint32_t* __restrict__ pos, int64_t m,
                                                      int64_t n_user, int64_t* __restrict__ off) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u > n_user) return;
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)user[mid] < u) lo = mid + 1; else hi = mid;
    }
    off[u] = (int64_t)pos[lo];
}

// ---- union ----
__global__ __launch_bounds__(256) void k_is_probe(int64_t n_user, const int64_t* __restrict__ a_off, const int32_t* __restrict__ a_items,
                                                  const int64_t* __restrict__ b_off, const int32_t* __restrict__ b_items, int64_t nnz_b,
                                                  uint32_t* __restrict__ rank, uint32_t* __restrict__ fresh) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nnz_b) return;
    const int64_t u = owner_of(b_off, n_user, j);
    const int32_t x = b_items[j];
    const int64_t end = a_off[u + 1];
    const int64_t lb = lower_bound_i32(a_items, a_off[u], end, x);
    rank[j] = (uint32_t)lb;
    fresh[j] = (lb < end && a_items[lb] == x) ? 0u : 1u;
}

// lanes [0, nnz_a): a's elements; [nnz_a, nnz_a + nnz_b): b's; then n_user + 1 offsets
__global__ __launch_bounds__(256) void k_is_merge(int64_t n_user, const int64_t* __restrict__ a_off, const int32_t* __restrict__ a_items,
                                                  int64_t nnz_a, const int64_t* __restrict__ b_off, const int32_t* __restrict__ b_items,
                                                  int64_t nnz_b, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ npos,
                                                  int64_t* __restrict__ out_off, int32_t* __restrict__ out_items) {
    int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < nnz_a) {
        const int64_t u = owner_of(a_off, n_user, t);
        const int32_t x = a_items[t];
        const int64_t lb = lower_bound_i32(b_items, b_off[u], b_off[u + 1], x);
        out_items[t + (int64_t)npos[lb]] = x;
        return;
    }
    t -= nnz_a;
    if (t < nnz_b) {
        const uint32_t p = npos[t];
        if (npos[t + 1] != p) out_items[(int64_t)rank[t] + (int64_t)p] = b_items[t];
        return;
    }
    t -= nnz_b;
    if (t <= n_user) out_off[t] = a_off[t] + (int64_t)npos[b_off[t]];
}

// ---- contains ----
__global__ __launch_bounds__(256) void k_is_contains(const int64_t* __restrict__ rows, int64_t m, int n_cols, const int64_t* __restrict__ off,
                                                     const int32_t* __restrict__ items, uint8_t* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const int64_t u = rows[r * n_cols];
    const int32_t x = (int32_t)rows[r * n_cols + 1];
    const int64_t end = off[u + 1];
    const int64_t lb = lower_bound_i32(items, off[u], end, x);
    out[r] = (lb < end && items[lb] == x) ? 1 : 0;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }
inline int64_t tiles_of(int64_t n) { return (n + IS_TILE - 1) / IS_TILE; }

// radix passes that cover the values 0 .. n - 1
inline int passes_for(int64_t n) {
    int p = 0;
    for (uint64_t top = (uint64_t)(n - 1); top; top >>= 8) ++p;
    return p;
}

struct Carver {
    char* p;
    int64_t off = 0;
    explicit Carver(void* base) : p((char*)base) {}
    template <typename T> T* take(int64_t count) {
        T* q = p ? (T*)(p + off) : nullptr;
        off += ((int64_t)sizeof(T) * count + 255) & ~(int64_t)255;
        return q;
    }
};

struct BuildScratch {
    uint32_t *user[2], *item[2], *pos, *counts, *tot, *sums;
    int64_t bytes;
};
BuildScratch build_layout(void* base, int64_t m) {
    BuildScratch s;
    Carver c(base);
    const int64_t n_tiles = tiles_of(m);
    for (int b = 0; b < 2; ++b) {
        s.user[b] = c.take<uint32_t>(m);
        s.item[b] = c.take<uint32_t>(m);
    }
    s.pos = c.take<uint32_t>(m + 1);
    s.counts = c.take<uint32_t>(256 * n_tiles);
    s.tot = c.take<uint32_t>(256);
    s.sums = c.take<uint32_t>(n_tiles + 1);
    s.bytes = c.off;
    return s;
}

struct UnionScratch {
    uint32_t *rank, *npos, *sums;
    int64_t bytes;
};
UnionScratch union_layout(void* base, int64_t nnz_b) {
    UnionScratch s;
    Carver c(base);
    s.rank = c.take<uint32_t>(nnz_b);
    s.npos = c.take<uint32_t>(nnz_b + 1);
    s.sums = c.take<uint32_t>(tiles_of(nnz_b) + 1);
    s.bytes = c.off;
    return s;
}

// x[0 .. n) <- its exclusive scan, x[n] <- the total (n = 0: x[0] = 0)
void scan_in_place(uint32_t* x, int64_t n, uint32_t* sums, hipStream_t st) {
    const int64_t n_tiles = tiles_of(n);
    if (n_tiles) k_is_tile_sum<<<dim3((unsigned)n_tiles), dim3(256), 0, st>>>(x, n, sums);
    k_is_scan_sums<<<dim3(1), dim3(256), 0, st>>>(sums, n_tiles, x, n);
    if (n_tiles) k_is_tile_scan<<<dim3((unsigned)n_tiles), dim3(256), 0, st>>>(x, n, sums);
}

}  // namespace

int64_t sml_iset_build_scratch_size(int64_t m) { return build_layout(nullptr, m).bytes; }
int64_t sml_iset_union_scratch_size(int64_t nnz_b) { return union_layout(nullptr, nnz_b).bytes; }

hipError_t sml_launch_iset_build(const int64_t* rows, int64_t m, int n_cols, int64_t n_user, int64_t n_item, void* scratch,
                                 int64_t* off, int32_t* items, hipStream_t st) {
    const BuildScratch s = build_layout(scratch, m);
    int cur = 0;                                   // the buffer pair that holds the rows
    if (m) {
        k_is_split<<<dim3(blocks_of(m)), dim3(256), 0, st>>>(rows, m, n_cols, s.user[0], s.item[0]);
        for (int phase = 0; phase < 2; ++phase) {  // by item, then (stably) by user
            const int passes = passes_for(phase == 0 ? n_item : n_user);
            for (int pass = 0; pass < passes; ++pass, cur ^= 1) {
                uint32_t* const* key = phase == 0 ? s.item : s.user;
                uint32_t* const* val = phase == 0 ? s.user : s.item;
                rw_sort_pass(key[cur], val[cur], key[cur ^ 1], val[cur ^ 1], m, 8 * pass, s.counts, s.tot, st);
            }
        }
        k_is_heads<<<dim3(blocks_of(m)), dim3(256), 0, st>>>(s.user[cur], s.item[cur], m, s.pos);
    }
    scan_in_place(s.pos, m, s.sums, st);
    if (m) k_is_emit<<<dim3(blocks_of(m)), dim3(256), 0, st>>>(s.item[cur], s.pos, m, items);
    k_is_build_off<<<dim3(blocks_of(n_user + 1)), dim3(256), 0, st>>>(s.user[cur], s.pos, m, n_user, off);
    return hipGetLastError();
}

hipError_t sml_launch_iset_union(int64_t n_user, const int64_t* a_off, const int32_t* a_items, int64_t nnz_a, const int64_t* b_off,
                                 const int32_t* b_items, int64_t nnz_b, void* scratch, int64_t* out_off, int32_t* out_items,
                                 hipStream_t st) {
    const UnionScratch s = union_layout(scratch, nnz_b);
    if (nnz_b) k_is_probe<<<dim3(blocks_of(nnz_b)), dim3(256), 0, st>>>(n_user, a_off, a_items, b_off, b_items, nnz_b, s.rank, s.npos);
    scan_in_place(s.npos, nnz_b, s.sums, st);
    k_is_merge<<<dim3(blocks_of(nnz_a + nnz_b + n_user + 1)), dim3(256), 0, st>>>(n_user, a_off, a_items, nnz_a, b_off, b_items, nnz_b,
                                                                                  s.rank, s.npos, out_off, out_items);
    return hipGetLastError();
}

hipError_t sml_launch_iset_contains(const int64_t* rows, int64_t m, int n_cols, const int64_t* off, const int32_t* items, uint8_t* out,
                                    hipStream_t st) {
    if (m <= 0) return hipSuccess;
    k_is_contains<<<dim3(blocks_of(m)), dim3(256), 0, st>>>(rows, m, n_cols, off, items, out);
    return hipGetLastError();
}
