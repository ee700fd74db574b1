// Closed-form fold-in on gfx950 (include/sml_hip.h, "FOLD-IN"): the Gram matrix of a table and the iALS half-step, one regularised
// least-squares solve per row from its interaction set.  All arithmetic is fp64 and every rounding is named by the header, so the
// bytes depend on no launch geometry; there are no atomics and no matrix instructions.
//
// k_gram<D, T>       one workgroup per chunk of kGramChunk rows.  The rows go through LDS 64 at a time (widened to fp32, exact for
//               both element types); thread t owns a (D / 16) x (D / 16) tile of G and runs the chunk's serial adds for it.  The
//               partial of chunk c lands in scratch[c][D][D].
// k_gram_sum    adds the partials in chunk order, one thread per entry of G.
// k_als_solve<D, T>  one wavefront per row, rows walked grid-stride, kAlsWaves rows per workgroup in flight.  Lane a owns row a of
//               the lower triangle IN REGISTERS (D doubles; at d = 32 the upper half of the wave idles: serving two rows per wave
//               was not built).  alpha0 * G + reg * I is formed once per workgroup in LDS (transposed, so that lane a reads
//               consecutive words).  A member's row arrives once per wave (lane a loads y[m][a]) and is broadcast by v_readlane;
//               kAlsBatch members are requested before the first is added.
//               The factorisation is RIGHT-LOOKING: once column k is known every entry (i, j > k) takes its k-th update
//               fma(-L[i][k], L[j][k] * D[k], .), so each entry still sees its updates in k ascending order -- the order the
//               header defines -- while the D - k - 1 updates of one step are independent of each other: the dependent chain of a
//               row is D steps long, not D^2 / 2.  The forward substitution is right-looking too.  The backward substitution is
//               serial by definition (p[j] starts from p[j + 1]): L goes through a packed LDS triangle per wave so that lane j
//               holds column j, and lane j runs its own chain against the broadcast p[k].
// The kernel and the single-threaded host walks share the als_* step functions.  Contraction is OFF in the whole file: every fused
// step is an explicit fma().
#include <cmath>
#include <type_traits>
#include "sml_dev.h"
#include "sml_kernels.h"
#include "width_dispatch.h"
#include "../../include/sml_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kGramChunk = SML_GRAM_CHUNK;   // rows per partial: a constant of the definition
constexpr int kGramStage = 64;               // rows staged in LDS at a time
constexpr int kAlsWaves = 8;                 // rows in flight per workgroup: one wavefront each (d = 64: 145.7 KB of LDS, 2 waves / SIMD)
constexpr int kAlsBatch = 4;                 // members whose values a lane has in flight before the serial adds
static_assert(kGramChunk % kGramStage == 0, "a chunk is a whole number of stages");

// acc + ya * yb: the product of two widened fp32 / fp16 values is exact in fp64, so fused or not gives the same bits and only the
// add rounds
__host__ __device__ __forceinline__ double als_mac(double acc, double ya, double yb) { return fma(ya, yb, acc); }
// alpha0 * G[a][b] + (a == b ? reg : 0), one rounding
__host__ __device__ __forceinline__ double als_base(double alpha0, double g, double diag) { return fma(alpha0, g, diag); }
// t - l * v, one rounding
__host__ __device__ __forceinline__ double als_sub(double t, double l, double v) { return fma(-l, v, t); }
// correctly rounded fp64 division
__host__ __device__ __forceinline__ double als_div(double t, double d) { return t / d; }
// double -> float -> T, each to nearest even
template <class T>
__host__ __device__ __forceinline__ T als_out(double p) { return (T)(float)p; }

// ---- Gram ----------------------------------------------------------------------------------------------------------------------
template <int D, class T>
__global__ __launch_bounds__(256) void k_gram(const T* __restrict__ w, int64_t n_rows, double* __restrict__ part) {
    constexpr int TS = D / 16;
    __shared__ float s[kGramStage * D];
    const int t = threadIdx.x, ta = (t >> 4) * TS, tb = (t & 15) * TS;
    const int64_t r0 = (int64_t)blockIdx.x * kGramChunk;
    const int64_t r1 = r0 + kGramChunk < n_rows ? r0 + kGramChunk : n_rows;
    double acc[TS][TS];
#pragma unroll
    for (int x = 0; x < TS; ++x)
#pragma unroll
        for (int y = 0; y < TS; ++y) acc[x][y] = 0.0;
    for (int64_t base = r0; base < r1; base += kGramStage) {
        const int cnt = (int)(r1 - base < kGramStage ? r1 - base : kGramStage);
        __syncthreads();
        for (int e = t; e < cnt * D; e += 256) s[e] = (float)w[base * D + e];
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            double ya[TS], yb[TS];
#pragma unroll
            for (int x = 0; x < TS; ++x) { ya[x] = (double)s[i * D + ta + x]; yb[x] = (double)s[i * D + tb + x]; }
#pragma unroll
            for (int x = 0; x < TS; ++x)
#pragma unroll
                for (int y = 0; y < TS; ++y) acc[x][y] = als_mac(acc[x][y], ya[x], yb[y]);
        }
    }
    double* out = part + (int64_t)blockIdx.x * (D * D);
#pragma unroll
    for (int x = 0; x < TS; ++x)
#pragma unroll
        for (int y = 0; y < TS; ++y) out[(ta + x) * D + tb + y] = acc[x][y];
}

__global__ __launch_bounds__(256) void k_gram_sum(const double* __restrict__ part, int64_t n_chunks, int dd, double* __restrict__ gram) {
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e >= dd) return;
    double g = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) g += part[c * dd + e];
    gram[e] = g;
}

template <int D, class T>
void gram_host_walk(const T* w, int64_t n_rows, double* gram) {
    for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) {
            double g = 0.0;
            for (int64_t r0 = 0; r0 < n_rows; r0 += kGramChunk) {
                const int64_t r1 = r0 + kGramChunk < n_rows ? r0 + kGramChunk : n_rows;
                double part = 0.0;
                for (int64_t i = r0; i < r1; ++i) part = als_mac(part, (double)w[i * D + a], (double)w[i * D + b]);
                g += part;
            }
            gram[a * D + b] = g;
        }
}

// ---- row solve -----------------------------------------------------------------------------------------------------------------
#ifdef __HIP_DEVICE_COMPILE__
// lane `src` (a compile-time constant after unrolling) of a double, as a wave-uniform value
__device__ __forceinline__ double als_bcast(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
#endif

template <int D, class T>
__global__ __launch_bounds__(64 * kAlsWaves) void k_als_solve(const T* __restrict__ y, const double* __restrict__ gram, double alpha0, double reg,
                                                               const int64_t* __restrict__ set_off, const int32_t* __restrict__ set_items,
                                                               const int64_t* __restrict__ rows, int64_t n, T* __restrict__ out,
                                                               int32_t* __restrict__ status) {
#ifdef __HIP_DEVICE_COMPILE__
    constexpr int TRI = D * (D - 1) / 2;
    __shared__ double s_base[D * (D + 1) / 2];        // alpha0 * G[a][b] + (a == b ? reg : 0) for a >= b, packed by b: consecutive in a
    __shared__ double s_tri[kAlsWaves][TRI];          // per wave: L packed by rows, L[k][j] (j < k) at k (k - 1) / 2 + j
    for (int e = threadIdx.x; e < D * D; e += 64 * kAlsWaves) {
        const int b = e / D, a = e % D;
        if (a >= b) s_base[b * D - b * (b - 1) / 2 + a - b] = als_base(alpha0, gram ? gram[a * D + b] : 0.0, a == b ? reg : 0.0);
    }
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = lane < D;                       // d = 32: the upper half of the wave idles
    const int la = live ? lane : 0;                   // (an idle lane computes on lane 0's addresses and writes nothing)
    double* tri = s_tri[wv];
    for (int64_t x = (int64_t)blockIdx.x * kAlsWaves + wv; x < n; x += (int64_t)gridDim.x * kAlsWaves) {
        const int64_t row = rows ? rows[x] : x;
        const int64_t lo = set_off ? set_off[row] : 0, hi = set_off ? set_off[row + 1] : 0;
        if (hi <= lo) {                               // the exact solution of an empty set
            if (live) out[row * D + lane] = als_out<T>(0.0);
            if (lane == 0) status[x] = 1;
            continue;
        }
        double A[D];
#pragma unroll
        for (int b = 0; b < D; ++b) A[b] = s_base[b * D - b * (b - 1) / 2 + (la > b ? la - b : 0)];      // (above the diagonal: unused)
        double rhs = 0.0;
        for (int64_t m = lo; m < hi; m += kAlsBatch) {
            float v[kAlsBatch];
#pragma unroll
            for (int q = 0; q < kAlsBatch; ++q)
                if (m + q < hi) v[q] = (float)y[(int64_t)set_items[m + q] * D + la];
#pragma unroll
            for (int q = 0; q < kAlsBatch; ++q) {
                if (m + q < hi) {
                    const double ya = (double)v[q];
                    rhs += ya;
#pragma unroll
                    for (int b = 0; b < D; ++b)
                        A[b] = als_mac(A[b], ya, (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[q]), b)));
                }
            }
        }
        // LDL^T, right-looking.  Lane i keeps L[i][k] in A[k] for k < i; what it holds at and above its diagonal is never used
        bool ok = true;
        double dmine = 1.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double dk = als_bcast(A[k], k);
            ok = ok && (dk > 0.0);
            if (lane == k) dmine = dk;
            const double lk = als_div(A[k], dk);
            A[k] = lk;
            const double wk = lk * dk;                // v[k] of row `lane`
#pragma unroll
            for (int j = k + 1; j < D; ++j) A[j] = als_sub(A[j], lk, als_bcast(wk, j));
        }
        if (!ok) {                                    // (wave-uniform: dk is)
            if (lane == 0) status[x] = 2;
            continue;
        }
        // forward, right-looking: z[j] takes its updates in k ascending order
        double z = rhs;
#pragma unroll
        for (int k = 0; k < D - 1; ++k) {
            const double zk = als_bcast(z, k);
            const double zn = als_sub(z, A[k], zk);
            z = lane > k ? zn : z;
        }
        const double wj = als_div(z, dmine);
        // L through the wave's triangle: lane j then holds L[k][j] in A[k] for k > j
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < D - 1; ++k)
            if (live && lane > k) tri[lane * (lane - 1) / 2 + k] = A[k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 1; k < D; ++k)
            if (lane < k) A[k] = tri[k * (k - 1) / 2 + lane];
        // backward: lane j runs p[j] = w[j]; p[j] = fma(-L[k][j], p[k], p[j]) for k = j + 1 .. D - 1 against the broadcast p[k]
        double pv = 0.0;                              // p[lane], once known
#pragma unroll
        for (int j = D - 1; j >= 0; --j) {
            double acc = wj;
#pragma unroll
            for (int k = j + 1; k < D; ++k) acc = als_sub(acc, A[k], als_bcast(pv, k));
            if (lane == j) pv = acc;
        }
        const bool fin = !live || __builtin_isfinite(pv);
        if (__builtin_amdgcn_ballot_w64(fin) != ~0ull) {
            if (lane == 0) status[x] = 2;
            continue;
        }
        if (live) out[row * D + lane] = als_out<T>(pv);
        if (lane == 0) status[x] = 0;
    }
#endif
}

// the definition as the header writes it: left-looking, one row at a time
template <int D, class T>
int als_row_host(const T* y, const double* gram, double alpha0, double reg, const int32_t* mem, int64_t len, T* out) {
    if (len <= 0) {
        for (int s = 0; s < D; ++s) out[s] = als_out<T>(0.0);
        return 1;
    }
    static thread_local double A[D][D];
    double dg[D], rhs[D], v[D], z[D], p[D];
    for (int a = 0; a < D; ++a) {
        for (int b = 0; b <= a; ++b) {
            double acc = als_base(alpha0, gram ? gram[a * D + b] : 0.0, a == b ? reg : 0.0);
            for (int64_t m = 0; m < len; ++m) acc = als_mac(acc, (double)y[(int64_t)mem[m] * D + a], (double)y[(int64_t)mem[m] * D + b]);
            A[a][b] = acc;
        }
        double r = 0.0;
        for (int64_t m = 0; m < len; ++m) r += (double)y[(int64_t)mem[m] * D + a];
        rhs[a] = r;
    }
    for (int j = 0; j < D; ++j) {                     // A's strict lower triangle becomes L
        for (int k = 0; k < j; ++k) v[k] = A[j][k] * dg[k];
        double dj = A[j][j];
        for (int k = 0; k < j; ++k) dj = als_sub(dj, A[j][k], v[k]);
        if (!(dj > 0.0)) return 2;
        dg[j] = dj;
        for (int i = j + 1; i < D; ++i) {
            double t = A[i][j];
            for (int k = 0; k < j; ++k) t = als_sub(t, A[i][k], v[k]);
            A[i][j] = als_div(t, dj);
        }
    }
    for (int j = 0; j < D; ++j) {
        double t = rhs[j];
        for (int k = 0; k < j; ++k) t = als_sub(t, A[j][k], z[k]);
        z[j] = t;
    }
    for (int j = D - 1; j >= 0; --j) {
        double t = als_div(z[j], dg[j]);
        for (int k = j + 1; k < D; ++k) t = als_sub(t, A[k][j], p[k]);
        p[j] = t;
    }
    for (int s = 0; s < D; ++s)
        if (!std::isfinite(p[s])) return 2;
    for (int s = 0; s < D; ++s) out[s] = als_out<T>(p[s]);
    return 0;
}

}  // namespace

bool sml_als_supports(int d, int elem_bytes) {
    return with_pair<FoldInPairs>(d, elem_bytes, [](auto, auto*) {});
}

int64_t sml_gram_chunks(int64_t n_rows) { return (n_rows + kGramChunk - 1) / kGramChunk; }

hipError_t sml_launch_gram(int d, int elem_bytes, const void* w, int64_t n_rows, double* part, double* gram, hipStream_t st) {
    const int64_t chunks = sml_gram_chunks(n_rows);
    if (!with_pair<FoldInPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        k_gram<dd(), T><<<dim3((unsigned)chunks), dim3(256), 0, st>>>(static_cast<const T*>(w), n_rows, part);
    }))
        return hipErrorInvalidValue;
    k_gram_sum<<<dim3((unsigned)((d * d + 255) / 256)), dim3(256), 0, st>>>(part, chunks, d * d, gram);
    return hipGetLastError();
}

bool sml_gram_host_walk(int d, int elem_bytes, const void* w, int64_t n_rows, double* gram) {
    return with_pair<FoldInPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        gram_host_walk<dd(), T>(static_cast<const T*>(w), n_rows, gram);
    });
}

hipError_t sml_launch_als_solve(int d, int elem_bytes, const void* w_other, const double* gram, double alpha0, double reg, const int64_t* set_off,
                                const int32_t* set_items, const int64_t* rows, int64_t n, void* w_out, int max_workgroups, int32_t* status,
                                hipStream_t st) {
    int64_t blocks = (n + kAlsWaves - 1) / kAlsWaves;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : 1024;      // the kernel's own choice: 4 workgroups per CU of 256
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(64 * kAlsWaves);
    if (!with_pair<FoldInPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        k_als_solve<dd(), T><<<grid, block, 0, st>>>(static_cast<const T*>(w_other), gram, alpha0, reg, set_off, set_items, rows, n,
                                                     static_cast<T*>(w_out), status);
    }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

bool sml_als_host_walk(int d, int elem_bytes, const void* w_other, const double* gram, double alpha0, double reg, const int64_t* set_off,
                       const int32_t* set_items, const int64_t* rows, int64_t n, void* w_out, int32_t* status) {
    return with_pair<FoldInPairs>(d, elem_bytes, [&](auto dd, auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        constexpr int D = dd();
        for (int64_t x = 0; x < n; ++x) {
            const int64_t row = rows ? rows[x] : x;
            const int64_t lo = set_off ? set_off[row] : 0, hi = set_off ? set_off[row + 1] : 0;
            T tmp[D];
            const int st = als_row_host<D, T>(static_cast<const T*>(w_other), gram, alpha0, reg, set_items ? set_items + lo : nullptr, hi - lo, tmp);
            status[x] = st;
            if (st != 2)
                for (int s = 0; s < D; ++s) static_cast<T*>(w_out)[row * D + s] = tmp[s];
        }
    });
}
