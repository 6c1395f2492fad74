// Posterior-predictive (Student-t) emission densities from the frames: per component
//     l[t,k] = c_k - h_k L_k(x_t),   L >= 0 a sum of log1p terms,
// and per state the mixture  ln sum_g E[pi_g] exp(l[t,s,g])  by an online log-sum-exp, the
// [T, S G] matrix never written.  The per-component tables (mean, scaled precision factor, c,
// h) come from expfam.hip (`beer_*_predictive_table`); formulas in include/beer_hip.h and
// DESIGN.md section 26.
//
// There is no GEMM form: the diagonal case is T K D evaluations of log1p(u_d), and the
// centred frame (x - m) is different for every (frame, component) pair.  ONE kernel form for
// every covariance type, dtype and shape:
//   * a workgroup owns NF frames (one per thread) and a run of whole states whose
//     components it walks in order; the frame tile sits transposed in LDS ([D][NF + 1]: the
//     tile's global reads are one contiguous run, its LDS reads conflict-free),
//   * the components' table rows are staged in LDS a chunk at a time and read as wave-wide
//     broadcasts (every lane works on the same component),
//   * a thread scans the components of a state with a running (max, sum) pair and writes
//     M + ln S at the state's last component; a state of one component (the per-component
//     entry point) writes the value itself, untouched.
//
// log1p.  On a trained Gaussian u = kappa' (x - m)^2 / (2 b) ~ z^2 / (2 a) is ~1e-5 and h ~ a
// is 1e4..1e6: ln(1 + u) computed from the rounded 1 + u carries 6e-8 of absolute error in
// float32, 1e-3..1e-2 after the multiplication by h.  Everything here goes through log1p_t
// below (accurate relative to its ARGUMENT).  The diagonal family shares its shape
// a among the dimensions, so h sum_d log1p(u_d) = h ln prod_d (1 + u_d): kFold dimensions are
// folded into one logarithm -- not as the product, which loses the small u_d the same way, but
// as p = prod (1 + u_d) - 1 by the recurrence p <- p + u + p u: sums and products of
// non-negative numbers, 2 kFold roundings relative to p.  An outlier frame may overflow the
// product of kFold factors (each u_d alone is finite): such a group is redone dimension by
// dimension.

#include <math.h>

#include "common.h"

using namespace beer;

namespace {

constexpr int kFold = 8;      // dimensions per logarithm, diagonal covariance
constexpr int kChunk = 16;    // components staged in LDS at a time (diagonal, isotropic)
constexpr int kCB = 4;        // ... of which a thread works on this many at once
constexpr int kRows = 8;      // rows of R a thread accumulates at once (full covariance)

__device__ __forceinline__ float exp_t(float x) { return expf(x); }
__device__ __forceinline__ double exp_t(double x) { return exp(x); }
__device__ __forceinline__ float log_t(float x) { return logf(x); }
__device__ __forceinline__ double log_t(double x) { return log(x); }
__device__ __forceinline__ float div_t(float a, float b) { return __fdividef(a, b); }
__device__ __forceinline__ double div_t(double a, double b) { return a / b; }

// log1p(p), p >= 0, accurate relative to p: with w = fl(1 + p), ln(w) p / (w - 1) -- the
// rounding of 1 + p is undone by the ratio, for w - 1 is exact below 2 and the logarithm
// (the library's: one hardware log2 and a compensated product with ln 2) is accurate relative
// to its result next to 1.  A few ulp in all (the float32 quotient is the fast one), a fifth
// of the instructions of the library's log1pf (measured: DESIGN.md section 26).  p below half
// an ulp of 1 is its own logarithm; a huge or infinite w is past the point where the ratio
// matters (and inf / inf would be a NaN).
template <typename T>
__device__ __forceinline__ T log1p_t(T p) {
    const T w = (T)1 + p, lw = log_t(w);
    const T r = lw * div_t(p, w - (T)1);
    return w == (T)1 ? p : (w > (T)1e30 ? lw : r);
}
template <typename T> __device__ __forceinline__ T lowest();
template <> __device__ __forceinline__ float lowest<float>() { return -3.0e38f; }
template <> __device__ __forceinline__ double lowest<double>() { return -1.0e300; }
template <typename T> __device__ __forceinline__ bool finite_t(T x) {
    return x <= (sizeof(T) == 4 ? (T)3.4028234e38f : (T)1.79769e308);
}

__host__ __device__ inline int round_up(int n, int m) { return (n + m - 1) / m * m; }

// LDS elements of a staged chunk of components (one component with full covariance)
__host__ __device__ inline size_t chunk_elems(int cov, int D) {
    if (cov == BEER_FULL) return (size_t)D * round_up(D, kRows) + D + 2;   // R^T padded, m, c, h
    if (cov == BEER_DIAG) return (size_t)D * kChunk * 2 + 3 * kChunk;     // (m, f) pairs, c, h, lw
    return (size_t)D * kChunk + 4 * kChunk;                               // m, f, c, h, lw
}

// Running log-sum-exp of one state: S exp(M) = sum of exp(v) so far; one exponential per
// value.  M starts at the lowest finite number: the first value always replaces it.
template <typename T>
struct Lse {
    T M, S;
    __device__ __forceinline__ void reset() { M = lowest<T>(); S = 0; }
    __device__ __forceinline__ void add(T v) {
        const T d = v - M, e = exp_t(-fabs(d));
        S = d > 0 ? S * e + (T)1 : S + e;
        M = d > 0 ? v : M;
    }
    __device__ __forceinline__ T value() const { return M + log_t(S); }
};

// X [T, D], table [S G, stats_dim(COV, D)], lw [S, G] nullable -> out [T, S].
// Workgroup b: frame tile b / nsb, states [(b % nsb) spb, ... + spb).
template <typename T, int COV>
__global__ __launch_bounds__(256) void predictive_kernel(
    int64_t nframes, int D, int S, int G, int spb, int nsb, const T* __restrict__ X,
    const T* __restrict__ table, const T* __restrict__ lw, T* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NF = blockDim.x, NFP = NF + 1, tid = threadIdx.x;
    T* xs = reinterpret_cast<T*>(smem);                              // [D][NFP]
    T* cs = xs + round_up(D * NFP, 16 / (int)sizeof(T));             // the staged chunk
    const int64_t tile = blockIdx.x / nsb, t0 = tile * NF;
    const int s0 = (int)(blockIdx.x % nsb) * spb;
    const int ns = min(spb, S - s0);                                 // states of this workgroup
    const int ncols = ns * G;                                        // ... and their components
    const int W = stats_dim(COV, D);
    const int nf = (int)min((int64_t)NF, nframes - t0);
    const bool live = tid < nf;
    const int64_t t = t0 + tid;

    // the frame tile: a contiguous run of nf * D values, transposed into LDS; the rows of the
    // missing frames of the last tile are zeros (their results are not written)
    for (int idx = tid; idx < NF * D; idx += NF) {
        const int f = idx / D, d = idx - f * D;
        xs[d * NFP + f] = f < nf ? X[t0 * D + idx] : (T)0;
    }

    constexpr int CC = COV == BEER_FULL ? 1 : kChunk;
    Lse<T> lse;
    lse.reset();
    for (int col0 = 0; col0 < ncols; col0 += CC) {
        const int nc = min(CC, ncols - col0);
        const T* rows = table + ((size_t)s0 * G + col0) * W;
        __syncthreads();                   // the frame tile is there / the last chunk is done with
        if (COV == BEER_FULL) {
            // Rt[j][i] = R[i][j], i padded to a multiple of kRows with zeros; m; c, h
            const int DP = round_up(D, kRows);
            T* Rt = cs;
            T* ms = Rt + D * DP;
            for (int idx = tid; idx < D * DP; idx += NF) {
                const int j = idx / DP, i = idx - j * DP;
                Rt[idx] = i < D ? rows[D + i * D + j] : (T)0;
            }
            for (int i = tid; i < D + 2; i += NF) ms[i] = i < D ? rows[i] : rows[W - 2 + (i - D)];
        } else if (COV == BEER_DIAG) {
            // [d][c] (m, f) pairs; then c, h, lw per component; missing components repeat the
            // chunk's first (finite work, results dropped)
            T* mf = cs;
            T* ch = mf + D * kChunk * 2;
            for (int idx = tid; idx < D * kChunk; idx += NF) {
                const int d = idx / kChunk, c = idx - d * kChunk, cc = c < nc ? c : 0;
                mf[2 * idx] = rows[(size_t)cc * W + d];
                mf[2 * idx + 1] = rows[(size_t)cc * W + D + d];
            }
            for (int c = tid; c < kChunk; c += NF) {
                const int cc = c < nc ? c : 0;
                ch[c] = rows[(size_t)cc * W + W - 2];
                ch[kChunk + c] = rows[(size_t)cc * W + W - 1];
            }
        } else {
            T* ms = cs;                                             // [d][c]
            T* fs = ms + D * kChunk;                                // f, c, h per component
            for (int idx = tid; idx < D * kChunk; idx += NF) {
                const int d = idx / kChunk, c = idx - d * kChunk, cc = c < nc ? c : 0;
                ms[idx] = rows[(size_t)cc * W + d];
            }
            for (int c = tid; c < kChunk; c += NF) {
                const int cc = c < nc ? c : 0;
                fs[c] = rows[(size_t)cc * W + D];
                fs[kChunk + c] = rows[(size_t)cc * W + W - 2];
                fs[2 * kChunk + c] = rows[(size_t)cc * W + W - 1];
            }
        }
        __syncthreads();

        // one value of a component: into the state's running sum, or out
        auto emit = [&](int col, T v) {
            const int s = col / G, g = col - s * G;
            if (G == 1) {
                if (live) out[t * S + s0 + s] = lw ? v + lw[s0 + s] : v;
                return;
            }
            lse.add(lw ? v + lw[(size_t)(s0 + s) * G + g] : v);
            if (g == G - 1) {
                if (live) out[t * S + s0 + s] = lse.value();
                lse.reset();
            }
        };

        if (COV == BEER_FULL) {
            const int DP = round_up(D, kRows);
            const T* Rt = cs;
            const T* ms = Rt + D * DP;
            T q = 0;
            for (int i0 = 0; i0 < D; i0 += kRows) {
                T z[kRows];
#pragma unroll
                for (int r = 0; r < kRows; ++r) z[r] = 0;
                for (int j = i0; j < D; ++j) {                      // R is upper triangular
                    const T y = xs[j * NFP + tid] - ms[j];
                    const T* col = Rt + j * DP + i0;
#pragma unroll
                    for (int r = 0; r < kRows; ++r) z[r] = fma(col[r], y, z[r]);
                }
#pragma unroll
                for (int r = 0; r < kRows; ++r) q = fma(z[r], z[r], q);
            }
            emit(col0, fma(-ms[D + 1], log1p_t(q), ms[D]));
        } else if (COV == BEER_DIAG) {
            const T* mf = cs;
            const T* ch = mf + D * kChunk * 2;
            for (int c0 = 0; c0 < nc; c0 += kCB) {
                T L[kCB];
#pragma unroll
                for (int j = 0; j < kCB; ++j) L[j] = 0;
                for (int d0 = 0; d0 < D; d0 += kFold) {
                    const int d1 = min(d0 + kFold, D);
                    T p[kCB];
#pragma unroll
                    for (int j = 0; j < kCB; ++j) p[j] = 0;
                    for (int d = d0; d < d1; ++d) {
                        const T x = xs[d * NFP + tid];
                        const T* e = mf + (d * kChunk + c0) * 2;
#pragma unroll
                        for (int j = 0; j < kCB; ++j) {
                            const T y = x - e[2 * j];
                            const T u = (y * y) * e[2 * j + 1];
                            p[j] = fma(p[j], u, p[j] + u);
                        }
                    }
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < kCB; ++j) ok = ok && finite_t(p[j]);
                    if (ok) {
#pragma unroll
                        for (int j = 0; j < kCB; ++j) L[j] += log1p_t(p[j]);
                    } else {
                        // the product of the group overflowed: one logarithm per dimension
                        for (int d = d0; d < d1; ++d) {
                            const T x = xs[d * NFP + tid];
                            const T* e = mf + (d * kChunk + c0) * 2;
#pragma unroll
                            for (int j = 0; j < kCB; ++j) {
                                const T y = x - e[2 * j];
                                L[j] += log1p_t((y * y) * e[2 * j + 1]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < kCB; ++j)
                    if (c0 + j < nc)
                        emit(col0 + c0 + j, fma(-ch[kChunk + c0 + j], L[j], ch[c0 + j]));
            }
        } else {
            const T* ms = cs;
            const T* fs = ms + D * kChunk;
            for (int c0 = 0; c0 < nc; c0 += kCB) {
                T q[kCB];
#pragma unroll
                for (int j = 0; j < kCB; ++j) q[j] = 0;
                for (int d = 0; d < D; ++d) {
                    const T x = xs[d * NFP + tid];
                    const T* e = ms + d * kChunk + c0;
#pragma unroll
                    for (int j = 0; j < kCB; ++j) {
                        const T y = x - e[j];
                        q[j] = fma(y, y, q[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < kCB; ++j)
                    if (c0 + j < nc)
                        emit(col0 + c0 + j, fma(-fs[2 * kChunk + c0 + j],
                                                log1p_t(q[j] * fs[c0 + j]), fs[kChunk + c0 + j]));
            }
        }
    }
}

// Frames per workgroup: the most of 256, 128, 64 whose tile and chunk fit a CU's LDS.
inline int frames_per_group(int cov, int D, size_t elem, size_t* lds) {
    for (int nf = 256; nf >= 64; nf /= 2) {
        const size_t tile = (size_t)round_up(D * (nf + 1), (int)(16 / elem));
        const size_t need = (tile + chunk_elems(cov, D)) * elem;
        if (need <= (size_t)beer::kMaxDynLds) {
            *lds = need;
            return nf;
        }
    }
    return 0;
}

template <typename T>
int predictive_launch(int cov, int64_t nframes, int D, int S, int G, const void* X,
                      const void* table, const void* lw, void* out, void* stream) {
    BEER_REQUIRE(cov >= 0 && cov <= 2 && nframes >= 0 && D >= 1 && S >= 1 && G >= 1);
    BEER_REQUIRE((int64_t)S * G < (int64_t)2147483647);
    size_t lds = 0;
    const int NF = frames_per_group(cov, D, sizeof(T), &lds);
    BEER_REQUIRE(NF > 0);                      // the frame tile of this dimension does not fit LDS
    if (nframes == 0) return BEER_OK;
    BEER_REQUIRE(X && table && out);
    // whole states per workgroup: as many as fill a chunk (diagonal, isotropic; 8 components
    // per frame tile with full covariance), at least one
    const int fill = cov == BEER_FULL ? 8 : kChunk;
    const int spb = G >= fill ? 1 : (S < fill / G ? S : fill / G);
    const int nsb = (S + spb - 1) / spb;
    const int64_t tiles = (nframes + NF - 1) / NF;
    BEER_REQUIRE(tiles * nsb < (int64_t)2147483647);
    const dim3 grid((unsigned)(tiles * nsb)), block(NF);
    hipStream_t s = as_stream(stream);
#define BEER_PRED_LAUNCH(COV)                                                                   \
    do {                                                                                        \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(predictive_kernel<T, COV>),     \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, beer::kMaxDynLds); \
        hipLaunchKernelGGL((predictive_kernel<T, COV>), grid, block, lds, s, nframes, D, S, G,  \
                           spb, nsb, (const T*)X, (const T*)table, (const T*)lw, (T*)out);      \
    } while (0)
    if (cov == BEER_FULL) BEER_PRED_LAUNCH(BEER_FULL);
    else if (cov == BEER_DIAG) BEER_PRED_LAUNCH(BEER_DIAG);
    else BEER_PRED_LAUNCH(BEER_ISO);
#undef BEER_PRED_LAUNCH
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

}  // namespace

extern "C" {

int beer_predictive_llh(int dtype, int cov, int64_t T, int D, int K, const void* X,
                        const void* table, void* out, void* stream) {
    BEER_DISPATCH(dtype, predictive_launch, cov, T, D, K, 1, X, table, nullptr, out, stream);
}

int beer_mixtureset_predictive(int dtype, int cov, int64_t T, int D, int S, int G, const void* X,
                               const void* table, const void* log_mean_weights, void* log_norm,
                               void* stream) {
    BEER_DISPATCH(dtype, predictive_launch, cov, T, D, S, G, X, table, log_mean_weights, log_norm,
                  stream);
}

}  // extern "C"
