// Generic (any D, K, covariance type, fp32 / fp64) E-step kernels:
//   * per-component expected log-likelihood straight from the frames -- the
//     [T, Q] statistics tensor of the reference is never formed,
//   * per-state mixture normaliser + component responsibilities,
//   * responsibility-weighted sufficient statistics, accumulated in fp64.
// The MFMA fast path for full covariance lives in estep_mfma.hip and is
// selected by the C entry points below when its shape constraints hold.
//
// Reference restated: beer/models/normalset.py:117-123, mixture.py:70-102,
// mixtureset.py:85-112, dists/normalwishart.py:30-38,88-92 (and the
// normalgamma / isonormalgamma equivalents).

#include "common.h"
#include "estep_mfma.h"

using namespace beer;

namespace {

constexpr int kFrameTile = 64;      // frames per workgroup tile (lane = frame)
constexpr int kLlhThreads = 256;    // 4 waves, each walks a share of the comps
constexpr int kCompChunk = 64;      // components per workgroup

// ---------------------------------------------------------------------------
// Pass 1: w[t,k] = stat_scale * phi(x_t) . E[T]_k - D/2 ln2pi (+ log_weights)
// Lane = frame, the component's parameters are wave-uniform (scalar loads).
// Results are staged through LDS so that global writes are row-contiguous.
// ---------------------------------------------------------------------------
// With `fuse_G` > 0 (G divides the component chunk) the per-state logsumexp and
// the responsibilities are finished here, from the LDS tile, and the separate
// normalisation pass (one more read + write of the [T, K] buffer) is skipped.
template <typename T, int COV>
__global__ __launch_bounds__(kLlhThreads) void llh_kernel(
    int64_t nframes, int D, int K, const T* __restrict__ X, const T* __restrict__ expT,
    const T* __restrict__ logw, double stat_scale, T* __restrict__ pc_llh,
    T* __restrict__ w_out, int fuse_G, T* __restrict__ log_norm,
    double* __restrict__ llh_sum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldx = D + 1;
    T* xs = reinterpret_cast<T*>(smem);                 // [64][D+1]
    T* outs = xs + kFrameTile * ldx;                    // [64][kCompChunk+1]
    const int ldo = kCompChunk + 1;
    const int Q = stats_dim(COV, D);
    const int64_t t0 = (int64_t)blockIdx.x * kFrameTile;
    const int k0 = blockIdx.y * kCompChunk;
    const int nk = min(kCompChunk, K - k0);
    const int nt = (int)min<int64_t>(kFrameTile, nframes - t0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int idx = tid; idx < nt * D; idx += kLlhThreads)
        xs[(idx / D) * ldx + idx % D] = X[t0 * D + idx];
    __syncthreads();

    const T* x = xs + lane * ldx;
    const double base = -0.5 * (double)D * kLog2Pi;
    if (lane < nt) {
        for (int kk = wave; kk < nk; kk += kLlhThreads / 64) {
            const T* e = expT + (size_t)(k0 + kk) * Q;
            double acc = 0.0;
            if (COV == BEER_FULL) {
                const T* L = e + D;
                for (int i = 0; i < D; ++i) {
                    T s = 0;
                    const T* Li = L + i * D;
                    for (int j = 0; j < D; ++j) s += Li[j] * x[j];
                    acc += (double)x[i] * ((double)e[i] - 0.5 * (double)s);
                }
            } else if (COV == BEER_DIAG) {
                for (int i = 0; i < D; ++i) {
                    const double xi = (double)x[i];
                    acc += xi * ((double)e[i] - 0.5 * (double)e[D + i] * xi);
                }
            } else {
                double x2 = 0.0;
                for (int i = 0; i < D; ++i) {
                    const double xi = (double)x[i];
                    acc += xi * (double)e[i];
                    x2 += xi * xi;
                }
                acc -= 0.5 * (double)e[D] * x2;
            }
            const double zero = (COV == BEER_ISO) ? 0.5 * (double)D : 0.5;
            acc += -0.5 * (double)e[Q - 2] + zero * (double)e[Q - 1];
            outs[lane * ldo + kk] = (T)(stat_scale * acc + base);
        }
    }
    __syncthreads();
    if (fuse_G == 0) {
        for (int idx = tid; idx < nt * nk; idx += kLlhThreads) {
            const int t = idx / nk, kk = idx % nk;
            const T v = outs[t * ldo + kk];
            const size_t o = (size_t)(t0 + t) * K + k0 + kk;
            if (pc_llh) pc_llh[o] = v;
            if (w_out) w_out[o] = logw ? (T)(v + logw[k0 + kk]) : v;
        }
        return;
    }
    __shared__ double red[8];
    const int G = fuse_G, ngrp = nk / G, S = K / G;
    double mine = 0.0;
    for (int idx = tid; idx < nt * ngrp; idx += kLlhThreads) {
        const int t = idx / ngrp, grp = idx % ngrp;
        const T* row = outs + t * ldo + grp * G;
        const T* lw = logw ? logw + k0 + grp * G : nullptr;
        T m = row[0] + (lw ? lw[0] : (T)0);
        for (int gi = 1; gi < G; ++gi) {
            const T w = row[gi] + (lw ? lw[gi] : (T)0);
            m = w > m ? w : m;
        }
        T ln = m;
        if (m != (T)-INFINITY && m != (T)INFINITY) {
            double sum = 0.0;
            for (int gi = 0; gi < G; ++gi)
                sum += exp((double)(row[gi] + (lw ? lw[gi] : (T)0)) - (double)m);
            ln = (T)((double)m + log(sum));
        }
        const size_t o = (size_t)(t0 + t) * K + k0 + grp * G;
        for (int gi = 0; gi < G; ++gi) {
            if (pc_llh) pc_llh[o + gi] = row[gi];
            if (w_out)
                w_out[o + gi] = (T)exp((double)(row[gi] + (lw ? lw[gi] : (T)0)) - (double)ln);
        }
        if (log_norm) log_norm[(size_t)(t0 + t) * S + (k0 / G) + grp] = ln;
        mine += (double)ln;
    }
    if (llh_sum) {
        const double tot = block_sum(mine, red);
        if (threadIdx.x == 0) atomicAdd(llh_sum, tot);
    }
}

// ---------------------------------------------------------------------------
// Pass 2: per (frame, state) logsumexp over the G components, responsibilities
// in place.  One thread per (t, s).
// ---------------------------------------------------------------------------
template <typename T>
__global__ void normalise_kernel(int64_t nframes, int S, int G, T* __restrict__ w,
                                 T* __restrict__ log_norm, bool write_resps,
                                 double* __restrict__ llh_sum) {
    __shared__ double red[8];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double mine = 0.0;
    if (idx < nframes * S) {
        T* row = w + idx * G;
        T m = row[0];
        for (int g = 1; g < G; ++g) m = row[g] > m ? row[g] : m;
        T ln;
        if (m == -INFINITY || m == INFINITY) {
            ln = m;
        } else {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += exp((double)row[g] - (double)m);
            ln = (T)((double)m + log(s));
        }
        if (write_resps)
            for (int g = 0; g < G; ++g) row[g] = (T)exp((double)row[g] - (double)ln);
        if (log_norm) log_norm[idx] = ln;
        mine = (double)ln;
    }
    if (llh_sum) {
        const double tot = block_sum(mine, red);
        if (threadIdx.x == 0) atomicAdd(llh_sum, tot);
    }
}

// labels= branch of Mixture.expected_log_likelihood (mixture.py:85-87).
template <typename T>
__global__ void labels_kernel(int64_t nframes, int K, const int64_t* __restrict__ labels,
                              const T* __restrict__ pc, T* __restrict__ resps,
                              T* __restrict__ log_norm, double* __restrict__ llh_sum) {
    __shared__ double red[8];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double mine = 0.0;
    if (t < nframes) {
        const int64_t lab = labels[t];
        const T v = pc[t * K + lab];          // read before the row is overwritten
        if (resps)
            for (int k = 0; k < K; ++k) resps[t * K + k] = (T)(k == lab ? 1 : 0);
        if (log_norm) log_norm[t] = v;
        mine = (double)v;
    }
    if (llh_sum) {
        const double tot = block_sum(mine, red);
        if (threadIdx.x == 0) atomicAdd(llh_sum, tot);
    }
}

// ---------------------------------------------------------------------------
// Accumulation: acc[k, q] += sum_t r[t,k] * phi_q(x_t).  Lane = statistic q,
// each lane keeps KB components in registers; the responsibilities are
// wave-uniform scalars.  fp32 partial sums are flushed to fp64 every frame
// tile, fp64 atomics at the end of the block's frame range.
// ---------------------------------------------------------------------------
constexpr int kAccThreads = 256;
constexpr int kAccKB = 8;
constexpr int kAccTile = 64;

template <typename T, int COV>
__global__ __launch_bounds__(kAccThreads) void accumulate_kernel(
    int64_t nframes, int D, int S, int G, const T* __restrict__ X,
    const T* __restrict__ comp_resps, const T* __restrict__ state_resps,
    int64_t frames_per_block, double* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);                // [kAccTile][D]
    T* ws = xs + kAccTile * D;                          // [kAccTile][kAccKB]
    const int K = S * G, Q = stats_dim(COV, D);
    const int q = blockIdx.x * kAccThreads + threadIdx.x;
    const int k0 = blockIdx.y * kAccKB;
    const int nkb = min(kAccKB, K - k0);
    const int64_t tb = (int64_t)blockIdx.z * frames_per_block;
    const int64_t te = min(nframes, tb + frames_per_block);

    // which statistic this lane owns
    int qi = 0, qj = 0, kind;    // kind 0: x_i, 1: x_i*x_j*-.5, 2: -.5, 3: +.5 (iso .5 D), 4: -.5|x|^2
    if (q < D) { kind = 0; qi = q; }
    else if (q == Q - 2) kind = 2;
    else if (q == Q - 1) kind = 3;
    else if (q >= Q) kind = -1;
    else if (COV == BEER_FULL) { kind = 1; qi = (q - D) / D; qj = (q - D) % D; }
    else if (COV == BEER_DIAG) { kind = 1; qi = qj = q - D; }
    else kind = 4;

    double dacc[kAccKB];
#pragma unroll
    for (int b = 0; b < kAccKB; ++b) dacc[b] = 0.0;

    for (int64_t t0 = tb; t0 < te; t0 += kAccTile) {
        const int nt = (int)min<int64_t>(kAccTile, te - t0);
        __syncthreads();
        for (int idx = threadIdx.x; idx < nt * D; idx += kAccThreads) xs[idx] = X[t0 * D + idx];
        for (int idx = threadIdx.x; idx < nt * kAccKB; idx += kAccThreads) {
            const int t = idx / kAccKB, b = idx % kAccKB;
            T w = 0;
            if (b < nkb) {
                const int k = k0 + b;
                w = comp_resps ? comp_resps[(t0 + t) * K + k] : (T)1;
                if (state_resps) w *= state_resps[(t0 + t) * S + k / G];
            }
            ws[idx] = w;
        }
        __syncthreads();
        if (kind < 0) continue;
        T facc[kAccKB];
#pragma unroll
        for (int b = 0; b < kAccKB; ++b) facc[b] = 0;
        for (int t = 0; t < nt; ++t) {
            const T* x = xs + t * D;
            T phi;
            if (kind == 0) phi = x[qi];
            else if (kind == 1) phi = (T)-0.5 * (x[qi] * x[qj]);
            else if (kind == 2) phi = (T)-0.5;
            else if (kind == 3) phi = (COV == BEER_ISO) ? (T)(0.5 * D) : (T)0.5;
            else {
                T s = 0;
                for (int d = 0; d < D; ++d) s += x[d] * x[d];
                phi = (T)-0.5 * s;
            }
            const T* w = ws + t * kAccKB;
#pragma unroll
            for (int b = 0; b < kAccKB; ++b) facc[b] += w[b] * phi;
        }
#pragma unroll
        for (int b = 0; b < kAccKB; ++b) dacc[b] += (double)facc[b];
    }
    if (kind < 0) return;
#pragma unroll
    for (int b = 0; b < kAccKB; ++b)
        if (b < nkb) atomicAdd(acc + (size_t)(k0 + b) * Q + q, dacc[b]);
}

// One wave per state; lanes stride over its G components.
__global__ __launch_bounds__(64) void weights_from_acc_kernel(int S, int G, int Q,
                                                              const double* __restrict__ acc,
                                                              double* __restrict__ out) {
    const int s = blockIdx.x, lane = threadIdx.x;
    double tot = 0.0;
    for (int g = lane; g < G; g += 64) {
        const double n = -2.0 * acc[(size_t)(s * G + g) * Q + Q - 2];
        tot += n;
        if (g < G - 1) out[s * G + g] += n;
    }
    tot = wave_sum(tot);
    if (lane == 0) out[s * G + G - 1] += tot;
}

template <typename T>
__global__ void segment_sum_kernel(const int64_t* __restrict__ frame_off,
                                   const T* __restrict__ v, double* __restrict__ out) {
    __shared__ double red[8];
    const int u = blockIdx.x;
    const int64_t b = frame_off[u], e = frame_off[u + 1];
    double s = 0.0;
    for (int64_t t = b + threadIdx.x; t < e; t += blockDim.x) s += (double)v[t];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[u] += s;
}

// ---- launchers -------------------------------------------------------------

template <typename T, int COV>
int llh_launch(int64_t nframes, int D, int K, const void* X, const void* expT, const void* logw,
               double stat_scale, void* pc_llh, void* w_out, int fuse_G, void* log_norm,
               double* llh_sum, hipStream_t s) {
    const size_t lds = ((size_t)kFrameTile * (D + 1) + (size_t)kFrameTile * (kCompChunk + 1)) * sizeof(T);
    const int64_t tiles = (nframes + kFrameTile - 1) / kFrameTile;
    // gridDim.x is 2^31-1 on gfx950; frames beyond that would need a loop.
    BEER_REQUIRE(tiles < (int64_t)2147483647);
    const dim3 grid((unsigned)tiles, (unsigned)((K + kCompChunk - 1) / kCompChunk));
    hipLaunchKernelGGL((llh_kernel<T, COV>), grid, dim3(kLlhThreads), lds, s, nframes, D, K,
                       (const T*)X, (const T*)expT, (const T*)logw, stat_scale, (T*)pc_llh,
                       (T*)w_out, fuse_G, (T*)log_norm, llh_sum);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

// What beer_mixtureset_estep does with a call, decided on the host from the shape and from
// which arguments are given: refused, one of the matrix-core families (estep_mfma.h), or the
// generic kernels above.  estep_launch acts on it, beer_estep_route reports it.
struct EstepPlan {
    int rc;                 // BEER_EINVAL: the entry point refuses the call
    bool exact_mfma;        // the exact fp32 / fp64 MFMA kernel (estep_mfma.hip)
    bool use_x;             // the bf16x3 kernels (estep_bf16.hip)
    // generic: pass 1 writes the per-component values to pc_llh and, when a normalisation
    // follows (need_norm), the logits to comp_resps ...
    bool need_norm;
    bool fuse;              // ... which happens inside pass 1: it writes log_norm and llh_sum
    bool pc_in_resps;       // labels without pc_llh: labels_kernel reads them from comp_resps
};

EstepPlan estep_plan(size_t elem, bool exact, int cov, int D, int S, int G, bool pc_llh,
                     bool log_norm, bool comp_resps, bool llh_sum, bool labels, bool unscaled,
                     bool ws, size_t ws_bytes) {
    EstepPlan p = {};
    p.rc = BEER_EINVAL;
    if (!(D >= 1 && S >= 1 && G >= 1 && cov >= 0 && cov <= 2)) return p;
    if (labels && S != 1) return p;
    // The normaliser works in place on the responsibilities buffer; without one
    // (pc_llh only, or G == 1 log_norm only) pass 1 alone is enough.
    p.need_norm = (log_norm || comp_resps || llh_sum) && !labels;
    // group-aligned shapes on every arithmetic; any G on the split path when only the
    // log-normalisers are wanted (groups padded to a power of two)
    // (the exact kernels take D <= 96 / 64, the bf16x3 kernels D <= 128)
    const bool aligned = beer_mfma::supported_llh(D, S, G, elem) &&
                         ws_bytes >= beer_mfma::estep_workspace_bytes(elem, cov, D, S, G);
    const bool split_ws = elem == 4 && !exact &&
                          ws_bytes >= beer_mfma::estepx_workspace_bytes(cov, D, S, G) &&
                          beer_mfma::estepx_workspace_bytes(cov, D, S, G) > 0;
    const bool aligned_x = split_ws && beer_mfma::supported_llh_x(D, S, G);
    const bool padded = split_ws && !comp_resps && beer_mfma::supported_llh_split(D, S, G);
    p.use_x = aligned_x || padded;
    const bool mfma_ok = !labels && !pc_llh && unscaled && ws && (aligned || p.use_x) &&
                         (log_norm || comp_resps || llh_sum);
    p.use_x = mfma_ok && p.use_x;
    p.exact_mfma = mfma_ok && !p.use_x;
    // G == 1: log_norm == w; the fused pass 1 writes log_norm and no logits (the matrix-core
    // path keeps the responsibilities in registers and needs no buffer for any G).
    if (p.need_norm && !comp_resps && !mfma_ok && !(G == 1 && log_norm)) return p;
    if (labels && !(pc_llh || comp_resps)) return p;
    p.pc_in_resps = labels && !pc_llh;
    // generic kernels; the normalisation is fused when a component chunk holds
    // whole states
    p.fuse = !mfma_ok && p.need_norm && !labels && (kCompChunk % G == 0) && (comp_resps || G == 1);
    p.rc = BEER_OK;
    return p;
}

template <typename T>
int estep_launch(int cov, int64_t nframes, int D, int S, int G, const void* X, const void* expT,
                 const void* logw, const int64_t* labels, double stat_scale, void* pc_llh,
                 void* log_norm, void* comp_resps, double* llh_sum, void* ws, size_t ws_bytes,
                 void* stream, bool exact) {
    BEER_REQUIRE(nframes >= 0 && X && expT);
    const EstepPlan p = estep_plan(sizeof(T), exact, cov, D, S, G, pc_llh, log_norm, comp_resps,
                                   llh_sum, labels, stat_scale == 1.0, ws, ws_bytes);
    if (p.rc != BEER_OK || nframes == 0) return p.rc;
    hipStream_t s = as_stream(stream);
    // gfx950 matrix-core path: GEMM + (grouped) softmax fused, one kernel
    if (p.use_x)
        return beer_mfma::estep_bf16x3(cov, nframes, D, S, G, (const float*)X, (const float*)expT,
                                       (const float*)logw, (float*)comp_resps, (float*)log_norm,
                                       llh_sum, ws, ws_bytes, s);
    if (p.exact_mfma)
        return sizeof(T) == 4
                   ? beer_mfma::estep_f32(cov, nframes, D, S, G, (const float*)X,
                                          (const float*)expT, (const float*)logw,
                                          (float*)comp_resps, (float*)log_norm, llh_sum, ws,
                                          ws_bytes, s)
                   : beer_mfma::estep_f64(cov, nframes, D, S, G, (const double*)X,
                                          (const double*)expT, (const double*)logw,
                                          (double*)comp_resps, (double*)log_norm, llh_sum, ws,
                                          ws_bytes, s);
    const int K = S * G;
    void* pc = p.pc_in_resps ? comp_resps : pc_llh;
    static_assert(BEER_FULL == 0 && BEER_DIAG == 1 && BEER_ISO == 2, "pass1 is indexed by cov");
    constexpr decltype(&llh_launch<T, BEER_FULL>) pass1[] = {
        llh_launch<T, BEER_FULL>, llh_launch<T, BEER_DIAG>, llh_launch<T, BEER_ISO>};
    const int rc = pass1[cov](nframes, D, K, X, expT, logw, stat_scale, pc,
                              p.need_norm ? comp_resps : nullptr, p.fuse ? G : 0,
                              p.fuse ? log_norm : nullptr, p.fuse ? llh_sum : nullptr, s);
    if (rc != BEER_OK) return rc;
    if (labels) {
        // when pc aliases comp_resps the kernel reads pc[t,label] before it
        // overwrites the row: one thread owns the whole row.
        hipLaunchKernelGGL(labels_kernel<T>, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0,
                           s, nframes, K, labels, (const T*)pc, (T*)comp_resps, (T*)log_norm,
                           llh_sum);
        BEER_LAUNCH_CHECK();
    } else if (p.need_norm && !p.fuse) {
        // (a normalisation that is not fused has a responsibilities buffer: estep_plan)
        const int64_t n = nframes * S;
        hipLaunchKernelGGL(normalise_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                           nframes, S, G, (T*)comp_resps, (T*)log_norm, true, llh_sum);
        BEER_LAUNCH_CHECK();
    }
    return BEER_OK;
}

template <typename T, int COV>
int acc_launch(int64_t nframes, int D, int S, int G, const void* X, const void* cr,
               const void* sr, double* acc, hipStream_t s) {
    const int K = S * G, Q = stats_dim(COV, D);
    const int gx = (Q + kAccThreads - 1) / kAccThreads, gy = (K + kAccKB - 1) / kAccKB;
    // aim for ~4 workgroups per CU, at least 512 frames per workgroup -- one frame tile (64) for
    // inputs so small that the launch is a handful of workgroups either way: a lane walks its
    // workgroup's frames one by one, and the notebook-sized mixture (1000 frames, 8 x 6 statistics:
    // BASELINE config 1) spent 66 of its iteration's 142 us in two workgroups of 512 frames
    int64_t gz = (256LL * 4 + (int64_t)gx * gy - 1) / ((int64_t)gx * gy);
    const int64_t min_frames = nframes >= 65536 ? 512 : kAccTile;
    const int64_t max_z = (nframes + min_frames - 1) / min_frames;
    if (gz > max_z) gz = max_z;
    if (gz < 1) gz = 1;
    if (gz > 65535) gz = 65535;
    const beer_mfma::FrameSplit z = beer_mfma::frame_split(nframes, gz, kAccTile);
    const size_t lds = ((size_t)kAccTile * D + (size_t)kAccTile * kAccKB) * sizeof(T);
    hipLaunchKernelGGL((accumulate_kernel<T, COV>), dim3(gx, gy, (unsigned)z.gz), dim3(kAccThreads),
                       lds, s, nframes, D, S, G, (const T*)X, (const T*)cr, (const T*)sr, z.fpb, acc);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

// What beer_normal_accumulate does with a call, in this order of precedence.
struct AccPlan {
    int rc;                 // BEER_EINVAL: the entry point refuses the call
    bool diag;              // acc_diag.hip: the float32 weights split inside the kernel
    bool exact_mfma;        // the exact fp32 / fp64 MFMA kernel (estep_mfma.hip)
};                          // neither: accumulate_kernel above

AccPlan accumulate_plan(size_t elem, bool exact, int cov, int64_t nframes, int D, int S, int G,
                        bool cr, bool sr, bool ws, size_t ws_bytes) {
    AccPlan p = {};
    p.rc = BEER_EINVAL;
    if (!(nframes >= 0 && D >= 1 && S >= 1 && G >= 1 && cov >= 0 && cov <= 2)) return p;
    p.rc = BEER_OK;
    // (float32 responsibilities [T, K] in memory: the exact fp32 / fp64 MFMA kernels;
    // the bf16x3 accumulation takes packed tiles -- beer_pack_resps +
    // beer_normal_accumulate_packed -- whose size depends on T)
    // ... except diagonal / isotropic Gaussians without state posteriors (a set of single
    // Gaussians under an HMM: the prior of a VAE): few statistics per Gaussian, the float32
    // weights are split inside the kernel (acc_diag.hip)
    p.diag = elem == 4 && !exact && cr && !sr &&
             beer_mfma::supported_acc_diag(cov, nframes, D, S * G);
    p.exact_mfma = !p.diag && cr && ws && beer_mfma::supported_acc(D, S * G, elem) &&
                   ws_bytes >= beer_mfma::acc_workspace_bytes(cov, D, S * G, elem);
    return p;
}

template <typename T>
int accumulate_launch(int cov, int64_t nframes, int D, int S, int G, const void* X,
                      const void* cr, const void* sr, double* acc, void* ws, size_t ws_bytes,
                      void* stream, bool exact) {
    const AccPlan p = accumulate_plan(sizeof(T), exact, cov, nframes, D, S, G, cr, sr, ws, ws_bytes);
    BEER_REQUIRE(p.rc == BEER_OK && X && acc);
    if (nframes == 0) return BEER_OK;
    hipStream_t s = as_stream(stream);
    if (p.diag)
        return beer_mfma::acc_diag_bf16x3(cov, nframes, D, S * G, (const float*)X,
                                          (const float*)cr, acc, ws, ws_bytes, s);
    if (p.exact_mfma)
        return sizeof(T) == 4
                   ? beer_mfma::acc_f32(cov, nframes, D, S, G, (const float*)X, (const float*)cr,
                                        (const float*)sr, acc, ws, ws_bytes, s)
                   : beer_mfma::acc_f64(cov, nframes, D, S, G, (const double*)X,
                                        (const double*)cr, (const double*)sr, acc, ws, ws_bytes,
                                        s);
    constexpr decltype(&acc_launch<T, BEER_FULL>) generic[] = {
        acc_launch<T, BEER_FULL>, acc_launch<T, BEER_DIAG>, acc_launch<T, BEER_ISO>};
    return generic[cov](nframes, D, S, G, X, cr, sr, acc, s);
}

template <typename T>
int segment_sum_launch(int32_t nutt, const int64_t* frame_off, const void* v, double* out,
                       void* stream) {
    BEER_REQUIRE(nutt >= 0);
    if (nutt == 0) return BEER_OK;
    hipLaunchKernelGGL(segment_sum_kernel<T>, dim3(nutt), dim3(256), 0, as_stream(stream),
                       frame_off, (const T*)v, out);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

// What the packed (one mixture, or `set`) and the image entry points refuse, from the shape,
// the arguments given and the workspace (0 bytes: none): they call it with what they were
// handed, beer_estep_route with its mask.  The rest is estep_bf16x3's own (llhx_form).
int estepx_refusal(int entry, bool set, int cov, int D, int S, int G, unsigned args,
                   size_t ws_bytes) {
    const bool packed = entry == BEER_ESTEP_PACKED, resps = args & BEER_ARG_RESPS;
    BEER_REQUIRE(D >= 1 && S >= 1 && G >= 1 && cov >= 0 && cov <= 2);
    BEER_REQUIRE(!(args & (BEER_ARG_PC_LLH | BEER_ARG_LABELS | BEER_ARG_SCALED)));
    // packed: responsibilities; one mixture needs its weights, a set a shape the packed
    // accumulation takes too.  Image: log-normalisers only
    if (packed)
        BEER_REQUIRE(resps && (set ? beer_mixtureset_packed_supported(cov, D, S, G)
                                   : S == 1 && (args & BEER_ARG_LOG_WEIGHTS)));
    else
        BEER_REQUIRE((args & BEER_ARG_LOG_NORM) && !resps);
    return beer_mfma::llhx_form(cov, D, S, G, packed, packed, !packed, ws_bytes).rc;
}

// ... and what they do once their own pointer checks are through
int estepx_entry(int entry, bool set, int cov, int64_t T, int D, int S, int G, const float* X,
                 const float* exp_stats, const float* logw, const void* image, float* log_norm,
                 void* resps, double* llh_sum, void* ws, size_t ws_bytes, void* stream) {
    const unsigned args = (log_norm ? BEER_ARG_LOG_NORM : 0u) | (resps ? BEER_ARG_RESPS : 0u) |
                          (llh_sum ? BEER_ARG_LLH_SUM : 0u) | (logw ? BEER_ARG_LOG_WEIGHTS : 0u);
    const int rc = estepx_refusal(entry, set, cov, D, S, G, args, ws ? ws_bytes : 0);
    if (rc != BEER_OK || T == 0) return rc;
    return beer_mfma::estep_bf16x3(cov, T, D, S, G, X, exp_stats, logw, (float*)resps, log_norm,
                                   llh_sum, ws, ws_bytes, as_stream(stream),
                                   entry == BEER_ESTEP_PACKED, image);
}

// What the packed accumulation entry points (one mixture of G components, or a `set`) and the
// fused one refuse, from the shape and the workspace (0 bytes: none): they call it with what
// they were handed, beer_accumulate_route with its arguments.
int accx_refusal(bool set, int cov, int64_t T, int D, int S, int G, size_t ws_bytes) {
    BEER_REQUIRE(T >= 0 && D >= 1 && S >= 1 && G >= 1 && cov >= 0 && cov <= 2);
    BEER_REQUIRE(!set || beer_mixtureset_packed_supported(cov, D, S, G));
    BEER_REQUIRE(beer_mfma::accx_form(cov, D, S * G, S, G, set).rc == BEER_OK);
    const size_t need = beer_mfma::accx_layout(cov, T, D, S * G, S, G, set).bytes;
    BEER_REQUIRE(need > 0 && ws_bytes >= need);
    return BEER_OK;
}
int accf_refusal(int cov, int64_t T, int D, int S, int G, size_t ws_bytes) {
    BEER_REQUIRE(T >= 0 && D >= 1 && S >= 1 && G >= 1 && cov >= 0 && cov <= 2);
    BEER_REQUIRE(beer_mfma::accf_form(cov, D, S, G, false).rc == BEER_OK);
    const size_t need = beer_mfma::accf_layout(cov, D, S, G).bytes;
    BEER_REQUIRE(need > 0 && ws_bytes >= need);
    return BEER_OK;
}

}  // namespace

extern "C" {

int beer_mixtureset_estep(int dtype, int cov, int64_t T, int D, int S, int G, const void* X,
                          const void* exp_stats, const void* log_weights,
                          const int64_t* labels, double stat_scale, void* pc_llh,
                          void* log_norm, void* comp_resps, double* llh_sum, void* workspace,
                          size_t workspace_bytes, void* stream) {
    const bool exact = (dtype & BEER_EXACT) != 0;
    BEER_DISPATCH(dtype & ~BEER_EXACT, estep_launch, cov, T, D, S, G, X, exp_stats, log_weights,
                  labels, stat_scale, pc_llh, log_norm, comp_resps, llh_sum, workspace,
                  workspace_bytes, stream, exact);
}

int beer_estep_route(int entry, int dtype, int cov, int D, int S, int G, unsigned args,
                     size_t workspace_bytes) {
    const bool exact = (dtype & BEER_EXACT) != 0;
    dtype &= ~BEER_EXACT;
    BEER_REQUIRE(dtype == BEER_F32 || dtype == BEER_F64);
    const bool resps = args & BEER_ARG_RESPS, labels = args & BEER_ARG_LABELS;
    bool packed = false;
    if (entry == BEER_ESTEP_PLAIN) {
        const EstepPlan p = estep_plan(dtype == BEER_F64 ? 8 : 4, exact, cov, D, S, G,
                                       args & BEER_ARG_PC_LLH, args & BEER_ARG_LOG_NORM, resps,
                                       args & BEER_ARG_LLH_SUM, labels, !(args & BEER_ARG_SCALED),
                                       workspace_bytes > 0, workspace_bytes);
        if (p.rc != BEER_OK) return p.rc;
        if (p.exact_mfma) {
            const beer_mfma::LlhForm f = beer_mfma::llh_form(S, G);
            return (dtype == BEER_F64 ? BEER_ESTEP_EXACT_F64 : BEER_ESTEP_EXACT_F32) | f.NT |
                   f.GQ << 5 | f.jw << 8 | (f.nchunks > 0xfff ? 0xfff : f.nchunks) << 16;
        }
        if (!p.use_x)
            return BEER_ESTEP_GENERIC | (labels ? BEER_ESTEP_GENERIC_LABELS
                                         : !p.need_norm ? BEER_ESTEP_GENERIC_PASS1
                                         : p.fuse ? BEER_ESTEP_GENERIC_FUSED
                                                  : BEER_ESTEP_GENERIC_NORMALISE);
    } else if (entry == BEER_ESTEP_PACKED || entry == BEER_ESTEP_IMAGE) {
        // the float32 entry points of the bf16x3 kernels; packed: beer_mixture_estep_packed for
        // one mixture (K = G), beer_mixtureset_estep_packed for a set
        BEER_REQUIRE(dtype == BEER_F32 && !exact);
        BEER_REQUIRE(estepx_refusal(entry, S != 1, cov, D, S, G, args, workspace_bytes) == BEER_OK);
        packed = entry == BEER_ESTEP_PACKED;
    } else {
        return BEER_EINVAL;
    }
    const beer_mfma::LlhxForm x = beer_mfma::llhx_form(cov, D, S, G, resps, packed,
                                                       entry == BEER_ESTEP_IMAGE, workspace_bytes);
    if (x.rc != BEER_OK) return x.rc;
    const int nchunks = (x.nchunks > 0xfff ? 0xfff : x.nchunks) << 16;
    if (x.lnfi) return BEER_ESTEP_LNFI | x.NT | x.nku << 5 | x.lnfi_g << 8 | nchunks;
    return BEER_ESTEP_LLHX | x.NT | x.GQ << 5 | (x.packed ? BEER_ESTEP_X_PACKED : 0) |
           (x.lno ? BEER_ESTEP_X_LNO : 0) | (x.img ? BEER_ESTEP_X_IMG : 0) |
           (x.bl ? BEER_ESTEP_X_BL : 0) | (x.narrow ? BEER_ESTEP_X_NARROW : 0) |
           (x.lane_major ? BEER_ESTEP_X_LANE_MAJOR : 0) | (x.Gp != G ? BEER_ESTEP_X_PADDED : 0) |
           (x.xt ? BEER_ESTEP_X_XT : 0) | nchunks;
}

size_t beer_estep_workspace_bytes(int dtype, int cov, int D, int S, int G) {
    if (cov < 0 || cov > 2) return 0;
    dtype &= ~BEER_EXACT;
    const size_t exact = beer_mfma::estep_workspace_bytes(dtype == BEER_F64 ? 8 : 4, cov, D, S, G);
    if (dtype == BEER_F64) return exact;
    const size_t split = beer_mfma::estepx_workspace_bytes(cov, D, S, G);
    return exact > split ? exact : split;                 // either fp32 mode fits
}

size_t beer_accumulate_workspace_bytes(int dtype, int cov, int D, int S, int G) {
    if (cov < 0 || cov > 2) return 0;
    return beer_mfma::acc_workspace_bytes(cov, D, S * G, (dtype & ~BEER_EXACT) == BEER_F64 ? 8 : 4);
}

size_t beer_accumulate_frames_workspace_bytes(int dtype, int cov, int64_t T, int D, int S, int G) {
    const size_t base = beer_accumulate_workspace_bytes(dtype, cov, D, S, G);
    if (dtype != BEER_F32 || T < 0 || S < 1 || G < 1) return base;
    const size_t rows = beer_mfma::acc_diag_workspace_bytes(cov, T, D, S * G);
    return rows > base ? rows : base;
}

int beer_normal_accumulate(int dtype, int cov, int64_t T, int D, int S, int G, const void* X,
                           const void* comp_resps, const void* state_resps, double* acc,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const bool exact = (dtype & BEER_EXACT) != 0;
    BEER_DISPATCH(dtype & ~BEER_EXACT, accumulate_launch, cov, T, D, S, G, X, comp_resps,
                  state_resps, acc, workspace, workspace_bytes, stream, exact);
}

int beer_accumulate_route(int entry, int dtype, int cov, int64_t T, int D, int S, int G,
                          unsigned args, size_t workspace_bytes) {
    const bool exact = (dtype & BEER_EXACT) != 0;
    dtype &= ~BEER_EXACT;
    BEER_REQUIRE(dtype == BEER_F32 || dtype == BEER_F64);
    const bool sets = args & BEER_ARG_STATE_RESPS;
    if (entry == BEER_ACC_PLAIN) {
        const size_t elem = dtype == BEER_F64 ? 8 : 4;
        const AccPlan p = accumulate_plan(elem, exact, cov, T, D, S, G, args & BEER_ARG_RESPS, sets,
                                          workspace_bytes > 0, workspace_bytes);
        if (p.rc != BEER_OK) return p.rc;
        if (p.diag) {
            const beer_mfma::AccdForm f = beer_mfma::accd_form(cov, T, D, S * G, workspace_bytes);
            return f.rc != BEER_OK ? f.rc
                                   : BEER_ACC_DIAG | f.NJ2 | f.NC << 4 |
                                         (f.partial ? BEER_ACC_D_PARTIAL : 0);
        }
        if (p.exact_mfma) {
            const beer_mfma::AccForm f = beer_mfma::acc_form(elem, cov, D, S * G, sets);
            return f.rc != BEER_OK ? f.rc
                                   : (elem == 8 ? BEER_ACC_EXACT_F64 : BEER_ACC_EXACT_F32) | f.NQ |
                                         (f.has_sr ? BEER_ACC_SR : 0);
        }
        return BEER_ACC_GENERIC;
    }
    // the float32 entry points of the bf16x3 kernels
    BEER_REQUIRE(dtype == BEER_F32 && !exact);
    if (entry == BEER_ACC_PACKED) {
        // beer_normal_accumulate_packed (K = S G), beer_mixtureset_accumulate_packed with
        // state posteriors; both need the packed tiles
        BEER_REQUIRE(args & BEER_ARG_RESPS);
        BEER_REQUIRE(accx_refusal(sets, cov, T, D, S, G, workspace_bytes) == BEER_OK);
        const beer_mfma::AccxForm f = beer_mfma::accx_form(cov, D, S * G, S, G, sets);
        return BEER_ACC_ACCX | f.NQ | (f.sr ? BEER_ACC_SR : 0) | (f.sx ? BEER_ACC_X_SX : 0) |
               (f.xt_reused ? BEER_ACC_X_XT_REUSED : 0);
    }
    if (entry == BEER_ACC_FUSED) {
        BEER_REQUIRE(accf_refusal(cov, T, D, S, G, workspace_bytes) == BEER_OK);
        const beer_mfma::AccfForm f = beer_mfma::accf_form(cov, D, S, G, args & BEER_ARG_IMAGE);
        if (f.use_image)
            return BEER_ACC_ACCF | BEER_ACC_F_IMAGE | f.NKU << 4 | f.ns_img << 16 | f.waves << 21;
        return BEER_ACC_ACCF | f.NQT | (f.blk ? BEER_ACC_F_BLK : 0) | f.waves << 21;
    }
    return BEER_EINVAL;
}

int beer_mixture_estep_packed(int cov, int64_t T, int D, int K, const float* X,
                              const float* exp_stats, const float* log_weights, float* log_norm,
                              void* packed_resps, double* llh_sum, void* workspace,
                              size_t workspace_bytes, void* stream) {
    BEER_REQUIRE(T >= 0 && X && exp_stats);
    return estepx_entry(BEER_ESTEP_PACKED, false, cov, T, D, 1, K, X, exp_stats, log_weights, nullptr,
                        log_norm, packed_resps, llh_sum, workspace, workspace_bytes, stream);
}

int beer_normal_accumulate_packed(int cov, int64_t T, int D, int K, const float* X,
                                  const void* packed_resps, double* acc, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    BEER_REQUIRE(X && packed_resps && acc && workspace);
    BEER_REQUIRE(accx_refusal(false, cov, T, D, 1, K, workspace_bytes) == BEER_OK);
    if (T == 0) return BEER_OK;
    return beer_mfma::acc_bf16x3_packed(cov, T, D, K, X, packed_resps, acc, workspace,
                                        workspace_bytes, as_stream(stream));
}

int beer_mixtureset_packed_supported(int cov, int D, int S, int G) {
    return cov >= 0 && cov <= 2 && D >= 1 && D <= beer_mfma::kMaxDimX && S >= 1 && G >= 1 &&
           beer_mfma::supported_llh_packed_sets(cov, D, S, G) &&
           beer_mfma::supported_acc_sets(cov, D, S, G);
}

size_t beer_mixtureset_accumulate_packed_workspace_bytes(int cov, int64_t T, int D, int S, int G) {
    if (T < 0 || !beer_mixtureset_packed_supported(cov, D, S, G)) return 0;
    return beer_mfma::accxs_workspace_bytes(cov, T, D, S, G);
}

int beer_mixtureset_estep_packed(int cov, int64_t T, int D, int S, int G, const float* X,
                                 const float* exp_stats, const float* log_weights,
                                 float* log_norm, void* packed_resps, double* llh_sum,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    BEER_REQUIRE(T >= 0 && X && exp_stats);
    return estepx_entry(BEER_ESTEP_PACKED, true, cov, T, D, S, G, X, exp_stats, log_weights, nullptr,
                        log_norm, packed_resps, llh_sum, workspace, workspace_bytes, stream);
}

int beer_mixtureset_accumulate_packed(int cov, int64_t T, int D, int S, int G, const float* X,
                                      const void* packed_resps, const float* state_resps,
                                      double* acc, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    BEER_REQUIRE(X && packed_resps && state_resps && acc && workspace);
    BEER_REQUIRE(accx_refusal(true, cov, T, D, S, G, workspace_bytes) == BEER_OK);
    if (T == 0) return BEER_OK;
    return beer_mfma::acc_bf16x3_packed(cov, T, D, S * G, X, packed_resps, acc, workspace,
                                        workspace_bytes, as_stream(stream), S, G, state_resps);
}

size_t beer_accumulate_fused_workspace_bytes(int cov, int D, int S, int G) {
    if (cov < 0 || cov > 2 || D < 1 || S < 1 || G < 1) return 0;
    return beer_mfma::accf_workspace_bytes(cov, D, S, G);
}

int beer_mixtureset_lognorm_image(int cov, int64_t T, int D, int S, int G, const float* X,
                                  const float* exp_stats, const float* log_weights,
                                  const void* frame_image, float* log_norm, double* llh_sum,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    // (an empty batch of a shape the image kernels do not take is refused like a full one)
    BEER_REQUIRE(T >= 0 && frame_image && (T == 0 || (X && exp_stats)));
    return estepx_entry(BEER_ESTEP_IMAGE, true, cov, T, D, S, G, X, exp_stats, log_weights,
                        frame_image, log_norm, nullptr, llh_sum, workspace, workspace_bytes, stream);
}

size_t beer_frame_image_bytes(int cov, int64_t T, int D) {
    if (cov < 0 || cov > 2 || T < 0 || D < 1) return 0;
    return beer_mfma::frame_image_bytes(cov, T, D);
}

int beer_frame_image(int cov, int64_t T, int D, const float* X, void* image, size_t image_bytes,
                     void* stream) {
    BEER_REQUIRE(cov >= 0 && cov <= 2 && T >= 0 && D >= 1);
    const size_t need = beer_mfma::frame_image_bytes(cov, T, D);
    BEER_REQUIRE(need > 0 && image && image_bytes >= need && (T == 0 || X));
    return beer_mfma::frame_image(cov, T, D, X, image, as_stream(stream));
}

int beer_mixtureset_accumulate_fused(int cov, int64_t T, int D, int S, int G, const float* X,
                                     const float* exp_stats, const float* log_weights,
                                     const float* log_norm, const float* state_resps,
                                     const void* frame_image, double* acc, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    BEER_REQUIRE(accf_refusal(cov, T, D, S, G, workspace ? workspace_bytes : 0) == BEER_OK);
    if (T == 0) return BEER_OK;
    BEER_REQUIRE(X && exp_stats && log_norm && acc);
    return beer_mfma::acc_fused_bf16x3(cov, T, D, S, G, X, exp_stats, log_weights, log_norm,
                                       state_resps, frame_image, acc, workspace, workspace_bytes,
                                       as_stream(stream));
}

size_t beer_packed_resps_bytes(int64_t T, int D, int K) {
    return T < 0 || D < 1 || D > beer_mfma::kMaxDimX || K < 1 ? 0 : beer_mfma::packed_resps_bytes(T, D, K);
}

size_t beer_accumulate_packed_workspace_bytes(int cov, int64_t T, int D, int K) {
    if (cov < 0 || cov > 2 || T < 0 || D < 1 || K < 1) return 0;
    return beer_mfma::accx_workspace_bytes(cov, T, D, K);
}

int beer_pack_resps(int64_t T, int D, int S, int G, const float* X, const float* comp_resps,
                    const float* state_resps, void* packed_resps, void* stream) {
    BEER_REQUIRE(T >= 0 && D >= 1 && D <= beer_mfma::kMaxDimX && S >= 1 && G >= 1 && (S * G) % 4 == 0);
    BEER_REQUIRE(T == 0 || (X && comp_resps && packed_resps));
    return beer_mfma::pack_resps(T, D, S, G, X, comp_resps, state_resps, packed_resps,
                                 as_stream(stream));
}

int beer_unpack_resps(int64_t T, int K, const void* packed_resps, float* resps, void* stream) {
    BEER_REQUIRE(T >= 0 && K >= 1 && (T == 0 || (packed_resps && resps)));
    return beer_mfma::unpack_resps(T, K, packed_resps, resps, as_stream(stream));
}

int beer_weights_from_acc(int S, int G, int Q, const double* acc, double* out, void* stream) {
    BEER_REQUIRE(S >= 0 && G >= 1 && Q >= 2 && acc && out);
    if (S == 0) return BEER_OK;
    hipLaunchKernelGGL(weights_from_acc_kernel, dim3(S), dim3(64), 0,
                       as_stream(stream), S, G, Q, acc, out);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

int beer_segment_sum(int dtype, int32_t nutt, const int64_t* frame_off, const void* v,
                     double* out, void* stream) {
    BEER_DISPATCH(dtype, segment_sum_launch, nutt, frame_off, v, out, stream);
}

}  // extern "C"
