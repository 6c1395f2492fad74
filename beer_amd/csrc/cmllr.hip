// Speaker-adaptive affine feature transforms (CMLLR / fMLLR): the statistics of the row
// update and the transform itself.  Definitions in include/beer_hip.h and DESIGN.md
// section 28.
//
//   frame_params   [omega | nu | c][t] += sum_k r_tk [E[lambda]_k | E[lambda mu]_k | 1]
//                  a [T, K] x [K, P + D + 1] product in float64 on v_mfma_f64_16x16x4_f64:
//                  a workgroup owns 64 frames (a wave 16) and every column tile, the
//                  responsibilities (component x state, multiplied while they are staged)
//                  and the table rows go through LDS 32 components at a time.
//   accumulate     G_{s,i} = sum_t omega_ti xi_t xi_t^T,  k_{s,i} = sum_t nu_ti xi_t,
//                  beta_s = sum_t c_t,  xi = [x; 1], E = D + 1 <= 64 entries = NT <= 4
//                  tiles of 16.  A workgroup owns an ITEM of the host-built table (a speaker
//                  and a chunk of that speaker's frames, listed as runs inside utterances)
//                  and, blockIdx.y, either eight dimensions i (a wave two of them: the
//                  NT (NT + 1) / 2 lower-triangle tiles of each in registers) or the linear
//                  statistics (wave w: rows 16 w .. of [nu | c]^T xi -- beta is its entry
//                  (D, D), where xi_D = 1 meets c).  xi is staged in LDS as float64, 64
//                  frames at a time; one MFMA step sums four frames:
//                      A[row][frame] = omega_ti xi_t[16 ti + row],  B[frame][col] = xi_t[16 tj + col]
//                  (lane l: i16 = l & 15 is the row of A and the column of B, g = l >> 4 the
//                  frame; C row g + 4 r, column i16 -- the mapping at the head of
//                  estep_mfma.hip).  Partial results go to the workspace, one slab per item;
//                  a second kernel adds the slabs of a speaker in chunk order into G, k and
//                  beta.  No atomics: two runs give the same bits.
//   apply          y_t = A_s x_t + b_s in float64, one thread per output value; the
//                  utterance of a frame by bisection of the offsets.
//
// Frames that the table names outside [0, T) are skipped, not read: the table is checked on
// the host (its structure, the speaker and utterance indices), the frame numbers come from
// the device's offsets and are checked where they are used.

#include <vector>

#include "common.h"
#include "estep_tiles.h"

using namespace beer;

namespace {

using beer_mfma::f64x4;
using M64 = beer_mfma::Mma<double>;

constexpr int kMaxDim = BEER_CMLLR_MAX_DIM;   // D + 1 <= 64: four tiles of 16
constexpr int kTileFrames = 64;               // frames staged in LDS at a time
constexpr int kDimsPerWave = 2;               // Gram matrices a wave keeps in registers
constexpr int kDimsPerBlock = 4 * kDimsPerWave;
constexpr int kDefaultChunk = 1024;           // frames of an item (chunk_frames = 0)
constexpr int kStageComps = 32;               // components staged at a time (frame_params)

// the table: header, then spk_ptr [n_spk + 1], item_spk [n_items], item_ptr [n_items + 1],
// seg [n_segs][3] = (utterance, first frame inside it, frames)
struct Table {
    int n_items, n_segs, n_spk, nutt;
    const int32_t *spk_ptr, *item_spk, *item_ptr, *seg;
};
__host__ __device__ inline size_t table_ints(int n_spk, int n_items, int n_segs) {
    return 4 + ((size_t)n_spk + 1) + (size_t)n_items + ((size_t)n_items + 1) + 3 * (size_t)n_segs;
}
__host__ __device__ inline Table table_of(const int32_t* tab) {
    Table t;
    t.n_items = tab[0]; t.n_segs = tab[1]; t.n_spk = tab[2]; t.nutt = tab[3];
    t.spk_ptr = tab + 4;
    t.item_spk = t.spk_ptr + t.n_spk + 1;
    t.item_ptr = t.item_spk + t.n_items;
    t.seg = t.item_ptr + t.n_items + 1;
    return t;
}
__host__ __device__ inline int tri_of(int E) { return E * (E + 1) / 2; }
// doubles of one item's slab (and of one speaker's statistics): G packed, k, beta
__host__ __device__ inline size_t slab_doubles(int D, int P) {
    return (size_t)P * tri_of(D + 1) + (size_t)D * (D + 1) + 1;
}
// row stride of the staged frames: 16 NT columns, and a multiple of 16 that is not one of 32
// (the four frames of an MFMA step then start 128 bytes apart modulo 256)
__host__ __device__ inline int row_stride(int NT) { return (NT & 1) ? 16 * NT : 16 * NT + 16; }

// ---------------------------------------------------------------------------
// frame_params
// ---------------------------------------------------------------------------
template <typename T, int NC>
__global__ __launch_bounds__(256) void frame_params_kernel(
    int64_t nframes, int D, int P, int S, int G, int Q, const T* __restrict__ cr,
    const T* __restrict__ sr, const T* __restrict__ E, double* __restrict__ out) {
    constexpr int KC = kStageComps, RP = KC + 4, NCP = (NC & 1) ? 16 * NC : 16 * NC + 16;
    __shared__ double rt[kTileFrames * RP];        // [frame][component]
    __shared__ double tb[KC * NCP];                // [component][column]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const int K = S * G, W = P + D + 1;
    const int64_t t0 = (int64_t)blockIdx.x * kTileFrames;
    f64x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f64x4{0., 0., 0., 0.};
    for (int k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();                           // the last stage is done with
        for (int idx = tid; idx < kTileFrames * KC; idx += 256) {
            const int f = idx / KC, c = idx - f * KC, k = k0 + c;
            const int64_t t = t0 + f;
            double v = 0.;
            if (t < nframes && k < K) {
                v = cr ? (double)cr[(size_t)t * K + k] : 1.;
                if (sr) v *= (double)sr[(size_t)t * S + k / G];
            }
            rt[f * RP + c] = v;
        }
        for (int idx = tid; idx < KC * NCP; idx += 256) {
            const int c = idx / NCP, n = idx - c * NCP, k = k0 + c;
            double v = 0.;
            if (k < K) {
                const T* e = E + (size_t)k * Q;
                if (n < P) v = (double)e[D + n];
                else if (n < P + D) v = (double)e[n - P];
                else if (n == P + D) v = 1.;
            }
            tb[idx] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const double a = rt[(16 * w + i16) * RP + 4 * kk + g];
            const double* brow = tb + (4 * kk + g) * NCP + i16;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = M64::mma(a, brow[16 * c], acc[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t t = t0 + 16 * w + M64::row(g, r);
        if (t >= nframes) continue;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = 16 * c + i16;
            if (col < W) out[(size_t)t * W + col] += acc[c][r];
        }
    }
}

template <typename T>
int frame_params_launch(int64_t nframes, int D, int P, int S, int G, int Q, const void* cr,
                        const void* sr, const void* E, double* out, void* stream) {
    BEER_REQUIRE(nframes >= 0 && D >= 1 && D <= kMaxDim && (P == 1 || P == D));
    BEER_REQUIRE(S >= 1 && G >= 1 && (int64_t)S * G < (int64_t)2147483647 && Q >= D + P);
    if (nframes == 0) return BEER_OK;
    BEER_REQUIRE(E && out && (cr || G == 1));
    const int64_t blocks = (nframes + kTileFrames - 1) / kTileFrames;
    BEER_REQUIRE(blocks < (int64_t)2147483647);
    const int NC = (P + D + 1 + 15) / 16;
    hipStream_t s = as_stream(stream);
#define BEER_FP_LAUNCH(N)                                                                    \
    case N:                                                                                   \
        hipLaunchKernelGGL((frame_params_kernel<T, N>), dim3((unsigned)blocks), dim3(256), 0, \
                           s, nframes, D, P, S, G, Q, (const T*)cr, (const T*)sr,             \
                           (const T*)E, out);                                                 \
        break
    switch (NC) {
        BEER_FP_LAUNCH(1); BEER_FP_LAUNCH(2); BEER_FP_LAUNCH(3); BEER_FP_LAUNCH(4);
        BEER_FP_LAUNCH(5); BEER_FP_LAUNCH(6); BEER_FP_LAUNCH(7); BEER_FP_LAUNCH(8);
        default: return BEER_EINVAL;
    }
#undef BEER_FP_LAUNCH
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

// ---------------------------------------------------------------------------
// accumulate
// ---------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(256) void cmllr_partial_kernel(
    int64_t nframes, int D, int P, int nutt, int n_gblocks, const T* __restrict__ X,
    const double* __restrict__ prm, const int64_t* __restrict__ frame_off,
    const int32_t* __restrict__ tab, double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int EP = (NT & 1) ? 16 * NT : 16 * NT + 16, NTRI = NT * (NT + 1) / 2;
    double* xi = reinterpret_cast<double*>(smem);          // [64][EP]: xi_t, zeros beyond E
    double* wv = xi + kTileFrames * EP;                    // [64][EP]: the block's weights
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, g = lane >> 4;
    const int E = D + 1, PW = P + D + 1;
    const Table tb = table_of(tab);
    const int item = blockIdx.x, blk = blockIdx.y;
    const bool linear = blk == n_gblocks;
    const int s0 = tb.item_ptr[item], s1 = tb.item_ptr[item + 1];
    int n_item = 0;                                        // frames of the item
    for (int s = s0; s < s1; ++s) n_item += tb.seg[3 * s + 2];
    // staging: thread (fl, q) fills columns q, q + 4, .. of frame slot fl; its cursor into the
    // item's runs only moves forward
    const int fl = tid >> 2, q = tid & 3;
    int cs = s0, cum = 0;

    f64x4 acc[kDimsPerWave][NTRI];
#pragma unroll
    for (int d = 0; d < kDimsPerWave; ++d)
#pragma unroll
        for (int n = 0; n < NTRI; ++n) acc[d][n] = f64x4{0., 0., 0., 0.};
    const int dim0 = kDimsPerBlock * blk + kDimsPerWave * w;   // the wave's first dimension
    const bool busy = linear ? w < NT : dim0 < P;

    for (int base = 0; base < n_item; base += kTileFrames) {
        if (base) __syncthreads();
        const int local = base + fl;
        while (cs < s1 && local >= cum + tb.seg[3 * cs + 2]) {
            cum += tb.seg[3 * cs + 2];
            ++cs;
        }
        int64_t fr = -1;
        if (cs < s1 && local < n_item) {
            const int u = tb.seg[3 * cs];
            if ((unsigned)u < (unsigned)nutt) fr = frame_off[u] + tb.seg[3 * cs + 1] + (local - cum);
        }
        const bool valid = fr >= 0 && fr < nframes;
        for (int c = q; c < EP; c += 4) {
            xi[fl * EP + c] = !valid ? 0. : (c < D ? (double)X[(size_t)fr * D + c] : (c == D ? 1. : 0.));
            double v = 0.;
            if (valid) {
                if (linear) { if (c < E) v = prm[(size_t)fr * PW + P + c]; }
                else if (c < kDimsPerBlock && kDimsPerBlock * blk + c < P)
                    v = prm[(size_t)fr * PW + kDimsPerBlock * blk + c];
            }
            wv[fl * EP + c] = v;
        }
        __syncthreads();
        if (!busy) continue;
#pragma unroll 4
        for (int step = 0; step < kTileFrames / 4; ++step) {
            const int f = 4 * step + g;
            double xv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) xv[t] = xi[f * EP + 16 * t + i16];
            if (linear) {
                const double a = wv[f * EP + 16 * w + i16];
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) acc[0][tj] = M64::mma(a, xv[tj], acc[0][tj]);
            } else {
#pragma unroll
                for (int d = 0; d < kDimsPerWave; ++d) {
                    const double om = wv[f * EP + kDimsPerWave * w + d];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) {
                        const double a = om * xv[ti];
#pragma unroll
                        for (int tj = 0; tj <= ti; ++tj)
                            acc[d][ti * (ti + 1) / 2 + tj] = M64::mma(a, xv[tj], acc[d][ti * (ti + 1) / 2 + tj]);
                    }
                }
            }
        }
    }
    if (!busy) return;
    const int tri = tri_of(E);
    double* slab = ws + (size_t)item * slab_doubles(D, P);
    if (linear) {
        double* kp = slab + (size_t)P * tri;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + M64::row(g, r), col = 16 * tj + i16;
                if (row < D && col < E) kp[row * E + col] = acc[0][tj][r];
                else if (row == D && col == D) kp[D * E] = acc[0][tj][r];
            }
        return;
    }
#pragma unroll
    for (int d = 0; d < kDimsPerWave; ++d) {
        if (dim0 + d >= P) continue;
        double* gp = slab + (size_t)(dim0 + d) * tri;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj <= ti; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + M64::row(g, r), col = 16 * tj + i16;
                    if (row < E && col <= row) gp[row * (row + 1) / 2 + col] = acc[d][ti * (ti + 1) / 2 + tj][r];
                }
    }
}

// the slabs of a speaker's items, in chunk order, into the statistics (+=)
__global__ __launch_bounds__(256) void cmllr_fold_kernel(
    int D, int P, const int32_t* __restrict__ tab, const double* __restrict__ ws,
    double* __restrict__ Gs, double* __restrict__ ks, double* __restrict__ beta) {
    const Table tb = table_of(tab);
    const size_t per = slab_doubles(D, P), ng = (size_t)P * tri_of(D + 1), nk = (size_t)D * (D + 1);
    const size_t total = per * (size_t)tb.n_spk;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const size_t s = idx / per, e = idx - s * per;
        int j0 = tb.spk_ptr[s], j1 = tb.spk_ptr[s + 1];
        j0 = j0 < 0 ? 0 : j0;
        j1 = j1 > tb.n_items ? tb.n_items : j1;
        if (j1 <= j0) continue;
        double sum = 0.;
        for (int j = j0; j < j1; ++j) sum += ws[(size_t)j * per + e];
        if (e < ng) Gs[s * ng + e] += sum;
        else if (e < ng + nk) ks[s * nk + (e - ng)] += sum;
        else beta[s] += sum;
    }
}

// the structure of a table, from its host copy
bool table_ok(const int32_t* tab, size_t n_ints, int n_spk, int nutt, int chunk) {
    if (!tab || n_ints < 4) return false;
    if (tab[0] < 0 || tab[1] < 0 || tab[2] != n_spk || tab[3] != nutt) return false;
    if (n_ints != table_ints(tab[2], tab[0], tab[1])) return false;
    const Table t = table_of(tab);
    if (t.spk_ptr[0] != 0 || t.spk_ptr[n_spk] != t.n_items) return false;
    for (int s = 0; s < n_spk; ++s) {
        if (t.spk_ptr[s + 1] < t.spk_ptr[s]) return false;
        for (int j = t.spk_ptr[s]; j < t.spk_ptr[s + 1]; ++j)
            if (j >= t.n_items || t.item_spk[j] != s) return false;
    }
    if (t.item_ptr[0] != 0 || t.item_ptr[t.n_items] != t.n_segs) return false;
    for (int j = 0; j < t.n_items; ++j) {
        if (t.item_ptr[j + 1] < t.item_ptr[j] || t.item_ptr[j + 1] > t.n_segs) return false;
        if (t.item_spk[j] < 0 || t.item_spk[j] >= n_spk) return false;
        int64_t frames = 0;
        for (int s = t.item_ptr[j]; s < t.item_ptr[j + 1]; ++s) {
            const int32_t* seg = t.seg + 3 * (size_t)s;
            if (seg[0] < 0 || seg[0] >= nutt || seg[1] < 0 || seg[2] < 1) return false;
            frames += seg[2];
        }
        if (frames > chunk) return false;
    }
    return true;
}

template <typename T>
int accumulate_launch(int64_t nframes, int D, int P, int nutt, int n_spk, const void* X,
                      const double* prm, const int64_t* frame_off, const int32_t* table_host,
                      const int32_t* table_dev, size_t n_ints, int chunk, double* Gs, double* ks,
                      double* beta, void* ws, size_t ws_bytes, void* stream) {
    BEER_REQUIRE(D >= 1 && D <= kMaxDim && (P == 1 || P == D));
    BEER_REQUIRE(nframes >= 0 && nutt >= 0 && n_spk >= 0 && chunk >= 0);
    if (chunk == 0) chunk = kDefaultChunk;
    BEER_REQUIRE(table_ok(table_host, n_ints, n_spk, nutt, chunk));
    const int n_items = table_host[0];
    if (n_items == 0 || n_spk == 0) return BEER_OK;
    BEER_REQUIRE(X && prm && frame_off && table_dev && Gs && ks && beta);
    BEER_REQUIRE(ws && ws_bytes >= (size_t)n_items * slab_doubles(D, P) * sizeof(double));
    const int NT = (D + 1 + 15) / 16;
    const int n_gblocks = (P + kDimsPerBlock - 1) / kDimsPerBlock;
    const size_t lds = 2 * (size_t)kTileFrames * row_stride(NT) * sizeof(double);
    const dim3 grid((unsigned)n_items, (unsigned)(n_gblocks + 1)), block(256);
    hipStream_t s = as_stream(stream);
#define BEER_CMLLR_LAUNCH(N)                                                                      \
    case N:                                                                                       \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cmllr_partial_kernel<T, N>),      \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, beer::kMaxDynLds);  \
        hipLaunchKernelGGL((cmllr_partial_kernel<T, N>), grid, block, lds, s, nframes, D, P,      \
                           nutt, n_gblocks, (const T*)X, prm, frame_off, table_dev, (double*)ws); \
        break
    switch (NT) {
        BEER_CMLLR_LAUNCH(1); BEER_CMLLR_LAUNCH(2); BEER_CMLLR_LAUNCH(3); BEER_CMLLR_LAUNCH(4);
        default: return BEER_EINVAL;
    }
#undef BEER_CMLLR_LAUNCH
    BEER_LAUNCH_CHECK();
    const size_t total = slab_doubles(D, P) * (size_t)n_spk;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(cmllr_fold_kernel, dim3(blocks), dim3(256), 0, s, D, P, table_dev,
                       (const double*)ws, Gs, ks, beta);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

// ---------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cmllr_apply_kernel(
    int64_t nframes, int D, int nutt, int n_spk, const T* __restrict__ X,
    const double* __restrict__ W, const int64_t* __restrict__ frame_off,
    const int32_t* __restrict__ utt_spk, T* __restrict__ Y) {
    const int64_t total = nframes * D;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = idx / D;
        const int i = (int)(idx - t * D);
        // the last utterance whose first frame is <= t (utterances of no frames are passed over)
        int lo = 0, hi = nutt;
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            if (frame_off[mid + 1] <= t) lo = mid + 1; else hi = mid;
        }
        const int s = lo < nutt && frame_off[lo] <= t ? utt_spk[lo] : -1;
        const T* x = X + t * D;
        if (s < 0 || s >= n_spk) { Y[idx] = x[i]; continue; }
        const double* w = W + ((size_t)s * D + i) * (D + 1);
        double acc = 0.;
        for (int a = 0; a < D; ++a) acc = fma(w[a], (double)x[a], acc);
        Y[idx] = (T)(acc + w[D]);
    }
}

template <typename T>
int apply_launch(int64_t nframes, int D, int nutt, int n_spk, const void* X, const double* W,
                 const int64_t* frame_off, const int32_t* utt_spk, const int32_t* utt_spk_host,
                 void* Y, void* stream) {
    BEER_REQUIRE(D >= 1 && D <= kMaxDim && nframes >= 0 && nutt >= 0 && n_spk >= 0);
    if (utt_spk_host)
        for (int u = 0; u < nutt; ++u) BEER_REQUIRE(utt_spk_host[u] >= -1 && utt_spk_host[u] < n_spk);
    if (nframes == 0) return BEER_OK;
    BEER_REQUIRE(X && Y && X != Y && frame_off && utt_spk && (W || n_spk == 0));
    const int64_t total = nframes * D;
    const unsigned blocks = (unsigned)((total + 255) / 256 < (1 << 20) ? (total + 255) / 256 : (1 << 20));
    hipLaunchKernelGGL((cmllr_apply_kernel<T>), dim3(blocks), dim3(256), 0, as_stream(stream),
                       nframes, D, nutt, n_spk, (const T*)X, W, frame_off, utt_spk, (T*)Y);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

}  // namespace

extern "C" {

int beer_cmllr_frame_params(int dtype, int cov, int64_t T, int D, int S, int G,
                            const void* comp_resps, const void* state_resps, const void* E,
                            double* out, void* stream) {
    BEER_REQUIRE(cov == BEER_DIAG || cov == BEER_ISO);
    BEER_REQUIRE(D >= 1 && D <= kMaxDim);
    const int P = cov == BEER_DIAG ? D : 1;
    BEER_DISPATCH(dtype, frame_params_launch, T, D, P, S, G, stats_dim(cov, D), comp_resps,
                  state_resps, E, out, stream);
}

int beer_cmllr_table(int32_t nutt, int32_t n_spk, const int64_t* lengths, const int32_t* utt_spk,
                     int32_t chunk_frames, int32_t* table, size_t* n_ints) {
    BEER_REQUIRE(nutt >= 0 && n_spk >= 0 && chunk_frames >= 0 && n_ints);
    BEER_REQUIRE(nutt == 0 || (lengths && utt_spk));
    const int chunk = chunk_frames ? chunk_frames : kDefaultChunk;
    for (int u = 0; u < nutt; ++u) {
        BEER_REQUIRE(utt_spk[u] >= -1 && utt_spk[u] < n_spk);
        BEER_REQUIRE(lengths[u] >= 0 && lengths[u] < (int64_t)2147483647);
    }
    // the utterances of every speaker, in utterance order (a counting sort)
    std::vector<int> first(n_spk + 1, 0), utts(nutt);
    for (int u = 0; u < nutt; ++u)
        if (utt_spk[u] >= 0) ++first[utt_spk[u] + 1];
    for (int s = 0; s < n_spk; ++s) first[s + 1] += first[s];
    {
        std::vector<int> next(first.begin(), first.end() - 1);
        for (int u = 0; u < nutt; ++u)
            if (utt_spk[u] >= 0) utts[next[utt_spk[u]]++] = u;
    }
    std::vector<int32_t> spk_ptr(n_spk + 1, 0), item_spk, item_ptr, seg;
    for (int s = 0; s < n_spk; ++s) {
        int room = 0;                                  // frames the open item still takes
        for (int n = first[s]; n < first[s + 1]; ++n) {
            const int u = utts[n];
            int64_t begin = 0, left = lengths[u];
            while (left > 0) {
                if (room == 0) {                       // a new item begins with the next run
                    BEER_REQUIRE(item_spk.size() < (size_t)2147483647 / 4);
                    item_spk.push_back(s);
                    item_ptr.push_back((int32_t)(seg.size() / 3));
                    room = chunk;
                }
                const int take = (int)(left < room ? left : room);
                BEER_REQUIRE(seg.size() / 3 < (size_t)2147483647 / 4);
                seg.push_back(u); seg.push_back((int32_t)begin); seg.push_back(take);
                begin += take; left -= take; room -= take;
            }
        }
        spk_ptr[s + 1] = (int32_t)item_spk.size();
    }
    item_ptr.push_back((int32_t)(seg.size() / 3));
    const size_t need = table_ints(n_spk, (int)item_spk.size(), (int)(seg.size() / 3));
    if (!table) { *n_ints = need; return BEER_OK; }
    BEER_REQUIRE(*n_ints >= need);
    *n_ints = need;
    int32_t* p = table;
    *p++ = (int32_t)item_spk.size(); *p++ = (int32_t)(seg.size() / 3); *p++ = n_spk; *p++ = nutt;
    for (int32_t v : spk_ptr) *p++ = v;
    for (int32_t v : item_spk) *p++ = v;
    for (int32_t v : item_ptr) *p++ = v;
    for (int32_t v : seg) *p++ = v;
    return BEER_OK;
}

size_t beer_cmllr_workspace_bytes(int D, int P, int64_t n_items) {
    if (D < 1 || D > kMaxDim || (P != 1 && P != D) || n_items < 0) return 0;
    return (size_t)n_items * slab_doubles(D, P) * sizeof(double);
}

int beer_cmllr_accumulate(int dtype, int64_t T, int D, int P, int32_t nutt, int32_t n_spk,
                          const void* X, const double* params, const int64_t* frame_off,
                          const int32_t* table_host, const int32_t* table, size_t table_ints,
                          int32_t chunk_frames, double* G, double* k, double* beta,
                          void* workspace, size_t workspace_bytes, void* stream) {
    BEER_DISPATCH(dtype, accumulate_launch, T, D, P, nutt, n_spk, X, params, frame_off,
                  table_host, table, table_ints, chunk_frames, G, k, beta, workspace,
                  workspace_bytes, stream);
}

int beer_cmllr_apply(int dtype, int64_t T, int D, int32_t nutt, int32_t n_spk, const void* X,
                     const double* W, const int64_t* frame_off, const int32_t* utt_spk,
                     const int32_t* utt_spk_host, void* Y, void* stream) {
    BEER_DISPATCH(dtype, apply_launch, T, D, nutt, n_spk, X, W, frame_off, utt_spk, utt_spk_host,
                  Y, stream);
}

}  // extern "C"
