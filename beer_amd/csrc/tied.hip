// Tied-mixture (semi-continuous) emissions on gfx950: S mixtures over ONE pool of K
// Gaussians that differ in their weights only.  With l[t,k] the expected log-likelihoods
// of the pool and lw[s,k] = E[ln pi_sk] (fp64 whatever the model's dtype: the E[ln pi] of a
// component nobody uses is about -1 / concentration, and float32 holds -130 to 8e-6 only --
// an error the responsibilities would inherit; w = exp(lw) rounded to float32 has none of it):
//
//   m[t]  = max_k l[t,k]      e[t,k] = exp(l[t,k] - m[t])      w[s,k] = exp(lw[s,k])
//   p[t,s] = sum_k e[t,k] w[s,k]                               q[t,s] = g[t,s] / p[t,s]
//
//   beer_tied_lognorm      pc = m + ln(E W^T)
//   beer_tied_accumulate   R  = E o (Q W)          C += W o (Q^T E)
//
// three products on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, the
// exact arithmetic of estep_mfma.hip; operand mapping there).  E is recomputed from l and m
// by both kernels and never stored.
//
// Range.  The products live in the linear domain: e <= 1 (the frame's best Gaussian has
// e = 1), w <= 1.  A term e w below the smallest normal number `tiny` of the dtype may be
// lost (the factor or the product flushed to zero); all terms are non-negative, so that is
// the only error beyond the usual K roundings: |p_computed - p| <= K tiny + K eps p.  For
// the relative error of p -- the absolute error of pc -- to stay below delta the entry
// needs p >= K tiny / delta.  With K <= 4096 (the entry points refuse more) and delta =
// 2^-20 (float32: a tenth of the 1e-5 tolerance), 2^-40 (float64: 1e-12) this gives the
// thresholds
//       float32  2^12 * 2^-126 * 2^20 = 2^-94        float64  2^12 * 2^-1022 * 2^40 = 2^-970
// An entry (t, s) whose p is below the threshold is redone in log space:
// pc = logsumexp_k(l + lw) directly (beer_tied_lognorm, counted in `log_count`), and its
// responsibilities g exp(l + lw - pc) are added after the products by the workgroup that
// owns the frame (beer_tied_accumulate: q of such an entry is 0 in the products, as is q
// of every entry with g = 0).  Either way is accurate for an entry near the threshold, so
// the two kernels need not agree on which side it falls.

#include <type_traits>

#include "common.h"
#include "estep_tiles.h"

using namespace beer;
using beer_mfma::Mma;

namespace {

constexpr int kTiedThreads = 256;      // 4 waves
constexpr int kTiedMaxK = 4096;        // the range rule above is derived for K <= 2^12
constexpr int kKC = 64;                // Gaussians per LDS chunk
constexpr int kLnFW = 32;              // beer_tied_lognorm: frames per wave (two row tiles)
constexpr int kLnFT = 4 * kLnFW;       //                    frames per workgroup
constexpr int kLnLD = kKC + 4;         // row stride of its LDS tiles: lane (i, g) reads
                                       // [i][4 ks + g] -> bank 4 i + g, no conflict (fp32)
constexpr int kAcFT = 64;              // beer_tied_accumulate: frames per LDS tile
constexpr int kAcLD = kKC + 16;        // E and W tiles read as B[k = g][n = i] -> bank 16 g + i
constexpr int kAcChain = 4096;         // frames a workgroup sums in the model's dtype before
                                       // its partial C meets the others in fp64

template <typename T> __device__ __forceinline__ T tied_threshold();
template <> __device__ __forceinline__ float tied_threshold<float>() { return 0x1p-94f; }
template <> __device__ __forceinline__ double tied_threshold<double>() { return 0x1p-970; }

__device__ __forceinline__ float tied_exp(float x) { return expf(x); }
__device__ __forceinline__ double tied_exp(double x) { return exp(x); }
// w = exp(lw) in the model's dtype from the fp64 log-weight.  float32: lw = hi + lo with hi
// its float32 rounding, exp(hi) (1 + lo) -- |lo| <= 2^-17 here, the second-order term is
// below float32's rounding -- instead of an fp64 exponential per staged weight.
template <typename T> __device__ __forceinline__ T tied_weight(double lw);
template <> __device__ __forceinline__ double tied_weight<double>(double lw) { return exp(lw); }
template <> __device__ __forceinline__ float tied_weight<float>(double lw) {
    const float hi = (float)lw;
    const float lo = (float)(lw - (double)hi);
    const float e = expf(hi);
    return fmaf(e, lo, e);
}
__device__ __forceinline__ float tied_log(float x) { return logf(x); }
__device__ __forceinline__ double tied_log(double x) { return log(x); }

// logsumexp_k(l[k] + lw[k]) of one entry, in fp64 (the rare path)
template <typename T>
__device__ double tied_lse(const T* __restrict__ l, const double* __restrict__ lw, int K) {
    double mx = neg_inf();
    for (int k = 0; k < K; ++k) {
        const double v = (double)l[k] + lw[k];
        if (v > mx) mx = v;
    }
    if (!(mx > neg_inf())) return mx;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp((double)l[k] + lw[k] - mx);
    return mx + log(s);
}

// the same by a whole wave (all lanes get the result)
template <typename T>
__device__ double tied_lse_wave(const T* __restrict__ l, const double* __restrict__ lw, int K,
                                int lane) {
    double mx = neg_inf();
    for (int k = lane; k < K; k += 64) {
        const double v = (double)l[k] + lw[k];
        if (v > mx) mx = v;
    }
    mx = wave_max(mx);
    if (!(mx > neg_inf())) return mx;
    double s = 0.0;
    for (int k = lane; k < K; k += 64) s += exp((double)l[k] + lw[k] - mx);
    return mx + log(wave_sum(s));
}

// ---------------------------------------------------------------------------
// pc = m + ln(E W^T).  A workgroup owns 128 frames (a wave 32: two row tiles) and
// 16 NS states; the contraction runs over chunks of 64 Gaussians whose W tile
// [16 NS][64] is staged once per workgroup and chunk, the E tile per wave.
// blockIdx.x = frame tile * state chunks + state chunk.
// ---------------------------------------------------------------------------
template <typename T, int NS>
__global__ __launch_bounds__(kTiedThreads) void tied_lognorm_kernel(
    int64_t nframes, int K, int S, int nsch, const T* __restrict__ l,
    const double* __restrict__ lw, T* __restrict__ pc, T* __restrict__ m_out, unsigned long long* __restrict__ log_count) {
    using M = Mma<T>;
    using acc_t = typename M::acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* const Ws = reinterpret_cast<T*>(smem);              // [16 NS][kLnLD]
    T* const Es = Ws + 16 * NS * kLnLD;                    // [kLnFT][kLnLD]
    T* const ms = Es + kLnFT * kLnLD;                      // [kLnFT]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int sc = (int)(blockIdx.x % (unsigned)nsch);
    const int s0 = sc * 16 * NS;
    const int64_t f0 = (int64_t)(blockIdx.x / (unsigned)nsch) * kLnFT + wave * kLnFW;
    const int row0 = wave * kLnFW;

    // row maxima of the wave's frames (0 for a row without a finite entry or past the end)
    // (four rows at a time, rows past the end clamped to the last one: the loads of a group
    //  are independent and unconditional, so they are in flight together)
    for (int r = 0; r < kLnFW; r += 4) {
        T v[4];
        const T* row[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t f = f0 + r + u;
            row[u] = l + (f < nframes ? f : nframes - 1) * K;
            v[u] = (T)neg_inf();
        }
        for (int k = lane; k < K; k += 64)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T x = row[u][k];
                v[u] = x > v[u] ? x : v[u];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t f = f0 + r + u;
            T w = wave_max(v[u]);
            if (!(w > (T)neg_inf())) w = 0;
            if (lane == 0) {
                ms[row0 + r + u] = w;
                if (sc == 0 && f < nframes) m_out[f] = w;
            }
        }
    }

    acc_t acc[2][NS];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NS; ++nt) acc[mt][nt] = acc_t{0, 0, 0, 0};

    for (int kc = 0; kc < K; kc += kKC) {
        __syncthreads();                                   // the previous chunk has been read
        for (int idx = tid; idx < 16 * NS * kKC; idx += kTiedThreads) {
            const int s = idx / kKC, kk = idx - s * kKC;
            T v = 0;
            if (s0 + s < S && kc + kk < K) v = tied_weight<T>(lw[(size_t)(s0 + s) * K + kc + kk]);
            Ws[s * kLnLD + kk] = v;
        }
        const int kcl = kc + lane < K ? kc + lane : K - 1;     // (clamped: unconditional loads)
#pragma unroll 8
        for (int r = 0; r < kLnFW; ++r) {
            const int64_t f = f0 + r;
            const T x = l[(f < nframes ? f : nframes - 1) * K + kcl];
            const T v = tied_exp(x - ms[row0 + r]);
            Es[(row0 + r) * kLnLD + lane] = (f < nframes && kc + lane < K) ? v : (T)0;
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < kKC / 4; ++ks) {
            T a[2], b[NS];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) a[mt] = Es[(row0 + mt * 16 + i) * kLnLD + 4 * ks + g];
#pragma unroll
            for (int nt = 0; nt < NS; ++nt) b[nt] = Ws[(nt * 16 + i) * kLnLD + 4 * ks + g];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NS; ++nt) acc[mt][nt] = M::mma(a[mt], b[nt], acc[mt][nt]);
        }
    }

    int nlog = 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NS; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + M::row(g, r);
                const int64_t f = f0 + row;
                const int s = s0 + nt * 16 + i;
                if (f < nframes && s < S) {
                    const T p = acc[mt][nt][r];
                    T v;
                    if (p < tied_threshold<T>()) {
                        v = (T)tied_lse(l + f * K, lw + (size_t)s * K, K);
                        ++nlog;
                    } else {
                        v = ms[row0 + row] + tied_log(p);
                    }
                    pc[f * S + s] = v;
                }
            }
    nlog = wave_sum(nlog);
    if (lane == 0 && nlog && log_count) atomicAdd(log_count, (unsigned long long)nlog);
}

// ---------------------------------------------------------------------------
// R = E o (Q W), C += W o (Q^T E) for `sn` <= 16 NS states s0 .. s0 + sn - 1.  A workgroup
// owns a chunk of 64 Gaussians (its W tile [16 NS][64] is staged once) and a run of at
// most kAcChain frames, walked in tiles of 64: Q [64][16 NS] and E [64][64] go to LDS,
// wave w multiplies for the 16 Gaussians 16 w .. 16 w + 15 of the chunk -- four row tiles
// of R, NS tiles of C kept in registers over the run and added to C in fp64 at its end.
// blockIdx.x = frame run * chunks + chunk.
// ---------------------------------------------------------------------------
template <typename T, int NS>
__global__ __launch_bounds__(kTiedThreads) void tied_accumulate_kernel(
    int64_t nframes, int K, int S, int s0, int sn, int add_r, int nkc,
    const T* __restrict__ l, const T* __restrict__ m, const T* __restrict__ pc,
    const double* __restrict__ lw, const T* __restrict__ gam, T* __restrict__ R,
    double* __restrict__ C) {
    using M = Mma<T>;
    using acc_t = typename M::acc_t;
    constexpr int SP = 16 * NS, LDQ = SP + 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* const nflag = reinterpret_cast<int*>(smem);       // [2] (+ padding to 16 bytes)
    T* const Ws = reinterpret_cast<T*>(smem + 16);         // [SP][kAcLD]
    T* const Es = Ws + SP * kAcLD;                         // [kAcFT][kAcLD]
    T* const Qs = Es + kAcFT * kAcLD;                      // [kAcFT][LDQ]
    unsigned char* const Fs = reinterpret_cast<unsigned char*>(Qs + kAcFT * LDQ);  // [kAcFT][SP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int kc = (int)(blockIdx.x % (unsigned)nkc) * kKC;
    const int64_t fb = (int64_t)(blockIdx.x / (unsigned)nkc) * kAcChain;
    const int64_t fe = fb + kAcChain < nframes ? fb + kAcChain : nframes;
    const int kcol = kc + wave * 16 + i;                   // this lane's Gaussian in C tiles

    for (int idx = tid; idx < SP * kKC; idx += kTiedThreads) {
        const int s = idx / kKC, kk = idx - s * kKC;
        T v = 0;
        if (s < sn && kc + kk < K) v = tied_weight<T>(lw[(size_t)(s0 + s) * K + kc + kk]);
        Ws[s * kAcLD + kk] = v;
    }
    if (tid < 2) nflag[tid] = 0;

    acc_t cacc[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) cacc[st] = acc_t{0, 0, 0, 0};

    int par = 0;
    for (int64_t f0 = fb; f0 < fe; f0 += kAcFT, par ^= 1) {
        __syncthreads();                                   // the previous tile has been read
        // (entries past the end read a clamped address and are zeroed afterwards: the loads
        //  are unconditional and independent, the unrolled loop has them in flight together)
#pragma unroll 8
        for (int idx = tid; idx < kAcFT * SP; idx += kTiedThreads) {
            const int t = idx / SP, s = idx - t * SP;
            const int64_t f = f0 + t;
            const bool in = f < fe && s < sn;
            const int64_t at = in ? f * S + s0 + s : fb * S + s0;
            const T gg = gam[at];
            const T p = tied_exp(pc[at] - m[in ? f : fb]);
            const bool live = in && gg != 0;
            const bool flag = live && p < tied_threshold<T>();
            Qs[t * LDQ + s] = (live && !flag) ? gg / p : (T)0;
            Fs[idx] = flag ? 1 : 0;
            if (flag) atomicAdd(&nflag[par], 1);
        }
        const int kcl = kc + lane < K ? kc + lane : K - 1;
#pragma unroll
        for (int r = wave * 16; r < wave * 16 + 16; ++r) {
            const int64_t f = f0 + r < fe ? f0 + r : fe - 1;
            const T v = tied_exp(l[f * K + kcl] - m[f]);
            Es[r * kAcLD + lane] = (f0 + r < fe && kc + lane < K) ? v : (T)0;
        }
        __syncthreads();
        if (tid == 0) nflag[par ^ 1] = 0;                  // the next tile's (read two barriers ago)

        // U = Q W, then R = E o U
        acc_t u[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) u[mt] = acc_t{0, 0, 0, 0};
#pragma unroll 4
        for (int ss = 0; ss < SP / 4; ++ss) {
            const T b = Ws[(4 * ss + g) * kAcLD + wave * 16 + i];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                u[mt] = M::mma(Qs[(mt * 16 + i) * LDQ + 4 * ss + g], b, u[mt]);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + M::row(g, r);
                const int64_t f = f0 + row;
                if (f < fe && kcol < K) {
                    T v = Es[row * kAcLD + wave * 16 + i] * u[mt][r];
                    if (add_r) v += R[f * K + kcol];
                    R[f * K + kcol] = v;
                }
            }
        // C tile += Q^T E
#pragma unroll 4
        for (int ts = 0; ts < kAcFT / 4; ++ts) {
            const T b = Es[(4 * ts + g) * kAcLD + wave * 16 + i];
#pragma unroll
            for (int st = 0; st < NS; ++st)
                cacc[st] = M::mma(Qs[(4 * ts + g) * LDQ + st * 16 + i], b, cacc[st]);
        }
        // entries below the threshold: g exp(l + lw - logsumexp_k(l + lw)), added to what the
        // products left (the normaliser recomputed in fp64: the stored pc is rounded to dtype)
        if (nflag[par]) {
            __threadfence();                               // this tile's rows of R are out
            __syncthreads();
            for (int idx = wave; idx < kAcFT * SP; idx += kTiedThreads / 64) {
                if (!Fs[idx]) continue;
                const int t = idx / SP, s = idx - t * SP;
                const int64_t f = f0 + t;
                const double norm = tied_lse_wave(l + f * K, lw + (size_t)(s0 + s) * K, K, lane);
                const int k = kc + lane;
                if (k < K && norm > neg_inf() && norm < -neg_inf()) {
                    const double a = (double)l[f * K + k] + lw[(size_t)(s0 + s) * K + k] - norm;
                    const double j = (double)gam[f * S + s0 + s] * exp(a);
                    if (j != 0.0) {
                        atomicAdd(&R[f * K + k], (T)j);
                        atomicAdd(&C[(size_t)(s0 + s) * K + k], j);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int st = 0; st < NS; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = st * 16 + M::row(g, r);
            if (s < sn && kcol < K) {
                const double v = (double)cacc[st][r] * exp(lw[(size_t)(s0 + s) * K + kcol]);
                if (v != 0.0) atomicAdd(&C[(size_t)(s0 + s) * K + kcol], v);
            }
        }
}

// state tiles per workgroup: float32 up to 8 (128 states), float64 up to 4 (LDS, registers)
template <typename T> constexpr int max_state_tiles() { return sizeof(T) == 4 ? 8 : 4; }

template <typename T>
int state_tiles(int S) {
    int ns = 1;
    while (16 * ns < S && ns < max_state_tiles<T>()) ns *= 2;
    return ns;
}

template <typename T>
int tied_lognorm_launch(int64_t nframes, int K, int S, const void* l, const double* lw, void* pc,
                        void* m, int64_t* log_count, void* stream) {
    const int ns = state_tiles<T>(S);
    const int nsch = (S + 16 * ns - 1) / (16 * ns);
    const int64_t nblocks = (nframes + kLnFT - 1) / kLnFT * nsch;
    BEER_REQUIRE(nblocks < (int64_t)1 << 31);
    const size_t lds = (size_t)(16 * ns * kLnLD + kLnFT * kLnLD + kLnFT) * sizeof(T);
#define BEER_TIED_LN(NS_)                                                                        \
    do {                                                                                         \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(tied_lognorm_kernel<T, NS_>),    \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);       \
        hipLaunchKernelGGL((tied_lognorm_kernel<T, NS_>), dim3((unsigned)nblocks),               \
                           dim3(kTiedThreads), lds, as_stream(stream), nframes, K, S, nsch,      \
                           (const T*)l, (const double*)lw, (T*)pc, (T*)m,                             \
                           (unsigned long long*)log_count);                                      \
    } while (0)
    if (ns == 1) BEER_TIED_LN(1);
    else if (ns == 2) BEER_TIED_LN(2);
    else if (ns == 4) BEER_TIED_LN(4);
    else if constexpr (sizeof(T) == 4) BEER_TIED_LN(8);
#undef BEER_TIED_LN
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

template <typename T>
int tied_accumulate_launch(int64_t nframes, int K, int S, const void* l, const void* m,
                           const void* pc, const double* lw, const void* g, void* r, double* C,
                           void* stream) {
    const int nkc = (K + kKC - 1) / kKC;
    const int64_t nblocks = (nframes + kAcChain - 1) / kAcChain * nkc;
    BEER_REQUIRE(nblocks < (int64_t)1 << 31);
    // more states than a workgroup takes: one launch per run of them, the later ones
    // adding to the R of the earlier (the stream orders them)
    const int per = 16 * max_state_tiles<T>();
    for (int s0 = 0; s0 < S; s0 += per) {
        const int sn = S - s0 < per ? S - s0 : per;
        const int ns = state_tiles<T>(sn);
        const int sp = 16 * ns;
        const size_t lds = (size_t)(sp * kAcLD + kAcFT * kAcLD + kAcFT * (sp + 4)) * sizeof(T) +
                           (size_t)kAcFT * sp + 16;
#define BEER_TIED_AC(NS_)                                                                        \
    do {                                                                                         \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(tied_accumulate_kernel<T, NS_>), \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);       \
        hipLaunchKernelGGL((tied_accumulate_kernel<T, NS_>), dim3((unsigned)nblocks),            \
                           dim3(kTiedThreads), lds, as_stream(stream), nframes, K, S, s0, sn,    \
                           s0 > 0 ? 1 : 0, nkc, (const T*)l, (const T*)m, (const T*)pc,          \
                           (const double*)lw, (const T*)g, (T*)r, C);                                 \
    } while (0)
        if (ns == 1) BEER_TIED_AC(1);
        else if (ns == 2) BEER_TIED_AC(2);
        else if (ns == 4) BEER_TIED_AC(4);
        else if constexpr (sizeof(T) == 4) BEER_TIED_AC(8);
#undef BEER_TIED_AC
        BEER_LAUNCH_CHECK();
    }
    return BEER_OK;
}

}  // namespace

extern "C" {

int beer_tied_lognorm(int dtype, int64_t T, int K, int S, const void* l, const double* lw,
                      void* pc, void* m, int64_t* log_count, void* stream) {
    BEER_REQUIRE(T >= 0 && K >= 1 && K <= kTiedMaxK && S >= 1);
    if (T == 0) return BEER_OK;
    BEER_REQUIRE(l && lw && pc && m);
    BEER_DISPATCH(dtype, tied_lognorm_launch, T, K, S, l, lw, pc, m, log_count, stream);
}

int beer_tied_accumulate(int dtype, int64_t T, int K, int S, const void* l, const void* m,
                         const void* pc, const double* lw, const void* g, void* r, double* C,
                         void* stream) {
    BEER_REQUIRE(T >= 0 && K >= 1 && K <= kTiedMaxK && S >= 1);
    if (T == 0) return BEER_OK;
    BEER_REQUIRE(l && m && pc && lw && g && r && C);
    BEER_DISPATCH(dtype, tied_accumulate_launch, T, K, S, l, m, pc, lw, g, r, C, stream);
}

}  // extern "C"
