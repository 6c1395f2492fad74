// What the HMM kernel families beside hmm.hip share (hmm_score, hmm_sample, hmm_nbest, hmm_arcs,
// hmm_lattice, hmm_segments, hmm_segposts, hsmm, hmm_bigram): the log-space arithmetic of a
// workgroup that owns an utterance, and the host formulas of their launch plans.  A new family
// includes this header; it does not copy it.
#pragma once

#include "common.h"

namespace beer {

// ---------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------
// exp / log of a log-sum-exp relative to its maximum, in the model's precision; differences, sums
// and the trellis stay fp64 (hmm.hip's Rel<T> is the same rule with float-typed values)
template <typename T> struct LogRel;
template <> struct LogRel<float> {
    static __device__ __forceinline__ double ex(double d) {
        return (double)__builtin_amdgcn_exp2f((float)d * 1.44269504088896340736f);
    }
    static __device__ __forceinline__ double lg(double s) {
        return (double)(__builtin_amdgcn_logf((float)s) * 0.69314718055994530942f);
    }
};
template <> struct LogRel<double> {
    static __device__ __forceinline__ double ex(double d) { return exp(d); }
    static __device__ __forceinline__ double lg(double s) { return log(s); }
};

// exp(d) over fp64's range with the mantissa in the model's precision: 2^n 2^f with
// n = rint(d log2 e) and f in [-1/2, 1/2] formed in fp64, 2^f by v_exp_f32 -- relative error ~1e-7
// whatever |d|; d = -inf and anything below 2^-1100 give 0 after the ldexp (and so does NaN)
template <typename T> struct LinExp;
template <> struct LinExp<float> {
    static __device__ __forceinline__ double ex(double d) {
        const double y = d * 1.4426950408889634074;
        const double yc = __builtin_fmax(y, -1100.0);
        const double n = __builtin_rint(yc);
        const double r = (double)__builtin_amdgcn_exp2f((float)(yc - n));
        return __builtin_amdgcn_ldexp(r, (int)n);
    }
};
template <> struct LinExp<double> {
    static __device__ __forceinline__ double ex(double d) { return exp(d); }
};

// biased exponent of a non-negative double (0: zero or denormal)
__device__ __forceinline__ int expo_field(double v) {
    return (int)((__builtin_bit_cast(unsigned long long, v) >> 52) & 0x7ffull);
}

__device__ __forceinline__ double dmax(double a, double b) { return b > a ? b : a; }

// A log-sum-exp as the pair (m, s): sum = s * exp(m), m the largest term so far (-inf and 0: no
// finite term yet).  One walk over an arc list instead of two (maximum, then sum): the walk is a
// chain of dependent LDS reads and sets the time of a frame.
template <typename T>
__device__ __forceinline__ void lse_add(double& m, double& s, double v) {
    if (v > m) {
        s = s * LogRel<T>::ex(m - v) + 1.0;        // (m = -inf: s = 0 stays 0 * 0)
        m = v;
    } else if (v > neg_inf()) {
        s += LogRel<T>::ex(v - m);
    }
}
// ... of two such pairs
template <typename T>
__device__ __forceinline__ void lse_join(double& m, double& s, double om, double os) {
    const double M = dmax(m, om);
    if (M > neg_inf())
        s = (s > 0.0 ? s * LogRel<T>::ex(m - M) : 0.0) + (os > 0.0 ? os * LogRel<T>::ex(om - M) : 0.0);
    m = M;
}
// ... and its value
template <typename T>
__device__ __forceinline__ double lse_value(double m, double s) {
    return s > 0.0 ? m + LogRel<T>::lg(s) : neg_inf();
}

// ln sum_j exp(val(j)) over the states j = j0, j0 + step, ... < S of every thread (-inf: nothing
// finite), the same value in every thread.  Two barriers: the waves' maxima go through
// red[0 .. 7], their sums through red[8 .. 15]; a caller puts one more barrier between two calls.
constexpr int kBlockRed = 16;            // doubles of `red`: 8 waves, twice
template <typename T, typename F>
__device__ __forceinline__ double block_lse(int S, int j0, int step, F val, double* red) {
    const int tid = threadIdx.x, nt_ = blockDim.x;
    const int lane = tid & 63, w = tid >> 6, nw = (nt_ + 63) >> 6;
    double lm = neg_inf();
    for (int j = j0; j < S; j += step) lm = dmax(lm, val(j));
    lm = wave_max(lm);
    if (lane == 0) red[w] = lm;
    __syncthreads();
    double m = red[0];
    for (int i = 1; i < nw; ++i) m = dmax(m, red[i]);
    const double base = m > neg_inf() ? m : 0.0;
    double ls = 0.0;
    for (int j = j0; j < S; j += step) ls += LogRel<T>::ex(val(j) - base);
    ls = wave_sum(ls);
    if (lane == 0) red[kBlockRed / 2 + w] = ls;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[kBlockRed / 2 + i];
    // (written out: through lse_value the fp64 kernels come out with another branch order)
    return s > 0.0 ? base + LogRel<T>::lg(s) : neg_inf();
}
// ... a thread per state, strided beyond the workgroup
template <typename T, typename F>
__device__ __forceinline__ double block_lse(int S, F val, double* red) {
    return block_lse<T>(S, (int)threadIdx.x, (int)blockDim.x, val, red);
}

// Order-preserving keys: a < b as numbers exactly when key(a) < key(b) as signed integers
// (-inf is the smallest key in use; NaN is outside the contract).
template <typename V> struct OrderedKey;
template <> struct OrderedKey<double> {
    using K = long long;
    static __device__ __forceinline__ K key(double v) {
        const K b = __builtin_bit_cast(K, v);
        return b >= 0 ? b : (b ^ 0x7fffffffffffffffLL);
    }
    static __device__ __forceinline__ double val(K k) {
        return __builtin_bit_cast(double, k >= 0 ? k : (k ^ 0x7fffffffffffffffLL));
    }
};
template <> struct OrderedKey<float> {
    using K = int;
    static __device__ __forceinline__ K key(float v) {
        const K b = __builtin_bit_cast(K, v);
        return b >= 0 ? b : (b ^ 0x7fffffff);
    }
    static __device__ __forceinline__ float val(K k) {
        return __builtin_bit_cast(float, k >= 0 ? k : (k ^ 0x7fffffff));
    }
};

// ---------------------------------------------------------------------------
// host side: the plans
// ---------------------------------------------------------------------------
constexpr size_t kBlockArcBytes = 64 * 1024;     // arcs stay in LDS below this total
constexpr size_t kBlockBinRows = 96 * 1024;      // bins are kept in LDS beside rows up to this
constexpr size_t kBlockTeamBytes = 64 * 1024;    // the rows and slots of a workgroup's teams

// What every block kernel asks of a batch (a state index takes 15 bits of what the kernels pack)
inline bool block_batch_ok(int dtype, const beer_batch* b) {
    return b && b->nutt >= 0 && b->max_states >= 1 && b->max_states <= 32767 &&
           b->max_arcs >= 0 && (dtype == BEER_F32 || dtype == BEER_F64);
}
// two fp64 rows of the states and the reduction scratch
inline size_t block_rows_bytes(size_t S) { return (2 * S + kBlockRed) * 8; }
// The largest graph's arc lists in LDS, weights of w bytes: the row pointers, an arc's other end
// (with_cats: and its category) and its weight.  bins_follow: 8-byte values lie behind the
// weights, which then end on 8 bytes.
inline size_t csr_bytes(size_t S, size_t A, size_t w, bool with_cats, bool bins_follow) {
    return (S + 2 + (with_cats ? 2 : 1) * A) * 4 + (A + (bins_follow ? 1 : 0)) * w;
}
// the n with 2^n >= v
inline int ceil_log2(int v) {
    int n = 0;
    while ((1 << n) < v) ++n;
    return n;
}
// The expand launch of the segment kernels: a team of 4 .. `threads` lanes (the power of two that
// covers max_closure) per entry, in LDS doubles_per_row rows of the closure and `slots` doubles
// per team.  false: the teams of a workgroup do not fit `budget`.
inline bool team_plan(int max_closure, int threads, int doubles_per_row, int slots, size_t budget,
                      int* team, int* row, size_t* team_lds) {
    int lanes = 4;
    while (lanes < threads && lanes < max_closure) lanes *= 2;
    *team = lanes;
    *row = max_closure > 1 ? max_closure : 1;
    *team_lds = (size_t)(threads / lanes) * ((size_t)doubles_per_row * (size_t)*row + slots) * 8;
    return *team_lds <= budget;
}

}  // namespace beer
