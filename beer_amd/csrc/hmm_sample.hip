// Sampling HMM state paths from the posterior: forward filtering, backward sampling.
//
// Two launches over a ragged batch (include/beer_hip.h: beer_hmm_sample_paths):
//  1. the forward pass, one workgroup per utterance over the graph's full in-CSR (hub
//     arcs included, as Viterbi reads them), in log space with fp64 arithmetic whatever
//     the storage type (hmm.hip's rule); every frame is normalised before it is stored:
//         alpha_ws[llh_off[u] + t*S + j] = ln alpha_t(j) - ln sum_i alpha_t(i)
//     (double, -inf for unreachable states).  Log space: no range flags, no redo path.
//  2. the backward draw, one wave per (utterance, sample): a chain of T dependent steps
//     like Viterbi's back-trace, so nothing inside the chain comes from global memory --
//     the trellis rows and the uniforms are staged into LDS a chunk of frames at a time
//     and the arc lists live in LDS when they fit.
//
// The sampling rule.  Last frame: weights w_j = exp(alpha_{T-1}(j) + final_j) over the
// states; frame t < T-1 given s_{t+1}: w_e = exp(alpha_t(src_e) + in_w_e) over the
// in-arcs of s_{t+1} in CSR order (source ascending).  The chosen term is the first
// whose inclusive running sum exceeds u * total; if rounding leaves none, the last term
// of non-zero weight; a term of weight 0 is never chosen.  total == 0 or not finite (an
// utterance the graph cannot explain): the row's first arc, state 0 at the last frame
// (and state 0 where a row has no arc) -- Viterbi's "all -inf -> 0".  Weights are formed
// relative to the row's largest term, which leaves the ratios as they are.

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kSmpQuadThreads = 512;     // forward pass: four lanes per state ...
constexpr int kSmpThreads = 256;         // ... or one thread per state (strided beyond)
constexpr int kSmpWaves = 4;             // draw: samples of one utterance per workgroup
static_assert(kSmpQuadThreads / 64 <= kBlockRed / 2, "a slot per wave in either half");
constexpr size_t kSmpChunkBytes = 32 * 1024;   // what a chunk of trellis rows may take

// ---------------------------------------------------------------------------
// forward pass
// ---------------------------------------------------------------------------
// nxt -> normalised -> cur and the trellis row `row`
template <typename T>
__device__ __forceinline__ void smp_normalise(int S, const double* nxt, double* cur, double* red,
                                              double* __restrict__ row) {
    const int tid = threadIdx.x, nt_ = blockDim.x;
    const int lane = tid & 63, w = tid >> 6, nw = (nt_ + 63) >> 6;
    __syncthreads();                                   // nxt written, cur read by everyone
    // block_lse's body, kept here: with lz taken from block_lse's value the kernel's code changes.
    // (maxima in red[0 .. 7], sums in red[8 .. 15]: a barrier each, and two more between a
    //  frame's reads and the next frame's writes of either half)
    double lm = neg_inf();
    for (int j = tid; j < S; j += nt_) lm = dmax(lm, nxt[j]);
    lm = wave_max(lm);
    if (lane == 0) red[w] = lm;
    __syncthreads();
    double m = red[0];
    for (int i = 1; i < nw; ++i) m = dmax(m, red[i]);
    const double base = m > neg_inf() ? m : 0.0;
    double ls = 0.0;
    for (int j = tid; j < S; j += nt_) ls += LogRel<T>::ex(nxt[j] - base);
    ls = wave_sum(ls);
    if (lane == 0) red[kBlockRed / 2 + w] = ls;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[kBlockRed / 2 + i];
    const double lz = s > 0.0 ? base + LogRel<T>::lg(s) : 0.0;   // nothing reachable: all stay -inf
    for (int j = tid; j < S; j += nt_) {
        const double a = nxt[j] - lz;
        cur[j] = a;
        row[j] = a;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kSmpQuadThreads) void sample_forward_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, double* __restrict__ alpha_ws, int arcs_in_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int u = blockIdx.x, tid = threadIdx.x, nt_ = blockDim.x;
    const beer_graph g = b.graphs[b.graph_id[u]];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t T_ = b.frame_off[u + 1] - b.frame_off[u];
    if (T_ <= 0) return;
    const T* llh = pc_llhs + b.llh_off[u];
    double* alpha = alpha_ws + b.llh_off[u];
    const T* init = (const T*)g.init;
    double* cur = reinterpret_cast<double*>(smem);
    double* nxt = cur + b.max_states;
    double* red = nxt + b.max_states;
    int32_t* l_ptr = reinterpret_cast<int32_t*>(red + kBlockRed);      // [S + 1]
    int32_t* l_src = l_ptr + b.max_states + 1;                         // [A]
    T* l_w = reinterpret_cast<T*>(l_src + b.max_arcs + ((b.max_states + 1 + b.max_arcs) & 1));
    const int32_t* in_ptr = g.in_ptr;
    const int32_t* in_src = g.in_src;
    const T* in_w = (const T*)g.in_w;
    if (arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.in_ptr[j];
        for (int e = tid; e < A; e += nt_) { l_src[e] = g.in_src[e]; l_w[e] = in_w[e]; }
        in_ptr = l_ptr; in_src = l_src; in_w = l_w;
    }
    for (int j = tid; j < S; j += nt_) nxt[j] = (double)llh[j] + (double)init[j];
    smp_normalise<T>(S, nxt, cur, red, alpha);
    // four lanes per state when the workgroup has them (a phone start has one arc per
    // phone while most states have two: the longest list sets the time of the step), the
    // emission row of frame t + 1 loaded during frame t
    const bool quad = 4 * b.max_states <= nt_;
    const bool one = S <= nt_;
    const int qj = tid >> 2, qp = tid & 3;
    const int pj = quad ? (qp == 0 && qj < S ? qj : -1) : (one && tid < S ? tid : -1);
    T ll_next = (T)0;
    if (pj >= 0 && T_ > 1) ll_next = llh[S + pj];
    for (int64_t t = 1; t < T_; ++t) {
        const T ll_cur = ll_next;
        if (pj >= 0 && t + 1 < T_) ll_next = llh[(t + 1) * S + pj];
        if (quad) {
            const int e0 = qj < S ? in_ptr[qj] + qp : 0, e1 = qj < S ? in_ptr[qj + 1] : 0;
            double m = neg_inf(), s = 0.0;
            for (int e = e0; e < e1; e += 4) lse_add<T>(m, s, cur[in_src[e]] + (double)in_w[e]);
            lse_join<T>(m, s, wave_detail::dpp<double, 0xB1>(m), wave_detail::dpp<double, 0xB1>(s));
            lse_join<T>(m, s, wave_detail::dpp<double, 0x4E>(m), wave_detail::dpp<double, 0x4E>(s));
            if (pj >= 0) nxt[qj] = (double)ll_cur + lse_value<T>(m, s);
        } else {
            for (int j = tid; j < S; j += nt_) {
                double m = neg_inf(), s = 0.0;
                for (int e = in_ptr[j]; e < in_ptr[j + 1]; ++e)
                    lse_add<T>(m, s, cur[in_src[e]] + (double)in_w[e]);
                const double ll = one ? (double)ll_cur : (double)llh[t * S + j];
                nxt[j] = ll + lse_value<T>(m, s);
            }
        }
        smp_normalise<T>(S, nxt, cur, red, alpha + t * S);
    }
}

// ---------------------------------------------------------------------------
// backward draw
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_incl_scan(double x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// Index in [0, n) of the term drawn by `uu` among the n log-weights term(0..n-1), by the rule
// in this file's header; the same value in every lane of the wave.  Rows of at most BEER_SEG
// terms are scanned by every lane on its own (in CSR order, as a sequential sum), longer ones
// by the wave: lanes take terms, a prefix sum runs over the wave and a ballot finds the first
// lane over the target.
template <typename T, typename F>
__device__ __forceinline__ int smp_pick(int n, F term, double uu, int lane) {
    if (n <= BEER_SEG) {
        double v[BEER_SEG];
        double m = neg_inf();
#pragma unroll
        for (int i = 0; i < BEER_SEG; ++i) {
            v[i] = i < n ? term(i) : neg_inf();
            m = dmax(m, v[i]);
        }
        if (!(m > neg_inf())) return 0;
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < BEER_SEG; ++i) {
            v[i] = LogRel<T>::ex(v[i] - m);
            tot += v[i];
        }
        if (!(tot > 0.0) || !(tot < __builtin_huge_val())) return 0;
        const double target = uu * tot;
        double c = 0.0;
        int hit = -1, last = 0;
#pragma unroll
        for (int i = 0; i < BEER_SEG; ++i) {
            c += v[i];
            if (v[i] > 0.0) {
                last = i;
                if (hit < 0 && c > target) hit = i;
            }
        }
        return hit >= 0 ? hit : last;
    }
    double m = neg_inf();
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        if (i < n) m = dmax(m, term(i));
    }
    m = wave_max(m);
    if (!(m > neg_inf())) return 0;
    double tot = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        if (i < n) tot += LogRel<T>::ex(term(i) - m);
    }
    tot = wave_sum(tot);
    if (!(tot > 0.0) || !(tot < __builtin_huge_val())) return 0;
    const double target = uu * tot;
    double carry = 0.0;
    int last = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const double x = i < n ? LogRel<T>::ex(term(i) - m) : 0.0;
        const double incl = carry + wave_incl_scan(x, lane);
        const unsigned long long nz = __builtin_amdgcn_ballot_w64(x > 0.0);
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(x > 0.0 && incl > target);
        if (hit) return base + __builtin_ctzll(hit);
        if (nz) last = base + 63 - __builtin_clzll(nz);
        carry = __shfl(incl, 63);
    }
    return last;
}

template <typename T>
__global__ __launch_bounds__(64 * kSmpWaves) void sample_draw_kernel(
    beer_batch b, const double* __restrict__ alpha_ws, const double* __restrict__ uniforms,
    int nsamples, int64_t* __restrict__ path, int map_pdf, int arcs_in_lds, int chunk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int u = blockIdx.x, tid = threadIdx.x, nt_ = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nt_ >> 6;
    const int gid = b.graph_id[u];
    const beer_graph g = b.graphs[gid];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u], T_ = b.frame_off[u + 1] - f0;
    const int64_t n_frames = b.frame_off[b.nutt];
    if (T_ <= 0) return;
    const double* alpha = alpha_ws + b.llh_off[u];
    const T* fin = (const T*)g.final;
    double* rows = reinterpret_cast<double*>(smem);                    // [chunk][S]
    double* uni = rows + (size_t)chunk * b.max_states;                 // [kSmpWaves][chunk]
    int32_t* l_ptr = reinterpret_cast<int32_t*>(uni + kSmpWaves * chunk);
    int32_t* l_src = l_ptr + b.max_states + 1;
    T* l_w = reinterpret_cast<T*>(l_src + b.max_arcs + ((b.max_states + 1 + b.max_arcs) & 1));
    const int32_t* in_ptr = g.in_ptr;
    const int32_t* in_src = g.in_src;
    const T* in_w = (const T*)g.in_w;
    if (arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.in_ptr[j];
        for (int e = tid; e < A; e += nt_) { l_src[e] = g.in_src[e]; l_w[e] = in_w[e]; }
        in_ptr = l_ptr; in_src = l_src; in_w = l_w;
    }
    const int k = blockIdx.y * nw + wave;                   // this wave's sample
    const bool active = k < nsamples;
    const int32_t* ids = b.pdf_ids + b.pdf_off[gid];
    int64_t* out = path + (active ? (int64_t)k * n_frames + f0 : 0);
    int st = 0;
    for (int64_t hi = T_ - 1; hi >= 0; hi -= chunk) {
        const int64_t lo = hi - chunk + 1 > 0 ? hi - chunk + 1 : 0;    // frames lo .. hi
        const int len = (int)(hi - lo + 1);
        __syncthreads();                                    // arcs staged / previous chunk done
        for (int64_t e = tid; e < (int64_t)len * S; e += nt_) rows[e] = alpha[lo * S + e];
        for (int e = tid; e < nw * len; e += nt_) {
            const int w_ = e / len, i = e - w_ * len;
            const int kk = blockIdx.y * nw + w_;
            uni[w_ * chunk + i] = kk < nsamples ? uniforms[(int64_t)kk * n_frames + f0 + lo + i] : 0.0;
        }
        __syncthreads();
        if (!active) continue;
        for (int64_t t = hi; t >= lo; --t) {
            const double* row = rows + (size_t)(t - lo) * S;
            const double uu = uni[wave * chunk + (int)(t - lo)];
            if (t == T_ - 1) {
                st = smp_pick<T>(S, [&](int j) { return row[j] + (double)fin[j]; }, uu, lane);
            } else {
                const int e0 = in_ptr[st], n = in_ptr[st + 1] - e0;
                st = n > 0 ? in_src[e0 + smp_pick<T>(n, [&](int i) {
                                 return row[in_src[e0 + i]] + (double)in_w[e0 + i]; }, uu, lane)]
                           : 0;
            }
            if (lane == 0) out[t] = map_pdf ? (int64_t)ids[st] : (int64_t)st;
        }
    }
}

// The forms of a launch, from the batch maxima (beer_hmm_sample_route packs them): false
// where the launch refuses.
struct SamplePlan {
    int chunk, arcs_in_lds, quad, waves;
    size_t fwd_lds, draw_lds;
};
inline bool sample_plan(int dtype, const beer_batch* b, int32_t nsamples, SamplePlan* p) {
    if (!block_batch_ok(dtype, b) || nsamples < 1) return false;
    const size_t S = (size_t)b->max_states, A = (size_t)b->max_arcs;
    const size_t row = 8 * S + 8 * kSmpWaves;                 // a trellis row and its uniforms
    p->chunk = 32 * row <= kSmpChunkBytes ? 32 : (8 * row <= kSmpChunkBytes ? 8 : 2);
    const size_t fwd = block_rows_bytes(S), draw = p->chunk * row;
    const size_t arcs = csr_bytes(S, A, dtype == BEER_F32 ? 4 : 8, false, false);
    const size_t base = fwd > draw ? fwd : draw;
    if (base > (size_t)kMaxDynLds) return false;
    p->arcs_in_lds = base + arcs <= kBlockArcBytes;
    p->quad = 4 * S <= (size_t)kSmpQuadThreads;
    p->waves = nsamples == 1 ? 1 : kSmpWaves;
    if ((nsamples + p->waves - 1) / p->waves > 65535) return false;
    p->fwd_lds = fwd + (p->arcs_in_lds ? arcs : 0);
    p->draw_lds = draw + (p->arcs_in_lds ? arcs : 0);
    return true;
}

template <typename T>
int sample_launch(const beer_batch* b, const SamplePlan& p, const void* pc_llhs,
                  const double* uniforms, int32_t nsamples, double* alpha_ws, int64_t* path,
                  int map_pdf, void* stream) {
    const int rc = launch_full_lds(sample_forward_kernel<T>, dim3(b->nutt),
                                   dim3(p.quad ? kSmpQuadThreads : kSmpThreads), p.fwd_lds,
                                   as_stream(stream), *b, (const T*)pc_llhs, alpha_ws,
                                   p.arcs_in_lds);
    if (rc != BEER_OK) return rc;
    return launch_full_lds(sample_draw_kernel<T>,
                           dim3(b->nutt, (unsigned)((nsamples + p.waves - 1) / p.waves)),
                           dim3(64 * p.waves), p.draw_lds, as_stream(stream), *b, alpha_ws,
                           uniforms, nsamples, path, map_pdf, p.arcs_in_lds, p.chunk);
}

}  // namespace

extern "C" {

int beer_hmm_sample_paths(int dtype, const beer_batch* b, const void* pc_llhs,
                          const double* uniforms, int32_t nsamples, double* alpha_ws,
                          int64_t* path, int map_pdf, void* stream) {
    SamplePlan p;
    BEER_REQUIRE(sample_plan(dtype, b, nsamples, &p));
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && uniforms && alpha_ws && path);
    BEER_DISPATCH(dtype, sample_launch, b, p, pc_llhs, uniforms, nsamples, alpha_ws, path, map_pdf,
                  stream);
}

int beer_hmm_sample_route(int dtype, const beer_batch* b, int32_t nsamples) {
    SamplePlan p;
    BEER_REQUIRE(sample_plan(dtype, b, nsamples, &p));
    return p.chunk | (p.arcs_in_lds ? BEER_SAMPLE_ARCS_LDS : 0) | (p.quad ? BEER_SAMPLE_QUAD : 0) |
           p.waves << 12;
}

}  // extern "C"
