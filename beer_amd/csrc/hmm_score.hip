// Scoring utterances under an HMM: the forward log-evidence ln p(x_0 .. x_{T-1}), summed over
// all state paths, for every utterance of a ragged batch (include/beer_hip.h:
// beer_hmm_log_evidence).
//
// Definition, over the graph's full in-CSR (hub and bigram arcs included, as Viterbi and the
// path sampler read it):
//     a_0(j) = init_j + l_0(j)
//     a_t(j) = l_t(j) + ln sum_i exp(â_{t-1}(i) + w_ij)
//     c_t    = ln sum_j exp(a_t(j)),        â_t = a_t - c_t
//     frame_evidence[frame_off[u] + t] = c_t                  (= ln p(x_t | x_0 .. x_{t-1}))
//     utt_evidence[u] = sum_t c_t + ln sum_j exp(â_{T-1}(j) + final_j)
// Only the forward pass, and no trellis: the normalised row of the previous frame is all a
// frame needs.  Log space with fp64 arithmetic whatever the storage type (hmm.hip's rule):
// maxima, differences, running sums and the per-utterance sum are fp64, exp / log of a
// difference to the maximum are in the model's precision.  No range flags and no redo path
// outside the kernel.
//
// Edges.  -inf log-likelihoods and unreachable states are legal.  From the first frame at
// which no state is reachable c_t = -inf for the rest of the utterance and so is its total;
// when only the final term is unreachable the frames stay finite and the total is -inf.  No
// NaN comes out of inputs without NaN, and no utterance sees another's values.
//
// Two forms (beer_hmm_evidence_route):
//  * one WAVE per utterance, four utterances per workgroup, for small graphs: a lane keeps
//    the values of its 1, 2 or 4 states in registers, the normalised row and the utterance's
//    OWN arc lists (alignment graphs: every utterance has another graph) sit in the wave's
//    slice of LDS, a frame is normalised by two wave reductions and nothing in the frame loop
//    waits for a workgroup barrier; utterances go to waves longest first (batch->order).
//    The wave works on scaled probabilities and owns the hand-over to log space: an utterance
//    that leaves fp64's range is started again in log space by the same wave (see the kernel);
//  * one WORKGROUP per utterance: four lanes per state on 512 threads while 4 S <= 512, else
//    a thread per state on 256 threads, strided beyond; arc lists in LDS when they fit; three
//    barriers per frame (a state's value is reduced by the thread that computed it).
// Both load the emission row of frame t + 1 during frame t.

#include <limits>

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kEvWaves = 4;              // wave form: utterances (waves) per workgroup
constexpr int kEvWaveStates = 256;       // ... up to four states a lane
constexpr size_t kEvWaveBytes = 16 * 1024;        // ... and this much LDS per wave
constexpr int kEvQuadThreads = 512;      // workgroup form: four lanes per state ...
constexpr int kEvThreads = 256;          // ... or one thread per state (strided beyond)
static_assert(kEvQuadThreads / 64 <= kBlockRed / 2, "a slot per wave in either half");

// ---------------------------------------------------------------------------
// one wave per utterance
// ---------------------------------------------------------------------------
// ln sum over the wave's SPL * 64 values (-inf: nothing finite)
template <typename T, int SPL>
__device__ __forceinline__ double ev_wave_lse(const double (&v)[SPL]) {
    double m = v[0];
#pragma unroll
    for (int p = 1; p < SPL; ++p) m = dmax(m, v[p]);
    m = wave_max(m);
    const double base = m > neg_inf() ? m : 0.0;
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < SPL; ++p) s += LogRel<T>::ex(v[p] - base);
    s = wave_sum(s);
    return lse_value<T>(base, s);
}

// a frame's normaliser below this has left the range in which the scaled recursion is exact
constexpr double kEvMinNorm = 0x1p-800;

// The wave runs an utterance on SCALED PROBABILITIES first (hmm.hip's fb_wave_kernel shows what
// that buys): with q_{t-1} = exp(â_{t-1}) in the row and W = exp(w) on the arcs,
//     r(j) = sum_i q_{t-1}(i) W_ij                    fp64 multiply-adds, no exp on an arc
//     m_t = max of l_t(j) over the states with r(j) > 0
//     q'(j) = r(j) exp(l_t(j) - m_t),  n_t = sum_j q'(j),  c_t = m_t + ln n_t,  q_t = q' / n_t
// -- one exponential per state and frame instead of one or two per arc.  A state whose mass falls
// below 2^-1022 of its frame's total is lost to this recursion; where that shows -- no reachable
// state, n_t below 2^-800 or not finite, a final term below 2^-800, an arc whose W the model's
// type cannot hold -- the wave owns the hand-over: it starts the utterance again in LOG SPACE
// (nothing was stored but the per-frame values, which are rewritten), which is exact for every
// input and says -inf where the answer is -inf.
template <typename T, int SPL>
__global__ __launch_bounds__(64 * kEvWaves) void evidence_wave_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, double* __restrict__ utt_evidence,
    double* __restrict__ frame_evidence, int wave_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.x * kEvWaves + wave;
    if (slot >= b.nutt) return;                           // (no workgroup barrier below)
    const int u = b.order ? __builtin_amdgcn_readfirstlane(b.order[slot]) : slot;
    const beer_graph g = b.graphs[b.graph_id[u]];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u];
    const int64_t T_ = b.frame_off[u + 1] - f0;
    if (T_ <= 0) {
        if (lane == 0) utt_evidence[u] = 0.0;
        return;
    }
    const T* llh = pc_llhs + b.llh_off[u];
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;
    const T* in_w = (const T*)g.in_w;
    // the wave's slice: the normalised row [64 SPL], then the utterance's arc lists
    constexpr int NS = 64 * SPL;
    char* mine = smem + (size_t)wave * wave_stride;
    double* cur = reinterpret_cast<double*>(mine);
    int32_t* l_ptr = reinterpret_cast<int32_t*>(cur + NS);              // [S + 1]
    int32_t* l_src = l_ptr + b.max_states + 1;                          // [A]
    T* l_w = reinterpret_cast<T*>(l_src + b.max_arcs + ((b.max_states + 1 + b.max_arcs) & 1));
    for (int j = lane; j <= S; j += 64) l_ptr[j] = g.in_ptr[j];
    // W = exp(w) in the model's type; an arc it cannot hold (w below the type's smallest normal
    // number) sends the utterance to log space at once
    bool lost = false;
    for (int e = lane; e < A; e += 64) {
        const T w = in_w[e];
        const T W = (T)LinExp<T>::ex((double)w);
        l_src[e] = g.in_src[e];
        l_w[e] = W;
        lost |= (double)w > neg_inf() && !(W >= std::numeric_limits<T>::min());
    }
    const bool scaled = __builtin_amdgcn_ballot_w64(lost) == 0;          // (wave-uniform)
    wave_order();
    // the lane's states j = lane + 64 p (lanes without one carry nothing and an empty arc list)
    bool st[SPL];
    int e0[SPL], e1[SPL];
    T ll_next[SPL];
#pragma unroll
    for (int p = 0; p < SPL; ++p) {
        const int j = lane + 64 * p;
        st[p] = j < S;
        e0[p] = st[p] ? l_ptr[j] : 0;
        e1[p] = st[p] ? l_ptr[j + 1] : 0;
    }
    double* fev = frame_evidence ? frame_evidence + f0 : nullptr;

    // ---- scaled probabilities ----
    if (scaled) {
        double r[SPL], q[SPL];
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            const int j = lane + 64 * p;
            r[p] = st[p] ? LinExp<T>::ex((double)init[j]) : 0.0;
            ll_next[p] = st[p] ? llh[j] : (T)0;
        }
        double total = 0.0;
        bool ok = true;                                     // (wave-uniform)
        for (int64_t t = 0; t < T_; ++t) {
            T ll[SPL];
#pragma unroll
            for (int p = 0; p < SPL; ++p) {
                ll[p] = ll_next[p];
                if (st[p] && t + 1 < T_) ll_next[p] = llh[(t + 1) * S + lane + 64 * p];
            }
            if (t > 0) {
#pragma unroll
                for (int p = 0; p < SPL; ++p) {
                    double acc = 0.0;
                    for (int e = e0[p]; e < e1[p]; ++e) acc += cur[l_src[e]] * (double)l_w[e];
                    r[p] = acc;
                }
                wave_order();                            // the row is read: it may be rewritten
            }
            double m = neg_inf();
#pragma unroll
            for (int p = 0; p < SPL; ++p) m = dmax(m, r[p] > 0.0 ? (double)ll[p] : neg_inf());
            m = wave_max(m);
            if (!(m > neg_inf()) || !(m < __builtin_huge_val())) { ok = false; break; }
            double n = 0.0;
#pragma unroll
            for (int p = 0; p < SPL; ++p) {
                q[p] = r[p] > 0.0 ? r[p] * LinExp<T>::ex((double)ll[p] - m) : 0.0;
                n += q[p];
            }
            n = wave_sum(n);
            if (!(n >= kEvMinNorm) || !(n < __builtin_huge_val())) { ok = false; break; }
            const double c = m + log(n);
            total += c;
            if (fev && lane == 0) fev[t] = c;
            const double inv = 1.0 / n;
#pragma unroll
            for (int p = 0; p < SPL; ++p) {
                q[p] *= inv;
                cur[lane + 64 * p] = q[p];
            }
            wave_order();
        }
        if (ok) {
            double v = 0.0;
#pragma unroll
            for (int p = 0; p < SPL; ++p)
                if (st[p]) v += q[p] * LinExp<T>::ex((double)fin[lane + 64 * p]);
            v = wave_sum(v);
            if (v >= kEvMinNorm && v < __builtin_huge_val()) {
                if (lane == 0) utt_evidence[u] = total + log(v);
                return;
            }
        }
    }

    // ---- the same utterance in log space ----
    for (int e = lane; e < A; e += 64) l_w[e] = in_w[e];
    wave_order();
    double a[SPL];
#pragma unroll
    for (int p = 0; p < SPL; ++p) {
        const int j = lane + 64 * p;
        a[p] = st[p] ? (double)llh[j] + (double)init[j] : neg_inf();
        ll_next[p] = (T)0;
        if (st[p] && T_ > 1) ll_next[p] = llh[S + j];
    }
    double total = 0.0;
    for (int64_t t = 0;; ++t) {
        // a_t is in the registers: c_t, and the normalised row for frame t + 1 and the tail
        const double c = ev_wave_lse<T, SPL>(a);
        const double lz = c > neg_inf() ? c : 0.0;          // nothing reachable: all stay -inf
        total += c;
        if (fev && lane == 0) fev[t] = c;
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            a[p] -= lz;
            cur[lane + 64 * p] = a[p];
        }
        wave_order();
        if (t + 1 >= T_) break;
        T ll_cur[SPL];
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            ll_cur[p] = ll_next[p];
            if (st[p] && t + 2 < T_) ll_next[p] = llh[(t + 2) * S + lane + 64 * p];
        }
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            double m = neg_inf(), s = 0.0;
            for (int e = e0[p]; e < e1[p]; ++e) lse_add<T>(m, s, cur[l_src[e]] + (double)l_w[e]);
            a[p] = st[p] ? (double)ll_cur[p] + lse_value<T>(m, s) : neg_inf();
        }
        wave_order();                                    // the row is read: it may be rewritten
    }
    double v[SPL];
#pragma unroll
    for (int p = 0; p < SPL; ++p) v[p] = st[p] ? a[p] + (double)fin[lane + 64 * p] : neg_inf();
    const double tail = ev_wave_lse<T, SPL>(v);
    if (lane == 0) utt_evidence[u] = total + tail;
}

// ---------------------------------------------------------------------------
// one workgroup per utterance
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kEvQuadThreads) void evidence_block_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, double* __restrict__ utt_evidence,
    double* __restrict__ frame_evidence, int arcs_in_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nt_ = blockDim.x;
    const int u = b.order ? b.order[blockIdx.x] : (int)blockIdx.x;
    const beer_graph g = b.graphs[b.graph_id[u]];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u];
    const int64_t T_ = b.frame_off[u + 1] - f0;
    if (T_ <= 0) {
        if (tid == 0) utt_evidence[u] = 0.0;
        return;
    }
    const T* llh = pc_llhs + b.llh_off[u];
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;
    double* cur = reinterpret_cast<double*>(smem);                     // â_{t-1}
    double* nxt = cur + b.max_states;                                  // a_t
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
    // Four lanes per state when the workgroup has them (a phone start has one arc per phone
    // while most states have two: the longest list sets the time of the step).  A state's
    // value is written to `nxt` and read back for the frame's reductions by ONE thread, its
    // owner -- lane 0 of its four, else thread j mod blockDim: no barrier in between.
    const bool quad = 4 * b.max_states <= nt_;
    const bool one = S <= nt_;
    const int qj = tid >> 2, qp = tid & 3;
    const int j0 = quad ? (qp == 0 ? qj : S) : tid, step = quad ? S : nt_;
    const int pj = quad ? (qp == 0 && qj < S ? qj : -1) : (one && tid < S ? tid : -1);
    for (int j = j0; j < S; j += step) nxt[j] = (double)llh[j] + (double)init[j];
    T ll_next = (T)0;
    if (pj >= 0 && T_ > 1) ll_next = llh[S + pj];
    double total = 0.0;
    double* fev = frame_evidence ? frame_evidence + f0 : nullptr;
    for (int64_t t = 0;; ++t) {
        // (first barrier inside: every thread is done reading `cur`, the arc lists are staged)
        const double c = block_lse<T>(S, j0, step, [&](int j) { return nxt[j]; }, red);
        const double lz = c > neg_inf() ? c : 0.0;          // nothing reachable: all stay -inf
        total += c;
        if (fev && tid == 0) fev[t] = c;
        for (int j = j0; j < S; j += step) cur[j] = nxt[j] - lz;
        __syncthreads();
        if (t + 1 >= T_) break;
        const T ll_cur = ll_next;
        if (pj >= 0 && t + 2 < T_) ll_next = llh[(t + 2) * S + pj];
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
                const double ll = one ? (double)ll_cur : (double)llh[(t + 1) * S + j];
                nxt[j] = ll + lse_value<T>(m, s);
            }
        }
    }
    const double tail = block_lse<T>(S, j0, step,
                                        [&](int j) { return cur[j] + (double)fin[j]; }, red);
    if (tid == 0) utt_evidence[u] = total + tail;
}

// The form of a launch, from the batch maxima (beer_hmm_evidence_route packs it): false where
// the launch refuses -- exactly where beer_hmm_sample_paths refuses a batch.
struct EvidencePlan {
    int spl;                 // wave form: states per lane (1, 2, 4); 0: the workgroup form
    int arcs_in_lds, quad;   // workgroup form
    size_t lds;              // dynamic LDS of the launch
    int wave_stride;         // wave form: bytes of a wave's slice
};
inline bool evidence_plan(int dtype, const beer_batch* b, EvidencePlan* p) {
    if (!block_batch_ok(dtype, b)) return false;
    const size_t S = (size_t)b->max_states, A = (size_t)b->max_arcs;
    const size_t rows = block_rows_bytes(S);
    if (rows > (size_t)kMaxDynLds) return false;
    const size_t arcs = csr_bytes(S, A, dtype == BEER_F32 ? 4 : 8, false, false);
    const int spl = S <= 64 ? 1 : (S <= 128 ? 2 : 4);
    const size_t slice = 8 * 64 * (size_t)spl + arcs;         // the row of a wave and its arcs
    p->spl = 0;
    p->arcs_in_lds = p->quad = 0;
    p->wave_stride = 0;
    if (S <= (size_t)kEvWaveStates && slice <= kEvWaveBytes) {
        p->spl = spl;
        p->wave_stride = (int)((slice + 15) & ~(size_t)15);
        p->lds = (size_t)kEvWaves * p->wave_stride;
        return true;
    }
    p->arcs_in_lds = rows + arcs <= kBlockArcBytes;
    p->quad = 4 * S <= (size_t)kEvQuadThreads;
    p->lds = rows + (p->arcs_in_lds ? arcs : 0);
    return true;
}

template <typename T, int SPL>
int evidence_launch_wave(const beer_batch* b, const EvidencePlan& p, const void* pc_llhs,
                         double* utt_evidence, double* frame_evidence, void* stream) {
    return launch_full_lds(evidence_wave_kernel<T, SPL>, dim3((b->nutt + kEvWaves - 1) / kEvWaves),
                           dim3(64 * kEvWaves), p.lds, as_stream(stream), *b, (const T*)pc_llhs,
                           utt_evidence, frame_evidence, p.wave_stride);
}

template <typename T>
int evidence_launch(const beer_batch* b, const EvidencePlan& p, const void* pc_llhs,
                    double* utt_evidence, double* frame_evidence, void* stream) {
    if (p.spl == 1)
        return evidence_launch_wave<T, 1>(b, p, pc_llhs, utt_evidence, frame_evidence, stream);
    if (p.spl == 2)
        return evidence_launch_wave<T, 2>(b, p, pc_llhs, utt_evidence, frame_evidence, stream);
    if (p.spl == 4)
        return evidence_launch_wave<T, 4>(b, p, pc_llhs, utt_evidence, frame_evidence, stream);
    return launch_full_lds(evidence_block_kernel<T>, dim3(b->nutt),
                           dim3(p.quad ? kEvQuadThreads : kEvThreads), p.lds, as_stream(stream), *b,
                           (const T*)pc_llhs, utt_evidence, frame_evidence, p.arcs_in_lds);
}

}  // namespace

extern "C" {

int beer_hmm_log_evidence(int dtype, const beer_batch* b, const void* pc_llhs,
                          double* utt_evidence, double* frame_evidence, void* stream) {
    EvidencePlan p;
    BEER_REQUIRE(evidence_plan(dtype, b, &p));
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && utt_evidence);
    BEER_DISPATCH(dtype, evidence_launch, b, p, pc_llhs, utt_evidence, frame_evidence, stream);
}

int beer_hmm_evidence_route(int dtype, const beer_batch* b) {
    EvidencePlan p;
    BEER_REQUIRE(evidence_plan(dtype, b, &p));
    if (p.spl) return BEER_EVIDENCE_WAVE | p.spl;
    return BEER_EVIDENCE_BLOCK | (p.arcs_in_lds ? BEER_EVIDENCE_ARCS_LDS : 0) |
           (p.quad ? BEER_EVIDENCE_QUAD : 0);
}

}  // extern "C"
