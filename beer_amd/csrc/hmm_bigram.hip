// Forward-backward of a phone loop with a BIGRAM language model: one launch per
// sub-batch does the pdf-id gather (with the acoustic scale), the recursions, the
// scatter of the posteriors to pdf ids and the per-utterance sum_t sum_s gamma * l,
// and leaves behind what the bigram counts are reduced from.
//
// A bigram loop's end -> start block is a full P x P matrix,
//     trans[end_i, start_j] = ln(1 - loop_i) + E[ln w][i, j]
// (beer/models/phoneloop.py:147-156), so the hub of the unigram loop's one-wave kernel
// (hmm.hip: fb_wave_kernel) does not apply.  Here the block is a dense matrix
// W = exp(block) kept ONCE per workgroup in LDS and shared by its waves (one wave per
// utterance: a free loop has one graph for every utterance); what is left of the
// graph (self-loops, the arcs inside a phone) is a low-degree CSR held in registers.
// The numerics are those of fb_wave_kernel: scaled linear domain, the column brought
// back to [1/2, 1) by a power of two every frame, fp64 trellis, one exponential per
// state, frame and direction.  Per frame the block is a matrix-vector product:
//
//   forward:   entry_t[j] = sum_i a_{t-1}(src_i) W[i, j]
//   backward:  exit_t[i]  = sum_j W[i, j] lb_{t+1}(dst_j),     lb = b beta
//
// The transition posteriors of the block, xi_t(src_i -> dst_j) =
// u_t(i) W[i, j] v_t(j) with u_t = a_t(src) / n_t (n_t the frame's normaliser) and
// v_t = lb_{t+1}(dst), are not summed here: the kernel streams u_t and v_t (P doubles
// each per frame) to a workspace, and the caller reduces C = W o (U^T V) with one GEMM
// -- a wave cannot hold a P x P accumulator, and the LDS already holds W.
//
// An utterance whose column or normaliser leaves fp64's range (see fb_wave_kernel:
// 2^-800) is FLAGGED and adds nothing; the caller then redoes the sub-batch on the
// general log-space path.
//
// Reference restated: beer/graph.py:270-326, beer/models/hmm.py:73-95,
// beer/models/phoneloop.py:104-191.

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kBgMaxPhones = 128;      // BEER_BIGRAM_MAX_PHONES
constexpr int kBgMaxStates = 512;      // BEER_BIGRAM_MAX_STATES
constexpr int kBgMaxWaves = 8;         // waves (utterances) per workgroup
constexpr int kBgVec = kBgMaxPhones;   // doubles of one block vector per wave

// W is kept in fp64 for float models too: a bigram prior with concentrations 1 / P
// (mkphoneloopbigram's dirichlet2) puts every block entry near -P, below float's range
// (exp(-104) is 0 in float), while fp64 holds it down to -745.  At the recipe's P = 100 the
// 80 KiB of W and eight waves' columns still fit one workgroup per CU.
// LDS layout (doubles): W [P][ldw] in the weight type WT, then per wave
// cur[NS] lb[NS] vin[kBgVec] vout[kBgVec]
template <typename WT>
__host__ __device__ inline size_t bg_w_bytes(int P) {
    return ((size_t)P * (size_t)(P + 1) * sizeof(WT) + 15) & ~(size_t)15;
}
__host__ __device__ inline int bg_wave_doubles(int ns) { return 2 * ns + 2 * kBgVec; }

// The launch shape, shared by the launcher and beer_hmm_bigram_route (host only).
// States per lane (5: the recipe's 100 phones of 3 states)
inline int bg_spl(int S) { return S <= 64 ? 1 : (S <= 128 ? 2 : (S <= 256 ? 4 : (S <= 320 ? 5 : 8))); }
// Residual arcs of a state unrolled per side
inline int bg_deg(int max_degree) { return max_degree <= 2 ? 2 : (max_degree <= 4 ? 4 : 8); }
// Waves whose columns fit the LDS behind W (0: not even one)
template <typename WT>
inline int bg_lds_waves(int P, int spl) {
    const size_t wbytes = bg_w_bytes<WT>(P);
    const size_t per_wave = (size_t)bg_wave_doubles(64 * spl) * sizeof(double);
    if (wbytes + per_wave > (size_t)kMaxDynLds) return 0;
    return (int)(((size_t)kMaxDynLds - wbytes) / per_wave);
}
// n_cu <= 0: the current device's CUs, 256 if it cannot be asked
inline int bg_n_cu(int n_cu) {
    if (n_cu > 0) return n_cu;
    int dev = 0;
    n_cu = 256;
    if (hipGetDevice(&dev) == hipSuccess)
        (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    return n_cu;
}
// Waves per workgroup: enough workgroups to spread the utterances over the CUs, as many waves
// as the LDS allows (`room`, at most kBgMaxWaves) to share one copy of W
inline int bg_waves(int room, int32_t nutt, int n_cu) {
    const int want = (nutt + n_cu - 1) / (n_cu > 0 ? n_cu : 1);
    const int waves = room < kBgMaxWaves ? room : kBgMaxWaves;
    return want < waves ? (want > 0 ? want : 1) : waves;
}

template <typename T, typename WT, int SPL, int DEG>
__global__ __launch_bounds__(64 * kBgMaxWaves) void fb_bigram_kernel(
    beer_bigram g, int32_t nutt, int64_t n_frames, const int64_t* __restrict__ frame_off,
    const int32_t* __restrict__ order, int S_total, const T* __restrict__ pc, T scale,
    double* __restrict__ alpha_ws, double* __restrict__ uv_ws, T* __restrict__ out,
    int atomic_out, double* __restrict__ utt_llh, int32_t* __restrict__ flags) {
    typedef LinExp<T> R;
    constexpr int NS = 64 * SPL;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int P = g.n_phones, S = g.n_states, ldw = P + 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;

    // ---- W = exp(block) into LDS, once for the workgroup ----
    WT* Wl = reinterpret_cast<WT*>(smem);
    {
        const T* bw = (const T*)g.block_w;
        for (int e = threadIdx.x; e < P * P; e += blockDim.x) {
            const int i = e / P, j = e - i * P;
            Wl[i * ldw + j] = (WT)exp((double)bw[e]);
        }
    }
    __syncthreads();                                      // (the only workgroup barrier)
    const int slot = blockIdx.x * n_waves + wave;
    if (slot >= nutt) return;
    const int u = order ? __builtin_amdgcn_readfirstlane(order[slot]) : slot;
    const int64_t f0 = frame_off[u];
    const int T_ = __builtin_amdgcn_readfirstlane((int)(frame_off[u + 1] - f0));
    if (T_ <= 0) {
        if (lane == 0) { flags[u] = 0; utt_llh[u] = 0.0; }
        return;
    }

    double* wl = reinterpret_cast<double*>(smem + bg_w_bytes<WT>(P)) + wave * bg_wave_doubles(NS);
    double* cur = wl;                 // a_t (forward), a_t / n_t (backward)
    double* lb = wl + NS;             // b_{t+1} beta_{t+1}
    double* vin = wl + 2 * NS;        // the block's input vector
    double* vout = vin + kBgVec;      // the block's output vector

    const T* in_w = (const T*)g.in_w;
    const T* out_w = (const T*)g.out_w;
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;

    // ---- the lane's states (lanes without one: weights 0, the zero slot) ----
    int isrc[SPL][DEG], odst[SPL][DEG], ent[SPL], ext[SPL], id[SPL];
    double iw[SPL][DEG], ow[SPL][DEG], fin_w[SPL];
    bool st[SPL];
#pragma unroll
    for (int p = 0; p < SPL; ++p) {
        const int j = lane + 64 * p;
        st[p] = j < S;
        int ib = 0, ie = 0, ob = 0, oe = 0;
        fin_w[p] = 0.0;
        ent[p] = ext[p] = -1;
        id[p] = 0;
        if (st[p]) {
            ib = g.in_ptr[j]; ie = g.in_ptr[j + 1];
            ob = g.out_ptr[j]; oe = g.out_ptr[j + 1];
            fin_w[p] = exp((double)fin[j]);
            ent[p] = g.dst_slot[j];
            ext[p] = g.src_slot[j];
            id[p] = g.pdf_ids[j];
        }
#pragma unroll
        for (int k = 0; k < DEG; ++k) {
            const bool a = ib + k < ie, o = ob + k < oe;
            isrc[p][k] = a ? g.in_src[ib + k] : -1;
            iw[p][k] = a ? exp((double)in_w[ib + k]) : 0.0;
            odst[p][k] = o ? g.out_dst[ob + k] : -1;
            ow[p][k] = o ? exp((double)out_w[ob + k]) : 0.0;
        }
    }
    // the lane's block members: q = lane, lane + 64
    int bsrc[2], bdst[2];
    bool bq[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int q = lane + 64 * c;
        bq[c] = q < P;
        bsrc[c] = bq[c] ? g.src[q] : 0;
        bdst[c] = bq[c] ? g.dst[q] : 0;
    }
    auto col = [&](const double* v, int s) -> double { return s >= 0 ? v[s] : 0.0; };
    auto slot_of = [&](const double* v, int q) -> double { return q >= 0 ? v[q] : 0.0; };
    // vout[q'] = sum_i vin[i] W[i, q']  (forward)  or  sum_j W[q', j] vin[j]  (backward)
    auto block_product = [&](bool transpose) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int q = lane + 64 * c;
            double acc = 0.0;
            if (bq[c]) {
                if (!transpose) {
                    for (int i = 0; i < P; ++i) acc = __builtin_fma(vin[i], (double)Wl[i * ldw + q], acc);
                } else {
                    const WT* row = Wl + q * ldw;
                    for (int j = 0; j < P; ++j) acc = __builtin_fma((double)row[j], vin[j], acc);
                }
                vout[q] = acc;
            }
        }
    };
    bool gave_up = false;
    auto rescale = [&](double (&v)[SPL]) {
        int e = 0;
#pragma unroll
        for (int p = 0; p < SPL; ++p) { const int ep = expo_field(v[p]); e = ep > e ? ep : e; }
        e = wave_max(e);
        gave_up |= e < 1023 - 800 || e >= 0x7ff;
        const int sh = (e > 0 && e < 0x7ff) ? 1022 - e : 0;
#pragma unroll
        for (int p = 0; p < SPL; ++p) v[p] = __builtin_amdgcn_ldexp(v[p], sh);
    };
    const T* llh = pc + f0 * (int64_t)S_total;
    auto load_ll = [&](int t, T (&l)[SPL]) -> double {
        float m = -INFINITY;
        bool bad = false;
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            l[p] = st[p] ? scale * llh[(int64_t)t * S_total + id[p]] : (T)0;
            if (st[p]) {
                m = __builtin_fmaxf(m, (float)l[p]);
                bad |= l[p] != l[p];
            }
        }
        m = wave_max(m);
        gave_up |= __builtin_amdgcn_ballot_w64(bad) != 0;
        return m > -INFINITY && m < INFINITY ? (double)m : 0.0;
    };
    double* alpha = alpha_ws + f0 * (int64_t)S;

    // ---- forward ----
    {
        T l[SPL];
        double a[SPL], l0[SPL];
        float m = -INFINITY;
        (void)load_ll(0, l);
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            l0[p] = st[p] ? (double)l[p] + (double)init[lane + 64 * p] : neg_inf();
            m = __builtin_fmaxf(m, (float)l0[p]);
        }
        m = wave_max(m);
        const double m0 = m > -INFINITY && m < INFINITY ? (double)m : 0.0;
#pragma unroll
        for (int p = 0; p < SPL; ++p) a[p] = st[p] ? R::ex(l0[p] - m0) : 0.0;
        rescale(a);
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            if (st[p]) {
                cur[lane + 64 * p] = a[p];
                alpha[lane + 64 * p] = a[p];
            }
        }
    }
    wave_order();
    for (int t = 1; t < T_; ++t) {
        T l[SPL];
        const double mt = load_ll(t, l);
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (bq[c]) vin[lane + 64 * c] = cur[bsrc[c]];
        wave_order();
        block_product(false);
        wave_order();
        double a[SPL];
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            double pred = slot_of(vout, ent[p]);
#pragma unroll
            for (int k = 0; k < DEG; ++k) pred = __builtin_fma(col(cur, isrc[p][k]), iw[p][k], pred);
            a[p] = st[p] ? R::ex((double)l[p] - mt) * pred : 0.0;
        }
        rescale(a);
        wave_order();                                // every read of the column is done
        double* at = alpha + (int64_t)t * S;
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            if (st[p]) {
                cur[lane + 64 * p] = a[p];
                at[lane + 64 * p] = a[p];
            }
        }
        wave_order();
    }

    // ---- backward + posteriors ----
    double llh_acc = 0.0;
    double* uv_u = uv_ws + f0 * (int64_t)P;               // U [n_frames, P]
    double* uv_v = uv_ws + (n_frames + f0) * (int64_t)P;  // V [n_frames, P] behind it
    for (int t = T_ - 1; t >= 0; --t) {
        T l[SPL];
        const double mt = load_ll(t, l);
        const bool inner = t < T_ - 1;
        double beta[SPL];
        if (inner) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (bq[c]) {
                    const double v = lb[bdst[c]];
                    vin[lane + 64 * c] = v;
                    uv_v[(int64_t)t * P + lane + 64 * c] = v;
                }
            }
            wave_order();
            block_product(true);
            wave_order();
#pragma unroll
            for (int p = 0; p < SPL; ++p) {
                double acc = slot_of(vout, ext[p]);
#pragma unroll
                for (int k = 0; k < DEG; ++k) acc = __builtin_fma(col(lb, odst[p][k]), ow[p][k], acc);
                beta[p] = st[p] ? acc : 0.0;
            }
        } else {
#pragma unroll
            for (int p = 0; p < SPL; ++p) beta[p] = fin_w[p];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (bq[c]) {
                    uv_u[(int64_t)t * P + lane + 64 * c] = 0.0;
                    uv_v[(int64_t)t * P + lane + 64 * c] = 0.0;
                }
            }
        }
        const double* at = alpha + (int64_t)t * S;
        double a_cur[SPL], gsum = 0.0;
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            a_cur[p] = st[p] ? at[lane + 64 * p] : 0.0;
            gsum += a_cur[p] * beta[p];
        }
        const double norm = wave_sum(gsum);
        gave_up |= !(norm >= 0x1p-800 && norm < __builtin_huge_val());
        const double inv = 1.0 / norm;
        T* orow = out + (f0 + t) * (int64_t)S_total;
#pragma unroll
        for (int p = 0; p < SPL; ++p) {
            if (!st[p]) continue;
            const T gv = (T)(a_cur[p] * beta[p] * inv);
            if (atomic_out) atomicAdd(orow + id[p], scale * gv);
            else orow[id[p]] = scale * gv;
            llh_acc += (double)(l[p] * gv);
        }
        if (inner) {
            // u_t = a_t(src) / n_t, through the (now free) forward column
            wave_order();
#pragma unroll
            for (int p = 0; p < SPL; ++p)
                if (st[p]) cur[lane + 64 * p] = a_cur[p] * inv;
            wave_order();
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (bq[c]) uv_u[(int64_t)t * P + lane + 64 * c] = cur[bsrc[c]];
        }
        if (t > 0) {
            rescale(beta);
            wave_order();                            // lb fully read
#pragma unroll
            for (int p = 0; p < SPL; ++p)
                if (st[p]) lb[lane + 64 * p] = R::ex((double)l[p] - mt) * beta[p];
            wave_order();
        }
    }
    llh_acc = wave_sum(llh_acc);
    if (lane == 0) {
        flags[u] = gave_up ? 1 : 0;
        utt_llh[u] = gave_up ? 0.0 : llh_acc;
    }
}

template <typename T, typename WT>
int bigram_launch(const beer_bigram* g, int32_t nutt, int64_t n_frames, const int64_t* frame_off,
                  const int32_t* order, int S_total, const void* pc_all, double scale,
                  double* alpha_ws, double* uv_ws, void* out, int atomic_out, double* utt_llh,
                  int32_t* flags, hipStream_t s) {
    const int spl = bg_spl(g->n_states), deg = bg_deg(g->max_degree);
    const int room = bg_lds_waves<WT>(g->n_phones, spl);
    if (room < 1) return BEER_EINVAL;
    const int waves = bg_waves(room, nutt, bg_n_cu(0));
    const size_t wbytes = bg_w_bytes<WT>(g->n_phones);
    const size_t per_wave = (size_t)bg_wave_doubles(64 * spl) * sizeof(double);
    const size_t lds = wbytes + (size_t)waves * per_wave;
    const dim3 grid((unsigned)((nutt + waves - 1) / waves)), block(64 * waves);
#define BEER_BG(SPL_, DEG_)                                                                      \
    return launch_full_lds(fb_bigram_kernel<T, WT, SPL_, DEG_>, grid, block, lds, s, *g, nutt,   \
                           n_frames, frame_off, order, S_total, (const T*)pc_all, (T)scale,      \
                           alpha_ws, uv_ws, (T*)out, atomic_out, utt_llh, flags)
#define BEER_BG_DEG(SPL_)                                                                        \
    do {                                                                                         \
        if (deg == 2) BEER_BG(SPL_, 2);                                                          \
        if (deg == 4) BEER_BG(SPL_, 4);                                                          \
        BEER_BG(SPL_, 8);                                                                        \
    } while (0)
    if (spl == 1) BEER_BG_DEG(1);
    if (spl == 2) BEER_BG_DEG(2);
    if (spl == 4) BEER_BG_DEG(4);
    if (spl == 5) BEER_BG_DEG(5);
    BEER_BG_DEG(8);
#undef BEER_BG_DEG
#undef BEER_BG
}

// What both entry points ask of the descriptor
inline bool bigram_graph_ok(int dtype, const beer_bigram* g, int32_t nutt) {
    return g && nutt >= 0 && (dtype == BEER_F32 || dtype == BEER_F64) &&
           g->n_states >= 1 && g->n_states <= kBgMaxStates &&
           g->n_phones >= 1 && g->n_phones <= kBgMaxPhones &&
           g->max_degree >= 0 && g->max_degree <= BEER_SEG;
}

}  // namespace

extern "C" {

int beer_hmm_posteriors_bigram(int dtype, const beer_bigram* g, int32_t nutt,
                               int64_t n_frames, const int64_t* frame_off, const int32_t* order, int S_total,
                               const void* pc_all, double scale, double* alpha_ws,
                               double* uv_ws, void* state_resps, int atomic_out,
                               double* utt_llh, int32_t* flags, void* stream) {
    BEER_REQUIRE(bigram_graph_ok(dtype, g, nutt) && S_total >= 1);
    BEER_REQUIRE(n_frames >= 0);
    if (nutt == 0) return BEER_OK;
    BEER_REQUIRE(frame_off && pc_all && alpha_ws && uv_ws && state_resps && utt_llh && flags);
    hipStream_t s = as_stream(stream);
    if (dtype == BEER_F32)
        return bigram_launch<float, double>(g, nutt, n_frames, frame_off, order, S_total, pc_all, scale,
                                           alpha_ws, uv_ws, state_resps, atomic_out, utt_llh,
                                           flags, s);
    return bigram_launch<double, double>(g, nutt, n_frames, frame_off, order, S_total, pc_all, scale,
                                         alpha_ws, uv_ws, state_resps, atomic_out, utt_llh,
                                         flags, s);
}

int beer_hmm_bigram_route(int dtype, const beer_bigram* g, int32_t nutt, int32_t n_cu) {
    BEER_REQUIRE(bigram_graph_ok(dtype, g, nutt));
    // (W is fp64 for either dtype)
    const int spl = bg_spl(g->n_states);
    const int room = bg_lds_waves<double>(g->n_phones, spl);
    BEER_REQUIRE(room >= 1);
    return spl | bg_deg(g->max_degree) << 8 | bg_waves(room, nutt, bg_n_cu(n_cu)) << 16;
}

}  // extern "C"
