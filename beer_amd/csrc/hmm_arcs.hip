// Arc posteriors by category: the posterior of every arc at every frame, folded into
// caller-chosen categories and kept per frame, summed per utterance, or both
// (include/beer_hip.h: beer_hmm_arc_posteriors).
//
// One workgroup per utterance, one launch, two passes over the frames.
//  1. Forward, over the graph's full in-CSR (hub and bigram arcs included), exactly the
//     recursion of beer_hmm_log_evidence; the normalised row â_t goes to the trellis in `ws`
//     and the normaliser c_t beside it.  An utterance whose evidence is -inf (a frame with
//     nothing reachable, an unreachable final) gets zeros and stops here.
//  2. Backward, over the full out-CSR.  With
//         d_t(j) = l_t(j) + b_t(j) - c_t               b_t: the normalised backward values,
//         b_{T-1}(j) = final_j - ln sum_k exp(â_{T-1}(k) + final_k)
//     the posterior of arc e = (i -> j) entering frame t is
//         xi_t(e) = exp(â_{t-1}(i) + w_e + d_t(j))
//     a probability, so the exponential needs no maximum: ONE exponential per arc and frame.
//     The same walk over the out-row of i gives its state posterior and its backward value:
//         gamma_{t-1}(i) = sum_e xi_t(e),     b_{t-1}(i) = ln(gamma_{t-1}(i) / G) - â_{t-1}(i)
//     with G = sum_i gamma_{t-1}(i), which is 1 but for rounding: dividing by it keeps the
//     rounding of one frame from drifting into the next (the backward values are not
//     normalised by anything else).  A state whose posterior underflows the model's precision
//     gets b = -inf: what enters it is below that precision too.  Two d rows live in LDS.
//     xi_t(e) is added to bin arc_cat[e] of row t; at t = 1 the walk leaves gamma_0, which is
//     folded by init_cat into row 0 (T = 1: gamma_0 from the final term alone).
//
// Arithmetic: hmm.hip's rule -- sums, differences and the trellis are fp64, exp / log are in
// the model's precision.
//
// Bins.  A frame's bins, and the utterance's, are fp64 in LDS while they fit, summed with the
// LDS's own fp64 add (ds_add_f64): categories are few against arcs and most arcs of the uses
// at hand carry -1, so per-wave partial bins would multiply the LDS by the waves and add a
// reduction per frame for adds that rarely meet.  Beyond LDS the bins are the output rows
// themselves, zeroed by the workgroup first, with global atomic adds.  When a frame's bins are in
// LDS the thread that writes bin c of the row also owns bin c of the utterance's sum: no
// second atomic.  The order of the adds is not fixed: results can differ in the last bits
// from run to run.

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kArcThreads = 256;
constexpr int kArcFrameCats = 1024;              // a frame's bins stay in LDS up to here ...
constexpr int kArcUttCats = 4096;                // ... and the utterance's up to here

struct ArcForm {
    int arcs_in_lds, frame_lds, utt_lds;
};

template <typename T>
__global__ __launch_bounds__(kArcThreads) void arc_posteriors_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, beer_arc_map map, int n_cat,
    double* __restrict__ ws, T* __restrict__ frame_out, double* __restrict__ utt_out,
    ArcForm form) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nt_ = blockDim.x;
    const int u = b.order ? b.order[blockIdx.x] : (int)blockIdx.x;
    const int gid = b.graph_id[u];
    const beer_graph g = b.graphs[gid];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u];
    const int64_t T_ = b.frame_off[u + 1] - f0;
    double* urow = utt_out ? utt_out + (int64_t)u * n_cat : nullptr;
    T* frows = frame_out ? frame_out + f0 * n_cat : nullptr;
    if (T_ <= 0) {
        if (urow)
            for (int c = tid; c < n_cat; c += nt_) urow[c] = 0.0;
        return;
    }
    const T* llh = pc_llhs + b.llh_off[u];
    double* norm = ws + f0;                                            // c_t
    double* alpha = ws + b.frame_off[b.nutt] + b.llh_off[u];           // â_t(j)
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;
    double* cur = reinterpret_cast<double*>(smem);
    double* nxt = cur + b.max_states;
    double* red = nxt + b.max_states;
    int32_t* l_ptr = reinterpret_cast<int32_t*>(red + kBlockRed);      // [S + 1]
    int32_t* l_end = l_ptr + b.max_states + 1;                         // [A] the arc's other end
    int32_t* l_cat = l_end + b.max_arcs;                               // [A] (backward only)
    T* l_w = reinterpret_cast<T*>(l_cat + b.max_arcs + ((b.max_states + 1) & 1));      // [A]
    char* after = form.arcs_in_lds ? reinterpret_cast<char*>(l_w + b.max_arcs + (b.max_arcs & 1))
                                   : reinterpret_cast<char*>(l_ptr);
    double* fbin = reinterpret_cast<double*>(after);                   // [n_cat] a frame's bins
    double* ubin = fbin + (form.frame_lds ? n_cat : 0);                // [n_cat] the utterance's
    const bool u_lds = urow && form.utt_lds;

    // ---- forward: beer_hmm_log_evidence's recursion, the rows kept ----
    const int32_t* a_ptr = g.in_ptr;
    const int32_t* a_end = g.in_src;
    const T* a_w = (const T*)g.in_w;
    if (form.arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.in_ptr[j];
        for (int e = tid; e < A; e += nt_) { l_end[e] = g.in_src[e]; l_w[e] = a_w[e]; }
        a_ptr = l_ptr; a_end = l_end; a_w = l_w;
    }
    for (int j = tid; j < S; j += nt_) nxt[j] = (double)llh[j] + (double)init[j];
    bool dead = false;
    for (int64_t t = 0;; ++t) {
        // (first barrier inside: every thread is done reading `cur`, the arc lists are staged)
        const double c = block_lse<T>(S, [&](int j) { return nxt[j]; }, red);
        dead = !(c > neg_inf());
        if (dead) break;
        if (tid == 0) norm[t] = c;
        for (int j = tid; j < S; j += nt_) {
            const double a = nxt[j] - c;
            cur[j] = a;
            alpha[t * S + j] = a;
        }
        __syncthreads();
        if (t + 1 >= T_) break;
        for (int j = tid; j < S; j += nt_) {
            double m = neg_inf(), s = 0.0;
            for (int e = a_ptr[j]; e < a_ptr[j + 1]; ++e)
                lse_add<T>(m, s, cur[a_end[e]] + (double)a_w[e]);
            nxt[j] = (double)llh[(t + 1) * S + j] + lse_value<T>(m, s);
        }
    }
    double tail = neg_inf();
    if (!dead) {
        tail = block_lse<T>(S, [&](int j) { return cur[j] + (double)fin[j]; }, red);
        dead = !(tail > neg_inf());
    }
    if (dead) {                                            // (the same in every thread)
        if (frows)
            for (int64_t e = tid; e < T_ * n_cat; e += nt_) frows[e] = (T)0;
        if (urow)
            for (int c = tid; c < n_cat; c += nt_) urow[c] = 0.0;
        return;
    }

    // ---- the bins ----
    if (frows && !form.frame_lds) {
        for (int64_t e = tid; e < T_ * n_cat; e += nt_) frows[e] = (T)0;
        __threadfence();
    }
    if (frows && form.frame_lds)
        for (int c = tid; c < n_cat; c += nt_) fbin[c] = 0.0;
    if (urow) {
        if (u_lds) {
            for (int c = tid; c < n_cat; c += nt_) ubin[c] = 0.0;
        } else {
            for (int c = tid; c < n_cat; c += nt_) urow[c] = 0.0;
            __threadfence();
        }
    }
    // an arc's posterior goes to the frame's bin and, unless the row's writer passes it on, to
    // the utterance's
    const bool f_lds = frows && form.frame_lds;
    const bool u_direct = urow && !f_lds;
    T* frow = frows;                                       // row t, set by the loop below
    auto fold = [&](int c, double p) {
        if (c < 0 || !(p > 0.0)) return;
        if (f_lds) atomicAdd(fbin + c, p);
        else if (frows) unsafeAtomicAdd(frow + c, (T)p);
        if (u_direct) {
            if (u_lds) atomicAdd(ubin + c, p);
            else unsafeAtomicAdd(urow + c, p);
        }
    };
    // row t leaves the LDS bins: thread c mod blockDim owns bin c of both sums
    auto flush = [&]() {
        if (!f_lds) return;
        for (int c = tid; c < n_cat; c += nt_) {
            const double v = fbin[c];
            frow[c] = (T)v;
            fbin[c] = 0.0;
            if (urow) {
                if (u_lds) ubin[c] += v;
                else urow[c] += v;
            }
        }
    };

    // ---- backward over the out-CSR ----
    const int32_t* cat = map.arc_cat + map.arc_off[gid];
    const int32_t* icat = map.init_cat + map.state_off[gid];
    a_ptr = g.out_ptr;
    a_end = g.out_dst;
    a_w = (const T*)g.out_w;
    // (`cur` = â_{T-1} was read by the tail above: its second barrier lies behind every read of
    //  the in-CSR, which may now be overwritten)
    if (form.arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.out_ptr[j];
        for (int e = tid; e < A; e += nt_) {
            l_end[e] = g.out_dst[e];
            l_w[e] = a_w[e];
            l_cat[e] = cat[e];
        }
        a_ptr = l_ptr; a_end = l_end; a_w = l_w; cat = l_cat;
    }
    double* dcur = nxt;                                    // d_t, read by the walk
    double* dnxt = cur;                                    // gamma_{t-1}, then d_{t-1}
    if (T_ == 1) {
        // (every thread reads and writes its own states of `cur`)
        for (int j = tid; j < S; j += nt_) dnxt[j] = LogRel<T>::ex(cur[j] + (double)fin[j] - tail);
    } else {
        const double cT = norm[T_ - 1];
        for (int j = tid; j < S; j += nt_)
            dcur[j] = (double)llh[(T_ - 1) * S + j] + (double)fin[j] - tail - cT;
    }
    __syncthreads();
    for (int64_t t = T_ - 1; t >= 1; --t) {
        if (frows) frow = frows + t * n_cat;
        const double* arow = alpha + (t - 1) * S;
        double part = 0.0;
        for (int i = tid; i < S; i += nt_) {
            const double a = arow[i];
            double gam = 0.0;
            if (a > neg_inf()) {
                for (int e = a_ptr[i]; e < a_ptr[i + 1]; ++e) {
                    const double p = LogRel<T>::ex(a + (double)a_w[e] + dcur[a_end[e]]);
                    gam += p;
                    fold(cat[e], p);
                }
            }
            dnxt[i] = gam;
            part += gam;
        }
        double G = block_sum(part, red);                   // (every fold is behind its barriers)
        if (!(G > 0.0) || !(G < __builtin_huge_val())) G = 1.0;
        if (t > 1) {
            const double cp = norm[t - 1];
            for (int i = tid; i < S; i += nt_) {
                const double gam = dnxt[i];
                const double bw = gam > 0.0 ? LogRel<T>::lg(gam / G) - arow[i] : neg_inf();
                dnxt[i] = (double)llh[(t - 1) * S + i] + bw - cp;
            }
        }
        flush();
        __syncthreads();
        double* sw = dcur; dcur = dnxt; dnxt = sw;
    }
    // row 0: gamma_0 by init_cat (T = 1: it is in `dnxt`, else the last swap left it in `dcur`)
    const double* gam0 = T_ == 1 ? dnxt : dcur;
    if (frows) frow = frows;
    for (int j = tid; j < S; j += nt_) fold(icat[j], gam0[j]);
    __syncthreads();
    flush();
    if (u_lds) {
        __syncthreads();
        for (int c = tid; c < n_cat; c += nt_) urow[c] = ubin[c];
    }
}

// The form of a launch, from the batch maxima (beer_hmm_arcs_route packs it): false where the
// launch refuses.
struct ArcPlan {
    ArcForm form;
    size_t lds;              // dynamic LDS of the launch (with_utt: the utterance's bins too)
};
inline bool arc_plan(int dtype, const beer_batch* b, int n_cat, bool want_frames, bool with_utt,
                     ArcPlan* p) {
    if (!block_batch_ok(dtype, b) || n_cat < 1) return false;
    const size_t S = (size_t)b->max_states, A = (size_t)b->max_arcs;
    const size_t rows = block_rows_bytes(S);
    if (rows > (size_t)kMaxDynLds) return false;
    // the out-CSR of the largest graph with its categories (the in-CSR is smaller)
    const size_t arcs = csr_bytes(S, A, dtype == BEER_F32 ? 4 : 8, true, true);
    const size_t bins = 8 * (size_t)n_cat;
    size_t lds = rows;
    p->form.arcs_in_lds = rows + arcs <= kBlockArcBytes;
    if (p->form.arcs_in_lds) lds += arcs;
    // (at most 64 + 8 + 32 KiB with the arcs, 96 + 8 + 32 KiB without: within a CU's LDS)
    const bool room = rows <= kBlockBinRows;
    p->form.frame_lds = want_frames && room && n_cat <= kArcFrameCats;
    if (p->form.frame_lds) lds += bins;
    p->form.utt_lds = room && n_cat <= kArcUttCats;
    if (p->form.utt_lds && with_utt) lds += bins;
    p->lds = lds;
    return true;
}

template <typename T>
int arc_launch(const beer_batch* b, const ArcPlan& p, const void* pc_llhs,
               const beer_arc_map* map, int n_cat, double* ws, void* frame_out, double* utt_out,
               void* stream) {
    return launch_full_lds(arc_posteriors_kernel<T>, dim3(b->nutt), dim3(kArcThreads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, *map, n_cat, ws, (T*)frame_out,
                           utt_out, p.form);
}

}  // namespace

extern "C" {

int beer_hmm_arc_posteriors(int dtype, const beer_batch* b, const void* pc_llhs,
                            const beer_arc_map* map, int n_cat, double* ws, void* frame_out,
                            double* utt_out, void* stream) {
    ArcPlan p;
    BEER_REQUIRE(arc_plan(dtype, b, n_cat, frame_out != nullptr, utt_out != nullptr, &p));
    BEER_REQUIRE(frame_out || utt_out);
    BEER_REQUIRE(map && map->arc_cat && map->init_cat && map->arc_off && map->state_off);
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && ws);
    BEER_DISPATCH(dtype, arc_launch, b, p, pc_llhs, map, n_cat, ws, frame_out, utt_out, stream);
}

size_t beer_hmm_arcs_scratch_doubles(int dtype, const beer_batch* b) {
    // the block form keeps nothing besides the trellis and the normalisers (a batch the launch
    // refuses has no size either)
    (void)dtype;
    (void)b;
    return 0;
}

int beer_hmm_arcs_route(int dtype, const beer_batch* b, int n_cat, int want_frames) {
    ArcPlan p;
    BEER_REQUIRE(arc_plan(dtype, b, n_cat, want_frames != 0, true, &p));
    return BEER_ARCS_BLOCK | (p.form.arcs_in_lds ? BEER_ARCS_ARCS_LDS : 0) |
           (p.form.frame_lds ? BEER_ARCS_FRAME_LDS : 0) | (p.form.utt_lds ? BEER_ARCS_UTT_LDS : 0);
}

}  // extern "C"
