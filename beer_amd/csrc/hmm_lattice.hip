// Viterbi max-marginals: for every frame and state (and every arc, folded into caller-chosen
// categories) the score of the best path forced through it, relative to the Viterbi score
// (include/beer_hip.h: beer_hmm_max_marginals).
//
// One workgroup per utterance, one launch, two max-plus passes over the frames, a thread per
// state (strided beyond the workgroup).  No exponential, no logarithm: every value is an fp64
// sum of inputs, every fold a maximum.
//  1. Forward, over the graph's full in-CSR (hub and bigram arcs included):
//         d_0(j) = l_0(j) + init_j,     d_t(j) = max_i (d_{t-1}(i) + w_ij) + l_t(j)
//     every row goes to the trellis in `ws`; best = max_j (d_{T-1}(j) + final_j).  An utterance
//     whose best is -inf gets -inf everywhere and stops here.
//  2. Backward, over the full out-CSR.  Two fp64 rows live in LDS: e_t and l_t.  The thread of
//     source i walks its out-row once per frame; the same walk gives
//         e_{t-1}(i) = max_j (w_ij + (l_t(j) + e_t(j)))
//         am_t(i->j) = (((d_{t-1}(i) + w_ij) + l_t(j)) + e_t(j)) - best     -> bin arc_cat
//     and mm_{t-1}(i) = (d_{t-1}(i) + e_{t-1}(i)) - best.  e_{t-1}(i) waits in a register (or,
//     when a thread owns several states, in the thread's own slot of the trellis, whose d is
//     spent) until every thread is done reading e_t.  The last walk leaves mm_0 in the same
//     place; it is folded by init_cat into row 0.
// The additions are made in exactly the order written: rounding is monotone, so the maximum of
// am_t over the arcs into j is mm_t(j) bit for bit.
//
// Bins.  Folding is by maximum, so its order does not matter and the outputs are the same bits
// on every run.  A bin is the order-preserving integer key of its value (hmm_block.h:
// OrderedKey) under an integer atomic max: 64-bit keys in LDS while the bins fit (a frame's,
// the utterance's, or both; the thread that writes bin c of a row also owns bin c of the
// utterance), else the output rows themselves hold keys of their own dtype, take global integer
// atomic max and are decoded in place at the end -- the rows of an utterance belong to its
// workgroup alone.

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kMmThreads = 256;
constexpr int kMmBinCats = 2048;                 // the bins stay in LDS up to this many categories
constexpr int kMmTurn = 8;                       // out-rows from here on start at their own arc

struct MmForm {
    int arcs_in_lds, bins_lds;
};

template <typename T>
__global__ __launch_bounds__(kMmThreads) void max_marginals_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, beer_arc_map map, int n_cat,
    double* __restrict__ ws, T* __restrict__ state_out, T* __restrict__ frame_out,
    double* __restrict__ utt_out, double* __restrict__ best_out, MmForm form) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using DK = OrderedKey<double>;
    using TK = OrderedKey<T>;
    const int tid = threadIdx.x, nt_ = blockDim.x;
    const int u = b.order ? b.order[blockIdx.x] : (int)blockIdx.x;
    const int gid = b.graph_id[u];
    const beer_graph g = b.graphs[gid];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u];
    const int64_t T_ = b.frame_off[u + 1] - f0;
    const bool cats = frame_out || utt_out;
    double* urow = utt_out ? utt_out + (int64_t)u * n_cat : nullptr;
    T* frows = frame_out ? frame_out + f0 * n_cat : nullptr;
    if (T_ <= 0) {                                         // no frame, no path
        if (tid == 0) best_out[u] = neg_inf();
        if (urow)
            for (int c = tid; c < n_cat; c += nt_) urow[c] = neg_inf();
        return;
    }
    const T* llh = pc_llhs + b.llh_off[u];
    double* dtr = ws + b.llh_off[u];                       // d_t(j), then what a thread holds
    T* srows = state_out ? state_out + b.llh_off[u] : nullptr;
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;
    double* cur = reinterpret_cast<double*>(smem);
    double* nxt = cur + b.max_states;
    double* red = nxt + b.max_states;
    int32_t* l_ptr = reinterpret_cast<int32_t*>(red + kBlockRed);      // [S + 1]
    int32_t* l_end = l_ptr + b.max_states + 1;                         // [A] the arc's other end
    int32_t* l_cat = l_end + b.max_arcs;                               // [A] (with categories)
    const int n_int = b.max_states + 1 + (cats ? 2 : 1) * b.max_arcs;
    T* l_w = reinterpret_cast<T*>(l_ptr + n_int + (n_int & 1));        // [A]
    char* after = form.arcs_in_lds ? reinterpret_cast<char*>(l_w + b.max_arcs + (b.max_arcs & 1))
                                   : reinterpret_cast<char*>(l_ptr);
    DK::K* fbin = reinterpret_cast<DK::K*>(after);         // [n_cat] a frame's bins
    DK::K* ubin = fbin + (frows ? n_cat : 0);              // [n_cat] the utterance's
    const DK::K low = DK::key(neg_inf());

    // ---- forward over the in-CSR, the rows kept ----
    const int32_t* a_ptr = g.in_ptr;
    const int32_t* a_end = g.in_src;
    const T* a_w = (const T*)g.in_w;
    if (form.arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.in_ptr[j];
        for (int e = tid; e < A; e += nt_) { l_end[e] = g.in_src[e]; l_w[e] = a_w[e]; }
        a_ptr = l_ptr; a_end = l_end; a_w = l_w;
    }
    for (int j = tid; j < S; j += nt_) {
        const double d = (double)llh[j] + (double)init[j];
        cur[j] = d;
        dtr[j] = d;
    }
    __syncthreads();
    for (int64_t t = 1; t < T_; ++t) {
        for (int j = tid; j < S; j += nt_) {
            double m = neg_inf();
            for (int e = a_ptr[j]; e < a_ptr[j + 1]; ++e)
                m = dmax(m, cur[a_end[e]] + (double)a_w[e]);
            const double d = m + (double)llh[t * S + j];
            nxt[j] = d;
            dtr[t * S + j] = d;
        }
        __syncthreads();
        double* sw = cur; cur = nxt; nxt = sw;
    }
    double part = neg_inf();
    for (int j = tid; j < S; j += nt_) part = dmax(part, cur[j] + (double)fin[j]);
    const double best = block_max(part, red);              // (the same in every thread)
    if (tid == 0) best_out[u] = best;
    if (!(best > neg_inf())) {
        if (srows)
            for (int64_t e = tid; e < T_ * S; e += nt_) srows[e] = (T)neg_inf();
        if (frows)
            for (int64_t e = tid; e < T_ * n_cat; e += nt_) frows[e] = (T)neg_inf();
        if (urow)
            for (int c = tid; c < n_cat; c += nt_) urow[c] = neg_inf();
        return;
    }

    // ---- the bins ----
    const bool f_lds = frows && form.bins_lds;
    const bool u_lds = urow && form.bins_lds;
    typename TK::K* fkeys = reinterpret_cast<typename TK::K*>(frows);
    DK::K* ukeys = reinterpret_cast<DK::K*>(urow);
    if (f_lds)
        for (int c = tid; c < n_cat; c += nt_) fbin[c] = low;
    if (u_lds)
        for (int c = tid; c < n_cat; c += nt_) ubin[c] = low;
    if (frows && !f_lds)
        for (int64_t e = tid; e < T_ * n_cat; e += nt_) fkeys[e] = TK::key((T)neg_inf());
    if (urow && !u_lds)
        for (int c = tid; c < n_cat; c += nt_) ukeys[c] = low;
    if (cats && !form.bins_lds) __threadfence();
    // a value goes to the frame's bin and, unless the row's writer passes it on, to the
    // utterance's
    const bool u_direct = urow && !f_lds;
    typename TK::K* fkrow = fkeys;                         // row t, set by the loop below
    auto fold = [&](int c, double v) {
        if (c < 0 || !(v > neg_inf())) return;
        if (f_lds) atomicMax(fbin + c, DK::key(v));
        else if (frows) atomicMax(fkrow + c, TK::key((T)v));
        if (u_direct) {
            if (u_lds) atomicMax(ubin + c, DK::key(v));
            else atomicMax(ukeys + c, DK::key(v));
        }
    };
    // row t leaves the LDS bins: thread c mod blockDim owns bin c of both
    auto flush = [&](int64_t t) {
        if (!f_lds) return;
        T* frow = frows + t * n_cat;
        for (int c = tid; c < n_cat; c += nt_) {
            const DK::K k = fbin[c];
            frow[c] = (T)DK::val(k);
            fbin[c] = low;
            if (urow && k > ubin[c]) ubin[c] = k;          // (LDS bins hold both or neither)
        }
    };

    // ---- backward over the out-CSR ----
    const int32_t* cat = cats ? map.arc_cat + map.arc_off[gid] : nullptr;
    const int32_t* icat = cats ? map.init_cat + map.state_off[gid] : nullptr;
    a_ptr = g.out_ptr;
    a_end = g.out_dst;
    a_w = (const T*)g.out_w;
    // (block_max's barriers lie behind every read of the in-CSR, which may now be overwritten)
    if (form.arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.out_ptr[j];
        for (int e = tid; e < A; e += nt_) {
            l_end[e] = g.out_dst[e];
            l_w[e] = a_w[e];
            if (cats) l_cat[e] = cat[e];
        }
        a_ptr = l_ptr; a_end = l_end; a_w = l_w;
        if (cats) cat = l_cat;
    }
    double* erow = nxt;                                    // e_t
    double* lrow = cur;                                    // l_t (every thread its own states)
    const bool one = S <= nt_;                             // a thread owns at most one state
    double held = neg_inf();                               // e_{t-1}(i), then mm_0(i), of it
    for (int j = tid; j < S; j += nt_) {
        const double f = (double)fin[j];
        const double mm = (dtr[(T_ - 1) * S + j] + f) - best;
        if (srows) srows[(T_ - 1) * S + j] = (T)mm;
        erow[j] = f;
        lrow[j] = (double)llh[(T_ - 1) * S + j];
        if (T_ == 1) {
            if (one) held = mm;
            else dtr[j] = mm;
        }
    }
    __syncthreads();
    for (int64_t t = T_ - 1; t >= 1; --t) {
        if (frows) fkrow = fkeys + t * n_cat;
        for (int i = tid; i < S; i += nt_) {
            const double d = dtr[(t - 1) * S + i];
            double m = neg_inf();
            const int e0 = a_ptr[i], e1 = a_ptr[i + 1];
            if (cats && e1 - e0 >= kMmTurn) {
                // A long row with categories is walked from an arc of the thread's own: the ends
                // of a phone loop's units all have the same row, and in step they would all fold
                // into one bin at a time (a maximum does not care where its walk starts).
                int e = e0 + i % (e1 - e0);
                for (int k = e0; k < e1; ++k) {
                    const int j = a_end[e];
                    const double w = (double)a_w[e], l = lrow[j], ev = erow[j];
                    m = dmax(m, w + (l + ev));
                    fold(cat[e], (((d + w) + l) + ev) - best);
                    if (++e == e1) e = e0;
                }
            } else {
                for (int e = e0; e < e1; ++e) {
                    const int j = a_end[e];
                    const double w = (double)a_w[e], l = lrow[j], ev = erow[j];
                    m = dmax(m, w + (l + ev));
                    if (cats) fold(cat[e], (((d + w) + l) + ev) - best);
                }
            }
            const double mm = (d + m) - best;
            if (srows) srows[(t - 1) * S + i] = (T)mm;
            const double keep = t > 1 ? m : mm;
            if (one) held = keep;
            else dtr[(t - 1) * S + i] = keep;
        }
        __syncthreads();                                   // (every read of e_t, every fold)
        if (t > 1)
            for (int i = tid; i < S; i += nt_) {
                erow[i] = one ? held : dtr[(t - 1) * S + i];
                lrow[i] = (double)llh[(t - 1) * S + i];
            }
        flush(t);
        __syncthreads();
    }
    if (!cats) return;
    // row 0: mm_0 by init_cat
    if (frows) fkrow = fkeys;
    for (int j = tid; j < S; j += nt_) fold(icat[j], one ? held : dtr[j]);
    __syncthreads();
    flush(0);
    if (u_lds) {
        __syncthreads();
        for (int c = tid; c < n_cat; c += nt_) urow[c] = DK::val(ubin[c]);
    }
    if (!form.bins_lds) {
        // the keys in the output rows become values: every atomic of this workgroup is behind
        // the barrier, and the loads go where the atomics went
        __threadfence();
        if (frows)
            for (int64_t e = tid; e < T_ * n_cat; e += nt_)
                frows[e] = TK::val(__hip_atomic_load(fkeys + e, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT));
        if (urow)
            for (int c = tid; c < n_cat; c += nt_)
                urow[c] = DK::val(__hip_atomic_load(ukeys + c, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT));
    }
}

// The form of a launch, from the batch maxima (beer_hmm_maxmarg_route packs it): false where the
// launch refuses.
struct MmPlan {
    MmForm form;
    size_t lds;              // dynamic LDS of the launch
};
inline bool mm_plan(int dtype, const beer_batch* b, int n_cat, bool want_state, bool want_frames,
                    bool want_utt, MmPlan* p) {
    if (!block_batch_ok(dtype, b)) return false;
    if (!(want_state || want_frames || want_utt)) return false;
    const bool cats = want_frames || want_utt;
    if (cats && n_cat < 1) return false;
    const size_t S = (size_t)b->max_states, A = (size_t)b->max_arcs;
    const size_t rows = block_rows_bytes(S);
    if (rows > (size_t)kMaxDynLds) return false;
    // the out-CSR of the largest graph, with its categories when they are read (the in-CSR is
    // smaller)
    const size_t arcs = csr_bytes(S, A, dtype == BEER_F32 ? 4 : 8, cats, true);
    size_t lds = rows;
    p->form.arcs_in_lds = rows + arcs <= kBlockArcBytes;
    if (p->form.arcs_in_lds) lds += arcs;
    // (at most 64 + 32 KiB with the arcs, 96 + 32 KiB without: within a CU's LDS)
    p->form.bins_lds = cats && rows <= kBlockBinRows && n_cat <= kMmBinCats;
    if (p->form.bins_lds) lds += 8 * (size_t)n_cat * ((want_frames ? 1 : 0) + (want_utt ? 1 : 0));
    p->lds = lds;
    return true;
}

template <typename T>
int mm_launch(const beer_batch* b, const MmPlan& p, const void* pc_llhs, const beer_arc_map* map,
              int n_cat, double* ws, void* state_out, void* frame_out, double* utt_out,
              double* best, void* stream) {
    const beer_arc_map none = {nullptr, nullptr, nullptr, nullptr};
    return launch_full_lds(max_marginals_kernel<T>, dim3(b->nutt), dim3(kMmThreads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, map ? *map : none, n_cat, ws,
                           (T*)state_out, (T*)frame_out, utt_out, best, p.form);
}

}  // namespace

extern "C" {

int beer_hmm_max_marginals(int dtype, const beer_batch* b, const void* pc_llhs,
                           const beer_arc_map* map, int n_cat, double* ws, void* state_out,
                           void* frame_out, double* utt_out, double* best, void* stream) {
    MmPlan p;
    BEER_REQUIRE(mm_plan(dtype, b, n_cat, state_out != nullptr, frame_out != nullptr,
                         utt_out != nullptr, &p));
    if (map) {
        BEER_REQUIRE(n_cat >= 1);
        BEER_REQUIRE(map->arc_cat && map->init_cat && map->arc_off && map->state_off);
    } else {
        BEER_REQUIRE(!frame_out && !utt_out);
    }
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && ws && best);
    BEER_DISPATCH(dtype, mm_launch, b, p, pc_llhs, map, n_cat, ws, state_out, frame_out, utt_out,
                  best, stream);
}

size_t beer_hmm_maxmarg_scratch_doubles(int dtype, const beer_batch* b) {
    // what a thread holds between two frames lives in a register or in the trellis itself (a
    // batch the launch refuses has no size either)
    (void)dtype;
    (void)b;
    return 0;
}

int beer_hmm_maxmarg_route(int dtype, const beer_batch* b, int n_cat, int want_state,
                           int want_frames, int want_utt) {
    MmPlan p;
    BEER_REQUIRE(mm_plan(dtype, b, n_cat, want_state != 0, want_frames != 0, want_utt != 0, &p));
    return BEER_MAXMARG_BLOCK | (p.form.arcs_in_lds ? BEER_MAXMARG_ARCS_LDS : 0) |
           (p.form.bins_lds ? BEER_MAXMARG_BINS_LDS : 0);
}

}  // extern "C"
