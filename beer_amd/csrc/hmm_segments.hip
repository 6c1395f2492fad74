// Unit segment lattices: the max-marginal of a whole segment (category c begins at frame s and
// lasts exactly until frame e), relative to the Viterbi score (include/beer_hip.h:
// beer_hmm_segment_trellis, beer_hmm_segment_margins).  No exponential, no logarithm: every value
// is an fp64 sum of inputs, every fold a maximum, the outputs the same bits on every run.
//
// Two kernels.
//  1. The trellis kernel has the shape of max_marginals_kernel (hmm_lattice.hip): one workgroup
//     per utterance, forward over the in-CSR, backward over the out-CSR, arcs in LDS while they
//     fit, the bins of a frame as order-preserving integer keys under an integer atomic max.  It
//     keeps the d trellis, writes beside it
//         X_{T-1}(i) = final_i,   X_{t-1}(i) = max over arcs i->j with arc_cat >= 0 of
//                                              (w_ij + (l_t(j) + e_t(j)))
//     ("the best way on from i when a segment ends at t-1") from the same walk of the out-row
//     that gives e_{t-1}(i), and writes best and the start margins with exactly
//     beer_hmm_max_marginals' arithmetic.  e_{t-1}(i) waits in a register or, when a thread owns
//     several states, in the utterance's row of `ws` (the d slot is not free here).
//  2. The expand kernel takes a list of entries (frame s, category c).  A team of L lanes owns an
//     entry and carries r over the category's closure -- the states reachable from the
//     category's entry states through arcs of category -1 -- for max_dur frames:
//         r_s(j) = d_0(j) [init_cat = c]  or  max over arcs i->j of category c of
//                                             ((d_{s-1}(i) + w_ij) + l_s(j))
//         r_t(j) = max over arcs i->j of category -1 of ((r_{t-1}(i) + w_ij) + l_t(j))
//         seg(c, s, s + k) = max_i (r_{s+k}(i) + X_{s+k}(i)) - best
//     Two ping-pong fp64 rows of the closure and two key slots per team in LDS; every team of a
//     workgroup runs the same max_dur steps with one barrier each (the fold of step k goes to
//     slot k & 1 and is written out and reset during step k + 1).

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kSgThreads = 256;
constexpr int kSgBinCats = 2048;                 // a frame's bins stay in LDS up to here
constexpr int kSgTurn = 8;                       // out-rows from here on start at their own arc

struct SgForm {
    int arcs_in_lds, bins_lds;
};

template <typename T>
__global__ __launch_bounds__(kSgThreads) void segment_trellis_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, beer_arc_map map, int n_cat,
    double* __restrict__ d_out, double* __restrict__ x_out, double* __restrict__ ws,
    T* __restrict__ frame_out, double* __restrict__ best_out, SgForm form) {
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
    if (T_ <= 0) {                                         // no frame, no path
        if (tid == 0) best_out[u] = neg_inf();
        return;
    }
    T* frows = frame_out + f0 * n_cat;
    const T* llh = pc_llhs + b.llh_off[u];
    double* dtr = d_out + b.llh_off[u];                    // d_t(j), kept
    double* xtr = x_out + b.llh_off[u];                    // X_t(i)
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;
    double* cur = reinterpret_cast<double*>(smem);
    double* nxt = cur + b.max_states;
    double* red = nxt + b.max_states;
    int32_t* l_ptr = reinterpret_cast<int32_t*>(red + kBlockRed);      // [S + 1]
    int32_t* l_end = l_ptr + b.max_states + 1;                         // [A] the arc's other end
    int32_t* l_cat = l_end + b.max_arcs;                               // [A]
    const int n_int = b.max_states + 1 + 2 * b.max_arcs;
    T* l_w = reinterpret_cast<T*>(l_ptr + n_int + (n_int & 1));        // [A]
    char* after = form.arcs_in_lds ? reinterpret_cast<char*>(l_w + b.max_arcs + (b.max_arcs & 1))
                                   : reinterpret_cast<char*>(l_ptr);
    DK::K* fbin = reinterpret_cast<DK::K*>(after);         // [n_cat] a frame's bins
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
        for (int64_t e = tid; e < T_ * n_cat; e += nt_) frows[e] = (T)neg_inf();
        for (int64_t e = tid; e < T_ * S; e += nt_) xtr[e] = neg_inf();
        return;
    }

    // ---- the bins ----
    const bool f_lds = form.bins_lds;
    typename TK::K* fkeys = reinterpret_cast<typename TK::K*>(frows);
    if (f_lds) {
        for (int c = tid; c < n_cat; c += nt_) fbin[c] = low;
    } else {
        for (int64_t e = tid; e < T_ * n_cat; e += nt_) fkeys[e] = TK::key((T)neg_inf());
        __threadfence();
    }
    typename TK::K* fkrow = fkeys;                         // row t, set by the loop below
    auto fold = [&](int c, double v) {
        if (c < 0 || !(v > neg_inf())) return;
        if (f_lds) atomicMax(fbin + c, DK::key(v));
        else atomicMax(fkrow + c, TK::key((T)v));
    };
    auto flush = [&](int64_t t) {
        if (!f_lds) return;
        T* frow = frows + t * n_cat;
        for (int c = tid; c < n_cat; c += nt_) {
            frow[c] = (T)DK::val(fbin[c]);
            fbin[c] = low;
        }
    };

    // ---- backward over the out-CSR ----
    const int32_t* cat = map.arc_cat + map.arc_off[gid];
    const int32_t* icat = map.init_cat + map.state_off[gid];
    a_ptr = g.out_ptr;
    a_end = g.out_dst;
    a_w = (const T*)g.out_w;
    // (block_max's barriers lie behind every read of the in-CSR, which may now be overwritten)
    if (form.arcs_in_lds) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.out_ptr[j];
        for (int e = tid; e < A; e += nt_) {
            l_end[e] = g.out_dst[e];
            l_w[e] = a_w[e];
            l_cat[e] = cat[e];
        }
        a_ptr = l_ptr; a_end = l_end; a_w = l_w;
        cat = l_cat;
    }
    double* erow = nxt;                                    // e_t
    double* lrow = cur;                                    // l_t (every thread its own states)
    const bool one = S <= nt_;                             // a thread owns at most one state
    double* wait = one ? nullptr : ws + (int64_t)u * b.max_states;     // where e_{t-1} waits
    double held = neg_inf();                               // e_{t-1}(i), then mm_0(i), of it
    for (int j = tid; j < S; j += nt_) {
        const double f = (double)fin[j];
        xtr[(T_ - 1) * S + j] = f;
        erow[j] = f;
        lrow[j] = (double)llh[(T_ - 1) * S + j];
        if (T_ == 1) {
            const double mm = (dtr[j] + f) - best;
            if (one) held = mm;
            else wait[j] = mm;
        }
    }
    __syncthreads();
    for (int64_t t = T_ - 1; t >= 1; --t) {
        fkrow = fkeys + t * n_cat;
        for (int i = tid; i < S; i += nt_) {
            const double d = dtr[(t - 1) * S + i];
            double m = neg_inf(), xm = neg_inf();
            const int e0 = a_ptr[i], e1 = a_ptr[i + 1];
            // A long row is walked from an arc of the thread's own, as in max_marginals_kernel:
            // the ends of a phone loop's units would otherwise fold into one bin at a time.
            int e = e1 - e0 >= kSgTurn ? e0 + i % (e1 - e0) : e0;
            for (int k = e0; k < e1; ++k) {
                const int j = a_end[e];
                const int c = cat[e];
                const double w = (double)a_w[e], l = lrow[j], ev = erow[j];
                const double on = w + (l + ev);
                m = dmax(m, on);
                if (c >= 0) xm = dmax(xm, on);
                fold(c, (((d + w) + l) + ev) - best);
                if (++e == e1) e = e0;
            }
            xtr[(t - 1) * S + i] = xm;
            const double keep = t > 1 ? m : (d + m) - best;
            if (one) held = keep;
            else wait[i] = keep;
        }
        __syncthreads();                                   // (every read of e_t, every fold)
        if (t > 1)
            for (int i = tid; i < S; i += nt_) {
                erow[i] = one ? held : wait[i];
                lrow[i] = (double)llh[(t - 1) * S + i];
            }
        flush(t);
        __syncthreads();
    }
    // row 0: mm_0 by init_cat
    fkrow = fkeys;
    for (int j = tid; j < S; j += nt_) fold(icat[j], one ? held : wait[j]);
    __syncthreads();
    flush(0);
    if (!f_lds) {
        // the keys in the output rows become values: every atomic of this workgroup is behind
        // the barrier, and the loads go where the atomics went
        __threadfence();
        for (int64_t e = tid; e < T_ * n_cat; e += nt_)
            frows[e] = TK::val(__hip_atomic_load(fkeys + e, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT));
    }
}

template <typename T>
__global__ __launch_bounds__(kSgThreads) void segment_margins_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, beer_seg_map sm, int n_cat,
    const double* __restrict__ d_in, const double* __restrict__ x_in,
    const double* __restrict__ best_in, const int64_t* __restrict__ entry_frame,
    const int32_t* __restrict__ entry_cat, const int64_t* __restrict__ entry_off,
    int64_t n_entries, int max_dur, T* __restrict__ out, int L, int row) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using DK = OrderedKey<double>;
    const int tid = threadIdx.x;
    const int team = tid / L, lane = tid - team * L;
    double* r0 = reinterpret_cast<double*>(smem) + (size_t)team * (2 * row + 2);
    double* r1 = r0 + row;
    DK::K* slot = reinterpret_cast<DK::K*>(r1 + row);      // [2]
    const DK::K low = DK::key(neg_inf());
    const int64_t en = (int64_t)blockIdx.x * (kSgThreads / L) + team;
    const bool mine = en < n_entries;                      // an idle team steps along
    bool live = mine;
    int S = 0, M = 0, m0 = 0;
    int64_t s = 0, T_ = 0;
    double best = neg_inf();
    const T* llh = nullptr;
    const T* w = nullptr;
    const double* xtr = nullptr;
    bool own = false;                                      // the lane has a member of its own
    int j0 = 0, a0 = 0, n0 = 0, s0 = 0, s1 = 0;
    double w0 = 0., w1 = 0., xv = 0., lv = 0.;             // (xv, lv: X_t and l_{t+1} of it)
    if (mine) {
        int lo = 0, hi = b.nutt;                           // entry_off[lo] <= en < entry_off[lo+1]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (entry_off[mid] <= en) lo = mid; else hi = mid;
        }
        const int u = lo;
        const int c = entry_cat[en];
        const int64_t f0 = b.frame_off[u];
        T_ = b.frame_off[u + 1] - f0;
        s = entry_frame[en] - f0;
        best = best_in[u];
        live = c >= 0 && c < n_cat && s >= 0 && s < T_ && best > neg_inf();
        if (live) {
            const int gid = b.graph_id[u];
            const beer_graph g = b.graphs[gid];
            S = g.n_states;
            w = (const T*)g.out_w;
            llh = pc_llhs + b.llh_off[u];
            xtr = x_in + b.llh_off[u];
            const double* dtr = d_in + b.llh_off[u];
            const int64_t k = (int64_t)gid * n_cat + c;
            m0 = sm.mem_ptr[k];
            M = sm.mem_ptr[k + 1] - m0;
            // r_s over the closure
            for (int m = lane; m < M; m += L) {
                const int j = sm.members[m0 + m];
                double r = neg_inf();
                if (s == 0) {
                    if (sm.mem_init[m0 + m]) r = dtr[j];
                } else {
                    const double l = (double)llh[s * S + j];
                    for (int a = sm.ent_ptr[m0 + m]; a < sm.ent_ptr[m0 + m + 1]; ++a)
                        r = dmax(r, (dtr[(s - 1) * S + sm.ent_src[a]] + (double)w[sm.ent_arc[a]]) + l);
                }
                r0[m] = r;
            }
            // The lane's first member stays in registers with its first two in-arcs (a unit's
            // state has a self loop and a predecessor): a step then waits for no index load.
            if (lane < M) {
                own = true;
                j0 = sm.members[m0 + lane];
                a0 = sm.in_ptr[m0 + lane];
                n0 = sm.in_ptr[m0 + lane + 1] - a0;
                if (n0 > 0) { s0 = sm.in_src[a0]; w0 = (double)w[sm.in_arc[a0]]; }
                if (n0 > 1) { s1 = sm.in_src[a0 + 1]; w1 = (double)w[sm.in_arc[a0 + 1]]; }
                xv = xtr[s * S + j0];
                if (s + 1 < T_) lv = (double)llh[(s + 1) * S + j0];
            }
        }
    }
    if (lane == 0) slot[0] = slot[1] = low;
    __syncthreads();
    T* orow = out + (mine ? en : 0) * max_dur;
    for (int k = 0; k < max_dur; ++k) {
        const int64_t t = s + k;
        const double* cur = (k & 1) ? r1 : r0;
        double* nxt = (k & 1) ? r0 : r1;
        if (live && t < T_) {
            const bool more = t + 1 < T_ && k + 1 < max_dur;
            double part = neg_inf();
            if (own) {
                // the next step's X and l are asked for now: they arrive behind the barrier
                double xn = 0., ln = 0.;
                if (t + 1 < T_) xn = xtr[(t + 1) * S + j0];
                if (t + 2 < T_) ln = (double)llh[(t + 2) * S + j0];
                part = cur[lane] + xv;
                if (more) {
                    double r = neg_inf();
                    if (n0 > 0) r = (cur[s0] + w0) + lv;
                    if (n0 > 1) r = dmax(r, (cur[s1] + w1) + lv);
                    for (int a = a0 + 2; a < a0 + n0; ++a)
                        r = dmax(r, (cur[sm.in_src[a]] + (double)w[sm.in_arc[a]]) + lv);
                    nxt[lane] = r;
                }
                xv = xn;
                lv = ln;
            }
            for (int m = lane + L; m < M; m += L) {             // (closures beyond 256 states)
                const int j = sm.members[m0 + m];
                part = dmax(part, cur[m] + xtr[t * S + j]);
                if (more) {
                    const double l = (double)llh[(t + 1) * S + j];
                    double r = neg_inf();
                    for (int a = sm.in_ptr[m0 + m]; a < sm.in_ptr[m0 + m + 1]; ++a)
                        r = dmax(r, (cur[sm.in_src[a]] + (double)w[sm.in_arc[a]]) + l);
                    nxt[m] = r;
                }
            }
            if (part > neg_inf()) atomicMax(slot + (k & 1), DK::key(part));
        }
        if (lane == 0 && k >= 1) {                         // the fold of the step before
            const double v = DK::val(slot[(k - 1) & 1]);
            slot[(k - 1) & 1] = low;
            if (mine) orow[k - 1] = (T)(v > neg_inf() ? v - best : neg_inf());
        }
        __syncthreads();
    }
    if (lane == 0 && mine) {
        const double v = DK::val(slot[(max_dur - 1) & 1]);
        orow[max_dur - 1] = (T)(v > neg_inf() ? v - best : neg_inf());
    }
}

// The form of the two launches, from the batch maxima (beer_hmm_segments_route packs it): false
// where they refuse.  The trellis kernel's part is max_marginals' plan with the frames' bins.
struct SgPlan {
    SgForm form;
    size_t lds;              // dynamic LDS of the trellis launch
    int team;                // lanes of a team of the expand launch
    int row;                 // doubles of a team's row
    size_t team_lds;         // dynamic LDS of the expand launch
};
inline bool sg_plan(int dtype, const beer_batch* b, int n_cat, int max_closure, SgPlan* p) {
    if (!block_batch_ok(dtype, b)) return false;
    if (n_cat < 1 || max_closure < 0 || max_closure > b->max_states) return false;
    const size_t S = (size_t)b->max_states, A = (size_t)b->max_arcs;
    const size_t rows = block_rows_bytes(S);
    if (rows > (size_t)kMaxDynLds) return false;
    // the out-CSR with its categories
    const size_t arcs = csr_bytes(S, A, dtype == BEER_F32 ? 4 : 8, true, true);
    size_t lds = rows;
    p->form.arcs_in_lds = rows + arcs <= kBlockArcBytes;
    if (p->form.arcs_in_lds) lds += arcs;
    p->form.bins_lds = rows <= kBlockBinRows && n_cat <= kSgBinCats;
    if (p->form.bins_lds) lds += 8 * (size_t)n_cat;
    p->lds = lds;
    // per team two rows of the closure and two key slots
    return team_plan(max_closure, kSgThreads, 2, 2, kBlockTeamBytes, &p->team, &p->row,
                     &p->team_lds);
}

template <typename T>
int sg_trellis_launch(const beer_batch* b, const SgPlan& p, const void* pc_llhs,
                      const beer_arc_map* map, int n_cat, double* d, double* x, double* ws,
                      void* frame_out, double* best, void* stream) {
    return launch_full_lds(segment_trellis_kernel<T>, dim3(b->nutt), dim3(kSgThreads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, *map, n_cat, d, x, ws,
                           (T*)frame_out, best, p.form);
}

template <typename T>
int sg_margins_launch(const beer_batch* b, const SgPlan& p, const void* pc_llhs,
                      const beer_seg_map* sm, int n_cat, const double* d, const double* x,
                      const double* best, const int64_t* entry_frame, const int32_t* entry_cat,
                      const int64_t* entry_off, int64_t n_entries, int max_dur, void* out,
                      void* stream) {
    const int64_t teams = kSgThreads / p.team;
    const int64_t blocks = (n_entries + teams - 1) / teams;
    return launch_full_lds(segment_margins_kernel<T>, dim3((unsigned)blocks), dim3(kSgThreads),
                           p.team_lds, as_stream(stream), *b, (const T*)pc_llhs, *sm, n_cat, d, x,
                           best, entry_frame, entry_cat, entry_off, n_entries, max_dur, (T*)out,
                           p.team, p.row);
}

}  // namespace

extern "C" {

int beer_hmm_segment_trellis(int dtype, const beer_batch* b, const void* pc_llhs,
                             const beer_arc_map* map, int n_cat, double* d, double* x, double* ws,
                             void* frame_out, double* best, void* stream) {
    SgPlan p;
    BEER_REQUIRE(sg_plan(dtype, b, n_cat, 0, &p));
    BEER_REQUIRE(map && map->arc_cat && map->init_cat && map->arc_off && map->state_off);
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && d && x && frame_out && best);
    BEER_REQUIRE(ws || b->max_states <= kSgThreads);
    BEER_DISPATCH(dtype, sg_trellis_launch, b, p, pc_llhs, map, n_cat, d, x, ws, frame_out, best,
                  stream);
}

int beer_hmm_segment_margins(int dtype, const beer_batch* b, const void* pc_llhs,
                             const beer_seg_map* sm, int n_cat, const double* d, const double* x,
                             const double* best, const int64_t* entry_frame,
                             const int32_t* entry_cat, const int64_t* entry_off,
                             int64_t n_entries, int max_dur, void* out, void* stream) {
    SgPlan p;
    BEER_REQUIRE(sm != nullptr);
    BEER_REQUIRE(sg_plan(dtype, b, n_cat, sm->max_closure, &p));
    BEER_REQUIRE(n_entries >= 0 && max_dur >= 1);
    BEER_REQUIRE(n_entries / (kSgThreads / p.team) < 0x7fffffff);
    if (n_entries == 0 || b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(sm->mem_ptr && sm->members && sm->mem_init && sm->in_ptr && sm->in_src &&
                 sm->in_arc && sm->ent_ptr && sm->ent_src && sm->ent_arc);
    BEER_REQUIRE(pc_llhs && d && x && best && entry_frame && entry_cat && entry_off && out);
    BEER_DISPATCH(dtype, sg_margins_launch, b, p, pc_llhs, sm, n_cat, d, x, best, entry_frame,
                  entry_cat, entry_off, n_entries, max_dur, out, stream);
}

size_t beer_hmm_segments_scratch_doubles(int dtype, const beer_batch* b) {
    // a row per utterance where a thread owns several states: e_{t-1} waits there (a batch the
    // launch refuses has no size)
    SgPlan p;
    if (!sg_plan(dtype, b, 1, 0, &p)) return 0;
    return b->max_states > kSgThreads ? (size_t)b->nutt * (size_t)b->max_states : 0;
}

int beer_hmm_segments_route(int dtype, const beer_batch* b, int n_cat, int max_closure) {
    SgPlan p;
    BEER_REQUIRE(sg_plan(dtype, b, n_cat, max_closure, &p));
    return BEER_SEGMENTS_BLOCK | (p.form.arcs_in_lds ? BEER_SEGMENTS_ARCS_LDS : 0) |
           (p.form.bins_lds ? BEER_SEGMENTS_BINS_LDS : 0) | ceil_log2(p.team);
}

}  // extern "C"
