// Segment posteriors: the probability that category c begins at frame s and lasts exactly until
// frame e -- the sum-product twin of the unit segment lattice (include/beer_hip.h:
// beer_hmm_segpost_trellis, beer_hmm_segment_posteriors).
//
// Two kernels.
//  1. The trellis kernel has the shape of arc_posteriors_kernel (hmm_arcs.hip): one workgroup per
//     utterance, forward over the in-CSR (beer_hmm_log_evidence's recursion, â and c_t kept),
//     backward over the out-CSR with ONE exponential per arc and frame
//         p = exp(â_{t-1}(i) + w_ij + l_t(j) + b_t(j) - c_t)
//     whose sum over the row is gamma_{t-1}(i) (which gives b_{t-1}(i)), whose sum over the arcs
//     of the row with arc_cat >= 0 gives, from the same walk,
//         Y_{t-1}(i) = ln(that sum) - â_{t-1}(i)
//     ("the mass that goes on from i when a segment ends at t-1"), and which is added to bin
//     arc_cat of row t of the start posteriors.  Every value of â and Y is written by the thread
//     that owns its state, the sums of a row in the order of the row: the same bits on every run.
//     Only the bins take atomic adds.
//  2. The expand kernel takes a list of entries (frame s, category c).  A team of L lanes owns an
//     entry and carries, over the category's closure, the RATIO rho_t(j) = exp(r_t(j) - â_t(j)),
//     which lies in [0, 1]:
//         rho_s(j) = [init_cat[j] == c]                                                   s = 0
//         rho_s(j) = sum over arcs i->j of category c of exp((â_{s-1}(i) + w_ij) + g_s(j))
//         rho_t(j) = sum over arcs i->j of category -1 of
//                    rho_{t-1}(i) exp((â_{t-1}(i) + w_ij) + g_t(j)),   g_t(j) = (l_t(j) - c_t) - â_t(j)
//         post(c, s, s + k) = sum_j rho_{s+k}(j) exp(â_{s+k}(j) + Y_{s+k}(j))
//     Every exponential is of a log-probability (<= 0 but for rounding): no maximum is taken, no
//     logarithm, and an underflow is a harmless 0.  Per team two ping-pong pairs of fp64 rows
//     (rho and â of the closure) in LDS; the fold is a sum in a fixed order -- cross-lane moves
//     within a wave, and for teams of 128 / 256 lanes the waves' partial sums in LDS slots that
//     lane 0 adds in order during the next step -- so one barrier per step and the same bits on
//     every run.
//
// Arithmetic: hmm.hip's rule -- sums, differences, the trellises and the folds are fp64, exp / log
// are in the model's precision.

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kSpThreads = 256;
constexpr int kSpBinCats = 1024;                 // a frame's bins stay in LDS up to here
constexpr int kSpSlots = 8;                      // doubles of a team's slots: 2 steps x 4 waves

// The sum of v over the L lanes of a team (L a power of two, 4 .. 64: the team lies within a
// wave), by the stages of wave_sum up to L: a fixed order, the same value in every lane of the team.
// Every lane of the wave takes part.
__device__ __forceinline__ double team_sum(double v, int L) {
    v += wave_detail::dpp<double, 0xB1>(v);                // quad_perm [1,0,3,2]
    v += wave_detail::dpp<double, 0x4E>(v);                // quad_perm [2,3,0,1]
    if (L >= 8) v += wave_detail::dpp<double, 0x141>(v);   // row_half_mirror
    if (L >= 16) v += wave_detail::dpp<double, 0x140>(v);  // row_mirror
    if (L >= 32) {
        double a, b;
        wave_detail::cross<double, false>(v, a, b);
        v = a + b;
    }
    if (L >= 64) {
        double a, b;
        wave_detail::cross<double, true>(v, a, b);
        v = a + b;
    }
    return v;
}

struct SpForm {
    int arcs_in_lds, bins_lds;
};

template <typename T>
__global__ __launch_bounds__(kSpThreads) void segpost_trellis_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, beer_arc_map map, int n_cat,
    double* __restrict__ alpha_out, double* __restrict__ y_out, double* __restrict__ norm_out,
    T* __restrict__ frame_out, double* __restrict__ evidence, SpForm form) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nt_ = blockDim.x;
    const int u = b.order ? b.order[blockIdx.x] : (int)blockIdx.x;
    const int gid = b.graph_id[u];
    const beer_graph g = b.graphs[gid];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u];
    const int64_t T_ = b.frame_off[u + 1] - f0;
    if (T_ <= 0) {                                         // (as beer_hmm_log_evidence has it)
        if (tid == 0) evidence[u] = 0.0;
        return;
    }
    T* frows = frame_out + f0 * n_cat;
    const T* llh = pc_llhs + b.llh_off[u];
    double* norm = norm_out + f0;                          // c_t
    double* alpha = alpha_out + b.llh_off[u];              // â_t(j)
    double* ytr = y_out + b.llh_off[u];                    // Y_t(i)
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
    double total = 0.0;                                    // sum_t c_t (the same in every thread)
    for (int64_t t = 0;; ++t) {
        // (first barrier inside: every thread is done reading `cur`, the arc lists are staged)
        const double c = block_lse<T>(S, [&](int j) { return nxt[j]; }, red);
        dead = !(c > neg_inf());
        if (dead) break;
        total += c;
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
        for (int64_t e = tid; e < T_ * n_cat; e += nt_) frows[e] = (T)0;
        if (tid == 0) evidence[u] = neg_inf();
        return;
    }
    if (tid == 0) evidence[u] = total + tail;

    // ---- the bins ----
    const bool f_lds = form.bins_lds;
    if (f_lds) {
        for (int c = tid; c < n_cat; c += nt_) fbin[c] = 0.0;
    } else {
        for (int64_t e = tid; e < T_ * n_cat; e += nt_) frows[e] = (T)0;
        __threadfence();
    }
    T* frow = frows;                                       // row t, set by the loop below
    auto fold = [&](int c, double p) {
        if (c < 0 || !(p > 0.0)) return;
        if (f_lds) atomicAdd(fbin + c, p);
        else unsafeAtomicAdd(frow + c, (T)p);
    };
    auto flush = [&]() {                                   // row t leaves the LDS bins
        if (!f_lds) return;
        for (int c = tid; c < n_cat; c += nt_) {
            frow[c] = (T)fbin[c];
            fbin[c] = 0.0;
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
    double* dcur = nxt;                                    // d_t = l_t + b_t - c_t, read by the walk
    double* dnxt = cur;                                    // gamma_{t-1}, then d_{t-1}
    for (int j = tid; j < S; j += nt_) ytr[(T_ - 1) * S + j] = (double)fin[j] - tail;
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
        frow = frows + t * n_cat;
        const double* arow = alpha + (t - 1) * S;
        double* yrow = ytr + (t - 1) * S;
        double part = 0.0;
        for (int i = tid; i < S; i += nt_) {
            const double a = arow[i];
            double gam = 0.0, on = 0.0;                    // (on: the arcs that end a segment)
            if (a > neg_inf()) {
                for (int e = a_ptr[i]; e < a_ptr[i + 1]; ++e) {
                    const int c = cat[e];
                    const double p = LogRel<T>::ex(a + (double)a_w[e] + dcur[a_end[e]]);
                    gam += p;
                    if (c >= 0) on += p;
                    fold(c, p);
                }
            }
            dnxt[i] = gam;
            yrow[i] = on;                                  // (its own slot: finished below)
            part += gam;
        }
        double G = block_sum(part, red);                   // (every fold is behind its barriers)
        if (!(G > 0.0) || !(G < __builtin_huge_val())) G = 1.0;
        const double cp = norm[t - 1];
        for (int i = tid; i < S; i += nt_) {
            const double a = arow[i];
            const double on = yrow[i];
            yrow[i] = on > 0.0 ? LogRel<T>::lg(on / G) - a : neg_inf();
            if (t > 1) {
                const double gam = dnxt[i];
                const double bw = gam > 0.0 ? LogRel<T>::lg(gam / G) - a : neg_inf();
                dnxt[i] = (double)llh[(t - 1) * S + i] + bw - cp;
            }
        }
        flush();
        __syncthreads();
        double* sw = dcur; dcur = dnxt; dnxt = sw;
    }
    // row 0: gamma_0 by init_cat (T = 1: it is in `dnxt`, else the last swap left it in `dcur`)
    const double* gam0 = T_ == 1 ? dnxt : dcur;
    frow = frows;
    for (int j = tid; j < S; j += nt_) fold(icat[j], gam0[j]);
    __syncthreads();
    flush();
}

template <typename T>
__global__ __launch_bounds__(kSpThreads) void segment_posteriors_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, beer_seg_map sm, int n_cat,
    const double* __restrict__ alpha_in, const double* __restrict__ y_in,
    const double* __restrict__ norm_in, const double* __restrict__ evidence,
    const int64_t* __restrict__ entry_frame, const int32_t* __restrict__ entry_cat,
    const int64_t* __restrict__ entry_off, int64_t n_entries, int max_dur, T* __restrict__ out,
    int L, int row) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int team = tid / L, lane = tid - team * L;
    // a team's LDS: rho and â of the closure, twice (ping-pong), and the slots of the fold
    double* base = reinterpret_cast<double*>(smem) + (size_t)team * (4 * row + kSpSlots);
    double* slot = base + 4 * row;                         // [2][4]
    const int nw = L > 64 ? L / 64 : 1;                    // waves of a team
    const int64_t en = (int64_t)blockIdx.x * (kSpThreads / L) + team;
    const bool mine = en < n_entries;                      // an idle team steps along
    bool live = mine;
    int S = 0, M = 0, m0 = 0;
    int64_t s = 0, T_ = 0;
    const T* llh = nullptr;
    const T* w = nullptr;
    const double* atr = nullptr;
    const double* ytr = nullptr;
    const double* norm = nullptr;
    bool own = false;                                      // the lane has a member of its own
    int j0 = 0, a0 = 0, n0 = 0, s0 = 0, s1 = 0;
    double w0 = 0., w1 = 0.;
    // of the lane's member, at the step's frame t: ev = â_t + Y_t; an = â_{t+1}; gn = g_{t+1}
    double ev = neg_inf(), an = neg_inf(), gn = 0.;
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
        live = c >= 0 && c < n_cat && s >= 0 && s < T_ && evidence[u] > neg_inf();
        if (live) {
            const int gid = b.graph_id[u];
            const beer_graph g = b.graphs[gid];
            S = g.n_states;
            w = (const T*)g.out_w;
            llh = pc_llhs + b.llh_off[u];
            atr = alpha_in + b.llh_off[u];
            ytr = y_in + b.llh_off[u];
            norm = norm_in + f0;
            const int64_t k = (int64_t)gid * n_cat + c;
            m0 = sm.mem_ptr[k];
            M = sm.mem_ptr[k + 1] - m0;
            // rho_s and â_s over the closure
            const double cs = norm[s];
            for (int m = lane; m < M; m += L) {
                const int j = sm.members[m0 + m];
                const double a = atr[s * S + j];
                double rho = 0.0;
                if (a > neg_inf()) {
                    if (s == 0) {
                        if (sm.mem_init[m0 + m]) rho = 1.0;
                    } else {
                        const double gs = ((double)llh[s * S + j] - cs) - a;
                        for (int e = sm.ent_ptr[m0 + m]; e < sm.ent_ptr[m0 + m + 1]; ++e)
                            rho += LogRel<T>::ex((atr[(s - 1) * S + sm.ent_src[e]] +
                                                (double)w[sm.ent_arc[e]]) + gs);
                    }
                }
                base[m] = rho;
                base[row + m] = a;
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
                ev = atr[s * S + j0] + ytr[s * S + j0];
                if (s + 1 < T_) {
                    an = atr[(s + 1) * S + j0];
                    gn = ((double)llh[(s + 1) * S + j0] - norm[s + 1]) - an;
                }
            }
        }
    }
    if (lane < kSpSlots) slot[lane] = 0.0;
    __syncthreads();
    T* orow = out + (mine ? en : 0) * max_dur;
    for (int k = 0; k < max_dur; ++k) {
        const int64_t t = s + k;
        const double* rcur = base + ((k & 1) ? 2 * row : 0);
        const double* acur = rcur + row;
        double* rnxt = base + ((k & 1) ? 0 : 2 * row);
        double* anxt = rnxt + row;
        double part = 0.0;
        if (live && t < T_) {
            const bool more = t + 1 < T_ && k + 1 < max_dur;
            if (own) {
                // the next step's â, Y, l and c_t are asked for now: they arrive behind the barrier
                double evn = neg_inf(), ann = neg_inf(), gnn = 0.;
                if (t + 1 < T_) evn = an + ytr[(t + 1) * S + j0];
                if (t + 2 < T_) {
                    ann = atr[(t + 2) * S + j0];
                    gnn = ((double)llh[(t + 2) * S + j0] - norm[t + 2]) - ann;
                }
                const double rho = rcur[lane];
                if (rho > 0.0) part = rho * LogRel<T>::ex(ev);
                if (more) {
                    double r = 0.0;
                    if (an > neg_inf()) {
                        if (n0 > 0) r = rcur[s0] * LogRel<T>::ex((acur[s0] + w0) + gn);
                        if (n0 > 1) r += rcur[s1] * LogRel<T>::ex((acur[s1] + w1) + gn);
                        for (int a = a0 + 2; a < a0 + n0; ++a) {
                            const int i = sm.in_src[a];
                            r += rcur[i] * LogRel<T>::ex((acur[i] + (double)w[sm.in_arc[a]]) + gn);
                        }
                    }
                    rnxt[lane] = r;
                    anxt[lane] = an;
                }
                ev = evn;
                an = ann;
                gn = gnn;
            }
            for (int m = lane + L; m < M; m += L) {             // (closures beyond 256 states)
                const int j = sm.members[m0 + m];
                const double rho = rcur[m];
                if (rho > 0.0) part += rho * LogRel<T>::ex(acur[m] + ytr[t * S + j]);
                if (more) {
                    const double a = atr[(t + 1) * S + j];
                    double r = 0.0;
                    if (a > neg_inf()) {
                        const double gj = ((double)llh[(t + 1) * S + j] - norm[t + 1]) - a;
                        for (int e = sm.in_ptr[m0 + m]; e < sm.in_ptr[m0 + m + 1]; ++e) {
                            const int i = sm.in_src[e];
                            r += rcur[i] * LogRel<T>::ex((acur[i] + (double)w[sm.in_arc[e]]) + gj);
                        }
                    }
                    rnxt[m] = r;
                    anxt[m] = a;
                }
            }
        }
        // the fold, in a fixed order: the team's lanes of a wave by cross-lane moves ...
        part = team_sum(part, L);
        if (nw == 1) {
            if (lane == 0 && mine) orow[k] = (T)part;
        } else {
            // ... and the waves of a larger team through the step's slots, added in order by
            // lane 0 during the next step
            if ((lane & 63) == 0) slot[(k & 1) * 4 + (lane >> 6)] = part;
            if (lane == 0 && k >= 1 && mine) {
                const double* sl = slot + ((k - 1) & 1) * 4;
                double v = sl[0];
                for (int i = 1; i < nw; ++i) v += sl[i];
                orow[k - 1] = (T)v;
            }
        }
        __syncthreads();
    }
    if (nw > 1 && lane == 0 && mine) {
        const double* sl = slot + ((max_dur - 1) & 1) * 4;
        double v = sl[0];
        for (int i = 1; i < nw; ++i) v += sl[i];
        orow[max_dur - 1] = (T)v;
    }
}

// The form of the two launches, from the batch maxima (beer_hmm_segposts_route packs it): false
// where they refuse.  The trellis kernel's part is arc_posteriors' plan with the frames' bins.
struct SpPlan {
    SpForm form;
    size_t lds;              // dynamic LDS of the trellis launch
    int team;                // lanes of a team of the expand launch
    int row;                 // doubles of a team's row
    size_t team_lds;         // dynamic LDS of the expand launch
};
inline bool sp_plan(int dtype, const beer_batch* b, int n_cat, int max_closure, SpPlan* p) {
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
    p->form.bins_lds = rows <= kBlockBinRows && n_cat <= kSpBinCats;
    if (p->form.bins_lds) lds += 8 * (size_t)n_cat;
    p->lds = lds;
    // per team rho and â of the closure, twice, and the slots of the fold
    return team_plan(max_closure, kSpThreads, 4, kSpSlots, kBlockTeamBytes, &p->team, &p->row,
                     &p->team_lds);
}

template <typename T>
int sp_trellis_launch(const beer_batch* b, const SpPlan& p, const void* pc_llhs,
                      const beer_arc_map* map, int n_cat, double* alpha, double* y, double* norm,
                      void* frame_out, double* evidence, void* stream) {
    return launch_full_lds(segpost_trellis_kernel<T>, dim3(b->nutt), dim3(kSpThreads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, *map, n_cat, alpha, y, norm,
                           (T*)frame_out, evidence, p.form);
}

template <typename T>
int sp_expand_launch(const beer_batch* b, const SpPlan& p, const void* pc_llhs,
                     const beer_seg_map* sm, int n_cat, const double* alpha, const double* y,
                     const double* norm, const double* evidence, const int64_t* entry_frame,
                     const int32_t* entry_cat, const int64_t* entry_off, int64_t n_entries,
                     int max_dur, void* out, void* stream) {
    const int64_t teams = kSpThreads / p.team;
    const int64_t blocks = (n_entries + teams - 1) / teams;
    return launch_full_lds(segment_posteriors_kernel<T>, dim3((unsigned)blocks), dim3(kSpThreads),
                           p.team_lds, as_stream(stream), *b, (const T*)pc_llhs, *sm, n_cat, alpha,
                           y, norm, evidence, entry_frame, entry_cat, entry_off, n_entries, max_dur,
                           (T*)out, p.team, p.row);
}

}  // namespace

extern "C" {

int beer_hmm_segpost_trellis(int dtype, const beer_batch* b, const void* pc_llhs,
                             const beer_arc_map* map, int n_cat, double* alpha, double* y,
                             double* norm, void* frame_out, double* evidence, void* stream) {
    SpPlan p;
    BEER_REQUIRE(sp_plan(dtype, b, n_cat, 0, &p));
    BEER_REQUIRE(map && map->arc_cat && map->init_cat && map->arc_off && map->state_off);
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && alpha && y && norm && frame_out && evidence);
    BEER_DISPATCH(dtype, sp_trellis_launch, b, p, pc_llhs, map, n_cat, alpha, y, norm, frame_out,
                  evidence, stream);
}

int beer_hmm_segment_posteriors(int dtype, const beer_batch* b, const void* pc_llhs,
                                const beer_seg_map* sm, int n_cat, const double* alpha,
                                const double* y, const double* norm, const double* evidence,
                                const int64_t* entry_frame, const int32_t* entry_cat,
                                const int64_t* entry_off, int64_t n_entries, int max_dur,
                                void* out, void* stream) {
    SpPlan p;
    BEER_REQUIRE(sm != nullptr);
    BEER_REQUIRE(sp_plan(dtype, b, n_cat, sm->max_closure, &p));
    BEER_REQUIRE(sm->mem_ptr && sm->members && sm->mem_init && sm->in_ptr && sm->in_src &&
                 sm->in_arc && sm->ent_ptr && sm->ent_src && sm->ent_arc);
    BEER_REQUIRE(n_entries >= 0 && max_dur >= 1);
    BEER_REQUIRE(n_entries / (kSpThreads / p.team) < 0x7fffffff);
    if (n_entries == 0 || b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && alpha && y && norm && evidence && entry_frame && entry_cat &&
                 entry_off && out);
    BEER_DISPATCH(dtype, sp_expand_launch, b, p, pc_llhs, sm, n_cat, alpha, y, norm, evidence,
                  entry_frame, entry_cat, entry_off, n_entries, max_dur, out, stream);
}

int beer_hmm_segposts_route(int dtype, const beer_batch* b, int n_cat, int max_closure) {
    SpPlan p;
    BEER_REQUIRE(sp_plan(dtype, b, n_cat, max_closure, &p));
    return BEER_SEGPOSTS_BLOCK | (p.form.arcs_in_lds ? BEER_SEGPOSTS_ARCS_LDS : 0) |
           (p.form.bins_lds ? BEER_SEGPOSTS_BINS_LDS : 0) | ceil_log2(p.team);
}

}  // extern "C"
