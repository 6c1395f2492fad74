// Explicit state durations (hidden semi-Markov model): forward-backward and Viterbi over
// (state, duration) for every utterance of a ragged batch (include/beer_hip.h:
// beer_hsmm_forward_backward, beer_hsmm_viterbi, beer_hsmm_arc_posteriors -- the definitions
// are there).
//
// One workgroup of 256 threads per utterance, at most 512 workgroups striding over the batch.
// fp64 log space throughout.  The running scores of the segments in progress sit in a ring
// [S][D] indexed by the segment's start (backward pass: its end) mod D.  A frame has three
// phases between barriers:
//   A  a thread per state: the arcs (beg_t from end_{t-1}; backward bend_t from bbeg_{t+1}),
//      after one wave per hub has reduced the hub's value;
//   B  a TEAM of 1 .. 64 lanes per state: every live slot += l_t(j) - c_t - n, the new slot is
//      written, and one log-sum-exp (Viterbi: max) over the slots with the rotated duration law
//      gives end_t(j) (backward: bbeg_t(j), and with the same exponentials the duration counts);
//   R  a block reduction: the next frame's offsets c_{t+1} and n_t.
// Offsets.  Stored values are true values minus a running offset that is the same for every
// state: forward O_t = sum_{tau<=t} c_tau + sum_{tau<t} n_tau, backward Q_t = sum_{tau>=t} c_tau +
// sum_{tau>t} n'_tau.  c_t = rint(max_j l_t(j)) and n = the frame's largest end (begin) value
// rounded to a multiple of 1/256: their running sums are exact, so a posterior's exponent
// N_t + N'_t' - Z is formed without cancellation error and a per-frame shift of the inputs moves
// nothing but the evidence.
// The posteriors come out of the backward pass: with B_t(j), E_t(j) the posteriors that a segment
// of j begins / ends at t, gamma_t = gamma_{t+1} - B_{t+1} + E_t from gamma_{T-1} = E_{T-1}.

#include <type_traits>

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kHsThreads = 256;
constexpr int kHsMaxGrid = 512;          // workgroups of a launch (each with a ring in `ws`)
constexpr int kHsRows = 8;               // per-state rows of doubles in LDS
constexpr int kHsMisc = 32;              // doubles: reduction scratch [16], hub values [4], spare
constexpr int kHsMaxHubs = 4;            // (kMaxHubs of hmm.hip)
constexpr double kHsQuant = 256.0;       // n is a multiple of 1 / kHsQuant

struct HsArgs {
    const double* log_dur;
    const double* leave_w;
    int D, S_total;
    double* ws;
    size_t ring_total;                   // doubles of `ws` taken by the rings (0: rings in LDS)
    int ring_lds, lowdeg, team_log2;
    // forward-backward
    void* gamma;
    double* utt_evidence;
    double* dur_counts;
    double* entry_sum;
    double* gamma0_sum;
    // Viterbi
    int64_t* path;
    double* score;
    int map_pdf;
};

// (fp64 throughout: a log-sum-exp is hmm_block.h's pair, lse_add<double> / lse_value<double>)

// Viterbi: the larger value, the smaller index among equals
__device__ __forceinline__ void hs_best(double& m, int& arg, double v, int i) {
    if (v > m || (v == m && v > neg_inf() && i < arg)) { m = v; arg = i; }
}

// the maxima of two values over the workgroup, in every thread; a barrier separates two calls
__device__ __forceinline__ void hs_block_max2(double& a, double& b, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    a = wave_max(a);
    b = wave_max(b);
    if (lane == 0) { red[w] = a; red[8 + w] = b; }
    __syncthreads();
    a = red[0]; b = red[8];
    for (int i = 1; i < kHsThreads / 64; ++i) { a = dmax(a, red[i]); b = dmax(b, red[8 + i]); }
}
__device__ __forceinline__ double hs_block_sum(double a, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    a = wave_sum(a);
    if (lane == 0) red[w] = a;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < kHsThreads / 64; ++i) r += red[i];
    return r;
}
__device__ __forceinline__ double hs_quant(double v) {
    return v > neg_inf() ? __builtin_rint(v * kHsQuant) / kHsQuant : 0.0;
}

// Arc posteriors by category (beer_hsmm_arc_posteriors): what the ARCS form of the body takes
// besides HsArgs.  Bins as in hmm_arcs.hip: fp64 in LDS behind the rows and the ring while they
// fit (hsmm_arcs_plan), else the output rows themselves with global atomic adds.
struct HsArcArgs {
    beer_arc_map map;
    int n_cat;
    int frame_lds, utt_lds;              // a frame's / the utterance's bins are in LDS
    size_t bins_at;                      // doubles from the start of LDS to the first bin
    void* frame_out;
    double* utt_out;
    double* total_out;
};

// ... and what the other two forms take in its place: nothing, every member a constant
struct HsNoArcs {
    static constexpr int n_cat = 0, frame_lds = 0, utt_lds = 0;
    static constexpr size_t bins_at = 0;
    static constexpr void* frame_out = nullptr;
    static constexpr double* utt_out = nullptr;
    static constexpr double* total_out = nullptr;
};

// fp64 add to a bin in LDS, with the LDS's own instruction (ds_add_f64)
__device__ __forceinline__ void hs_lds_add(double* p, double v) {
    typedef __attribute__((address_space(3))) double lds_double;
    __hip_atomic_fetch_add((lds_double*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

constexpr int kHsFrameCats = 1024;       // a frame's bins stay in LDS up to here ...
constexpr int kHsUttCats = 4096;         // ... and the utterance's up to here

// ARCS (never with VIT): the full CSR whatever the batch offers, and in phase A of the backward
// pass every arc's posterior exp(end_t(j) + w_jk + bbeg_{t+1}(k) - Z) -- the term of bend_t(j)
// that is in hand there, with E_t's own offset kapE -- folded into row t + 1.  false: the code
// of beer_hsmm_forward_backward / beer_hsmm_viterbi, in which `arc` is never read.
template <typename T, bool VIT, bool ARCS>
__global__ __launch_bounds__(kHsThreads) void hsmm_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, HsArgs a,
    typename std::conditional<ARCS, HsArcArgs, HsNoArcs>::type arc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int SM = b.max_states, D = a.D;
    double* rows = reinterpret_cast<double*>(smem);
    double* r0 = rows;                    // forward: end_{t-1}        backward: bbeg_{t+1}
    double* r1 = rows + SM;               // forward: end_{t-1} + leave  backward: bend_t
    double* r2 = rows + 2 * SM;           // forward: beg_t
    double* lv = rows + 3 * SM;           // leave_w[id(j)]
    double* g_row = rows + 4 * SM;        // gamma_{t+1}
    double* bprev = rows + 5 * SM;        // B_{t+1}
    double* ent = rows + 6 * SM;          // sum_{t>=1} B_t
    int* sid = reinterpret_cast<int*>(rows + 7 * SM);      // id(j), -1: outside the table
    double* red = rows + (size_t)kHsRows * SM;
    double* hubv = red + 16;
    double* ring = a.ring_lds ? red + kHsMisc
                              : a.ws + (size_t)blockIdx.x * 2 * (size_t)SM * (size_t)D;
    double* acc = ring + (size_t)SM * D;
    const int team = 1 << a.team_log2, nteams = kHsThreads / team;
    const int tj = tid >> a.team_log2, tl = tid & (team - 1);
    const int n_cat = ARCS ? arc.n_cat : 0;
    double* fbin = rows + (ARCS ? arc.bins_at : 0);          // [n_cat] a frame's bins
    double* ubin = fbin + ((ARCS && arc.frame_lds) ? n_cat : 0);   // [n_cat] the utterance's

    for (int slot = blockIdx.x; slot < b.nutt; slot += gridDim.x) {
        __syncthreads();                                     // the rows of the last utterance
        const int u = b.order ? b.order[slot] : slot;
        const int gi = b.graph_id[u];
        const beer_graph g = b.graphs[gi];
        const int S = g.n_states;
        const int64_t f0 = b.frame_off[u];
        const int64_t T_ = b.frame_off[u + 1] - f0;
        double* urow = (ARCS && arc.utt_out) ? arc.utt_out + (int64_t)u * n_cat : nullptr;
        T* frows = (ARCS && arc.frame_out) ? (T*)arc.frame_out + f0 * n_cat : nullptr;
        if (T_ <= 0) {
            if (tid == 0) {
                if (VIT) a.score[u] = 0.0;
                else if (a.utt_evidence) a.utt_evidence[u] = 0.0;
            }
            if (ARCS && urow)
                for (int c = tid; c < n_cat; c += kHsThreads) urow[c] = 0.0;
            continue;
        }
        const int64_t e0 = b.llh_off[u];
        const T* llh = pc_llhs + e0;
        const int32_t* ids = b.pdf_ids + b.pdf_off[gi];
        const T* init = (const T*)g.init;
        const T* fin = (const T*)g.final;
        double* region = a.ws + a.ring_total + 2 * (size_t)e0 + 2 * (size_t)f0;
        double* begT = region;                               // [T, S] beg_t(j) - O_{t-1}
        double* endT = region + (size_t)T_ * S;              // [T, S] end_t(j) - O_t
        double* ncum = endT + (size_t)T_ * S;                // [T] N_t = sum_{tau<=t} n_tau
        double* cfr = ncum + T_;                             // [T] c_t
        int32_t* bp = reinterpret_cast<int32_t*>(region);    // Viterbi: (source, duration)

        // arcs: the low-degree image and its hubs, or the full CSR
        const bool ld = !VIT && !ARCS && a.lowdeg && g.lowdeg != nullptr;
        beer_graph_lowdeg L = {};
        if (ld) L = *g.lowdeg;
        const int n_hubs = ld ? (L.n_hubs < kHsMaxHubs ? L.n_hubs : kHsMaxHubs) : 0;
        const int32_t* in_ptr = ld ? L.in_ptr : g.in_ptr;
        const int32_t* in_src = ld ? L.in_src : g.in_src;
        const T* in_w = (const T*)(ld ? L.in_w : g.in_w);
        const int32_t* out_ptr = ld ? L.out_ptr : g.out_ptr;
        const int32_t* out_dst = ld ? L.out_dst : g.out_dst;
        const T* out_w = (const T*)(ld ? L.out_w : g.out_w);
        const T* hsw = (const T*)L.hub_src_w;
        const T* hdw = (const T*)L.hub_dst_w;

        for (int j = tid; j < S; j += kHsThreads) {
            const int id = ids[j];
            const bool ok = id >= 0 && id < a.S_total;
            sid[j] = ok ? id : -1;
            lv[j] = (ok && a.leave_w) ? a.leave_w[id] : 0.0;
            ent[j] = 0.0;
        }
        for (int i = tid; i < S * D; i += kHsThreads) ring[i] = neg_inf();
        double cN, dummy = neg_inf();
        {
            double m = neg_inf();
            for (int j = tid; j < S; j += kHsThreads) m = dmax(m, (double)llh[j]);
            hs_block_max2(m, dummy, red);
            cN = m > neg_inf() ? __builtin_rint(m) : 0.0;
        }
        __syncthreads();

        // ------------------------------ forward ------------------------------
        double nprev = 0.0, Nprev = 0.0, Ctot = 0.0;         // n_{t-1}, N_{t-1}, C_{t-1}
        for (int64_t t = 0; t < T_; ++t) {
            if (t > 0 && n_hubs > 0) {
                for (int h = wave; h < n_hubs; h += kHsThreads / 64) {
                    const int p0 = L.src_ptr[h], p1 = L.src_ptr[h + 1];
                    double m = neg_inf();
                    for (int p = p0 + lane; p < p1; p += 64) {
                        const int i = L.src_list[p];
                        m = dmax(m, r1[i] + (double)hsw[i]);
                    }
                    m = wave_max(m);
                    const double base = m > neg_inf() ? m : 0.0;
                    double s = 0.0;
                    for (int p = p0 + lane; p < p1; p += 64) {
                        const int i = L.src_list[p];
                        s += exp(r1[i] + (double)hsw[i] - base);
                    }
                    s = wave_sum(s);
                    if (lane == 0) hubv[h] = lse_value<double>(base, s);
                }
                __syncthreads();
            }
            // A: beg_t
            for (int j = tid; j < S; j += kHsThreads) {
                double bg;
                int src = -1;
                if (t == 0) {
                    bg = (double)init[j];
                } else if (VIT) {
                    bg = neg_inf();
                    for (int e = in_ptr[j]; e < in_ptr[j + 1]; ++e) {
                        const int i = in_src[e];
                        if (i != j) hs_best(bg, src, r1[i] + (double)in_w[e], i);
                    }
                } else {
                    double m = neg_inf(), s = 0.0;
                    for (int e = in_ptr[j]; e < in_ptr[j + 1]; ++e) {
                        const int i = in_src[e];
                        if (i != j) lse_add<double>(m, s, r1[i] + (double)in_w[e]);
                    }
                    const int hd = n_hubs > 0 ? L.hub_dst_id[j] : -1;
                    if (hd >= 0 && hd < n_hubs) {
                        if (L.hub_src_id[j] == hd) {
                            // j feeds the hub that feeds it: the hub's value without j's own term
                            for (int p = L.src_ptr[hd]; p < L.src_ptr[hd + 1]; ++p) {
                                const int i = L.src_list[p];
                                if (i != j) lse_add<double>(m, s, r1[i] + (double)hsw[i] + (double)hdw[j]);
                            }
                        } else {
                            lse_add<double>(m, s, hubv[hd] + (double)hdw[j]);
                        }
                    }
                    bg = lse_value<double>(m, s);
                }
                r2[j] = bg;
                if (VIT) bp[2 * (t * S + j)] = src;
                else begT[t * S + j] = bg;
            }
            __syncthreads();
            // B: the ring and end_t
            const int kn = (int)(t % D);
            for (int jb = 0; jb < S; jb += nteams) {
                const int j = jb + tj;
                const bool valid = j < S;
                const int id = valid ? sid[j] : -1;
                const double aj = valid ? ((double)llh[t * S + j] - cN) - nprev : neg_inf();
                const double bgv = valid ? r2[j] : neg_inf();
                const double* lam = a.log_dur + (size_t)(id < 0 ? 0 : id) * D;
                double* R = ring + (size_t)(valid ? j : 0) * D;
                double m = neg_inf();
                int darg = D + 1;
                if (valid) {
                    for (int k = tl; k < D; k += team) {
                        const double r = (k == kn ? bgv : R[k]) + aj;
                        R[k] = r;
                        int dd = kn - k;
                        if (dd < 0) dd += D;
                        const double v = id < 0 ? neg_inf() : r + lam[dd];
                        if (VIT) hs_best(m, darg, v, dd + 1);
                        else m = dmax(m, v);
                    }
                }
                for (int o = team >> 1; o > 0; o >>= 1) {
                    const double om = __shfl_xor(m, o);
                    if (VIT) {
                        const int od = __shfl_xor(darg, o);
                        hs_best(m, darg, om, od);
                    } else {
                        m = dmax(m, om);
                    }
                }
                double endv = m;
                if (!VIT) {
                    const double base = m > neg_inf() ? m : 0.0;
                    double s = 0.0;
                    if (valid && id >= 0 && m > neg_inf()) {
                        for (int k = tl; k < D; k += team) {
                            int dd = kn - k;
                            if (dd < 0) dd += D;
                            s += exp(R[k] + lam[dd] - base);
                        }
                    }
                    for (int o = team >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    endv = lse_value<double>(base, s);
                }
                if (valid && tl == 0) {
                    r0[j] = endv;
                    r1[j] = endv + lv[j];
                    if (VIT) bp[2 * (t * S + j) + 1] = darg;
                    else endT[t * S + j] = endv;
                }
            }
            __syncthreads();
            // R: n_t and c_{t+1}
            double nm = neg_inf(), cm = neg_inf();
            for (int j = tid; j < S; j += kHsThreads) {
                nm = dmax(nm, r0[j]);
                if (t + 1 < T_) cm = dmax(cm, (double)llh[(t + 1) * S + j]);
            }
            hs_block_max2(nm, cm, red);
            const double nt = hs_quant(nm);
            if (!VIT && tid == 0) { ncum[t] = Nprev + nt; cfr[t] = cN; }
            Ctot += cN;
            if (t + 1 < T_) {
                Nprev += nt;
                nprev = nt;
                cN = cm > neg_inf() ? __builtin_rint(cm) : 0.0;
            }
        }
        // (here Nprev = N_{T-2}: the offset of end_{T-1} is C_{T-1} + N_{T-2})
        __syncthreads();

        if (VIT) {
            double m = neg_inf();
            int arg = S;
            for (int j = tid; j < S; j += kHsThreads) hs_best(m, arg, r0[j] + (double)fin[j], j);
            // the workgroup's best: through LDS, the smaller state among equals
            double* bm = red;
            int* ba = reinterpret_cast<int*>(hubv);
            for (int o = 32; o > 0; o >>= 1) {
                const double om = __shfl_xor(m, o);
                const int oa = __shfl_xor(arg, o);
                hs_best(m, arg, om, oa);
            }
            if (lane == 0) { bm[wave] = m; ba[wave] = arg; }
            __syncthreads();
            m = bm[0]; arg = ba[0];
            for (int i = 1; i < kHsThreads / 64; ++i) hs_best(m, arg, bm[i], ba[i]);
            if (!(m > neg_inf())) {
                for (int64_t t = tid; t < T_; t += kHsThreads) a.path[f0 + t] = -1;
                if (tid == 0) a.score[u] = neg_inf();
                continue;
            }
            if (tid == 0) {
                a.score[u] = (m + Nprev) + Ctot;
                int j = arg;
                int64_t t = T_ - 1;
                while (t >= 0) {
                    int d = bp[2 * (t * S + j) + 1];
                    if (d < 1 || d > t + 1) d = (int)(t + 1);          // (never on a finite path)
                    const int64_t s = t - d + 1;
                    const int64_t lab = a.map_pdf ? (int64_t)ids[j] : (int64_t)j;
                    for (int64_t tau = s; tau <= t; ++tau) a.path[f0 + tau] = lab;
                    if (s == 0) break;
                    const int i = bp[2 * (s * S + j)];
                    if (i < 0 || i >= S) break;                        // (never on a finite path)
                    j = i;
                    t = s - 1;
                }
            }
            continue;
        }

        // ------------------------------ evidence ------------------------------
        T* gamma = (T*)a.gamma + e0;
        double zs;
        {
            double m = neg_inf(), dm = neg_inf();
            for (int j = tid; j < S; j += kHsThreads) m = dmax(m, r0[j] + (double)fin[j]);
            hs_block_max2(m, dm, red);
            __syncthreads();
            const double base = m > neg_inf() ? m : 0.0;
            double s = 0.0;
            for (int j = tid; j < S; j += kHsThreads) s += exp(r0[j] + (double)fin[j] - base);
            s = hs_block_sum(s, red);
            // (written out, as in block_lse: through lse_value the branch order changes)
            zs = s > 0.0 ? base + log(s) : neg_inf();
        }
        if (!(zs > neg_inf())) {
            for (int64_t i = tid; i < T_ * S; i += kHsThreads) gamma[i] = (T)0;
            if (tid == 0 && a.utt_evidence) a.utt_evidence[u] = neg_inf();
            if (ARCS) {
                if (frows)
                    for (int64_t i = tid; i < T_ * n_cat; i += kHsThreads) frows[i] = (T)0;
                if (urow)
                    for (int c = tid; c < n_cat; c += kHsThreads) urow[c] = 0.0;
            }
            continue;
        }
        const double Zs = zs + Nprev;
        if (tid == 0 && a.utt_evidence) a.utt_evidence[u] = Zs + Ctot;
        const bool counts = a.dur_counts != nullptr;
        for (int i = tid; i < S * D; i += kHsThreads) {
            ring[i] = neg_inf();
            if (counts) acc[i] = 0.0;
        }
        // ---- the bins (ARCS) ----
        const bool f_lds = ARCS && frows && arc.frame_lds;
        const bool u_lds = ARCS && arc.utt_lds;
        // where the utterance's sum is kept when not in LDS: its row of utt_out, else total_out
        double* usum = urow ? urow : (ARCS ? arc.total_out : nullptr);
        const int32_t* cat = nullptr;
        const int32_t* icat = nullptr;
        T* frow = frows;                                     // the row the folds go to
        if constexpr (ARCS) {
            cat = arc.map.arc_cat + arc.map.arc_off[gi];
            icat = arc.map.init_cat + arc.map.state_off[gi];
            if (frows && !f_lds)
                for (int64_t i = tid; i < T_ * n_cat; i += kHsThreads) frows[i] = (T)0;
            if (f_lds)
                for (int c = tid; c < n_cat; c += kHsThreads) fbin[c] = 0.0;
            if (u_lds) {
                for (int c = tid; c < n_cat; c += kHsThreads) ubin[c] = 0.0;
            } else if (urow) {
                for (int c = tid; c < n_cat; c += kHsThreads) urow[c] = 0.0;
            }
            __threadfence();
        }
        // a posterior goes to the frame's bin and, unless the row's writer passes it on (flush),
        // to the utterance's
        auto fold = [&](int c, double p) {
            if (c < 0 || !(p > 0.0)) return;
            if (f_lds) {
                hs_lds_add(fbin + c, p);
                return;
            }
            if (frows) unsafeAtomicAdd(frow + c, (T)p);
            if (u_lds) hs_lds_add(ubin + c, p);
            else if (usum) unsafeAtomicAdd(usum + c, p);
        };
        // a row leaves the LDS bins: thread c mod 256 owns bin c of the row and of the sums
        auto flush = [&]() {
            if (!f_lds) return;
            for (int c = tid; c < n_cat; c += kHsThreads) {
                const double v = fbin[c];
                frow[c] = (T)v;
                fbin[c] = 0.0;
                if (u_lds) ubin[c] += v;
                else if (urow) urow[c] += v;
                else if (usum && v != 0.0) unsafeAtomicAdd(usum + c, v);
            }
        };
        __syncthreads();

        // ------------------------------ backward ------------------------------
        double npn = 0.0, Np1 = 0.0, Np2 = 0.0;              // n'_{t+1}, N'_{t+1}, N'_{t+2}
        if (ARCS && frows) frow = frows + (T_ - 1) * n_cat;  // iteration t folds into row t + 1
        for (int64_t t = T_ - 1; t >= 0; --t) {
            const double ct = cfr[t];
            const double Nt1 = t >= 1 ? ncum[t - 1] : 0.0, Nt2 = t >= 2 ? ncum[t - 2] : 0.0;
            const double kapE = (Nt1 + Np2) - Zs, kapB = (Nt2 + Np1) - Zs;
            if (t < T_ - 1 && n_hubs > 0) {
                for (int h = wave; h < n_hubs; h += kHsThreads / 64) {
                    const int p0 = L.dst_ptr[h], p1 = L.dst_ptr[h + 1];
                    double m = neg_inf();
                    for (int p = p0 + lane; p < p1; p += 64) {
                        const int k = L.dst_list[p];
                        m = dmax(m, r0[k] + (double)hdw[k]);
                    }
                    m = wave_max(m);
                    const double base = m > neg_inf() ? m : 0.0;
                    double s = 0.0;
                    for (int p = p0 + lane; p < p1; p += 64) {
                        const int k = L.dst_list[p];
                        s += exp(r0[k] + (double)hdw[k] - base);
                    }
                    s = wave_sum(s);
                    if (lane == 0) hubv[h] = lse_value<double>(base, s);
                }
                __syncthreads();
            }
            // A: bend_t, the end posterior E_t and gamma_t
            for (int j = tid; j < S; j += kHsThreads) {
                double bend;
                if (t == T_ - 1) {
                    bend = (double)fin[j];
                } else {
                    double m = neg_inf(), s = 0.0;
                    // (ARCS) what every arc of j shares in its posterior's exponent
                    const double pre = ARCS ? (endT[t * S + j] + lv[j]) + kapE : 0.0;
                    for (int e = out_ptr[j]; e < out_ptr[j + 1]; ++e) {
                        const int k = out_dst[e];
                        if (k != j) {
                            const double x = r0[k] + (double)out_w[e];
                            lse_add<double>(m, s, x);
                            if (ARCS) {
                                const int c = cat[e];
                                const double px = x + pre;
                                if (c >= 0 && px > neg_inf()) fold(c, exp(px));
                            }
                        }
                    }
                    const int hs = n_hubs > 0 ? L.hub_src_id[j] : -1;
                    if (hs >= 0 && hs < n_hubs) {
                        if (L.hub_dst_id[j] == hs) {
                            for (int p = L.dst_ptr[hs]; p < L.dst_ptr[hs + 1]; ++p) {
                                const int k = L.dst_list[p];
                                if (k != j) lse_add<double>(m, s, r0[k] + (double)hdw[k] + (double)hsw[j]);
                            }
                        } else {
                            lse_add<double>(m, s, hubv[hs] + (double)hsw[j]);
                        }
                    }
                    bend = lse_value<double>(m, s) + lv[j];
                }
                const double ex = endT[t * S + j] + bend + kapE;
                const double E = ex > neg_inf() ? exp(ex) : 0.0;
                const double gm = t == T_ - 1 ? E : (g_row[j] - bprev[j]) + E;
                g_row[j] = gm;
                gamma[t * S + j] = (T)(gm > 0.0 ? gm : 0.0);
                r1[j] = bend;
            }
            __syncthreads();
            // (ARCS) row t + 1 is complete; the next fold lies behind the barrier of phase B
            if (ARCS && t < T_ - 1) {
                flush();
                if (frows) frow -= n_cat;
            }
            // B: the ring, bbeg_t, the begin posterior B_t and the duration counts
            const int kn = (int)(t % D);
            for (int jb = 0; jb < S; jb += nteams) {
                const int j = jb + tj;
                const bool valid = j < S;
                const int id = valid ? sid[j] : -1;
                const double aj = valid ? ((double)llh[t * S + j] - ct) - npn : neg_inf();
                const double bev = valid ? r1[j] : neg_inf();
                const double* lam = a.log_dur + (size_t)(id < 0 ? 0 : id) * D;
                double* V = ring + (size_t)(valid ? j : 0) * D;
                double m = neg_inf();
                if (valid) {
                    for (int k = tl; k < D; k += team) {
                        const double r = (k == kn ? bev : V[k]) + aj;
                        V[k] = r;
                        int dd = k - kn;
                        if (dd < 0) dd += D;
                        m = dmax(m, id < 0 ? neg_inf() : r + lam[dd]);
                    }
                }
                for (int o = team >> 1; o > 0; o >>= 1) m = dmax(m, __shfl_xor(m, o));
                const double base = m > neg_inf() ? m : 0.0;
                double s = 0.0;
                if (valid && id >= 0 && m > neg_inf()) {
                    const double fx = base + begT[t * S + j] + kapB;
                    const double F = fx > neg_inf() ? exp(fx) : 0.0;
                    double* A = acc + (size_t)j * D;
                    for (int k = tl; k < D; k += team) {
                        int dd = k - kn;
                        if (dd < 0) dd += D;
                        const double p = exp(V[k] + lam[dd] - base);
                        s += p;
                        if (counts) A[dd] += p * F;
                    }
                    for (int o = team >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    if (tl == 0) {
                        const double Bv = s * F;
                        r0[j] = lse_value<double>(base, s);
                        bprev[j] = Bv;
                        if (t == 0) {
                            if (a.gamma0_sum) atomicAdd(a.gamma0_sum + j, Bv);
                        } else {
                            ent[j] += Bv;
                        }
                    }
                } else {
                    for (int o = team >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
                    if (valid && tl == 0) { r0[j] = neg_inf(); bprev[j] = 0.0; }
                }
            }
            __syncthreads();
            // R: n'_t
            double nm = neg_inf(), dm = neg_inf();
            for (int j = tid; j < S; j += kHsThreads) nm = dmax(nm, r0[j]);
            hs_block_max2(nm, dm, red);
            const double nt = hs_quant(nm);
            Np2 = Np1;
            Np1 += nt;
            npn = nt;
        }
        __syncthreads();
        if (ARCS) {
            // row 0: B_0(j) = sum_d q(j,0,d), which the last iteration left in `bprev`, by init_cat
            frow = frows;
            for (int j = tid; j < S; j += kHsThreads) fold(icat[j], bprev[j]);
            __syncthreads();
            flush();
            __syncthreads();
            if (u_lds) {
                for (int c = tid; c < n_cat; c += kHsThreads) {
                    const double v = ubin[c];
                    if (urow) urow[c] = v;
                    if (arc.total_out && v != 0.0) unsafeAtomicAdd(arc.total_out + c, v);
                }
            } else if (urow && arc.total_out) {
                // (the row took atomic adds: read it where they landed)
                __threadfence();
                for (int c = tid; c < n_cat; c += kHsThreads) {
                    const double v = unsafeAtomicAdd(urow + c, 0.0);
                    if (v != 0.0) unsafeAtomicAdd(arc.total_out + c, v);
                }
            }
        }
        if (a.entry_sum)
            for (int j = tid; j < S; j += kHsThreads) atomicAdd(a.entry_sum + j, ent[j]);
        if (counts) {
            for (int i = tid; i < S * D; i += kHsThreads) {
                const int j = i / D, id = sid[j];
                const double v = acc[i];
                if (id >= 0 && v != 0.0) atomicAdd(a.dur_counts + (size_t)id * D + (i - j * D), v);
            }
        }
    }
}

// The form of a launch (beer_hsmm_route packs it): false where the launch refuses
struct HsmmPlan {
    int team_log2, ring_lds, lowdeg, grid;
    size_t lds, ring_total;
};
inline bool hsmm_plan(int dtype, const beer_batch* b, int D, HsmmPlan* p) {
    if (!b || b->nutt < 0 || (dtype != BEER_F32 && dtype != BEER_F64) || D < 1 ||
        D > BEER_HSMM_MAX_DUR || b->max_states < 1 || b->max_states > BEER_HSMM_MAX_STATES)
        return false;
    const size_t S = (size_t)b->max_states;
    const size_t rows = (kHsRows * S + kHsMisc) * 8, ring = 2 * S * (size_t)D * 8;
    p->ring_lds = rows + ring <= (size_t)kMaxDynLds;
    p->lds = rows + (p->ring_lds ? ring : 0);
    p->lowdeg = b->all_lowdeg != 0 && b->max_degree > 0 && b->max_hubs <= kHsMaxHubs;
    int team = 1, lg = 0;
    while (team * 2 <= 64 && team < D && (size_t)team * 2 * S <= (size_t)kHsThreads) {
        team *= 2;
        ++lg;
    }
    p->team_log2 = lg;
    p->grid = b->nutt < kHsMaxGrid ? b->nutt : kHsMaxGrid;
    p->ring_total = p->ring_lds ? 0 : (size_t)p->grid * 2 * S * (size_t)D;
    return true;
}

template <typename T, bool VIT>
int hsmm_launch(const beer_batch* b, const HsmmPlan& p, const void* pc_llhs, const HsArgs& a,
                void* stream) {
    return launch_full_lds(hsmm_kernel<T, VIT, false>, dim3(p.grid), dim3(kHsThreads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, a, HsNoArcs{});
}
template <typename T>
int hsmm_launch_fb(const beer_batch* b, const HsmmPlan& p, const void* pc_llhs, const HsArgs& a,
                   void* stream) {
    return hsmm_launch<T, false>(b, p, pc_llhs, a, stream);
}
template <typename T>
int hsmm_launch_vit(const beer_batch* b, const HsmmPlan& p, const void* pc_llhs, const HsArgs& a,
                    void* stream) {
    return hsmm_launch<T, true>(b, p, pc_llhs, a, stream);
}

// The form of beer_hsmm_arc_posteriors (beer_hsmm_arcs_route packs it): the plan above without
// the low-degree images, and the bins behind the rows and the ring while they fit
struct HsmmArcsPlan {
    HsmmPlan base;
    int frame_lds, utt_lds;
    size_t bins_at;
};
inline bool hsmm_arcs_plan(int dtype, const beer_batch* b, int D, int n_cat, bool want_frames,
                           HsmmArcsPlan* p) {
    if (!hsmm_plan(dtype, b, D, &p->base) || n_cat < 1) return false;
    p->base.lowdeg = 0;
    const size_t bins = 8 * (size_t)n_cat;
    size_t lds = p->base.lds;
    p->bins_at = lds / 8;
    p->frame_lds = want_frames && n_cat <= kHsFrameCats && lds + bins <= (size_t)kMaxDynLds;
    if (p->frame_lds) lds += bins;
    p->utt_lds = n_cat <= kHsUttCats && lds + bins <= (size_t)kMaxDynLds;
    if (p->utt_lds) lds += bins;
    p->base.lds = lds;
    return true;
}

template <typename T>
int hsmm_launch_arcs(const beer_batch* b, const HsmmPlan& p, const void* pc_llhs, const HsArgs& a,
                     const HsArcArgs& arc, void* stream) {
    return launch_full_lds(hsmm_kernel<T, false, true>, dim3(p.grid), dim3(kHsThreads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, a, arc);
}

HsArgs hsmm_args(const HsmmPlan& p, const double* log_dur, const double* leave_w, int D,
                 int S_total, double* ws) {
    HsArgs a = {};
    a.log_dur = log_dur;
    a.leave_w = leave_w;
    a.D = D;
    a.S_total = S_total;
    a.ws = ws;
    a.ring_total = p.ring_total;
    a.ring_lds = p.ring_lds;
    a.lowdeg = p.lowdeg;
    a.team_log2 = p.team_log2;
    return a;
}

}  // namespace

extern "C" {

int beer_hsmm_forward_backward(int dtype, const beer_batch* b, const void* pc_llhs,
                               const double* log_dur, const double* leave_w, int D, int S_total,
                               double* ws, void* gamma, double* utt_evidence,
                               double* dur_counts, double* entry_sum, double* gamma0_sum,
                               void* stream) {
    HsmmPlan p;
    BEER_REQUIRE(hsmm_plan(dtype, b, D, &p));
    BEER_REQUIRE(S_total >= 1);
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && log_dur && ws && gamma);
    HsArgs a = hsmm_args(p, log_dur, leave_w, D, S_total, ws);
    a.gamma = gamma;
    a.utt_evidence = utt_evidence;
    a.dur_counts = dur_counts;
    a.entry_sum = entry_sum;
    a.gamma0_sum = gamma0_sum;
    BEER_DISPATCH(dtype, hsmm_launch_fb, b, p, pc_llhs, a, stream);
}

int beer_hsmm_viterbi(int dtype, const beer_batch* b, const void* pc_llhs, const double* log_dur,
                      const double* leave_w, int D, int S_total, double* ws, int64_t* path,
                      double* score, int map_pdf, void* stream) {
    HsmmPlan p;
    BEER_REQUIRE(hsmm_plan(dtype, b, D, &p));
    BEER_REQUIRE(S_total >= 1);
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && log_dur && ws && path && score);
    HsArgs a = hsmm_args(p, log_dur, leave_w, D, S_total, ws);
    a.path = path;
    a.score = score;
    a.map_pdf = map_pdf;
    BEER_DISPATCH(dtype, hsmm_launch_vit, b, p, pc_llhs, a, stream);
}

int beer_hsmm_arc_posteriors(int dtype, const beer_batch* b, const void* pc_llhs,
                             const double* log_dur, const double* leave_w, int D, int S_total,
                             const beer_arc_map* map, int n_cat, double* ws, void* gamma,
                             double* utt_evidence, double* dur_counts, double* entry_sum,
                             double* gamma0_sum, void* frame_out, double* utt_out,
                             double* total_out, void* stream) {
    HsmmArcsPlan p;
    BEER_REQUIRE(hsmm_arcs_plan(dtype, b, D, n_cat, frame_out != nullptr, &p));
    BEER_REQUIRE(S_total >= 1);
    BEER_REQUIRE(frame_out || utt_out || total_out);
    BEER_REQUIRE(map && map->arc_cat && map->init_cat && map->arc_off && map->state_off);
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && log_dur && ws && gamma);
    HsArgs a = hsmm_args(p.base, log_dur, leave_w, D, S_total, ws);
    a.gamma = gamma;
    a.utt_evidence = utt_evidence;
    a.dur_counts = dur_counts;
    a.entry_sum = entry_sum;
    a.gamma0_sum = gamma0_sum;
    HsArcArgs arc = {};
    arc.map = *map;
    arc.n_cat = n_cat;
    arc.frame_lds = p.frame_lds;
    arc.utt_lds = p.utt_lds;
    arc.bins_at = p.bins_at;
    arc.frame_out = frame_out;
    arc.utt_out = utt_out;
    arc.total_out = total_out;
    BEER_DISPATCH(dtype, hsmm_launch_arcs, b, p.base, pc_llhs, a, arc, stream);
}

size_t beer_hsmm_arcs_scratch_doubles(int dtype, const beer_batch* b, int D) {
    HsmmPlan p;
    if (!hsmm_plan(dtype, b, D, &p)) return 0;
    return p.ring_total;
}

int beer_hsmm_arcs_route(int dtype, const beer_batch* b, int D, int n_cat, int want_frames) {
    HsmmArcsPlan p;
    BEER_REQUIRE(hsmm_arcs_plan(dtype, b, D, n_cat, want_frames != 0, &p));
    return BEER_HSMM_BLOCK | (p.base.ring_lds ? BEER_HSMM_RING_LDS : 0) |
           (p.frame_lds ? BEER_HSMM_ARCS_FRAME_LDS : 0) |
           (p.utt_lds ? BEER_HSMM_ARCS_UTT_LDS : 0) | p.base.team_log2;
}

size_t beer_hsmm_scratch_doubles(int dtype, const beer_batch* b, int D) {
    HsmmPlan p;
    if (!hsmm_plan(dtype, b, D, &p)) return 0;
    return p.ring_total;
}

int beer_hsmm_route(int dtype, const beer_batch* b, int D) {
    HsmmPlan p;
    BEER_REQUIRE(hsmm_plan(dtype, b, D, &p));
    return BEER_HSMM_BLOCK | (p.ring_lds ? BEER_HSMM_RING_LDS : 0) |
           (p.lowdeg ? BEER_HSMM_LOWDEG : 0) | p.team_log2;
}

}  // extern "C"
