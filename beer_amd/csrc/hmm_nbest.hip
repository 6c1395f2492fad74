// N-best Viterbi: the k best state paths of every utterance of a ragged batch, with their scores
// (include/beer_hip.h: beer_hmm_viterbi_nbest).
//
// Definition.  All arithmetic in the dtype of pc_llhs, in the order viterbi_kernel (hmm.hip) uses:
//     omega_0[j][0] = llh[0,j] + init[j]                      (ranks 1 .. k-1: -inf)
//     candidate c = omega_{t-1}[i][r] + w_ij,   omega_t[j][q] = llh[t,j] + c
//     final candidate omega_{T-1}[j][r] + final[j]
// A cell (t, j) keeps the k best candidates over (arc i -> j, rank r), the end the k best over
// (state j, rank r): larger score first; on equal scores the arc that comes first in the in-CSR
// row (sources ascending), then the smaller rank.  Candidates are visited in exactly that order
// and a candidate enters a list only where it is STRICTLY larger than an entry, so the order of
// the visit is the tie rule and no key is compared.  A candidate of -inf never enters: a rank
// without a finite path has score -inf and a path of -1.
//
// One form: one workgroup per utterance, a thread per state (strided beyond the workgroup).  The
// thread keeps the state's list in registers (K = 1, 2, 4, 8, 16 >= k entries, inserted with
// static indices: no scratch), takes the first arc's candidates as the list they are, and leaves
// a later source's ranks at the first candidate that does not beat its last entry -- the sources'
// lists are sorted.  The two score columns sit in LDS RANK-major,
// [k][S]: the lanes of a wave read neighbouring sources of one rank, which neighbouring banks
// serve; [S][k] would put the lanes k words apart.  As in viterbi_kernel the arc lists are in LDS
// when they fit, the emissions of frame t + 1 are loaded during frame t, and the back-trace walks
// back-pointers staged in LDS by chunks of frames -- k lanes walk the k paths side by side.
// A back-pointer packs (source << 4 | rank) in an int32; -1: absent.

#include <math.h>

#include "hmm_block.h"

using namespace beer;

namespace {

constexpr int kNbThreads = 256;                   // at most; a multiple of 64 that covers S below it
constexpr size_t kNbChunkBytes = 16 * 1024;       // the staged back-pointers stay below this
constexpr int kNbSel = 16;                        // int32: where the k walks stand
static_assert(kNbSel >= BEER_NBEST_MAX, "a slot per path");
static_assert(BEER_NBEST_MAX <= 16, "the rank takes four bits of a back-pointer");

template <typename T>
__device__ __forceinline__ T nb_ninf() { return (T)-INFINITY; }

// The K best candidates seen so far, best first.  `insert` is a no-op for a candidate that does
// not beat the last entry; equal scores keep the order of arrival.
template <typename T, int K>
struct NbList {
    T s[K];
    int b[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < K; ++q) { s[q] = nb_ninf<T>(); b[q] = -1; }
    }
    __device__ __forceinline__ T last() const { return s[K - 1]; }
    __device__ __forceinline__ void insert(T c, int p) {
#pragma unroll
        for (int q = K - 1; q > 0; --q) {
            const bool up = c > s[q - 1];         // c goes above entry q - 1: that one moves down
            const bool at = c > s[q];
            b[q] = up ? b[q - 1] : (at ? p : b[q]);
            s[q] = up ? s[q - 1] : (at ? c : s[q]);
        }
        if (c > s[0]) { s[0] = c; b[0] = p; }
    }
};

// ARCS_LDS is a template argument, not a launch argument: pointers that may be either LDS or
// global memory are read with flat loads, two per arc in the chain of every frame.
template <typename T, int K, bool ARCS_LDS>
__global__ __launch_bounds__(kNbThreads) void nbest_kernel(
    beer_batch b, const T* __restrict__ pc_llhs, int k, int chunk, int32_t* __restrict__ bt_ws,
    int64_t* __restrict__ paths, double* __restrict__ scores, int map_pdf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int u = blockIdx.x, tid = threadIdx.x, nt_ = blockDim.x;
    const int gid = b.graph_id[u];
    const beer_graph g = b.graphs[gid];
    const int S = g.n_states, A = g.n_arcs;
    const int64_t f0 = b.frame_off[u];
    const int64_t T_ = b.frame_off[u + 1] - f0;
    const int64_t n_frames = b.frame_off[b.nutt];
    if (T_ <= 0) {                                          // no frame, no path
        if (tid < k) scores[(int64_t)u * k + tid] = -__builtin_huge_val();
        return;
    }
    const T* llh = pc_llhs + b.llh_off[u];
    int32_t* bt = bt_ws + (int64_t)k * b.llh_off[u];        // [T][k][S]
    const T* init = (const T*)g.init;
    const T* fin = (const T*)g.final;
    const size_t SM = (size_t)b.max_states;
    T* cur = reinterpret_cast<T*>(smem);                                // [k][S]
    T* nxt = cur + (size_t)k * SM;
    int32_t* sel = reinterpret_cast<int32_t*>(nxt + (size_t)k * SM);    // [kNbSel]
    int32_t* btc = sel + kNbSel;                                        // [chunk][k][S]
    int32_t* l_ptr = btc + (size_t)chunk * k * SM;                      // [S + 1]
    int32_t* l_src = l_ptr + SM + 1;                                    // [A]
    T* l_w = reinterpret_cast<T*>(l_src + b.max_arcs + ((b.max_states + 1 + b.max_arcs) & 1));
    if (ARCS_LDS) {
        for (int j = tid; j <= S; j += nt_) l_ptr[j] = g.in_ptr[j];
        for (int e = tid; e < A; e += nt_) { l_src[e] = g.in_src[e]; l_w[e] = ((const T*)g.in_w)[e]; }
    }
    const int32_t* in_ptr = ARCS_LDS ? l_ptr : g.in_ptr;
    const int32_t* in_src = ARCS_LDS ? l_src : g.in_src;
    const T* in_w = ARCS_LDS ? l_w : (const T*)g.in_w;
    for (int j = tid; j < S; j += nt_) {
        cur[j] = llh[j] + init[j];
        for (int r = 1; r < k; ++r) cur[r * S + j] = nb_ninf<T>();
    }
    __syncthreads();
    // (one state per thread in the common case: the prefetch register is per thread)
    const bool one = S <= nt_;
    T ll_next = (T)0;
    if (one && tid < S && T_ > 1) ll_next = llh[S + tid];
    NbList<T, K> L;
    for (int64_t t = 1; t < T_; ++t) {
        const T ll_cur = ll_next;
        if (one && tid < S && t + 1 < T_) ll_next = llh[(t + 1) * S + tid];
        int32_t* bt_t = bt + t * k * S;
        for (int j = tid; j < S; j += nt_) {
            const int e0 = in_ptr[j], e1 = in_ptr[j + 1];
            if (e0 < e1) {
                // the first arc's candidates ARE the list so far: sorted, -inf at its end
                const int src = in_src[e0];
                const T w = in_w[e0];
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const T c = q < k ? cur[q * S + src] + w : nb_ninf<T>();
                    L.s[q] = c;
                    L.b[q] = c > nb_ninf<T>() ? src << 4 | q : -1;
                }
            } else {
                L.clear();
            }
            // (unrolled: the loads of four arcs are in flight together -- a phone start walks
            //  one arc per phone while its neighbours have two)
#pragma unroll 4
            for (int e = e0 + 1; e < e1; ++e) {
                const int src = in_src[e];
                const T w = in_w[e];
                const T c0 = cur[src] + w;
                if (c0 > L.last()) {
                    L.insert(c0, src << 4);
                    for (int r = 1; r < k; ++r) {
                        const T c = cur[r * S + src] + w;
                        if (!(c > L.last())) break;         // (sorted: nor will a later rank)
                        L.insert(c, src << 4 | r);
                    }
                }
            }
            const T ll = one ? ll_cur : llh[t * S + j];
#pragma unroll
            for (int q = 0; q < K; ++q)
                if (q < k) {
                    nxt[q * S + j] = ll + L.s[q];
                    bt_t[q * S + j] = L.b[q];
                }
        }
        __syncthreads();
        T* tmp = cur; cur = nxt; nxt = tmp;
    }
    // the k best ends (thread 0), then the back-trace chunk by chunk
    if (tid == 0) {
        L.clear();
        for (int j = 0; j < S; ++j) {
            const T fj = fin[j];
            for (int r = 0; r < k; ++r) {
                const T c = cur[r * S + j] + fj;
                if (!(c > L.last())) break;
                L.insert(c, j << 4 | r);
            }
        }
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q < k) {
                sel[q] = L.b[q];
                scores[(int64_t)u * k + q] = L.b[q] >= 0 ? (double)L.s[q] : -__builtin_huge_val();
            }
    }
    const int32_t* ids = b.pdf_ids + b.pdf_off[gid];
    int64_t* out = paths + (int64_t)(tid < k ? tid : 0) * n_frames + f0;
    const int64_t frame = (int64_t)k * S;                   // back-pointers of one frame
    for (int64_t hi = T_ - 1; hi >= 0; hi -= chunk) {
        const int64_t lo = hi - chunk + 1 > 0 ? hi - chunk + 1 : 0;     // frames lo .. hi
        __syncthreads();                                    // bt stores / previous chunk done
        // back-pointers of frames max(lo, 1) .. hi (frame 0 has none)
        const int64_t first = lo > 0 ? lo : 1;
        for (int64_t e = tid; e < (hi - first + 1) * frame; e += nt_) btc[e] = bt[first * frame + e];
        __syncthreads();
        if (tid < k) {
            int p = sel[tid];
            for (int64_t t = hi; t >= lo; --t) {
                const int st = p >> 4;
                out[t] = p < 0 ? (int64_t)-1 : (map_pdf ? (int64_t)ids[st] : (int64_t)st);
                if (t > 0 && p >= 0) p = btc[((t - first) * k + (p & 15)) * S + st];
            }
            sel[tid] = p;
        }
    }
}

// The form of a launch, from the batch maxima and k (beer_hmm_nbest_route packs it): false where
// the launch refuses.
struct NbestPlan {
    int K;                   // list entries a thread keeps: the power of two >= k
    int chunk;               // frames of back-pointers staged at a time
    int arcs_in_lds;
    int threads;
    size_t lds;              // dynamic LDS of the launch
};
inline bool nbest_plan(int dtype, const beer_batch* b, int32_t k, NbestPlan* p) {
    if (!block_batch_ok(dtype, b) || k < 1 || k > BEER_NBEST_MAX) return false;
    const size_t S = (size_t)b->max_states, A = (size_t)b->max_arcs;
    const size_t w = dtype == BEER_F32 ? 4 : 8;
    const size_t cols = 2 * S * k * w;                        // two score columns [k][S]
    const size_t row = 4 * S * k;                             // a frame's back-pointers
    p->chunk = 32 * row <= kNbChunkBytes ? 32 : (8 * row <= kNbChunkBytes ? 8 : 2);
    const size_t base = cols + 4 * kNbSel + p->chunk * row;
    if (base > (size_t)kMaxDynLds) return false;
    const size_t arcs = csr_bytes(S, A, w, false, false);
    p->arcs_in_lds = base + arcs <= kBlockArcBytes;
    p->lds = base + (p->arcs_in_lds ? arcs : 0);
    p->K = BEER_NBEST_LIST(k);
    const size_t t64 = (S + 63) / 64 * 64;
    p->threads = (int)(t64 < (size_t)kNbThreads ? t64 : (size_t)kNbThreads);
    return true;
}

template <typename T, int K, bool ARCS_LDS>
int nbest_launch_form(const beer_batch* b, const NbestPlan& p, const void* pc_llhs, int32_t k,
                      int32_t* bt_ws, int64_t* paths, double* scores, int map_pdf, void* stream) {
    return launch_full_lds(nbest_kernel<T, K, ARCS_LDS>, dim3(b->nutt), dim3(p.threads), p.lds,
                           as_stream(stream), *b, (const T*)pc_llhs, (int)k, p.chunk, bt_ws, paths,
                           scores, map_pdf);
}

template <typename T, int K>
int nbest_launch_k(const beer_batch* b, const NbestPlan& p, const void* pc_llhs, int32_t k,
                   int32_t* bt_ws, int64_t* paths, double* scores, int map_pdf, void* stream) {
    if (p.arcs_in_lds)
        return nbest_launch_form<T, K, true>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
    return nbest_launch_form<T, K, false>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
}

template <typename T>
int nbest_launch(const beer_batch* b, const NbestPlan& p, const void* pc_llhs, int32_t k,
                 int32_t* bt_ws, int64_t* paths, double* scores, int map_pdf, void* stream) {
    switch (p.K) {
    case 1: return nbest_launch_k<T, 1>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
    case 2: return nbest_launch_k<T, 2>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
    case 4: return nbest_launch_k<T, 4>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
    case 8: return nbest_launch_k<T, 8>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
    default: return nbest_launch_k<T, 16>(b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
    }
}

}  // namespace

extern "C" {

int beer_hmm_viterbi_nbest(int dtype, const beer_batch* b, const void* pc_llhs, int32_t k,
                           int32_t* bt_ws, int64_t* paths, double* scores, int map_pdf,
                           void* stream) {
    NbestPlan p;
    BEER_REQUIRE(nbest_plan(dtype, b, k, &p));
    if (b->nutt == 0) return BEER_OK;
    BEER_REQUIRE(pc_llhs && bt_ws && paths && scores);
    BEER_DISPATCH(dtype, nbest_launch, b, p, pc_llhs, k, bt_ws, paths, scores, map_pdf, stream);
}

int beer_hmm_nbest_route(int dtype, const beer_batch* b, int32_t k) {
    NbestPlan p;
    BEER_REQUIRE(nbest_plan(dtype, b, k, &p));
    return p.chunk | (p.arcs_in_lds ? BEER_NBEST_ARCS_LDS : 0);
}

}  // extern "C"
