// Token sequences on the device: pdf-id paths collapsed into unit sequences, and the Levenshtein
// distance of a ragged batch of sequence pairs (include/beer_hip.h: beer_unit_sequences,
// beer_edit_distance, beer_edit_distance_route).  Integer arithmetic throughout: every answer is
// exact and a run gives the same bits every time (no atomics, no order left to the hardware).
//
// Edit distance.  D[i][j] is the cost of aligning the first i symbols of the SHORTER sequence of a
// pair (the rows) with the first j of the longer one (the columns):
//     D[i][0] = i * row,   D[0][j] = j * col,
//     D[i][j] = min(D[i-1][j-1] + (s_i == l_j ? 0 : sub), D[i-1][j] + row, D[i][j-1] + col)
// `row` is the step that consumes a row symbol alone -- a deletion when the rows are sequence a,
// an insertion when they are b -- and `col` the other one.  A cell is either the cost alone
// (uint32, every step 1) or the cost with the substitutions and deletions behind it in one uint64
// (EdCell<uint64_t>): a step adds its vector, the minimum is the integer minimum, which orders
// (cost, sub, del) lexicographically; adding the same vector to two cells keeps their order, so
// the recursion is still Bellman's and the cell of (n, m) is the smallest (cost, sub, del, ins)
// over ALL alignments.  No back-trace, no tie rule on directions.
//
// Form.  A team of 8 / 16 / 32 / 64 lanes owns a pair, lane r the row i0 + r + 1 of a strip of
// TEAM rows, and the strip is swept by anti-diagonals: at step s lane r fills column s - r + 1.
// What it needs is its own last value (left), the last value of the lane below it (up) and what
// that lane held a step earlier (diagonal): ONE cross-lane shift of the cells per step
// (v_mov_b32 with DPP wave_shr:1 -- no LDS crossbar, no LDS).  The column symbols travel down
// the lanes by the same shift.  Lane 0 of a team takes its column symbol and the cell above the
// strip from a second register that is loaded 64 (TEAM) columns at a time, one chunk ahead, and
// shifts the OTHER way every step (wave_shl:1): after k steps lane 0 holds what lane k loaded.
// What a neighbouring team shifts in at a team's last lane needs TEAM steps to reach lane 0, and
// the register is reloaded by then.
// A shorter sequence above 64 symbols runs as strips of 64 rows; the last row of a strip
// (len_long + 1 cells) waits for the next strip in a wave-private slice of LDS or, beyond 16 KiB,
// of the caller's workspace.  Lane 63 overwrites cell j of it 62 steps or more after the chunk
// that holds cell j was loaded: one row, in place.

#include "common.h"

using namespace beer;

namespace {

constexpr int kEdThreads = 256;                    // four waves
constexpr int kEdWaves = kEdThreads / 64;
constexpr size_t kEdRowBytes = 16 * 1024;          // a wave's slice of LDS for the boundary row
constexpr int kRowNone = 0, kRowLds = 1, kRowWs = 2;

template <typename C> struct EdCell;
template <> struct EdCell<uint32_t> {
    static constexpr uint32_t kSub = 1, kDel = 1, kIns = 1;
    static __device__ __forceinline__ void store(uint32_t c, int32_t* dist, int32_t* ops) {
        *dist = (int32_t)c;
    }
};
// cost << 42 | substitutions << 21 | deletions; insertions = cost - sub - del
template <> struct EdCell<uint64_t> {
    static constexpr int kField = 21;
    static_assert((1 << kField) - 1 == BEER_EDIT_MAX_LEN_OPS, "the header states the limit");
    static constexpr uint64_t kIns = 1ull << (2 * kField);
    static constexpr uint64_t kDel = kIns | 1ull;
    static constexpr uint64_t kSub = kIns | (1ull << kField);
    static __device__ __forceinline__ void store(uint64_t c, int32_t* dist, int32_t* ops) {
        const int32_t cost = (int32_t)(c >> (2 * kField));
        const int32_t sub = (int32_t)((c >> kField) & ((1u << kField) - 1));
        const int32_t del = (int32_t)(c & ((1u << kField) - 1));
        *dist = cost;
        ops[0] = sub;
        ops[1] = del;
        ops[2] = cost - sub - del;
    }
};

// lane i takes the value of lane i - 1 (DOWN = true; lane 0 gets 0) or of lane i + 1 (lane 63
// gets 0), over the whole wave
template <bool DOWN>
__device__ __forceinline__ uint32_t wave_shift1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, DOWN ? 0x138 : 0x130, 0xf, 0xf, true);
}
template <bool DOWN>
__device__ __forceinline__ int32_t wave_shift1(int32_t v) {
    return (int32_t)wave_shift1<DOWN>((uint32_t)v);
}
template <bool DOWN>
__device__ __forceinline__ uint64_t wave_shift1(uint64_t v) {
    return ((uint64_t)wave_shift1<DOWN>((uint32_t)(v >> 32)) << 32) | wave_shift1<DOWN>((uint32_t)v);
}

template <typename C>
__device__ __forceinline__ C cell_min(C a, C b) { return b < a ? b : a; }

template <typename C, int TEAM, int ROW>
__global__ __launch_bounds__(kEdThreads) void edit_kernel(
    const int32_t* __restrict__ sym, const int64_t* __restrict__ start,
    const int32_t* __restrict__ len, int64_t n_seq, const int32_t* __restrict__ pair_a,
    const int32_t* __restrict__ pair_b, int64_t n_pair, int row_cap, C* ws,
    int32_t* __restrict__ dist, int32_t* __restrict__ ops) {
    static_assert(ROW == kRowNone || TEAM == 64, "strips are whole waves");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = EdCell<C>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tl = lane & (TEAM - 1);
    const int64_t wave_id = (int64_t)blockIdx.x * kEdWaves + wave;
    const int64_t p = wave_id * (64 / TEAM) + lane / TEAM;
    const bool have = p < n_pair;
    // a pair this form cannot hold, or one that names no sequence, computes nothing: dist -1
    bool bad = false, a_rows = true;
    int ns = 0, nl = 0;
    const int32_t *S = sym, *L = sym;
    if (have) {
        const int64_t a = pair_a[p], b = pair_b[p];
        if (a < 0 || a >= n_seq || b < 0 || b >= n_seq) {
            bad = true;
        } else {
            const int la = len[a], lb = len[b];
            a_rows = la <= lb;
            ns = a_rows ? la : lb;
            nl = a_rows ? lb : la;
            S = sym + start[a_rows ? a : b];
            L = sym + start[a_rows ? b : a];
            bad = ns < 0 || (ROW == kRowNone ? ns > TEAM : nl + 1 > row_cap);
        }
        if (bad) ns = nl = 0;
    }
    const C step_row = a_rows ? E::kDel : E::kIns, step_col = a_rows ? E::kIns : E::kDel;
    C* row = nullptr;
    if (ROW == kRowLds) row = reinterpret_cast<C*>(smem) + (size_t)wave * row_cap;
    if (ROW == kRowWs) row = ws + (size_t)wave_id * row_cap;
    // one strip, the steps of the wave's longest team; or the strips of the wave's one pair
    int n_rows = ns;
    if (ROW != kRowNone) n_rows = __builtin_amdgcn_readfirstlane(ns);
    C cur = (C)nl * step_col;                               // (no rows at all: D[0][nl])
    for (int i0 = 0; i0 < (ROW == kRowNone ? 1 : n_rows); i0 += TEAM) {
        const int rows = ns - i0 < TEAM ? ns - i0 : TEAM;
        const int i = i0 + tl + 1;
        const bool row_ok = tl < rows;
        const bool first = i0 == 0, last = i0 + TEAM >= ns;
        const int32_t srow = row_ok ? S[i - 1] : 0;
        int steps = rows > 0 ? nl + rows - 1 : 0;
        steps = ROW == kRowNone ? wave_max(steps) : __builtin_amdgcn_readfirstlane(steps);
        if (rows > 0) cur = (C)i * step_row;                // D[i][0]
        C up_before = (C)i0 * step_row;                     // lane 0: D[i0][0]
        // the cells above the strip and the column symbols, TEAM columns at a time, one ahead
        auto top_of = [&](int j) -> C {
            if (ROW == kRowNone || first) return (C)j * step_col;
            return j <= nl ? row[j] : (C)0;
        };
        int32_t next_sym = tl < nl ? L[tl] : 0;
        C next_top = top_of(1 + tl);
        int32_t csym = 0;
        for (int s0 = 0; s0 < steps; s0 += TEAM) {
            int32_t feed_sym = next_sym;
            C feed_top = next_top;
            next_sym = s0 + TEAM + tl < nl ? L[s0 + TEAM + tl] : 0;
            next_top = top_of(s0 + TEAM + 1 + tl);
#pragma unroll 4
            for (int k = 0; k < TEAM; ++k) {
                C up = wave_shift1<true>(cur);
                csym = wave_shift1<true>(csym);
                if (tl == 0) { up = feed_top; csym = feed_sym; }
                feed_top = wave_shift1<false>(feed_top);
                feed_sym = wave_shift1<false>(feed_sym);
                const C diag = up_before;
                up_before = up;
                const int j = s0 + k - tl + 1;
                if (row_ok && j >= 1 && j <= nl) {
                    C best = diag + (csym == srow ? (C)0 : E::kSub);
                    best = cell_min(best, up + step_row);
                    cur = cell_min(best, cur + step_col);
                    if (ROW != kRowNone && !last && tl == TEAM - 1) row[j] = cur;
                }
            }
        }
        // the row this strip left is read by other lanes of the wave in the next
        if (ROW == kRowLds) wave_order();
        if (ROW == kRowWs) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (have && tl == (ns > 0 ? (ns - 1) & (TEAM - 1) : 0)) {
        if (bad) {
            dist[p] = -1;
            if (ops) ops[3 * p] = ops[3 * p + 1] = ops[3 * p + 2] = -1;
        } else {
            E::store(cur, dist + p, ops + 3 * p);
        }
    }
}

// The form of a launch, from the batch maxima (beer_edit_distance_route packs it): false where the
// launch refuses.
struct EditPlan {
    int team;                // lanes per pair
    int row;                 // kRowNone / kRowLds / kRowWs
    int ops;
    int row_cap;             // cells of a wave's boundary row
    size_t cell, lds;
};
inline bool edit_plan(int32_t max_short, int32_t max_long, int want_ops, EditPlan* p) {
    if (max_short < 0 || max_long < max_short) return false;
    if (max_long > (want_ops ? BEER_EDIT_MAX_LEN_OPS : BEER_EDIT_MAX_LEN)) return false;
    p->ops = want_ops != 0;
    p->cell = want_ops ? 8 : 4;
    p->team = max_short <= 8 ? 8 : (max_short <= 16 ? 16 : (max_short <= 32 ? 32 : 64));
    p->row = max_short <= 64 ? kRowNone
                             : (((size_t)max_long + 1) * p->cell <= kEdRowBytes ? kRowLds : kRowWs);
    p->row_cap = p->row == kRowNone ? 0 : max_long + 1;
    p->lds = p->row == kRowLds ? (size_t)kEdWaves * p->row_cap * p->cell : 0;
    return true;
}
inline int64_t edit_blocks(const EditPlan& p, int64_t n_pair) {
    const int64_t per_block = (int64_t)kEdWaves * (64 / p.team);
    return (n_pair + per_block - 1) / per_block;
}
inline size_t edit_scratch(const EditPlan& p, int64_t n_pair) {
    if (p.row != kRowWs) return 0;
    return (size_t)edit_blocks(p, n_pair) * kEdWaves * (size_t)p.row_cap * p.cell;
}

struct EditArgs {
    const int32_t* sym; const int64_t* start; const int32_t* len; int64_t n_seq;
    const int32_t* pair_a; const int32_t* pair_b; int64_t n_pair;
    int32_t* dist; int32_t* ops; void* ws;
};

template <typename C, int TEAM, int ROW>
int edit_launch_form(const EditPlan& p, const EditArgs& a, void* stream) {
    hipLaunchKernelGGL((edit_kernel<C, TEAM, ROW>), dim3((unsigned)edit_blocks(p, a.n_pair)),
                       dim3(kEdThreads), p.lds, as_stream(stream), a.sym, a.start, a.len, a.n_seq,
                       a.pair_a, a.pair_b, a.n_pair, p.row_cap, (C*)a.ws, a.dist, a.ops);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

template <typename C>
int edit_launch(const EditPlan& p, const EditArgs& a, void* stream) {
    if (p.row == kRowLds) return edit_launch_form<C, 64, kRowLds>(p, a, stream);
    if (p.row == kRowWs) return edit_launch_form<C, 64, kRowWs>(p, a, stream);
    switch (p.team) {
    case 8: return edit_launch_form<C, 8, kRowNone>(p, a, stream);
    case 16: return edit_launch_form<C, 16, kRowNone>(p, a, stream);
    case 32: return edit_launch_form<C, 32, kRowNone>(p, a, stream);
    default: return edit_launch_form<C, 64, kRowNone>(p, a, stream);
    }
}

// ---------------------------------------------------------------------------
// unit sequences
// ---------------------------------------------------------------------------
// One wave per sequence, 64 frames at a time: the frames that start a unit are a ballot, a
// start's place among the units the population count of the ballot below its lane plus the count
// the earlier chunks carried over; the previous frame's symbol comes from the lane below (the
// last lane's is carried to the next chunk).
__global__ __launch_bounds__(kEdThreads) void unit_kernel(
    const int64_t* __restrict__ sym, const int64_t* __restrict__ start,
    const int32_t* __restrict__ len, int64_t n_seq, const int32_t* __restrict__ unit_of_pdf,
    int n_pdf, int32_t* __restrict__ units, int32_t* __restrict__ n_units,
    int32_t* __restrict__ frame_unit) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * kEdWaves + (threadIdx.x >> 6);
    if (q >= n_seq) return;
    const int64_t st = start[q];
    const int n = len[q];
    int result = 0;
    if (n > 0 && sym[st] < 0) {
        result = -1;                                        // a rank without a path
    } else if (n > 0) {
        int count = 0, carry_unit = -1;
        int64_t carry_sym = -1;
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            const bool in = t < n;
            const int64_t pdf = in ? sym[st + t] : 0;
            const bool known = pdf >= 0 && pdf < n_pdf;
            const int u = in && known ? unit_of_pdf[pdf] : -1;
            // a pdf outside the table, or a first frame inside a unit
            if (__ballot(in && (!known || (t == 0 && u < 0)))) { count = -2; break; }
            uint64_t before = wave_shift1<true>((uint64_t)pdf);
            if (lane == 0) before = (uint64_t)carry_sym;
            const bool starts = in && (t == 0 || ((uint64_t)pdf != before && u >= 0));
            const unsigned long long mask = __ballot(starts);
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            if (starts) units[st + count + __popcll(below)] = u;
            if (frame_unit) {
                // the running unit: that of the last start at or below this lane
                const unsigned long long upto = below | (starts ? 1ull << lane : 0ull);
                const int from = upto ? 63 - __clzll((long long)upto) : 0;
                const int mine = __shfl(u, from);
                if (in) frame_unit[st + t] = upto ? mine : carry_unit;
            }
            if (mask) carry_unit = __shfl(u, 63 - __clzll((long long)mask));
            carry_sym = __shfl((long long)pdf, 63);
            count += __popcll(mask);
        }
        result = count;
    }
    if (lane == 0) n_units[q] = result;
}

}  // namespace

extern "C" {

int beer_unit_sequences(const int64_t* sym, const int64_t* start, const int32_t* len,
                        int64_t n_seq, const int32_t* unit_of_pdf, int32_t n_pdf, int32_t* units,
                        int32_t* n_units, int32_t* frame_unit, void* stream) {
    BEER_REQUIRE(n_seq >= 0 && n_seq <= (int64_t)0x7fffffff * kEdWaves && n_pdf >= 1);
    if (n_seq == 0) return BEER_OK;
    BEER_REQUIRE(sym && start && len && unit_of_pdf && units && n_units);
    hipLaunchKernelGGL(unit_kernel, dim3((unsigned)((n_seq + kEdWaves - 1) / kEdWaves)),
                       dim3(kEdThreads), 0, as_stream(stream), sym, start, len, n_seq, unit_of_pdf,
                       (int)n_pdf, units, n_units, frame_unit);
    BEER_LAUNCH_CHECK();
    return BEER_OK;
}

int beer_edit_distance(const int32_t* sym, const int64_t* start, const int32_t* len, int64_t n_seq,
                       const int32_t* pair_a, const int32_t* pair_b, int64_t n_pair,
                       int32_t max_short, int32_t max_long, int32_t* dist, int32_t* ops,
                       void* workspace, size_t workspace_bytes, void* stream) {
    EditPlan p;
    BEER_REQUIRE(edit_plan(max_short, max_long, ops != nullptr, &p));
    BEER_REQUIRE(n_seq >= 0 && n_pair >= 0 && edit_blocks(p, n_pair) <= 0x7fffffff);
    if (n_pair == 0) return BEER_OK;
    BEER_REQUIRE(n_seq >= 1 && sym && start && len && pair_a && pair_b && dist);
    const size_t need = edit_scratch(p, n_pair);
    BEER_REQUIRE(need == 0 || (workspace && workspace_bytes >= need));
    const EditArgs a = {sym, start, len, n_seq, pair_a, pair_b, n_pair, dist, ops, workspace};
    return p.ops ? edit_launch<uint64_t>(p, a, stream) : edit_launch<uint32_t>(p, a, stream);
}

size_t beer_edit_distance_scratch_bytes(int64_t n_pair, int32_t max_short, int32_t max_long,
                                        int want_ops) {
    EditPlan p;
    if (n_pair <= 0 || !edit_plan(max_short, max_long, want_ops, &p)) return 0;
    return edit_scratch(p, n_pair);
}

int beer_edit_distance_route(int32_t max_short, int32_t max_long, int want_ops) {
    EditPlan p;
    BEER_REQUIRE(edit_plan(max_short, max_long, want_ops, &p));
    return p.team | (p.ops ? BEER_EDIT_OPS : 0) |
           (p.row == kRowLds ? BEER_EDIT_ROW_LDS : (p.row == kRowWs ? BEER_EDIT_ROW_WS : 0));
}

}  // extern "C"
