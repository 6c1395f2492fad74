"""The float64 truth of the Viterbi max-marginals (csrc/hmm_lattice.hip): plain numpy on the
graphs and inputs of tests/fb_truth.py, float32 inputs upcast (no GPU needed).

 * `max_marginals`: (best, mm [T, S], frame [T, n_cat], utt [n_cat]) by the definition of
   include/beer_hip.h (beer_hmm_max_marginals), the additions in its bracketed order;
 * `brute_force`: the same by enumeration of all S^T state paths;
 * `bound`: B_u, what every term and every partial sum of an utterance is bounded by;
 * `tolerance`: the derived error bound of an output of an utterance of T frames;
 * `route_formula`: beer_hmm_maxmarg_route restated from the header's text."""

import itertools

import numpy as np

from arcs_truth import out_arcs, random_categories          # (the same arc order and categories)

EINVAL = -100000            # BEER_EINVAL
BLOCK, ARCS_LDS, BINS_LDS = 0x1000, 0x100, 0x200
NINF = -np.inf


def route_formula(S, A, itemsize, n_cat, want_state, want_frames, want_utt):
    """beer_hmm_maxmarg_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or A < 0 or itemsize not in (4, 8):
        return EINVAL
    if not (want_state or want_frames or want_utt):
        return EINVAL
    cats = bool(want_frames or want_utt)
    if cats and n_cat < 1:
        return EINVAL
    rows = 16 * S + 128
    if rows > 160 * 1024:
        return EINVAL
    arcs = 4 * (S + 2 + A) + itemsize * (A + 1) + (4 * A if cats else 0)
    route = BLOCK
    if rows + arcs <= 64 * 1024:
        route |= ARCS_LDS
    if cats and n_cat <= 2048 and rows <= 96 * 1024:
        route |= BINS_LDS
    return route


def _f64(graph):
    return tuple(np.asarray(graph[k], dtype=np.float64) for k in ('init', 'final', 'trans'))


def gamma_categories(graph):
    "(arc_cat, init_cat, n_cat) of the 'gamma' kind: an arc counts for its destination."
    return out_arcs(graph)[1].astype(np.int32), np.arange(graph['S'], dtype=np.int32), graph['S']


def arc_categories(graph):
    "(arc_cat, init_cat, n_cat) of the 'arc' kind: one category per arc, no state counts."
    A = len(out_arcs(graph)[0])
    return np.arange(A, dtype=np.int32), np.full(graph['S'], -1, dtype=np.int32), max(A, 1)


def _sub(x, best):
    'x - best, -inf where x is (never NaN: best is finite here).'
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(x), x - best, NINF)


def max_marginals(graph, llh, arc_cat=None, init_cat=None, n_cat=0):
    '''(best, mm [T, S], frame [T, n_cat] or None, utt [n_cat] or None) in float64 by the
    definition, the additions in the bracketed order of the header; a dead utterance (best =
    -inf) holds -inf everywhere.'''
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    cats = arc_cat is not None
    frame = np.full((T, n_cat), NINF) if cats else None
    with np.errstate(invalid='ignore'):
        d = np.empty((T, S))
        d[0] = llh[0] + init
        for t in range(1, T):
            d[t] = (d[t - 1][:, None] + trans).max(0) + llh[t]
        best = float((d[T - 1] + final).max())
        if not np.isfinite(best):
            return NINF, np.full((T, S), NINF), frame, (np.full(n_cat, NINF) if cats else None)
        e = np.empty((T, S))
        e[T - 1] = final
        for t in range(T - 2, -1, -1):
            e[t] = (trans + (llh[t + 1] + e[t + 1])[None, :]).max(1)
        mm = _sub(d + e, best)
        if cats:
            arc_cat, init_cat = np.asarray(arc_cat), np.asarray(init_cat)
            src, dst = out_arcs(graph)
            w = trans[src, dst]
            assert len(arc_cat) == len(src) and len(init_cat) == S
            keep = init_cat >= 0
            np.maximum.at(frame[0], init_cat[keep], mm[0][keep])
            keep = arc_cat >= 0
            for t in range(1, T):
                am = _sub(((d[t - 1][src] + w) + llh[t][dst]) + e[t][dst], best)
                np.maximum.at(frame[t], arc_cat[keep], am[keep])
    return best, mm, frame, (frame.max(0) if cats else None)


def brute_force(graph, llh, arc_cat=None, init_cat=None, n_cat=0):
    'The same by enumeration: every path raises the cells and bins it passes to its score.'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    cats = arc_cat is not None
    mm = np.full((T, S), NINF)
    frame = np.full((T, n_cat), NINF) if cats else None
    if cats:
        src, dst = out_arcs(graph)
        cat_of = -np.ones((S, S), dtype=np.int64)
        cat_of[src, dst] = np.asarray(arc_cat)
    best = NINF
    rows = np.arange(T)
    with np.errstate(invalid='ignore'):
        for path in itertools.product(range(S), repeat=T):
            p = np.asarray(path)
            # (left to right, as the forward recursion adds: exact on integer inputs anyway)
            s = llh[0, p[0]] + init[p[0]]
            for t in range(1, T):
                s = (s + trans[p[t - 1], p[t]]) + llh[t, p[t]]
            s = s + final[p[-1]]
            if not np.isfinite(s):
                continue
            best = max(best, s)
            mm[rows, p] = np.maximum(mm[rows, p], s)
            if cats:
                if init_cat[p[0]] >= 0:
                    frame[0, init_cat[p[0]]] = max(frame[0, init_cat[p[0]]], s)
                for t in range(1, T):
                    c = cat_of[p[t - 1], p[t]]
                    if c >= 0:
                        frame[t, c] = max(frame[t, c], s)
    if np.isfinite(best):
        mm = _sub(mm, best)
        if cats:
            frame = _sub(frame, best)
    return best, mm, frame, (frame.max(0) if cats else None)


def bound(graph, llh):
    '''B_u = sum_t max_j |l[t, j]| + T max |w| + max |init| + max |final| + 1 over the finite
    entries: every partial sum of every path score of the utterance lies within it.'''
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)

    def top(a):
        a = np.abs(a[np.isfinite(a)])
        return float(a.max()) if a.size else 0.

    return sum(top(row) for row in llh) + len(llh) * top(trans) + top(init) + top(final) + 1.


def tolerance(B, T, truth, r=0.):
    '''|out - truth| <= 4 (T + 1) 2^-52 B + r |truth|: an output is a float64 sum of at most
    2 T + 2 terms, each partial sum bounded by B (relative rounding 2^-53 per addition, in the
    output and in the truth), stored with relative rounding r.'''
    with np.errstate(invalid='ignore'):
        return 4 * (T + 1) * 2. ** -52 * B + r * np.where(np.isfinite(truth), np.abs(truth), 0.)
