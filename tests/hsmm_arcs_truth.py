"""The truth of the arc posteriors under explicit durations (csrc/hsmm.hip,
beer_hsmm_arc_posteriors): the definition of include/beer_hip.h as direct sums, in numpy's long
double like tests/hsmm_truth.py, whose graphs, tables and conventions it shares (no GPU needed).

 * `arc_posteriors`: (frame_out [T, n_cat], utt_out [n_cat]) of ONE utterance, float64;
 * `brute_force`: the same by enumeration of every segmentation (S <= 3, T <= 5);
 * `lifted_categories`: the categories on the count-down HMM of `hsmm_truth.expanded` under
   which the plain HMM's arc posteriors (tests/arcs_truth.py) are the same rows;
 * `route_formula` / `scratch_formula`: beer_hsmm_arcs_route and
   beer_hsmm_arcs_scratch_doubles restated from the header's text."""

import numpy as np

import hsmm_truth as ht
from arcs_truth import out_arcs, random_categories          # noqa: F401  (shared conventions)

L = np.longdouble
EINVAL = ht.EINVAL
FRAME_LDS, UTT_LDS = 0x400, 0x800
LDS_BYTES = 160 * 1024


def route_formula(S, D, itemsize, n_cat, want_frames):
    'beer_hsmm_arcs_route restated from the header\'s text (S = max_states).'
    base = ht.route_formula(S, D, itemsize)
    if base == EINVAL or n_cat < 1:
        return EINVAL
    used = 8 * (8 * S + 32) + (16 * S * D if base & ht.RING_LDS else 0)
    route = base
    if want_frames and n_cat <= 1024 and used + 8 * n_cat <= LDS_BYTES:
        route |= FRAME_LDS
        used += 8 * n_cat
    if n_cat <= 4096 and used + 8 * n_cat <= LDS_BYTES:
        route |= UTT_LDS
    return route


def scratch_formula(S, D, itemsize, nutt):
    'beer_hsmm_arcs_scratch_doubles restated from the header\'s text: beer_hsmm_scratch_doubles\'.'
    return ht.scratch_formula(S, D, itemsize, nutt)


def recursions(graph, log_dur, leave_w, llh, ids=None):
    '(beg, end, bend, bbeg [T, S], Z, W [S, S], lam [S, D]) in long double: the header\'s symbols.'
    S = graph['S']
    init, final, W, lam = ht.tables(graph, log_dur, leave_w, ids)
    l = np.asarray(llh, dtype=L)
    T, D = len(l), lam.shape[1]
    seg = lambda s, d: l[s:s + d].sum(0)                              # noqa: E731
    with np.errstate(invalid='ignore', divide='ignore'):
        beg = np.full((T, S), -np.inf, dtype=L)
        end = np.full((T, S), -np.inf, dtype=L)
        for t in range(T):
            beg[t] = init if t == 0 else ht._lse(end[t - 1][:, None] + W, 0)
            end[t] = ht._lse(np.stack([beg[t - d + 1] + lam[:, d - 1] + seg(t - d + 1, d)
                                       for d in range(1, min(D, t + 1) + 1)]), 0)
        Z = ht._lse(end[T - 1] + final, 0)
        bend = np.full((T, S), -np.inf, dtype=L)
        bbeg = np.full((T, S), -np.inf, dtype=L)
        for t in reversed(range(T)):
            bend[t] = final if t == T - 1 else ht._lse(W + bbeg[t + 1][None, :], 1)
            bbeg[t] = ht._lse(np.stack([lam[:, d - 1] + seg(t, d) + bend[t + d - 1]
                                        for d in range(1, min(D, T - t) + 1)]), 0)
    return beg, end, bend, bbeg, Z, W, lam


def arc_posteriors(graph, log_dur, leave_w, llh, arc_cat, init_cat, n_cat, ids=None):
    '''(frame_out [T, n_cat], utt_out [n_cat]) float64 by the definition: row 0 is sum_d q(j,0,d)
    folded by `init_cat`, row t >= 1 exp(end_{t-1}(i) + w_ij + bbeg_t(j) - Z) of the arcs i -> j,
    i != j, folded by `arc_cat` (which follows `out_arcs(graph)`, self-loops included); -1
    counts nothing; zeros when Z = -inf.'''
    arc_cat, init_cat = np.asarray(arc_cat), np.asarray(init_cat)
    l = np.asarray(llh, dtype=L)
    T = len(l)
    frame = np.zeros((T, n_cat), dtype=L)
    if T == 0:
        return frame.astype(np.float64), np.zeros(n_cat)
    beg, end, bend, bbeg, Z, W, lam = recursions(graph, log_dur, leave_w, llh, ids)
    src, dst = out_arcs(graph)
    assert len(arc_cat) == len(src) and len(init_cat) == graph['S']
    if not np.isfinite(Z):
        return frame.astype(np.float64), np.zeros(n_cat)
    D = lam.shape[1]
    with np.errstate(invalid='ignore'):
        q0 = np.zeros(graph['S'], dtype=L)
        for d in range(1, min(D, T) + 1):
            q = np.exp(beg[0] + lam[:, d - 1] + l[:d].sum(0) + bend[d - 1] - Z)
            q0 += np.where(np.isnan(q), 0., q)
        keep = init_cat >= 0
        np.add.at(frame[0], init_cat[keep], q0[keep])
        keep = (arc_cat >= 0) & (src != dst)
        for t in range(1, T):
            p = np.exp(end[t - 1][src] + W[src, dst] + bbeg[t][dst] - Z)
            p = np.where(np.isnan(p), 0., p)
            np.add.at(frame[t], arc_cat[keep], p[keep])
    return frame.astype(np.float64), frame.sum(0).astype(np.float64)


def brute_force(graph, log_dur, leave_w, llh, arc_cat, init_cat, n_cat, ids=None):
    'The same by enumeration: every segmentation adds its probability to the bins it passes.'
    S = graph['S']
    init, final, W, lam = ht.tables(graph, log_dur, leave_w, ids, np.float64)
    l = np.asarray(llh, dtype=np.float64)
    T, D = len(l), lam.shape[1]
    assert S <= 3 and T <= 5
    src, dst = out_arcs(graph)
    cat_of = -np.ones((S, S), dtype=np.int64)
    cat_of[src, dst] = np.asarray(arc_cat)
    segs = []

    def walk(t, prev, score, sofar):
        if t == T:
            segs.append((score + final[prev], list(sofar)))
            return
        for j in range(S):
            if j == prev:
                continue
            for d in range(1, min(D, T - t) + 1):
                with np.errstate(invalid='ignore'):
                    sc = score + (init[j] if prev < 0 else W[prev, j]) + lam[j, d - 1] + \
                        l[t:t + d, j].sum()
                sofar.append((j, t))
                walk(t + d, j, sc, sofar)
                sofar.pop()

    walk(0, -1, 0., [])
    frame = np.zeros((T, n_cat))
    scores = np.asarray([s for s, _ in segs])
    Z = float(ht._lse(scores, 0)) if len(scores) else -np.inf
    if np.isfinite(Z):
        for sc, seq in segs:
            p = np.exp(sc - Z) if np.isfinite(sc) else 0.
            for n, (j, s) in enumerate(seq):
                c = init_cat[j] if n == 0 else cat_of[seq[n - 1][0], j]
                if c >= 0:
                    frame[s, c] += p
    return frame, frame.sum(0)


def lifted_categories(graph, log_dur, leave_w, arc_cat, init_cat, ids=None):
    '''(expanded graph, arc_cat, init_cat) on the count-down HMM of `hsmm_truth.expanded`: every
    arc (i, 1) -> (j, d) takes the category of i -> j, every arc (j, r) -> (j, r - 1) takes -1,
    every state (j, d) takes init_cat[j].'''
    S = graph['S']
    eg = ht.expanded(graph, log_dur, leave_w, ids)
    D = eg['S'] // S
    src, dst = out_arcs(graph)
    cat_of = -np.ones((S, S), dtype=np.int64)
    cat_of[src, dst] = np.asarray(arc_cat)
    es, ed = out_arcs(eg)
    lifted = np.where(es // D != ed // D, cat_of[es // D, ed // D], -1)
    return eg, lifted.astype(np.int32), np.repeat(np.asarray(init_cat), D).astype(np.int32)
