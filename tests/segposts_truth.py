"""The float64 truth of the segment posteriors (csrc/hmm_segposts.hip): plain numpy on the graphs
and inputs of tests/fb_truth.py, float32 inputs upcast (no GPU needed).

With the categories, boundaries and "the path HAS THE SEGMENT (c, s, e)" of tests/segments_truth.py:
post(c, s, e) = P(the path has the segment (c, s, e) | x_0 .. x_{T-1}).

 * `segment_posteriors`: (post [T, n_cat, max_dur], starts [T, n_cat], evidence) by the recursion
   of include/beer_hip.h (beer_hmm_segpost_trellis) in plain log space: post[s, c, k] is the
   posterior of the segment (c, s, s + k), 0 where it is impossible or s + k >= T; `starts` the
   start posteriors (beer_hmm_arc_posteriors' frame_out) from the same trellises; a dead utterance
   holds zeros and evidence -inf;
 * `brute_force`: the same three by enumeration of all S^T state paths, from the definition in
   words;
 * `coverage`: for every frame the summed posterior of the segments that cover it, and their number;
 * `durations`: the expected duration histogram [n_cat, max_dur];
 * `route_formula`: beer_hmm_segposts_route restated from the header's text;
 * `loop_graph`, `chain_graph`, `closures`: those of tests/segments_truth.py."""

import itertools

import numpy as np

from arcs_truth import EINVAL, _f64, _lse, out_arcs                          # noqa: F401
from segments_truth import _labels, chain_graph, closures, loop_graph, team_of  # noqa: F401

NINF = -np.inf
BLOCK, ARCS_LDS, BINS_LDS = 0x1000, 0x100, 0x200


def route_formula(S, A, itemsize, n_cat, max_closure):
    """beer_hmm_segposts_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or A < 0 or itemsize not in (4, 8) or n_cat < 1:
        return EINVAL
    if max_closure < 0 or max_closure > S:
        return EINVAL
    rows = 16 * S + 128
    if rows > 160 * 1024:
        return EINVAL
    team = team_of(max_closure)
    if (256 // team) * (32 * max(max_closure, 1) + 64) > 64 * 1024:
        return EINVAL
    arcs = 4 * (S + 2 + 2 * A) + itemsize * (A + 1)
    route = BLOCK | (team.bit_length() - 1)
    if rows + arcs <= 64 * 1024:
        route |= ARCS_LDS
    if n_cat <= 1024 and rows <= 96 * 1024:
        route |= BINS_LDS
    return route


def segment_posteriors(graph, llh, arc_cat, init_cat, n_cat, max_dur):
    '(post [T, n_cat, max_dur], starts [T, n_cat], evidence) in float64 by the recursion.'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    init_cat = np.asarray(init_cat)
    cat_of = _labels(graph, arc_cat)
    post, starts = np.zeros((T, n_cat, max_dur)), np.zeros((T, n_cat))
    if T == 0:
        return post, starts, 0.
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        a, c = np.empty((T, S)), np.empty(T)
        row = init + llh[0]
        for t in range(T):
            if t:
                row = llh[t] + _lse(a[t - 1][:, None] + trans, axis=0)
            c[t] = float(_lse(row))
            if not np.isfinite(c[t]):
                return post, starts, NINF
            a[t] = row - c[t]
        f = float(_lse(a[T - 1] + final))
        if not np.isfinite(f):
            return post, starts, NINF
        ends = np.where(cat_of >= 0, trans, NINF)              # the arcs that end a segment
        stays = np.where(cat_of == -1, trans, NINF)            # ... and those that do not
        b, Y = np.empty((T, S)), np.empty((T, S))
        b[T - 1] = Y[T - 1] = final - f
        for t in range(T - 1, 0, -1):
            on = llh[t] + b[t]
            b[t - 1] = _lse(trans + on[None, :], axis=1) - c[t]
            Y[t - 1] = _lse(ends + on[None, :], axis=1) - c[t]
        for cat in range(n_cat):
            enters = np.where(cat_of == cat, trans, NINF)
            for s in range(T):
                if s == 0:
                    r = np.where(init_cat == cat, a[0], NINF)
                else:
                    r = _lse(a[s - 1][:, None] + enters, axis=0) + llh[s] - c[s]
                r = np.where(np.isnan(r), NINF, r)
                starts[s, cat] = np.exp(r + b[s])[np.isfinite(r) & np.isfinite(b[s])].sum()
                for k in range(min(max_dur, T - s)):
                    if k:
                        r = _lse(r[:, None] + stays, axis=0) + llh[s + k] - c[s + k]
                        r = np.where(np.isnan(r), NINF, r)
                    ok = np.isfinite(r) & np.isfinite(Y[s + k])
                    post[s, cat, k] = np.exp(r + Y[s + k])[ok].sum()
    return post, starts, float(c.sum() + f)


def brute_force(graph, llh, arc_cat, init_cat, n_cat, max_dur):
    'The same by enumeration: every path adds its probability to the segments it has.'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    assert S <= 5 and T <= 6
    cat_of = _labels(graph, arc_cat)
    post, starts = np.zeros((T, n_cat, max_dur)), np.zeros((T, n_cat))
    scored = []
    with np.errstate(invalid='ignore'):
        for p in itertools.product(range(S), repeat=T):
            score = llh[0, p[0]] + init[p[0]]
            for t in range(1, T):
                score = (score + trans[p[t - 1], p[t]]) + llh[t, p[t]]
            score = score + final[p[-1]]
            if np.isfinite(score):
                scored.append((p, score))
    if not scored:
        return post, starts, NINF
    top = max(s for _, s in scored)
    total = sum(np.exp(s - top) for _, s in scored)
    for p, score in scored:
        w = np.exp(score - top) / total
        marks = [(0, int(init_cat[p[0]]))] + \
            [(t, int(cat_of[p[t - 1], p[t]])) for t in range(1, T) if cat_of[p[t - 1], p[t]] >= 0]
        for n, (s, c) in enumerate(marks):
            end = marks[n + 1][0] - 1 if n + 1 < len(marks) else T - 1
            if c >= 0:
                starts[s, c] += w
                if end - s < max_dur:
                    post[s, c, end - s] += w
    return post, starts, float(top + np.log(total))


def coverage(post):
    '''(mass [T], count [T]): the summed posterior of the segments (c, s, s + k) with
    s <= t <= s + k, and the number of such segments that are possible (post > 0).'''
    T, _, max_dur = post.shape
    mass, count = np.zeros(T), np.zeros(T, dtype=np.int64)
    for s in range(T):
        for k in range(min(max_dur, T - s)):
            mass[s:s + k + 1] += post[s, :, k].sum()
            count[s:s + k + 1] += int((post[s, :, k] > 0).sum())
    return mass, count


def durations(post):
    'The expected duration histogram [n_cat, max_dur]: entry (c, k) is sum_s post(c, s, s + k).'
    return post.sum(0)
