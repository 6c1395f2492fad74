"""The float64 truth of the unit segment lattices (csrc/hmm_segments.hip): plain numpy on the
graphs and inputs of tests/fb_truth.py, float32 inputs upcast (no GPU needed).

 * `segments`: seg [T, n_cat, max_dur] by the definition of include/beer_hip.h
   (beer_hmm_segment_trellis), the additions in its bracketed order: seg[s, c, k] is the score of
   the best path on which category c begins at frame s and lasts exactly until frame s + k, minus
   the Viterbi score; -inf where there is none or s + k >= T;
 * `brute_force`: the same by enumeration of all S^T state paths, from the definition in words
   (boundaries and their labels);
 * `closures`: the member states of every category's closure, by a search of its own;
 * `route_formula`: beer_hmm_segments_route restated from the header's text;
 * `loop_graph`, `chain_graph`: phone loops and alignment chains with their unit-start categories;
 * `bound`, `tolerance`: those of tests/lattice_truth.py as they are -- a path has the same
   2 T + 2 terms."""

import itertools

import numpy as np

from arcs_truth import out_arcs
from lattice_truth import NINF, EINVAL, _f64, _sub, bound, tolerance, max_marginals   # noqa: F401

BLOCK, ARCS_LDS, BINS_LDS = 0x1000, 0x100, 0x200


def team_of(max_closure):
    'The smallest power of two in 4 .. 256 that is >= max_closure.'
    team = 4
    while team < 256 and team < max_closure:
        team *= 2
    return team


def route_formula(S, A, itemsize, n_cat, max_closure):
    """beer_hmm_segments_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or A < 0 or itemsize not in (4, 8) or n_cat < 1:
        return EINVAL
    if max_closure < 0 or max_closure > S:
        return EINVAL
    rows = 16 * S + 128
    if rows > 160 * 1024:
        return EINVAL
    team = team_of(max_closure)
    if (256 // team) * (16 * max(max_closure, 1) + 16) > 64 * 1024:
        return EINVAL
    arcs = 4 * (S + 2 + 2 * A) + itemsize * (A + 1)
    route = BLOCK | (team.bit_length() - 1)
    if rows + arcs <= 64 * 1024:
        route |= ARCS_LDS
    if n_cat <= 2048 and rows <= 96 * 1024:
        route |= BINS_LDS
    return route


def _labels(graph, arc_cat):
    '[S, S] the category of every arc; -2 where there is no arc.'
    src, dst = out_arcs(graph)
    assert len(arc_cat) == len(src)
    cat_of = np.full((graph['S'], graph['S']), -2, dtype=np.int64)
    cat_of[src, dst] = np.asarray(arc_cat)
    return cat_of


def segments(graph, llh, arc_cat, init_cat, n_cat, max_dur):
    'seg [T, n_cat, max_dur] in float64 by the recursion; a dead utterance holds -inf.'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    init_cat = np.asarray(init_cat)
    cat_of = _labels(graph, arc_cat)
    seg = np.full((T, n_cat, max_dur), NINF)
    with np.errstate(invalid='ignore'):
        d = np.empty((T, S))
        d[0] = llh[0] + init
        for t in range(1, T):
            d[t] = (d[t - 1][:, None] + trans).max(0) + llh[t]
        best = float((d[T - 1] + final).max())
        if not np.isfinite(best):
            return seg
        ends = np.where(cat_of >= 0, trans, NINF)              # the arcs that end a segment
        stays = np.where(cat_of == -1, trans, NINF)            # ... and those that do not
        e = np.empty((T, S))
        X = np.empty((T, S))
        e[T - 1] = X[T - 1] = final
        for t in range(T - 2, -1, -1):
            on = llh[t + 1] + e[t + 1]
            e[t] = (trans + on[None, :]).max(1)
            X[t] = (ends + on[None, :]).max(1)
        for c in np.union1d(cat_of[cat_of >= 0], init_cat[init_cat >= 0]):
            # (a category without an arc or a state has no segment: its rows stay -inf)
            enters = np.where(cat_of == c, trans, NINF)
            for s in range(T):
                if s == 0:
                    r = np.where(init_cat == c, d[0], NINF)
                else:
                    r = ((d[s - 1][:, None] + enters) + llh[s][None, :]).max(0)
                for k in range(min(max_dur, T - s)):
                    if k:
                        r = ((r[:, None] + stays) + llh[s + k][None, :]).max(0)
                    seg[s, c, k] = (r + X[s + k]).max()
        return _sub(seg, best)


def brute_force(graph, llh, arc_cat, init_cat, n_cat, max_dur):
    'The same by enumeration: every path raises the segments it has to its score.'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    cat_of = _labels(graph, arc_cat)
    seg = np.full((T, n_cat, max_dur), NINF)
    best = NINF
    with np.errstate(invalid='ignore'):
        for p in itertools.product(range(S), repeat=T):
            score = llh[0, p[0]] + init[p[0]]
            for t in range(1, T):
                score = (score + trans[p[t - 1], p[t]]) + llh[t, p[t]]
            score = score + final[p[-1]]
            if not np.isfinite(score):
                continue
            best = max(best, score)
            # the boundaries of the path and their labels (frame 0 is one whatever its label)
            marks = [(0, int(init_cat[p[0]]))] + \
                [(t, int(cat_of[p[t - 1], p[t]])) for t in range(1, T) if cat_of[p[t - 1], p[t]] >= 0]
            for n, (s, c) in enumerate(marks):
                end = marks[n + 1][0] - 1 if n + 1 < len(marks) else T - 1
                if c >= 0 and end - s < max_dur:
                    seg[s, c, end - s] = max(seg[s, c, end - s], score)
    return _sub(seg, best) if np.isfinite(best) else seg


def closures(graph, arc_cat, init_cat, n_cat):
    '''The closure of every category: the sorted states reachable from the destinations of its
    arcs and from the states with init_cat = c through arcs of category -1.'''
    src, dst = out_arcs(graph)
    free = {}
    for a, (i, j) in enumerate(zip(src.tolist(), dst.tolist())):
        if arc_cat[a] == -1:
            free.setdefault(i, []).append(j)
    out = []
    for c in range(n_cat):
        todo = [int(j) for a, j in enumerate(dst.tolist()) if arc_cat[a] == c] + \
            [j for j in range(graph['S']) if init_cat[j] == c]
        seen = set(todo)
        while todo:
            for j in free.get(todo.pop(), []):
                if j not in seen:
                    seen.add(j)
                    todo.append(j)
        out.append(np.asarray(sorted(seen), dtype=np.int32))
    return out


def viterbi_segments(path, arc_cat_of, init_cat):
    '''[(c, s, e)] read off one state path: `arc_cat_of` [S, S] as `_labels` gives it.  Segments
    whose label is -1 (frame 0 alone can have one) are left out.'''
    T = len(path)
    marks = [(0, int(init_cat[path[0]]))] + \
        [(t, int(arc_cat_of[path[t - 1], path[t]])) for t in range(1, T)
         if arc_cat_of[path[t - 1], path[t]] >= 0]
    out = []
    for n, (s, c) in enumerate(marks):
        end = marks[n + 1][0] - 1 if n + 1 < len(marks) else T - 1
        if c >= 0:
            out.append((c, s, end))
    return out


def _weights(rng, size, low, real):
    'Integers in (-low, 0], or with `real` multiples of 1/64 there: exact in float32 either way.'
    return -rng.randint(0, low * 64, size=size) / 64. if real else -rng.randint(0, low, size=size) * 1.


def loop_graph(sizes, seed=0, skips=(1,), open_end=False, labels=None, real=False):
    '''(graph, arc_cat, init_cat) of a phone loop whose unit u has sizes[u] states: inside a unit
    a self loop and an arc to the state k further on for every k of `skips`, from a unit's last
    state an arc to every unit's first.  A path starts in a first state and ends in a last one
    (`open_end`: anywhere).  Categories: an arc into a first state from another state begins that
    unit, every state belongs to its unit; `labels[u]` renames the category of unit u.'''
    sizes = np.asarray(sizes)
    S, n_units = int(sizes.sum()), len(sizes)
    rng = np.random.RandomState(seed + 7 * S + n_units)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    last = first + sizes - 1
    unit_of = np.repeat(np.arange(n_units), sizes)
    trans = np.full((S, S), NINF)
    for j in range(S):
        trans[j, j] = _weights(rng, None, 3, real)
        for k in skips:
            if j + k <= last[unit_of[j]]:
                trans[j, j + k] = _weights(rng, None, 3, real)
    for u in range(n_units):
        trans[last[u], first] = _weights(rng, n_units, 4, real)
    init = np.full(S, NINF)
    init[first] = _weights(rng, n_units, 3, real)
    final = np.full(S, NINF)
    final[last] = _weights(rng, n_units, 2, real)
    if open_end:
        final = _weights(rng, S, 3, real)
    g = dict(S=S, init=init, final=final, trans=trans, hub=None)
    src, dst = out_arcs(g)
    names = np.arange(n_units) if labels is None else np.asarray(labels)
    arc_cat = np.where((src != dst) & np.isin(dst, first), names[unit_of[dst]], -1)
    return g, arc_cat.astype(np.int32), names[unit_of].astype(np.int32)


def chain_graph(units, n_states, seed=0, real=False):
    '''(graph, arc_cat, init_cat) of an alignment chain over the unit sequence `units`, every
    instance `n_states` states with self loops: a repeated unit is ONE category.'''
    units = np.asarray(units)
    S = len(units) * n_states
    rng = np.random.RandomState(seed + 11 * S)
    trans = np.full((S, S), NINF)
    for j in range(S):
        trans[j, j] = _weights(rng, None, 3, real)
        if j + 1 < S:
            trans[j, j + 1] = _weights(rng, None, 3, real)
    init = np.full(S, NINF)
    init[0] = 0.
    final = np.full(S, NINF)
    final[S - 1] = 0.
    g = dict(S=S, init=init, final=final, trans=trans, hub=None)
    src, dst = out_arcs(g)
    unit_of = np.repeat(units, n_states)
    arc_cat = np.where((src != dst) & (dst % n_states == 0), unit_of[dst], -1)
    return g, arc_cat.astype(np.int32), unit_of.astype(np.int32)
