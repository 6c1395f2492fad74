"""The float64 truth of the posterior path sampler (csrc/hmm_sample.hip): plain numpy on the
graphs and inputs of tests/fb_truth.py, float32 inputs upcast (no GPU needed).

 * `forward`: the normalised forward values in log space, the kernel's trellis format;
 * `last_weights` / `row_weights`: the terms a draw chooses among -- the states at the last
   frame, the in-arcs of the drawn next state (finite entries of its column of the dense
   transition matrix, source ascending: the in-CSR order) before it;
 * `choose`: the rule -- the first term whose inclusive running sum exceeds u * total, the last
   term of non-zero weight if rounding leaves none, never a term of weight 0, term 0 when the
   total is 0 or not finite;
 * `sample`: the exact sampler built from them, for many draws at once;
 * `check_paths`: a sampler's paths held to the rule STEP BY STEP, each step given the sampler's
   own next state, so that one boundary case does not invalidate the rest of a path;
 * `path_frequencies`: state and consecutive-pair frequencies of a set of paths, to be held
   against the oracle's gamma and xi."""

import numpy as np

import fb_truth as ft
from helpers import orc

EINVAL = -100000            # BEER_EINVAL
ARCS_LDS, QUAD = 0x100, 0x200


def route_formula(S, A, itemsize, nsamples):
    """beer_hmm_sample_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or nsamples < 1 or itemsize not in (4, 8):
        return EINVAL
    row = 8 * S + 32
    chunk = 32 if 32 * row <= 32 * 1024 else (8 if 8 * row <= 32 * 1024 else 2)
    base = max(chunk * row, 16 * S + 128)
    if base > 160 * 1024:
        return EINVAL
    waves = 1 if nsamples == 1 else 4
    if (nsamples + waves - 1) // waves > 65535:
        return EINVAL
    arcs_lds = base + 4 * (S + 2 + A) + itemsize * A <= 64 * 1024
    return chunk | (ARCS_LDS if arcs_lds else 0) | (QUAD if 4 * S <= 512 else 0) | waves << 12


# the statistics case: a circulant graph of 6 states and 3 offsets, 20 frames, 4096 draws
STAT_S, STAT_T, STAT_N, STAT_SEED = 6, 20, 4096, 11
STAT_BOUND = 3 / np.sqrt(STAT_N)            # 0.047: six standard deviations at p = 1/2


def stat_case():
    '(graph, llh [T, S], uniforms [N, T]) of the statistics case, float64.'
    g = ft.make_graph(STAT_S, ft.offsets(3, STAT_S), STAT_SEED)
    _, (llh,) = ft.inputs(g, [STAT_T], np.arange(STAT_S), STAT_S, 1., STAT_SEED)
    U = np.random.RandomState(STAT_SEED).random_sample((STAT_N, STAT_T))
    return g, llh, U


def _f64(graph):
    return tuple(np.asarray(graph[k], dtype=np.float64) for k in ('init', 'final', 'trans'))


def forward(graph, llh):
    '[T, S] float64: ln alpha_t(j) - ln sum_i alpha_t(i); -inf for unreachable states.'
    init, _, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    out = np.empty(llh.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        a = llh[0] + init
        for t in range(len(llh)):
            if t:
                hyp = out[t - 1][:, None] + trans                   # [source, destination]
                m = hyp.max(0)
                base = np.where(np.isfinite(m), m, 0.)
                a = llh[t] + base + np.log(np.exp(hyp - base[None, :]).sum(0))
            m = a.max()
            base = m if np.isfinite(m) else 0.
            s = np.exp(a - base).sum()
            out[t] = a - (base + np.log(s)) if s > 0 else -np.inf
    return out


def last_weights(graph, la_last):
    'w_j = exp(alpha_{T-1}(j) + final_j), j = 0..S-1.'
    with np.errstate(invalid='ignore'):
        return np.exp(la_last + _f64(graph)[1])


def row_weights(graph, la_t, nxt):
    '(sources, weights) of the in-arcs of state `nxt`, source ascending.'
    col = _f64(graph)[2][:, nxt]
    src = np.nonzero(col > -np.inf)[0]
    with np.errstate(invalid='ignore'):
        return src, np.exp(la_t[src] + col[src])


def choose(w, u):
    'Index of the term of weights `w` that each uniform of `u` draws (an array like u).'
    u = np.asarray(u, dtype=np.float64)
    if len(w) == 0:
        return np.zeros(u.shape, dtype=np.int64)
    c = np.cumsum(w)
    tot = c[-1]
    if not (tot > 0 and np.isfinite(tot)):
        return np.zeros(u.shape, dtype=np.int64)
    idx = np.searchsorted(c, u * tot, side='right')                 # first c_i > u * total
    last = np.nonzero(w > 0)[0][-1]
    return np.where(idx < len(w), np.minimum(idx, last), last).astype(np.int64)


def sample(graph, llh, uniforms, la=None):
    '''State paths [n, T] int64 drawn by the uniforms [n, T] (frame t uses uniforms[:, t]):
    forward filtering, backward sampling, exactly by the rule.'''
    U = np.asarray(uniforms, dtype=np.float64)
    la = forward(graph, llh) if la is None else la
    n, T = U.shape
    path = np.zeros((n, T), dtype=np.int64)
    path[:, T - 1] = choose(last_weights(graph, la[T - 1]), U[:, T - 1])
    for t in range(T - 2, -1, -1):
        for s in np.unique(path[:, t + 1]):
            sel = path[:, t + 1] == s
            src, w = row_weights(graph, la[t], s)
            pick = choose(w, U[sel, t])
            path[sel, t] = src[pick] if len(src) else 0
    return path


def _step_ok(w, k, u, tol):
    '(within the rule, needed the widening) for the choice of term k of weights w at uniform u.'
    tot = w.sum()
    if not (tot > 0 and np.isfinite(tot)):
        return k == 0, False
    if not w[k] > 0:
        return False, False
    c = np.cumsum(w) / tot
    lo = c[k - 1] if k else 0.
    if lo <= u < c[k]:
        return True, False
    return lo - tol <= u < c[k] + tol, True


def check_paths(graph, llh, uniforms, paths, tol, la=None):
    '''Hold state paths [n, T] to the rule step by step: (steps, steps that needed the interval
    widened by `tol`).  Raises AssertionError at the first step outside the widened interval, on
    a term of weight 0 or on a state that is not a source of the row.'''
    U = np.asarray(uniforms, dtype=np.float64)
    P = np.asarray(paths)
    la = forward(graph, llh) if la is None else la
    n, T = P.shape
    S = la.shape[1]
    assert U.shape == P.shape and T == len(la)
    assert ((P >= 0) & (P < S)).all(), 'state index out of range'
    steps = widened = 0
    for i in range(n):
        for t in range(T - 1, -1, -1):
            if t == T - 1:
                w, k = last_weights(graph, la[t]), P[i, t]
            else:
                src, w = row_weights(graph, la[t], P[i, t + 1])
                if len(src) == 0:
                    assert P[i, t] == 0, f'sample {i} frame {t}: a row without arcs gives state 0'
                    continue
                hit = np.nonzero(src == P[i, t])[0]
                assert len(hit) == 1, f'sample {i} frame {t}: {P[i, t]} -> {P[i, t + 1]} is no arc'
                k = hit[0]
            ok, wide = _step_ok(w, int(k), U[i, t], tol)
            assert ok, f'sample {i} frame {t}: term {k} of {len(w)} at u = {U[i, t]!r}'
            steps += 1
            widened += wide
    return steps, widened


def path_frequencies(paths, S):
    '(state frequencies [T, S], pair frequencies [T-1, S, S]) of the paths [n, T].'
    P = np.asarray(paths)
    n, T = P.shape
    gam = np.zeros((T, S))
    xi = np.zeros((max(T - 1, 0), S, S))
    for t in range(T):
        np.add.at(gam[t], P[:, t], 1.)
        if t + 1 < T:
            np.add.at(xi[t], (P[:, t], P[:, t + 1]), 1.)
    return gam / n, xi / n


def posteriors(graph, llh):
    '(gamma [T, S], xi [T-1, S, S]) of the oracle in float64.'
    init, final, trans = _f64(graph)
    with np.errstate(invalid='ignore', divide='ignore'):
        gam, xi, _ = orc.posteriors(np.asarray(llh, dtype=np.float64), init, final, trans, True)
    return gam, xi


def valid_path(graph, path):
    'A finite start, finite arcs all the way and a finite end.'
    init, final, trans = _f64(graph)
    p = np.asarray(path)
    return bool(np.isfinite(init[p[0]]) and np.isfinite(final[p[-1]]) and
                np.isfinite(trans[p[:-1], p[1:]]).all())
