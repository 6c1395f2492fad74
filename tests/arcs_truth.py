"""The float64 truth of the arc posteriors by category (csrc/hmm_arcs.hip): plain numpy on the
graphs and inputs of tests/fb_truth.py, float32 inputs upcast (no GPU needed).

 * `trellis`: the normalised forward and backward rows;
 * `out_arcs`: (src, dst) of the full out-CSR, the order `arc_cat` follows: the finite entries of
   the transition matrix in row-major order, hub arcs included;
 * `arc_posteriors`: (frame_out [T, n_cat], utt_out [n_cat]) by the definition of
   include/beer_hip.h (beer_hmm_arc_posteriors): row 0 is gamma_0 folded by `init_cat`, row
   t >= 1 the posteriors of the arcs entering frame t folded by `arc_cat`, -1 counts nothing; an
   utterance whose evidence is -inf gets zeros;
 * `brute_force`: the same by enumeration of all S^T state paths;
 * `route_formula`: beer_hmm_arcs_route restated from the header's text."""

import itertools

import numpy as np

EINVAL = -100000            # BEER_EINVAL
BLOCK, ARCS_LDS, FRAME_LDS, UTT_LDS = 0x1000, 0x100, 0x200, 0x400


def route_formula(S, A, itemsize, n_cat, want_frames):
    """beer_hmm_arcs_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or A < 0 or itemsize not in (4, 8) or n_cat < 1:
        return EINVAL
    rows = 16 * S + 128
    if rows > 160 * 1024:
        return EINVAL
    arcs = 4 * (S + 2 + 2 * A) + itemsize * (A + 1)
    route = BLOCK
    if rows + arcs <= 64 * 1024:
        route |= ARCS_LDS
    if want_frames and n_cat <= 1024 and rows <= 96 * 1024:
        route |= FRAME_LDS
    if n_cat <= 4096 and rows <= 96 * 1024:
        route |= UTT_LDS
    return route


def out_arcs(graph):
    '(src, dst) of the arcs in the full out-CSR order: by source, destinations ascending.'
    return np.nonzero(np.isfinite(np.asarray(graph['trans'], dtype=np.float64)))


def _f64(graph):
    return tuple(np.asarray(graph[k], dtype=np.float64) for k in ('init', 'final', 'trans'))


def _lse(v, axis=None):
    'ln sum exp(v); -inf where nothing is finite.'
    m = np.max(v, axis=axis, keepdims=True)
    base = np.where(np.isfinite(m), m, 0.)
    with np.errstate(divide='ignore'):
        out = base + np.log(np.exp(v - base).sum(axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis)


def trellis(graph, llh):
    '''(alpha [T, S], beta [T, S]) in float64 log space, or None when the evidence is -inf: every
    forward row is normalised by its own log-sum and every backward row so that the state
    posteriors of its frame sum to 1 (long utterances keep their precision).'''
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    with np.errstate(invalid='ignore', divide='ignore'):
        alpha = np.empty((T, S))
        a = init + llh[0]
        for t in range(T):
            if t:
                a = llh[t] + _lse(alpha[t - 1][:, None] + trans, axis=0)
            c = float(_lse(a))
            if not np.isfinite(c):
                return None
            alpha[t] = a - c
        tail = float(_lse(alpha[T - 1] + final))
        if not np.isfinite(tail):
            return None
        beta = np.empty((T, S))
        beta[T - 1] = final - tail
        for t in range(T - 2, -1, -1):
            b = _lse(trans + (llh[t + 1] + beta[t + 1])[None, :], axis=1)
            beta[t] = b - float(_lse(alpha[t] + b))
    return alpha, beta


def _normalised(x):
    'exp(x) / sum exp(x) of log-values of which one at least is finite (NaN from -inf - -inf: 0).'
    x = np.where(np.isnan(x), -np.inf, x)
    return np.exp(x - float(_lse(x)))


def arc_posteriors(graph, llh, arc_cat, init_cat, n_cat):
    '(frame_out [T, n_cat], utt_out [n_cat]) float64, by the definition; zeros for a dead utterance.'
    arc_cat, init_cat = np.asarray(arc_cat), np.asarray(init_cat)
    llh = np.asarray(llh, dtype=np.float64)
    T = len(llh)
    frame = np.zeros((T, n_cat))
    tr = trellis(graph, llh)
    if tr is None:
        return frame, np.zeros(n_cat)
    alpha, beta = tr
    src, dst = out_arcs(graph)
    w = _f64(graph)[2][src, dst]
    assert len(arc_cat) == len(src) and len(init_cat) == alpha.shape[1]
    with np.errstate(invalid='ignore'):
        gamma0 = _normalised(alpha[0] + beta[0])
        keep = init_cat >= 0
        np.add.at(frame[0], init_cat[keep], gamma0[keep])
        keep = arc_cat >= 0
        for t in range(1, T):
            xi = _normalised(alpha[t - 1][src] + w + llh[t][dst] + beta[t][dst])
            np.add.at(frame[t], arc_cat[keep], xi[keep])
    return frame, frame.sum(0)


def brute_force(graph, llh, arc_cat, init_cat, n_cat):
    'The same by enumeration: every path adds its probability to the bins it passes.'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    src, dst = out_arcs(graph)
    cat_of = -np.ones((S, S), dtype=np.int64)
    cat_of[src, dst] = np.asarray(arc_cat)
    frame = np.zeros((T, n_cat))
    total = 0.
    scores = []
    with np.errstate(invalid='ignore'):
        for path in itertools.product(range(S), repeat=T):
            p = np.asarray(path)
            scores.append((p, init[p[0]] + llh[np.arange(T), p].sum() + trans[p[:-1], p[1:]].sum() +
                           final[p[-1]]))
    top = max(s for _, s in scores)
    if not np.isfinite(top):
        return frame, np.zeros(n_cat)
    for p, s in scores:
        w = np.exp(s - top)
        if not w > 0.:
            continue
        total += w
        if init_cat[p[0]] >= 0:
            frame[0, init_cat[p[0]]] += w
        for t in range(1, T):
            c = cat_of[p[t - 1], p[t]]
            if c >= 0:
                frame[t, c] += w
    frame /= total
    return frame, frame.sum(0)


def random_categories(graph, n_cat, seed, drop=0.):
    '(arc_cat, init_cat) drawn uniformly from [0, n_cat), a share `drop` of them -1.'
    rng = np.random.RandomState(seed)
    A, S = len(out_arcs(graph)[0]), graph['S']
    arc_cat = rng.randint(0, n_cat, size=A).astype(np.int32)
    init_cat = rng.randint(0, n_cat, size=S).astype(np.int32)
    if drop:
        arc_cat[rng.rand(A) < drop] = -1
        init_cat[rng.rand(S) < drop] = -1
    return arc_cat, init_cat
