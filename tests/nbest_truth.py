"""The truth of N-best Viterbi (csrc/hmm_nbest.hip): plain numpy on the graphs and inputs of
tests/fb_truth.py (no GPU needed).

 * `nbest`: the list-Viterbi of include/beer_hip.h (beer_hmm_viterbi_nbest) in a chosen dtype, with
   the header's order of operations and of candidates: at every cell the k best candidates over
   (source, rank), at the end over (state, rank); larger score first, then the smaller source (or
   final) state, then the smaller rank; a candidate of -inf is not a path;
 * `brute_force`: all finite paths of the S^T, sorted by (-score, reversed path);
 * `route_formula`: beer_hmm_nbest_route restated from the header's text;
 * `path_terms` / `score_bound`: the terms a path's score is the sum of, and the tolerance on a
   score from their magnitudes, tol * (sum |terms| + 1)."""

import itertools

import numpy as np

EINVAL = -100000            # BEER_EINVAL
NBEST_MAX = 16              # BEER_NBEST_MAX
ARCS_LDS = 0x100            # BEER_NBEST_ARCS_LDS


def list_entries(k):
    'BEER_NBEST_LIST restated.'
    return 1 if k <= 1 else (2 if k <= 2 else (4 if k <= 4 else (8 if k <= 8 else 16)))


def route_formula(S, A, itemsize, k):
    """beer_hmm_nbest_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or A < 0 or itemsize not in (4, 8) or not 1 <= k <= NBEST_MAX:
        return EINVAL
    row = 4 * S * k
    chunk = 32 if 32 * row <= 16 * 1024 else (8 if 8 * row <= 16 * 1024 else 2)
    base = 2 * S * k * itemsize + 64 + chunk * row
    if base > 160 * 1024:
        return EINVAL
    arcs = 4 * (S + 2 + A) + itemsize * A
    return chunk | (ARCS_LDS if base + arcs <= 64 * 1024 else 0)


def _in_lists(trans):
    '''(src [S, D], w [S, D]): the in-arcs of every state, sources ascending, rows padded with
    arcs of weight -inf at their end.'''
    S = trans.shape[0]
    present = trans > -np.inf
    D = max(int(present.sum(0).max()), 1)
    src = np.zeros((S, D), dtype=np.int64)
    w = np.full((S, D), -np.inf, dtype=trans.dtype)
    for j in range(S):
        s = np.nonzero(present[:, j])[0]
        src[j, :len(s)] = s
        w[j, :len(s)] = trans[s, j]
    return src, w


def _best(cand, k):
    '''The k best of every row of `cand` [n, m], the first of equal values first: (values [n, k],
    columns [n, k] with -1 where the value is -inf).'''
    n, m = cand.shape
    if m < k:
        cand = np.concatenate([cand, np.full((n, k - m), -np.inf, dtype=cand.dtype)], axis=1)
    order = np.argsort(-cand, axis=1, kind='stable')[:, :k]
    val = np.take_along_axis(cand, order, axis=1)
    return val, np.where(val > -np.inf, order, -1)


def nbest(graph, llh, k, dtype=np.float64):
    '''(paths int64 [k, T], scores float64 [k]) of one utterance, arithmetic in `dtype`; ranks
    without a finite path: -1 and -inf.'''
    init, final, trans = (np.asarray(graph[n], dtype=dtype) for n in ('init', 'final', 'trans'))
    llh = np.asarray(llh, dtype=dtype)
    T, S = llh.shape
    src, w = _in_lists(trans)
    D = src.shape[1]
    with np.errstate(invalid='ignore'):
        omega = np.full((S, k), -np.inf, dtype=dtype)
        omega[:, 0] = llh[0] + init
        back = []                                       # per frame: column (arc * k + rank) or -1
        for t in range(1, T):
            cand = (omega[src] + w[:, :, None]).reshape(S, D * k)       # (arc, rank) order
            val, col = _best(cand, k)
            omega = (llh[t][:, None] + val).astype(dtype)
            back.append(col)
        val, col = _best((omega + final[:, None]).reshape(1, S * k), k)
    scores = val[0].astype(np.float64)
    paths = np.full((k, T), -1, dtype=np.int64)
    for q in range(k):
        if col[0, q] < 0:
            continue
        j, r = divmod(int(col[0, q]), k)
        for t in range(T - 1, -1, -1):
            paths[q, t] = j
            if t:
                a, r = divmod(int(back[t - 1][j, r]), k)
                j = int(src[j, a])
    assert scores.dtype == np.float64 and (np.diff(scores[np.isfinite(scores)]) <= 0).all()
    return paths, scores


def brute_force(graph, llh, dtype=np.float64):
    '''(paths [n, T], scores [n]): every path of finite score among the S^T, sorted by
    (-score, reversed path); the score is summed in `dtype` in the header's order.'''
    init, final, trans = (np.asarray(graph[n], dtype=dtype) for n in ('init', 'final', 'trans'))
    llh = np.asarray(llh, dtype=dtype)
    T, S = llh.shape
    p = np.asarray(list(itertools.product(range(S), repeat=T)), dtype=np.int64).reshape(-1, T)
    with np.errstate(invalid='ignore'):
        s = llh[0, p[:, 0]] + init[p[:, 0]]
        for t in range(1, T):
            s = llh[t, p[:, t]] + (s + trans[p[:, t - 1], p[:, t]])
        s = s + final[p[:, -1]]
    keep = s > -np.inf
    p, s = p[keep], s[keep].astype(np.float64)
    order = np.lexsort(tuple(p[:, t] for t in range(T)) + (-s,))
    return p[order], s[order]


def path_terms(graph, llh, path):
    'The float64 terms whose sum is the score of `path`: init, the frames, the arcs, final.'
    init, final, trans = (np.asarray(graph[n], dtype=np.float64) for n in ('init', 'final', 'trans'))
    llh = np.asarray(llh, dtype=np.float64)
    path = np.asarray(path)
    return np.concatenate([[init[path[0]]], llh[np.arange(len(path)), path],
                           trans[path[:-1], path[1:]], [final[path[-1]]]])


def score_bound(terms, tol):
    'The bound on the error of a score: tol * (sum of |terms| along the path + 1).'
    return tol * (np.abs(np.asarray(terms, dtype=np.float64)).sum() + 1.)
