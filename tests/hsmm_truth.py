"""The truth of the explicit-duration (hidden semi-Markov) entry points of csrc/hsmm.hip: the
definitions of include/beer_hip.h restated in the plainest way, direct sums over (start, duration)
in numpy, float32 inputs upcast (no GPU needed).  The recursions run in numpy's long double (at
least float64; 64 bits of mantissa on x86), so that the truth of a 4096-frame utterance is good
to far below the 1e-10 it is asked to hold; `best_path` stays in float64, where the integer cases
are exact.

 * `posteriors`: gamma, Z, the duration counts by pdf id, the segment entries per state;
 * `best_path`: the best segmentation, ties broken as the header says;
 * `path_score`: the score of a given state path (its runs are the segments);
 * `brute_force`: the same quantities by enumeration of every segmentation (S <= 3, T <= 5);
 * `expanded`: the count-down HMM of S D states that computes the same thing with the
   repository's HMM oracle;
 * `route_formula`: beer_hsmm_route restated from the header's text;
 * `frame_terms`: per-frame magnitudes for evidence_truth.total_bound."""

import itertools

import numpy as np

L = np.longdouble
EINVAL = -100000
BLOCK, RING_LDS, LOWDEG = 0x1000, 0x100, 0x200
MAX_DUR, MAX_STATES = 128, 2048


def route_formula(S, D, itemsize, all_lowdeg=0, max_degree=0, max_hubs=0):
    'beer_hsmm_route restated from the header\'s text (S = max_states).'
    if itemsize not in (4, 8) or D < 1 or D > MAX_DUR or S < 1 or S > MAX_STATES:
        return EINVAL
    team = 1
    while team * 2 <= 64 and (team * 2) // 2 < D and team * 2 * S <= 256:
        team *= 2
    route = BLOCK | (team.bit_length() - 1)
    if 8 * (8 * S + 32 + 2 * S * D) <= 160 * 1024:
        route |= RING_LDS
    if all_lowdeg and max_degree > 0 and max_hubs <= 4:
        route |= LOWDEG
    return route


def scratch_formula(S, D, itemsize, nutt):
    'beer_hsmm_scratch_doubles restated from the header\'s text.'
    r = route_formula(S, D, itemsize)
    if r == EINVAL or r & RING_LDS:
        return 0
    return min(nutt, 512) * 2 * S * D


def _lse(v, axis=0):
    'ln sum exp along `axis`; -inf where nothing is finite.'
    v = np.asarray(v, dtype=L)
    with np.errstate(invalid='ignore', divide='ignore'):
        m = v.max(axis=axis)
        base = np.where(np.isfinite(m), m, 0.)
        s = np.exp(v - np.expand_dims(base, axis)).sum(axis=axis)
        return np.where(s > 0, base + np.log(s), -np.inf)


def tables(graph, log_dur, leave_w, ids=None, dtype=L):
    '''(init [S], final [S], W [S, S], lam [S, D]): W_ij = trans_ij + leave_w[id(i)] with the
    diagonal removed, lam_j = log_dur[id(j)].'''
    S = graph['S']
    ids = np.arange(S) if ids is None else np.asarray(ids)
    init, final, trans = (np.asarray(graph[k], dtype=dtype) for k in ('init', 'final', 'trans'))
    lv = np.zeros(S, dtype=dtype) if leave_w is None else np.asarray(leave_w, dtype=dtype)[ids]
    W = trans + lv[:, None]
    W[np.arange(S), np.arange(S)] = -np.inf
    return init, final, W, np.asarray(log_dur, dtype=dtype)[ids]


def posteriors(graph, log_dur, leave_w, llh, ids=None):
    '''dict(gamma [T, S], Z, dur_counts [S_total, D], dur_state [S, D], entry_sum [S],
    gamma0_sum [S]) of ONE utterance, float64.  Z = -inf: zeros everywhere.'''
    S = graph['S']
    ids = np.arange(S) if ids is None else np.asarray(ids)
    init, final, W, lam = tables(graph, log_dur, leave_w, ids)
    l = np.asarray(llh, dtype=L)
    T, D = len(l), lam.shape[1]
    seg = lambda s, d: l[s:s + d].sum(0)                              # noqa: E731
    with np.errstate(invalid='ignore', divide='ignore'):
        beg = np.full((T, S), -np.inf, dtype=L)
        end = np.full((T, S), -np.inf, dtype=L)
        for t in range(T):
            beg[t] = init if t == 0 else _lse(end[t - 1][:, None] + W, 0)
            end[t] = _lse(np.stack([beg[t - d + 1] + lam[:, d - 1] + seg(t - d + 1, d)
                                    for d in range(1, min(D, t + 1) + 1)]), 0)
        Z = _lse(end[T - 1] + final, 0)
        bend = np.full((T, S), -np.inf, dtype=L)
        bbeg = np.full((T, S), -np.inf, dtype=L)
        for t in reversed(range(T)):
            bend[t] = final if t == T - 1 else _lse(W + bbeg[t + 1][None, :], 1)
            bbeg[t] = _lse(np.stack([lam[:, d - 1] + seg(t, d) + bend[t + d - 1]
                                     for d in range(1, min(D, T - t) + 1)]), 0)
        gamma = np.zeros((T, S), dtype=L)
        dur = np.zeros((S, D), dtype=L)
        entry = np.zeros(S, dtype=L)
        g0 = np.zeros(S, dtype=L)
        if np.isfinite(Z):
            for s in range(T):
                for d in range(1, min(D, T - s) + 1):
                    q = np.exp(beg[s] + lam[:, d - 1] + seg(s, d) + bend[s + d - 1] - Z)
                    q = np.where(np.isnan(q), 0., q)
                    gamma[s:s + d] += q
                    dur[:, d - 1] += q
                    if s:
                        entry += q
                    else:
                        g0 += q
    counts = np.zeros((np.asarray(log_dur).shape[0], D))
    np.add.at(counts, ids, dur.astype(np.float64))
    return dict(gamma=gamma.astype(np.float64), Z=float(Z), dur_counts=counts,
                dur_state=dur.astype(np.float64), entry_sum=entry.astype(np.float64),
                gamma0_sum=g0.astype(np.float64))


def frame_terms(truth, llh):
    'c [T] = sum_j gamma_t(j) l_t(j): the per-frame magnitudes evidence_truth.total_bound sums.'
    l = np.asarray(llh, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(truth['gamma'] > 0, truth['gamma'] * l, 0.).sum(1)


def best_path(graph, log_dur, leave_w, llh, ids=None):
    '''(path [T] int64, score): max for lse.  Ties: the shorter duration first, then the smaller
    source state, then at the end the smaller final state.  No finite path: (-1 .., -inf).'''
    S = graph['S']
    init, final, W, lam = tables(graph, log_dur, leave_w, ids, np.float64)
    l = np.asarray(llh, dtype=np.float64)
    T, D = len(l), lam.shape[1]
    beg = np.full((T, S), -np.inf)
    end = np.full((T, S), -np.inf)
    src = np.full((T, S), -1, dtype=np.int64)
    dur = np.zeros((T, S), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for t in range(T):
            if t == 0:
                beg[0] = init
            else:
                hyp = end[t - 1][:, None] + W                        # [source, destination]
                src[t] = np.argmax(hyp, 0)                           # (first index: smaller source)
                beg[t] = hyp.max(0)
            cand = np.stack([beg[t - d + 1] + lam[:, d - 1] + l[t - d + 1:t + 1].sum(0)
                             for d in range(1, min(D, t + 1) + 1)])
            dur[t] = np.argmax(cand, 0) + 1                          # (first index: shorter)
            end[t] = cand.max(0)
        tot = end[T - 1] + final
    if not np.isfinite(tot.max()):
        return np.full(T, -1, dtype=np.int64), -np.inf
    j, t = int(np.argmax(tot)), T - 1
    path = np.zeros(T, dtype=np.int64)
    while True:
        d = int(dur[t, j])
        path[t - d + 1:t + 1] = j
        s = t - d + 1
        if s == 0:
            break
        j, t = int(src[s, j]), s - 1
    return path, float(tot.max())


def path_score(graph, log_dur, leave_w, llh, path, ids=None):
    'The score of the segmentation whose segments are the runs of `path` (-inf: not allowed).'
    init, final, W, lam = tables(graph, log_dur, leave_w, ids, np.float64)
    l = np.asarray(llh, dtype=np.float64)
    path = np.asarray(path)
    T, D = len(l), lam.shape[1]
    cuts = [0] + [t for t in range(1, T) if path[t] != path[t - 1]] + [T]
    score = init[path[0]]
    with np.errstate(invalid='ignore'):
        for s, e in zip(cuts[:-1], cuts[1:]):
            j, d = path[s], e - s
            if d > D:
                return -np.inf
            if s:
                score = score + W[path[s - 1], j]
            score = score + lam[j, d - 1] + l[s:e, j].sum()
    return float(score + final[path[-1]])


def brute_force(graph, log_dur, leave_w, llh, ids=None):
    '''The same dict as `posteriors`, plus `best` (the largest segmentation score), by enumeration
    of every segmentation: sequences of (state, duration) whose durations add up to T, neighbours
    in different states.'''
    S = graph['S']
    ids = np.arange(S) if ids is None else np.asarray(ids)
    init, final, W, lam = tables(graph, log_dur, leave_w, ids, np.float64)
    l = np.asarray(llh, dtype=np.float64)
    T, D = len(l), lam.shape[1]
    assert S <= 3 and T <= 5
    segs = []                                                        # (score, [(j, s, d)])

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
                sofar.append((j, t, d))
                walk(t + d, j, sc, sofar)
                sofar.pop()

    walk(0, -1, 0., [])
    scores = np.asarray([s for s, _ in segs])
    Z = float(_lse(scores, 0)) if len(scores) else -np.inf
    out = dict(gamma=np.zeros((T, S)), Z=Z, dur_state=np.zeros((S, D)), entry_sum=np.zeros(S),
               gamma0_sum=np.zeros(S), best=float(scores.max()) if len(scores) else -np.inf)
    if np.isfinite(Z):
        for sc, seq in segs:
            p = np.exp(sc - Z) if np.isfinite(sc) else 0.
            for j, s, d in seq:
                out['gamma'][s:s + d, j] += p
                out['dur_state'][j, d - 1] += p
                (out['entry_sum'] if s else out['gamma0_sum'])[j] += p
    counts = np.zeros((np.asarray(log_dur).shape[0], D))
    np.add.at(counts, ids, out['dur_state'])
    out['dur_counts'] = counts
    return out


def expanded(graph, log_dur, leave_w, ids=None):
    '''The count-down HMM: state (j, r) at index j D + r - 1 has r frames left to stay.
    (j, r) -> (j, r-1) with weight 0; (i, 1) -> (j, d) with w_ij + lam_j(d); init (j, d) =
    init_j + lam_j(d); final on (j, 1) only.  A graph dict for the HMM oracle (float64).'''
    S = graph['S']
    init, final, W, lam = tables(graph, log_dur, leave_w, ids, np.float64)
    D = lam.shape[1]
    n = S * D
    trans = np.full((n, n), -np.inf)
    with np.errstate(invalid='ignore'):
        for j in range(S):
            for r in range(2, D + 1):
                trans[j * D + r - 1, j * D + r - 2] = 0.
            for i in range(S):
                if i != j:
                    trans[i * D, j * D:(j + 1) * D] = W[i, j] + lam[j]
        e_init = (init[:, None] + lam).reshape(-1)
    e_final = np.full(n, -np.inf)
    e_final[::D] = final
    return dict(S=n, init=e_init, final=e_final, trans=trans, hub=None)


def geometric_log_dur(graph, D, ids=None, S_total=None):
    'log_dur[id(j)][d-1] = (d - 1) trans_jj, unnormalised: the HMM\'s own geometric stay.'
    S = graph['S']
    ids = np.arange(S) if ids is None else np.asarray(ids)
    out = np.zeros((S if S_total is None else S_total, D))
    diag = np.asarray(graph['trans'], dtype=np.float64)[np.arange(S), np.arange(S)]
    with np.errstate(invalid='ignore'):
        rows = np.arange(D)[None, :] * diag[:, None]
    rows[:, 0] = 0.
    out[ids] = rows
    return out
