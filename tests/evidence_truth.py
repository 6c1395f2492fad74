"""The float64 truth of the forward log-evidence (csrc/hmm_score.hip): plain numpy on the graphs
and inputs of tests/fb_truth.py, float32 inputs upcast (no GPU needed).

 * `evidence`: the per-frame terms c_t = ln p(x_t | x_0 .. x_{t-1}) and the utterance's total
   sum_t c_t + ln sum_j exp(â_{T-1}(j) + final_j), by the definition of include/beer_hip.h
   (beer_hmm_log_evidence), with its -inf rules: from the first frame at which nothing is
   reachable every c_t is -inf and so is the total; an unreachable final term alone leaves the
   frames finite and makes the total -inf;
 * `brute_force`: the logarithm of the sum over all S^T state paths of exp(path score);
 * `route_formula`: beer_hmm_evidence_route restated from the header's text;
 * `total_bound`: the tolerance on an utterance's total, from the magnitudes of the truth."""

import itertools

import numpy as np

EINVAL = -100000            # BEER_EINVAL
WAVE, BLOCK, ARCS_LDS, QUAD = 0x1000, 0x2000, 0x100, 0x200


def route_formula(S, A, itemsize):
    """beer_hmm_evidence_route restated from the header's text: S = max_states, A = max_arcs,
    `itemsize` 4 / 8 bytes of the dtype."""
    if S < 1 or S > 32767 or A < 0 or itemsize not in (4, 8):
        return EINVAL
    if 16 * S + 128 > 160 * 1024:
        return EINVAL
    arcs = 4 * (S + 2 + A) + itemsize * A
    spl = 1 if S <= 64 else (2 if S <= 128 else 4)
    if S <= 256 and 512 * spl + arcs <= 16 * 1024:
        return WAVE | spl
    return BLOCK | (ARCS_LDS if 16 * S + 128 + arcs <= 64 * 1024 else 0) | \
        (QUAD if 4 * S <= 512 else 0)


def _f64(graph):
    return tuple(np.asarray(graph[k], dtype=np.float64) for k in ('init', 'final', 'trans'))


def _lse(v):
    'ln sum exp(v) of a vector; -inf when nothing is finite.'
    m = v.max() if len(v) else -np.inf
    if not np.isfinite(m):
        return -np.inf
    return m + np.log(np.exp(v - m).sum())


def evidence(graph, llh):
    '(c [T] float64, total): total = c.sum() + the final term ln sum_j exp(â_{T-1}(j) + final_j).'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T = len(llh)
    c = np.empty(T)
    with np.errstate(invalid='ignore', divide='ignore'):
        a = llh[0] + init
        for t in range(T):
            if t:
                hyp = a[:, None] + trans                            # [source, destination]
                m = hyp.max(0)
                base = np.where(np.isfinite(m), m, 0.)
                a = llh[t] + base + np.log(np.exp(hyp - base[None, :]).sum(0))
                a = np.where(np.isfinite(m), a, -np.inf)
            c[t] = _lse(a)
            if not np.isfinite(c[t]):
                c[t:] = -np.inf
                return c, -np.inf
            a = a - c[t]
        tail = _lse(a + final)
    return c, (c.sum() + tail if np.isfinite(tail) else -np.inf)


def brute_force(graph, llh):
    'ln of the sum over all S^T paths of exp(init + sum llh + sum trans + final).'
    init, final, trans = _f64(graph)
    llh = np.asarray(llh, dtype=np.float64)
    T, S = llh.shape
    scores = []
    with np.errstate(invalid='ignore'):
        for path in itertools.product(range(S), repeat=T):
            p = np.asarray(path)
            scores.append(init[p[0]] + llh[np.arange(T), p].sum() + trans[p[:-1], p[1:]].sum() +
                          final[p[-1]])
    return _lse(np.asarray(scores))


def total_bound(c, total, tol):
    '''The bound on |utt_evidence - total|: tol * (sum_t |c_t| + |tail| + 1), the tail being the
    final term total - sum_t c_t (a relative bound on the total alone is ill-conditioned: short
    utterances have totals near 0).'''
    fin = np.isfinite(c)
    tail = abs(total - c.sum()) if np.isfinite(total) else 0.
    return tol * (np.abs(c[fin]).sum() + tail + 1.)
