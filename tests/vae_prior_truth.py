"""Inputs and float64 truth for the sweep of the kernels behind a VAE's prior
(tests/test_gpu_vae_prior_routes.py), numpy only.

Truth is the oracle (oracle/beer_oracle.py) in float64 on the exact values a kernel is handed:
the inputs of a float32 case are rounded to float32 first.  `orc.SUFFSTATS` gives the statistics,
`stats @ E.T + base` the log-likelihoods, `orc.mixtureset_accumulate` the accumulation,
`orc.suffstats_backward` and `orc.prior_gradient_wrt_samples` the gradients and
`orc.mixtureset_estep` the softmax over groups.  With several samples per frame the statistics are
the mean of `orc.SUFFSTATS` over each run of `ns` rows, and the gradient is
`orc.suffstats_backward` of the repeated upstream gradient divided by `ns`.

Beside every truth stands its error scale s: the same expression with every operand replaced by
its absolute value and every subtraction by an addition, s[m, n] = sum_k |A(m, k)| |B(k, n)| for a
product.  A dot product of n terms computed in any order in a format with unit roundoff u is
within (n + 2) u s of the truth (two more roundings than terms: the factors applied after it).

Inputs under which a misplaced tile cannot pass:

* every row and every column of every operand that is free to have one carries a scale of its
  own, `scales(n)` = 1 + 3 frac(i 0.618..) in [1, 4]: a swapped, clamped or dropped row or column
  moves the result by a fraction of itself;
* frames sit away from the origin (`estep_truth.geometry`: offset + spread * randn), so that the
  linear and the quadratic part of a gradient partly cancel, and the parameters of an operation
  that has a covariance type are `orc.FAMILIES[cov]['exp']` of `estep_truth.std_params`;
* weights are posteriors (non-negative, rows summing to one, a fifth of the entries exactly 0) or
  signed with zero mean (what `_FrameLlh.backward` and `_DenseLlh.backward` pass on: an upstream
  gradient of either sign times the posteriors); the per-frame factor has both signs as well;
* the dense accumulation on `gemm_kernel` in float32 with state posteriors gets statistics whose
  columns keep one sign each, as those of frames away from the origin do (positive first moments,
  negative second moments): its truth then equals its error scale up to the sign, which that form
  needs -- `gemm_kernel` forms the joint posterior w[t, k] sr[t, k / G] in the type of its
  operands, one float32 rounding per term that `2^-24 |truth|` covers only where nothing cancels.
  Every other accumulation case sums statistics of both signs.
"""

import numpy as np

import estep_truth as et
from helpers import orc

PHI = 0.6180339887498949
COVS = et.COVS


def scales(n, salt=0):
    'A deterministic factor in [1, 4] per index.'
    return 1. + 3. * np.modf((np.arange(n) + 1. + salt) * PHI)[0]


def stats_dim(cov, D):
    return orc.stats_dim(cov, D)


def posteriors(rng, T, S, G):
    '[T, S G]: non-negative, every group of G summing to one, a fifth of the entries exactly 0.'
    r = rng.random((T, S, G)) * scales(S * G, 3).reshape(1, S, G) * (rng.random((T, S, G)) < .8)
    r[:, :, 0] += 1e-3 * (r.sum(2) == 0)
    return (r / r.sum(2, keepdims=True)).reshape(T, S * G)


def row_posteriors(rng, T, K):
    '''[T, K] for the dense products, which take any weights: non-negative with a scale per
    component, a fifth of the entries exactly 0, rows summing to one over all K -- so that the
    weights differ from frame to frame and from component to component also where every group
    holds one component (`posteriors` gives ones there).  K = 1: a weight per frame in [0, 4).'''
    r = rng.random((T, K)) * scales(K, 3)[None, :] * (rng.random((T, K)) < .8)
    if K == 1:
        return r * scales(T, 29)[:, None]
    r[:, 0] += 1e-3 * (r.sum(1) == 0)
    return r / r.sum(1, keepdims=True)


def signed_weights(rng, T, K):
    '[T, K]: zero-mean, a scale per component and per frame.'
    return rng.standard_normal((T, K)) * scales(K, 5)[None, :] * scales(T, 11)[:, None]


def factor(rng, T):
    'The per-frame upstream gradient: either sign, magnitude in [1, 4].'
    return scales(T, 17) * np.where(rng.random(T) < .5, -1., 1.)


def state_posteriors(rng, T, S):
    'Sparse [T, S], the first frame dense.'
    sr = rng.random((T, S)) * (rng.random((T, S)) < .6)
    sr[0] = .25 + .5 * rng.random(S)
    return sr


def dense_inputs(T, Q, K, S, seed, dtype, one_signed=False):
    '''Operands of the three statistics-in products for T frames, Q statistics and K components
    in S groups, in `dtype`: statistics st [T, Q] (a scale per row and per column; away from zero;
    `one_signed`: every column keeps its sign), parameters E [K, Q] (signed, a scale per row and
    per column), posteriors w [T, K] (within each of the S groups; over the whole row where the
    groups hold one component each), signed weights ws [T, K], the per-frame factor g [T] and the
    state posteriors sr [T, S].'''
    rng = np.random.default_rng(seed)
    n = max(T, 1)
    st = (1.5 + .5 * rng.standard_normal((n, Q))) * scales(n, 1)[:, None] * scales(Q, 2)[None, :]
    st *= np.where(np.arange(Q) % 2, -1., 1.)[None, :]
    if not one_signed:
        st *= np.where(rng.random((n, 1)) < .3, -1., 1.)
    E = rng.standard_normal((K, Q)) / np.sqrt(Q) * scales(K, 7)[:, None] * scales(Q, 13)[None, :]
    w = posteriors(rng, n, S, K // S) if K // S > 1 else row_posteriors(rng, n, K)
    inp = dict(st=st, E=E, w=w, ws=signed_weights(rng, n, K),
               g=factor(rng, n), sr=state_posteriors(rng, n, S))
    return {k: np.ascontiguousarray(v[:T].astype(dtype) if k != 'E' else v.astype(dtype))
            for k, v in inp.items()}


def frame_inputs(cov, D, K, T, seed, dtype, ns=1):
    '''Operands of the kernels that take frames: X [T ns, D] (`estep_truth.geometry`), E [K, Q]
    (`orc.FAMILIES[cov]['exp']` of `estep_truth.std_params`), posteriors w, signed weights ws
    [T, K], the factor g [T] and an upstream gradient of the statistics gs [T, Q] (signed, a scale
    per row and per column).  A shorter T is a prefix of a longer one.'''
    rng = np.random.default_rng(seed)
    n = max(T, 1)
    offset, spread = et.geometry(cov, D)
    X = offset + spread * rng.standard_normal((n * ns, D))
    E = orc.FAMILIES[cov]['exp'](*et.std_params(cov, D, K, seed))
    Q = stats_dim(cov, D)
    gs = rng.standard_normal((n, Q)) * scales(n, 19)[:, None] * scales(Q, 23)[None, :]
    inp = dict(X=X, E=E, w=row_posteriors(rng, n, K), ws=signed_weights(rng, n, K), g=factor(rng, n),
               gs=gs)
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in inp.items()}


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# --- truth and error scale -----------------------------------------------------------------------

def llh(st, E, base):
    'beer_dense_llh: (truth, s, inner length).'
    st, E = f64(st), f64(E)
    return st @ E.T + base, np.abs(st) @ np.abs(E).T + abs(base), st.shape[1] + 1


def llh_backward(w, g, E):
    'beer_dense_llh_backward: g_t sum_k w[t, k] E[k, :].'
    w, E = f64(w), f64(E)
    gg = np.ones(len(w)) if g is None else f64(g)
    return gg[:, None] * (w @ E), np.abs(gg)[:, None] * (np.abs(w) @ np.abs(E)), w.shape[1] + 1


def accumulate(st, w, sr, S, G):
    'beer_dense_accumulate through orc.mixtureset_accumulate: (truth [S G, Q], s, inner length).'
    st, w = f64(st), f64(w)
    T = len(st)
    sr = np.ones((T, S)) if sr is None else f64(sr)
    truth = orc.mixtureset_accumulate(st, w.reshape(T, S, G), sr)[1]
    s = orc.mixtureset_accumulate(np.abs(st), np.abs(w).reshape(T, S, G), np.abs(sr))[1]
    return truth, s, 2 * T


def suffstats_mean(cov, X, ns):
    'beer_suffstats_mean: the mean of orc.SUFFSTATS over each run of ns rows.'
    X = f64(X)
    T, D = len(X) // ns, X.shape[1]
    st = orc.SUFFSTATS[cov](X)
    truth = st.reshape(T, ns, -1).mean(1)
    s = np.abs(st).reshape(T, ns, -1).mean(1)
    return truth, s, ns * (D if cov == 'isotropic' else 1) + 2


def abs_suffstats_backward(cov, X, gs):
    'orc.suffstats_backward with every operand positive and every subtraction an addition.'
    X, gs = np.abs(X), np.abs(gs)
    T, D = X.shape
    out = gs[:, :D].copy()
    if cov == 'full':
        G = gs[:, D:D + D * D].reshape(T, D, D)
        out += .5 * (np.einsum('tij,tj->ti', G, X) + np.einsum('tji,tj->ti', G, X))
    elif cov == 'diagonal':
        out += gs[:, D:2 * D] * X
    else:
        out += gs[:, D:D + 1] * X
    return out


def suffstats_backward(cov, X, gs, ns):
    'beer_suffstats_backward: orc.suffstats_backward of the repeated gradient divided by ns.'
    X, gs = f64(X), f64(gs)
    D = X.shape[1]
    rep = np.repeat(gs, ns, axis=0) / ns
    return (orc.suffstats_backward(cov, X, rep), abs_suffstats_backward(cov, X, rep),
            (2 * D if cov == 'full' else 1) + 3)


def frames_gradient(cov, X, w, E, g):
    'beer_frames_llh_backward through orc.prior_gradient_wrt_samples: (truth [T, D], s, inner).'
    X, w, E = f64(X), f64(w), f64(E)
    D, K = X.shape[1], w.shape[1]
    truth = orc.prior_gradient_wrt_samples(cov, X, w, E, f64(g))
    wa = np.abs(w) if g is None else np.abs(w) * np.abs(f64(g))[:, None]
    s = abs_suffstats_backward(cov, X, wa @ np.abs(E))
    return truth, s, K * ((2 * D if cov == 'full' else 1) + 1) + 3


def softmax_groups(pc, lw, S, G):
    '''beer_softmax_groups through orc.mixtureset_estep: every (frame, group) as a state of its
    own whose logits are pc + log-weights; (log_norm [T, S], resps [T, S G]).'''
    pc = f64(pc)
    T = len(pc)
    w = pc.reshape(T, S, G) + (0. if lw is None else f64(lw)[None])
    zero = np.zeros((1, 1))
    with np.errstate(invalid='ignore', over='ignore'):
        ln, r = orc.mixtureset_estep(zero, np.zeros((T * S * G, 1)), 0, w.reshape(T * S, G))
    return ln.reshape(T, S), r.reshape(T, S * G)


def rowdot(a, b):
    a, b = f64(a), f64(b)
    return (a * b).sum(1), (np.abs(a) * np.abs(b)).sum(1), a.shape[1]
