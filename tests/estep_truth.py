"""Inputs and float64 truth for the E-step sweep (tests/test_gpu_estep_routes.py), numpy only.

Truth is the oracle itself -- `orc.mixtureset_estep` over `orc.SUFFSTATS[cov]` and the expected
statistics of `orc.FAMILIES[cov]['exp']` -- in float64 on the exact values a kernel is handed: for
a float32 case the frames, E[T] and the log-weights are rounded to float32 first.  No vectorised
shortcut stands between the tests and the oracle.

The generator (`make`) builds inputs under which a wrong kernel cannot pass:

* every component has a mean, a precision and a log-weight of its own in every dimension; full
  covariances are dense (every off-diagonal pair carries a parameter, as `_full_cov_gaussians` of
  test_gpu_band_layout.py does it);
* the frames sit away from the origin (`X * spread + offset`), so that the terms of a logit
  (-1/2 x'Lx, (L mu)'x, the constant) are larger than their sum -- ten times larger wherever
  float32 can carry that.  The spread is sqrt(2.5 / D) capped at 0.5 and the mean precision 2 pi:
  the squared distance of a frame to a component is then about 5 at every D (30 in the tail of
  90 000 frame-component pairs), the per-dimension constants 1/2 (E ln L - ln 2 pi) cancel on
  average, and the log-normalisers stay below 100 nats (about 40) up to D = 128 -- the float32
  bound 1e-5 max |ln| is then small against what a misplaced slab does to a logit (0.1 .. 10).
  The linear terms (L mu)'x add up to M = 2 pi offset^2 D; `geometry` picks the offset (3 at
  most) for M = r |ln| with |ln| = 30 and r = min(10, 235 / D, 500 / a), which puts the worst
  rounding error of a CORRECT float32 kernel at half the bound, for the two float32 arithmetics:
    - the exact fp32 MFMA rounds to nearest: an accumulator that holds M rounds each of the n
      products it adds by up to 3e-8 M, 3e-8 M sqrt(n) in all; a dense covariance has n = D^2 / 2,
      so 1e-5 |ln| / 2 allows M = 235 |ln| / D;
    - the bf16x3 kernels accumulate in the MFMA's float32 accumulator, which TRUNCATES (DESIGN.md,
      estep_tiles.h: "the bf16 MFMA truncates"): one-sided, about 4e-8 of the running sum (M / 4
      on average: the quadratic terms first, then the linear ones) in each of the a = 6 x k-steps
      accumulations of a logit, 1e-8 a M in all, so 1e-5 |ln| / 2 allows M = 500 |ln| / a.
      Diagonal / isotropic: at most 10 k-steps (D = 128), r = 8 .. 10 throughout.  Full covariance
      (band layout: about Dp^2 / 64 k-steps): r = 10 up to D = 13, 3.1 at D = 37 .. 40, 2.1 at 48,
      1 at 72, 0.3 at D = 128 -- there float32 cannot hold terms larger than the sum to 1e-5 of
      it, and test_gpu_band_layout.py's own D = 128 inputs (logits of 700, terms below that) are
      no different.
  (Measured with larger terms, full covariance: r = 40 at every D -- exact fp32 1.55 x the bound
  at D = 44; r = 10 -- exact fp32 1.16 x at D = 96, bf16x3 up to 1.5 x at D = 37 .. 48; the model
  above without its factor 2 -- bf16x3 1.04 x at D = 40.  The errors follow M as the model says;
  the float64 instantiations of the same templates sat at 4e-12 throughout.);
* state 0 of a set has a dominant component (4 nats ahead), state 1 is near-uniform, the others
  draw their weights at random;
* optionally one component per state with log-weight -1e30 (the phantom of `wide_mixture_estep`:
  responsibility exactly 0, the state's normaliser that of the state without it) and one frame
  40 standard deviations out.
"""

import numpy as np

from helpers import orc

COVS = ('full', 'diagonal', 'isotropic')
PHANTOM = -1e30
MEAN_PRECISION = 2 * np.pi


MEAN_LN = 30.               # the low end of max |ln| over the cases (25 .. 65)


def ksteps(cov, D):
    'k-steps (8 slabs of 4 products) of a logit in the bf16x3 kernels: csrc/estep_tiles.h.'
    D4 = (D + 3) // 4
    if cov == 'full':
        Dp, h = 4 * D4, 2 * D4
        nslab = h * D4 + (h + 3) // 4 + D4 + 1                   # band_nslab + linear + constant
    else:
        nslab = 2 * D4 + (2 * D4 - 1) // 7 + 1                   # diag_walk
    return (nslab + 7) // 8


def geometry(cov, D):
    '(offset, spread) of the frames: see the module docstring.'
    r = min(10., 500. / (6 * ksteps(cov, D)))
    if cov == 'full':
        r = min(r, 235. / D)
    return min(3., np.sqrt(r * MEAN_LN / (MEAN_PRECISION * D))), min(.5, np.sqrt(2.5 / D))


def std_params(cov, D, K, seed, S=1):
    'Standard parameters of K posteriors of the family, float64 (oracle/beer_oracle.py FAMILIES).'
    rng = np.random.default_rng(seed)
    offset, spread = geometry(cov, D)
    G = K // S
    centre = offset + spread * .7 * rng.standard_normal((S, 1, D))
    mean = (centre + spread * .7 * rng.standard_normal((S, G, D))).reshape(K, D)
    scale = 40. + 20. * rng.random((K, 1)) + 4. * D
    lam = MEAN_PRECISION * np.exp(rng.uniform(-.3, .3, (K, D)))
    if cov == 'full':
        dof = 4. * D + 20. + rng.integers(0, 5, (K, 1))
        L = np.eye(D) + np.tril(rng.standard_normal((K, D, D)), -1) * (.5 / np.sqrt(D))
        prec = L @ L.transpose(0, 2, 1)
        d = np.sqrt(lam / np.einsum('kii->ki', prec))        # unit diagonal first, then lam
        prec = d[:, :, None] * prec * d[:, None, :]
        return mean, scale, prec / dof[:, :, None], dof
    if cov == 'diagonal':
        shape = 20. + 10. * rng.random((K, 1))
        return mean, scale, shape, shape / lam
    shape = 20. + 10. * rng.random((K, 1))
    return mean, scale, shape, shape / lam[:, :1]


def log_weights(S, G, seed, phantom=False):
    '''[S, G]: state 0 with a dominant component, state 1 near-uniform, the others random; with
    `phantom` the last-but-one component of every state (the last one where G == 2) is absent.'''
    rng = np.random.default_rng(seed + 7919)
    w = rng.standard_normal((S, G))
    w[0] = .3 * rng.standard_normal(G)
    w[0, rng.integers(G)] += 4.
    if S > 1:
        w[1] = .05 * rng.standard_normal(G)
    w -= orc.logsumexp(w, axis=1)[:, None]
    if phantom:
        assert G >= 3
        w[:, G - 2] = PHANTOM
    return w


def make(cov, D, S, G, T, seed, dtype=np.float64, phantom=False, outlier=False, weights=True):
    '''The arrays a kernel is handed, in `dtype`: frames X [T, D], expected statistics E [S G, Q],
    log-weights lw [S, G] (None without `weights`: the `normal_llh` form).  The frames of a case
    are the first T of one stream per (D, seed): a shorter T is a prefix of a longer one.'''
    K = S * G
    offset, spread = geometry(cov, D)
    X = np.random.default_rng(seed + 104729).standard_normal((max(T, 1), D))[:T] * spread + offset
    if outlier and T:
        X[T // 2] = offset + 40. * spread * np.where(np.arange(D) % 2, -1., 1.)
    E = orc.FAMILIES[cov]['exp'](*std_params(cov, D, K, seed, S))
    lw = log_weights(S, G, seed, phantom) if weights else None
    return dict(X=np.ascontiguousarray(X.astype(dtype)), E=np.ascontiguousarray(E.astype(dtype)),
                lw=None if lw is None else np.ascontiguousarray(lw.astype(dtype)))


def truth(cov, inp, S, G):
    '''(log_norm [T, S], responsibilities [T, S G], pc_llh [T, S G]) of the oracle in float64 on
    the values of `inp` as they are.'''
    X, E = inp['X'].astype(np.float64), inp['E'].astype(np.float64)
    lw = np.zeros((S, G)) if inp['lw'] is None else inp['lw'].astype(np.float64)
    D = X.shape[1]
    stats = orc.SUFFSTATS[cov](X)
    ln, resps = orc.mixtureset_estep(stats, E, D, lw)
    return ln, resps.reshape(len(X), S * G), orc.normal_llh(stats, E, D)


def labels_truth(cov, inp, labels):
    '(log_norm [T, 1], one-hot responsibilities [T, K]) of mixture.py:85-87.'
    _, _, pc = truth(cov, inp, 1, len(inp['E']))
    resps = np.zeros_like(pc)
    resps[np.arange(len(pc)), labels] = 1.
    return pc[np.arange(len(pc)), labels][:, None], resps
