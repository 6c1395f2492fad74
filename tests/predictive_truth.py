'''The truth of the posterior-predictive (Student-t) density tests (beer_amd/csrc/predictive.hip,
the `beer_*_predictive_table` kernels of csrc/expfam.hip): the three closed forms in
`np.longdouble`, ln Gamma from tests/expfam_truth.py, for parameters given in float32 or float64
and upcast as they are -- numpy only.  tests/test_predictive_host.py ties the closed forms to the
conjugacy identity  ln p(x | eta) = A(eta + phi(x)) - A(eta) - D/2 ln 2 pi  through the oracle's
natural-parameter maps and `expfam_truth`'s log-normalisers, to quadrature and to the Gaussian
limit.

With kappa' = kappa / (kappa + 1), every form is  l = c - h L(x),  L >= 0:
  diagonal   c = D [lnG(a + 1/2) - lnG(a)] + 1/2 sum_d ln(kappa' / (2 pi b_d)),  h = a + 1/2,
             L = sum_d log1p(kappa' (x_d - m_d)^2 / (2 b_d))
  isotropic  c = lnG(a + D/2) - lnG(a) + D/2 ln(kappa' / (2 pi b)),  h = a + D/2,
             L = log1p(kappa' |x - m|^2 / (2 b))
  full       c = lnG((nu + 1)/2) - lnG((nu + 1 - D)/2) + 1/2 ln|W| + D/2 ln(kappa' / pi),
             h = (nu + 1)/2,  L = log1p(kappa' (x - m)^T W (x - m))
Functions return (l [T, K], c [K]): the bounds of the GPU tests are built from |c| and |l - c|,
the magnitudes of the two terms whose difference the value is.'''

import numpy as np

import expfam_truth as et

LD = et.LD
COV_TYPES = ('full', 'diagonal', 'isotropic')


def _col(a, K):
    return et.ld(a).reshape(K)


def ng_predictive(X, mean, scale, shape, rates):
    'Diagonal: mean [K, D], scale [K(,1)], shape [K(,1)], rates [K, D] -> (l [T, K], c [K]).'
    X, m, b = et.ld(X), et.ld(mean), et.ld(rates)
    K, D = m.shape
    kappa, a = _col(scale, K), _col(shape, K)
    kp = kappa / (kappa + 1)
    c = D * (et.lgamma(a + LD(.5)) - et.lgamma(a)) \
        + (np.log(kp[:, None] / (2 * et.PI * b))).sum(-1) / 2
    u = kp[None, :, None] * (X[:, None, :] - m[None]) ** 2 / (2 * b[None])
    return c[None] - (a + LD(.5))[None] * np.log1p(u).sum(-1), c


def ing_predictive(X, mean, scale, shape, rate):
    'Isotropic: mean [K, D], scale, shape, rate [K(,1)] -> (l [T, K], c [K]).'
    X, m = et.ld(X), et.ld(mean)
    K, D = m.shape
    kappa, a, b = _col(scale, K), _col(shape, K), _col(rate, K)
    kp = kappa / (kappa + 1)
    hd = LD(D) / 2
    c = et.lgamma(a + hd) - et.lgamma(a) + hd * np.log(kp / (2 * et.PI * b))
    q = ((X[:, None, :] - m[None]) ** 2).sum(-1)
    return c[None] - (a + hd)[None] * np.log1p(kp[None] * q / (2 * b[None])), c


def nw_predictive(X, mean, scale, scale_matrix, dof):
    'Full: mean [K, D], scale [K(,1)], scale_matrix [K, D, D], dof [K(,1)] -> (l [T, K], c [K]).'
    X, m, W = et.ld(X), et.ld(mean), et.ld(scale_matrix)
    K, D = m.shape
    kappa, nu = _col(scale, K), _col(dof, K)
    kp = kappa / (kappa + 1)
    hd = LD(D) / 2
    L = et.cholesky((W + W.transpose(0, 2, 1)) / 2)                  # W = L L^T
    logdet = 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
    c = et.lgamma((nu + 1) / 2) - et.lgamma((nu + 1) / 2 - hd) + logdet / 2 \
        + hd * np.log(kp / et.PI)
    y = X[:, None, :] - m[None]                                      # [T, K, D]
    z = np.einsum('tkj,kji->tki', y, L)                              # L^T y
    q = (z * z).sum(-1)
    return c[None] - ((nu + 1) / 2)[None] * np.log1p(kp[None] * q), c


PREDICTIVE = {'full': nw_predictive, 'diagonal': ng_predictive, 'isotropic': ing_predictive}


def predictive(cov_type, X, params):
    '(l [T, K], c [K]) of the family of `cov_type`; `params`: its standard parameters in order.'
    return PREDICTIVE[cov_type](X, *params)


def log_mean_weights(conc):
    'ln E[pi] of Dirichlet rows: ln(c / sum c), longdouble.'
    conc = et.ld(conc)
    return np.log(conc / conc.sum(-1, keepdims=True))


def logsumexp(a, axis=-1):
    a = et.ld(a)
    m = a.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def mixture(l, log_mean_w, S, G):
    'ln sum_g exp(lmw[s, g] + l[t, s G + g]) -> [T, S]; `log_mean_w` [S, G] or None (= 0).'
    terms = et.ld(l).reshape(len(l), S, G)
    if log_mean_w is not None:
        terms = terms + et.ld(log_mean_w).reshape(1, S, G)
    return logsumexp(terms, -1)


def magnitude(l, c):
    '1 + |c_k| + |l_tk - c_k|: the size of the terms an entry is the difference of.'
    return 1 + np.abs(et.ld(c))[None] + np.abs(et.ld(l) - et.ld(c)[None])


def component_bound(l, c, tol):
    return tol * magnitude(l, c)


def state_bound(l, c, log_mean_w, S, G, tol, window=40.):
    '''tol x the largest `magnitude` among a state's components whose term lies within `window`
    nats of the state's largest (the others contribute less than exp(-40) of the sum).'''
    T = len(l)
    terms = et.ld(l).reshape(T, S, G)
    if log_mean_w is not None:
        terms = terms + et.ld(log_mean_w).reshape(1, S, G)
    near = terms >= terms.max(-1, keepdims=True) - window
    mag = np.where(near, magnitude(l, c).reshape(T, S, G), 0)
    return tol * mag.max(-1)


# ---- the conjugacy identity: the independent second derivation -----------------------------------

def log_norm_natural(cov_type, eta):
    '''A(eta) of one pdf given in the project's natural form: back to standard parameters with the
    oracle's `*_from_natural`, then `expfam_truth`'s log-normaliser in longdouble.'''
    from oracle import beer_oracle as orc
    eta = np.asarray(eta, dtype=np.float64)[None]
    if cov_type == 'full':
        mean, scale, W, dof = orc.nw_from_natural(eta)
        _, logdet = et.spd_solve(W=.5 * (W + W.transpose(0, 2, 1)))
        return et.nw_log_norm(scale[:, 0], dof[:, 0], logdet, mean.shape[1])[0]
    iso = cov_type == 'isotropic'
    mean, scale, shape, rates = (orc.ing_from_natural if iso else orc.ng_from_natural)(eta)
    return et.ng_log_norm(mean, scale, shape, rates, iso)[0]


def conjugacy_identity(cov_type, x, params):
    '''ln p(x | eta) = A(eta + phi(x)) - A(eta) - D/2 ln 2 pi of ONE pdf (`params`: its standard
    parameters with a leading dimension of 1, float64) at ONE frame x [D].'''
    from oracle import beer_oracle as orc
    natural = {'full': orc.nw_natural, 'diagonal': orc.ng_natural, 'isotropic': orc.ing_natural}
    eta = natural[cov_type](*params)[0]
    phi = orc.SUFFSTATS[cov_type](np.asarray(x, dtype=np.float64)[None])[0]
    return log_norm_natural(cov_type, eta + phi) - log_norm_natural(cov_type, eta) \
        - len(x) * et.LOG2PI / 2
