'''The truth of the distribution-kernel tests (beer_amd/csrc/expfam.hip): the parameter maps,
E[T], log-normalisers, KL, natural-gradient step and sufficient statistics of the five
families restated from the formulas of `oracle.beer_oracle` in `np.longdouble` (64-bit
mantissa where the platform has one), with psi and ln Gamma written here -- numpy only.
tests/test_expfam_host.py ties it to mpmath, to the g10 goldens and to the oracle.

Scale matrices come from two families:
  * exact:   W = L L^T, L lower triangular with off-diagonal multiples of 2^-5 in [-1/2, 1/2]
             and powers of two on the diagonal: W is exactly representable in float32, log|W| =
             2 sum log L_ii in closed form, W^-1 = L^-T L^-1 by a longdouble triangular solve;
  * generic: W = A A^T / D + c I, truth by a longdouble Cholesky factorisation.
A case holds a handful of distinct matrices `mats` [M, D, D] and `idx` [K] -> M: matrix
idx[k] belongs to pdf k, every k has its own mean, kappa and nu.'''

import numpy as np

from oracle import beer_oracle as orc

LD = np.longdouble
PI = LD('3.14159265358979323846264338327950288')
LOG2, LOGPI, LOG2PI = np.log(LD(2)), np.log(PI), np.log(2 * PI)
EPS64, EPS32 = 2. ** -53, 2. ** -24
F32_MAX = float(np.finfo(np.float32).max)
NP_DTYPE = {'float64': np.float64, 'float32': np.float32}


def ld(a):
    return np.asarray(a, dtype=LD)


# ---- special functions ----------------------------------------------------------------------

# Bernoulli numbers B_2, B_4, ... B_20
_B2K = [(1, 6), (-1, 30), (1, 42), (-1, 30), (5, 66), (-691, 2730), (7, 6), (-3617, 510),
        (43867, 798), (-174611, 330)]
_SHIFT = 20       # series from here: its 10th term is below 3e-25 at x = 20


def _recur(x, product):
    'x [..] > 0 -> (x + n >= _SHIFT, sum_{i<n} 1 / (x + i) or prod_{i<n} (x + i)).'
    x = np.array(x, dtype=LD, ndmin=1)
    acc = np.ones_like(x) if product else np.zeros_like(x)
    while True:
        low = x < _SHIFT
        if not low.any():
            return x, acc
        if product:
            acc[low] *= x[low]
        else:
            acc[low] += 1 / x[low]
        x[low] += 1


def digamma(x):
    'psi(x), x > 0: psi(x) = psi(x + n) - sum_i 1 / (x + i), asymptotic series at x + n >= 20.'
    shape = np.shape(x)
    x, acc = _recur(x, False)
    f = 1 / (x * x)
    s, p = np.zeros_like(x), f.copy()
    for k, (num, den) in enumerate(_B2K, 1):
        s += LD(num) / LD(den) / (2 * k) * p
        p *= f
    return (np.log(x) - 1 / (2 * x) - s - acc).reshape(shape)


def lgamma(x):
    'ln Gamma(x) = ln Gamma(x + n) - ln prod_i (x + i), x > 0: Stirling\'s series at x + n >= 20.'
    shape = np.shape(x)
    x, acc = _recur(x, True)
    f = 1 / (x * x)
    s, p = np.zeros_like(x), 1 / x
    for k, (num, den) in enumerate(_B2K, 1):
        s += LD(num) / LD(den) / (2 * k * (2 * k - 1)) * p
        p *= f
    return ((x - LD(.5)) * np.log(x) - x + LOG2PI / 2 + s - np.log(acc)).reshape(shape)


# ---- SPD matrices in longdouble ---------------------------------------------------------------

def cholesky(W):
    'W [M, D, D] -> lower factor [M, D, D] (longdouble, column by column).'
    W = ld(W)
    M, D, _ = W.shape
    L = np.zeros_like(W)
    for j in range(D):
        L[:, j, j] = np.sqrt(W[:, j, j] - (L[:, j, :j] ** 2).sum(-1))
        if j + 1 < D:
            L[:, j + 1:, j] = (W[:, j + 1:, j] - np.einsum('mik,mk->mi', L[:, j + 1:, :j],
                                                           L[:, j, :j])) / L[:, j, j, None]
    return L


def tri_inverse(L):
    'L [M, D, D] lower triangular -> L^-1 by forward substitution.'
    L = ld(L)
    M, D, _ = L.shape
    X = np.zeros_like(L)
    eye = np.eye(D, dtype=LD)
    for i in range(D):
        X[:, i, :] = (eye[i] - np.einsum('mk,mkj->mj', L[:, i, :i], X[:, :i, :])) / L[:, i, i, None]
    return X


def spd_solve(W=None, L=None):
    '(W^-1 [M, D, D], log|W| [M]) from W or from its lower factor L.'
    L = cholesky(W) if L is None else ld(L)
    Li = tri_inverse(L)
    logdet = 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
    return np.einsum('mki,mkj->mij', Li, Li), logdet


def exact_factor(rng, D, lo, hi, M=1):
    'L [M, D, D]: off-diagonal multiples of 2^-5 in [-1/2, 1/2], diagonal 2^lo .. 2^hi.'
    L = np.tril(rng.integers(-16, 17, (M, D, D)) / 32., -1)
    L[:, np.arange(D), np.arange(D)] = 2. ** rng.integers(lo, hi + 1, (M, D))
    return L


def generic_matrices(rng, D, c, M=1):
    'W = A A^T / D + c I [M, D, D], exactly symmetric.'
    A = rng.standard_normal((M, D, D))
    W = A @ A.transpose(0, 2, 1) / D + c * np.eye(D)
    return .5 * (W + W.transpose(0, 2, 1))


def _log_uniform(rng, lo, hi, n):
    'n values log-uniform in [lo, hi], the two ends among them (the low end first).'
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    v[0] = lo
    if n > 1:
        v[-1] = hi
    return v


# ---- Normal-Wishart ---------------------------------------------------------------------------

def nw_case(seed, K, D, family, span=1, c=.2, M=8, dyadic=False):
    '''dict(mats [M, D, D], idx [K], mean [K, D], scale [K], dof [K], ...).  `family` 'exact'
    draws M <= 3 factors L with diagonals from 2^-span .. 2^span (span = (lo, hi) for other
    ranges).  'generic' draws ONE matrix with `c` and takes M <= 8 symmetric permutations
    P W P^T of it: one spectrum, one scale and one truth (permuted), but M different sequences
    of pivots -- M samples of the rounding error of the oracle and of the kernel at the same
    conditioning, where one matrix would be one sample.  For the same reason nu = 1e7, which
    scales the log-normaliser and its error, is given to every other k.
    `dyadic`: means in multiples of 1/4 and kappa a power of two <= 8, so that the natural
    parameters with `mats` as the INVERSE scale matrices are exactly representable.'''
    rng = np.random.default_rng(seed)
    case = {'family': family, 'L': None, 'base': None, 'perms': None}
    if family == 'exact':
        M = min(M, K, 3)
        lo, hi = span if isinstance(span, tuple) else (-span, span)
        case['L'] = exact_factor(rng, D, lo, hi, M)
        case['mats'] = case['L'] @ case['L'].transpose(0, 2, 1)
    else:
        M = min(M, K)
        case['base'] = generic_matrices(rng, D, c)[0]
        case['perms'] = np.stack([np.arange(D)] + [rng.permutation(D) for _ in range(M - 1)])
        case['mats'] = _permuted(case['base'], case['perms'])
    scale = _log_uniform(rng, 1e-3, 1e7, K)
    # (means of the size of the component's standard deviation or below: kappa m m^T does
    # not bury W^-1 in the natural parameters)
    mean = rng.standard_normal((K, D)) * np.exp(rng.uniform(-2, 2, (K, 1))) \
        / np.sqrt(np.maximum(scale, 1.))[:, None]
    if dyadic:
        mean = rng.integers(-4, 5, (K, D)) / 4.
        scale = 2. ** rng.integers(-6, 4, K)
    dof = _log_uniform(rng, D - 1 + 1e-3, 1e7, K)
    dof[1::2] = 1e7
    if K == 1 and seed % 2:
        scale[0], dof[0] = (8. if dyadic else 1e7), 1e7
    case.update(idx=np.arange(K) % M, mean=mean, scale=scale, dof=dof)
    return case


def _permuted(W, perms):
    return np.stack([W[np.ix_(p, p)] for p in perms])


def rounded(case, dtype):
    'The case with every array rounded to `dtype` (held in float64).'
    out = dict(case)
    for name in ('mats', 'base', 'mean', 'scale', 'dof'):
        if case[name] is not None:
            out[name] = case[name].astype(NP_DTYPE[dtype]).astype(np.float64)
    return out


def nw_std(case):
    'The oracle\'s arguments: mean [K, D], scale [K, 1], W [K, D, D], dof [K, 1] in float64.'
    return (case['mean'], case['scale'][:, None], case['mats'][case['idx']],
            case['dof'][:, None])


def nw_solve(case):
    '(W^-1 [M, D, D], log|W| [M]) of the distinct matrices of a case.'
    if case['L'] is not None:
        return spd_solve(L=case['L'])
    Winv, logdet = spd_solve(W=case['base'][None])
    return _permuted(Winv[0], case['perms']), np.repeat(logdet, len(case['perms']))


def _nw_psi_args(dof, D):
    return (ld(dof)[:, None] + 1 - np.arange(1, D + 1, dtype=LD)) / 2


def nw_expected_stats(mean, scale, W, dof, logdet):
    'mean [K, D], scale [K], W [K, D, D], dof [K], log|W| [K] -> E[T] [K, D^2 + D + 2].'
    mean, scale, W, dof = ld(mean), ld(scale), ld(W), ld(dof)
    K, D = mean.shape
    Wm = np.einsum('kij,kj->ki', W, mean)
    return np.concatenate([
        dof[:, None] * Wm, (dof[:, None, None] * W).reshape(K, D * D),
        (D / scale + dof * (Wm * mean).sum(-1))[:, None],
        (digamma(_nw_psi_args(dof, D)).sum(-1) + D * LOG2 + ld(logdet))[:, None]], axis=-1)


def nw_log_norm(scale, dof, logdet, D):
    scale, dof = ld(scale), ld(dof)
    return (dof * ld(logdet) / 2 + dof * D * LOG2 / 2 + LD(D) * (D - 1) * LOGPI / 4
            + lgamma(_nw_psi_args(dof, D)).sum(-1) - D * np.log(scale) / 2 + D * LOG2PI / 2)


def nw_natural(mean, scale, Winv, dof):
    'Winv [K, D, D] = W^-1 -> eta [K, D^2 + D + 2].'
    mean, scale, dof = ld(mean), ld(scale), ld(dof)
    K, D = mean.shape
    quad = scale[:, None, None] * mean[:, :, None] * mean[:, None, :]
    return np.concatenate([scale[:, None] * mean, (-(ld(Winv) + quad) / 2).reshape(K, D * D),
                           -scale[:, None] / 2, (dof[:, None] - D) / 2], axis=-1)


def nw_truth(case):
    'E[T], log_norm and natural parameters of a case (one factorisation per distinct matrix).'
    Winv, logdet = nw_solve(case)
    idx, D = case['idx'], case['mean'].shape[1]
    return {'exp': nw_expected_stats(case['mean'], case['scale'], case['mats'][idx],
                                     case['dof'], logdet[idx]),
            'lnorm': nw_log_norm(case['scale'], case['dof'], logdet[idx], D),
            'nat': nw_natural(case['mean'], case['scale'], Winv[idx], case['dof'])}


def nw_inverse_parts(eta, D):
    '(mean [K, D], kappa [K], B [K, D, D] = -2 eta_2 - kappa m m^T, nu [K]) of eta [K, Q].'
    eta = ld(eta)
    K = len(eta)
    kappa = -2 * eta[:, -2]
    mean = eta[:, :D] / kappa[:, None]
    B = -2 * eta[:, D:D + D * D].reshape(K, D, D) \
        - kappa[:, None, None] * mean[:, :, None] * mean[:, None, :]
    return mean, kappa, B, 2 * eta[:, -1] + D


def nw_from_natural(eta, D, shared=None):
    '''(mean, kappa, W, nu, log|W|) of eta [K, Q]: every B factorised on its own, or -- where
    B is exactly one of the distinct matrices -- `shared` = (solve of them, idx).'''
    mean, kappa, B, nu = nw_inverse_parts(eta, D)
    if shared is None:
        W, logdet = spd_solve(W=.5 * (B + B.transpose(0, 2, 1)))
    else:
        (Winv, ld_), idx = shared
        W, logdet = Winv[idx], ld_[idx]
    return mean, kappa, W, nu, -logdet


def inverse_case_eta(case):
    '''Natural parameters whose INVERSE scale matrices are the case's matrices (a `dyadic`
    case: exactly representable, so that B above is the matrix itself).'''
    K, D = case['mean'].shape
    return np.asarray(nw_natural(case['mean'], case['scale'], case['mats'][case['idx']],
                                 case['dof']), dtype=np.float64)


# ---- Normal-Gamma, isotropic Normal-Gamma -----------------------------------------------------

def ng_case(seed, K, D, iso):
    rng = np.random.default_rng(seed)
    scale = _log_uniform(rng, 1e-3, 1e7, K)[:, None]
    # (as in nw_case: kappa m^2 stays of order one, or the rates that from_natural recovers as
    # -eta_2 - kappa m^2 / 2 are the difference of two numbers 1e3 x their size)
    return {'mean': rng.standard_normal((K, D)) * np.exp(rng.uniform(-2, 2, (K, 1)))
            / np.sqrt(np.maximum(scale, 1.)),
            'scale': scale,
            'shape': _log_uniform(rng, 1e-3, 1e7, K)[::-1].copy()[:, None],
            'rates': np.exp(rng.uniform(np.log(1e-3), np.log(1e7), (K, 1 if iso else D)))}


def ng_std(case, dtype='float64'):
    return tuple(case[n].astype(NP_DTYPE[dtype]).astype(np.float64)
                 for n in ('mean', 'scale', 'shape', 'rates'))


def ng_expected_stats(mean, scale, shape, rates, iso):
    mean, scale, shape, rates = ld(mean), ld(scale), ld(shape), ld(rates)
    D = mean.shape[-1]
    prec = shape / rates
    if iso:
        pqm = prec * (mean ** 2).sum(-1, keepdims=True) + D / scale
        logdet = digamma(shape) - np.log(rates)
    else:
        pqm = (prec * mean ** 2).sum(-1, keepdims=True) + D / scale
        logdet = D * digamma(shape) - np.log(rates).sum(-1, keepdims=True)
    return np.concatenate([prec * mean, prec, pqm, logdet], axis=-1)


def ng_log_norm(mean, scale, shape, rates, iso):
    scale, shape, rates = ld(scale), ld(shape), ld(rates)
    D = np.shape(mean)[-1]
    n = 1 if iso else D
    return (n * lgamma(shape) - shape * np.log(rates).sum(-1, keepdims=True)
            - D * np.log(scale) / 2).sum(-1)


def ng_natural(mean, scale, shape, rates, iso):
    mean, scale, shape, rates = ld(mean), ld(scale), ld(shape), ld(rates)
    D = mean.shape[-1]
    if iso:
        return np.concatenate([scale * mean, -scale * (mean ** 2).sum(-1, keepdims=True) / 2 - rates,
                               -scale / 2, shape - 1 + LD(D) / 2], axis=-1)
    return np.concatenate([scale * mean, -scale * mean ** 2 / 2 - rates, -scale / 2,
                           shape - LD(.5)], axis=-1)


def ng_from_natural(eta, iso):
    eta = ld(eta)
    D = eta.shape[-1] - 3 if iso else (eta.shape[-1] - 2) // 2
    scale = -2 * eta[:, -2:-1]
    mean = eta[:, :D] / scale
    if iso:
        return (mean, scale, eta[:, -1:] + 1 - LD(D) / 2,
                -eta[:, D:D + 1] - scale * (mean ** 2).sum(-1, keepdims=True) / 2)
    return mean, scale, eta[:, -1:] + LD(.5), -eta[:, D:2 * D] - scale * mean ** 2 / 2


# ---- Dirichlet, Gamma -------------------------------------------------------------------------

def dir_case(seed, S, G, mixed=True):
    '''Concentrations [S, G]: log-uniform in [1e-3, 1e7] within every row (`mixed`: what a
    trained model holds), else uniform in [.3, 4.3].'''
    rng = np.random.default_rng(seed)
    if not mixed:
        return rng.uniform(.3, 4.3, (S, G))
    c = np.exp(rng.uniform(np.log(1e-3), np.log(1e7), (S, G)))
    c[:, 0] = 1e-3
    c[:, -1] = 1e7 if G > 1 else 1e-3
    if S > 1:
        c[1, -1] = 1e-3                  # a row whose reference category is the small one
    return c


def dir_expected_stats(conc):
    c = ld(conc)
    psi_last = digamma(c[..., -1:])
    return np.concatenate([digamma(c[..., :-1]) - psi_last, psi_last - digamma(c.sum(-1, keepdims=True))],
                          axis=-1)


def dir_log_weights(conc):
    'E[ln pi_g] = psi(c_g) - psi(sum c).'
    c = ld(conc)
    return digamma(c) - digamma(c.sum(-1, keepdims=True))


def dir_log_norm(conc):
    c = ld(conc)
    return lgamma(c).sum(-1) - lgamma(c.sum(-1))


def dir_natural(conc):
    c = ld(conc)
    return np.concatenate([c[..., :-1] - 1, (c - 1).sum(-1, keepdims=True)], axis=-1)


def dir_from_natural(eta):
    e = ld(eta)
    return np.concatenate([e[..., :-1] + 1, e[..., -1:] - e[..., :-1].sum(-1, keepdims=True) + 1],
                          axis=-1)


def gamma_case(seed, n):
    rng = np.random.default_rng(seed)
    return _log_uniform(rng, 1e-3, 1e7, n), _log_uniform(rng, 1e-3, 1e7, n)[::-1].copy()


def gamma_expected_stats(shape, rate):
    a, b = ld(shape), ld(rate)
    return np.concatenate([a / b, digamma(a) - np.log(b)])


def gamma_log_norm(shape, rate):
    a, b = ld(shape), ld(rate)
    return (lgamma(a) - a * np.log(b)).sum()


def gamma_natural(shape, rate):
    return np.concatenate([-ld(rate), ld(shape) - 1])


def gamma_from_natural(eta):
    e = ld(eta)
    n = len(e) // 2
    return e[n:] + 1, -e[:n]


# psi on its own: near 0, at 1, near its root, across the kernel's recurrence / series switch
# at 10, and large
DIGAMMA_ARGS = (1e-6, 1e-3, .5, 1., 1.4616, 9.999, 10., 10.001, 1e3, 1e7)
PSI_10 = 2.2517525890667211


def digamma_bound(x, truth, eps=EPS64):
    '''Absolute bound on psi(x) of ANY fp64 implementation by upward recurrence: at most 10
    steps psi(x) = psi(x + 1) - 1 / x whose terms and partial sums are below max(1 / x,
    |psi(x)|, psi(10)), a logarithm, the series and the output rounding -- 16 roundings of at
    most one ulp of that magnitude.  (Near the root at 1.4616 this is the absolute bound: the
    result itself is about 0.)'''
    x = np.asarray(x, dtype=np.float64)
    mag = np.maximum(np.maximum(1 / x, np.abs(np.asarray(truth, dtype=np.float64))), PSI_10)
    return 16 * eps * mag


# ---- KL, natural-gradient step, sufficient statistics ----------------------------------------

def kl_case(seed, K, Q):
    '''E[T] in [.5, 1.5], eta_q in [-1, 0], eta_p in [0, 1]: every term of the sum is positive,
    so that the bound (relative to the result) is one on the sum's terms.'''
    rng = np.random.default_rng(seed)
    return {'es': rng.uniform(.5, 1.5, (K, Q)), 'eq': rng.uniform(-1, 0, (K, Q)),
            'ep': rng.uniform(0, 1, (K, Q)), 'lq': 10 * rng.standard_normal(K),
            'lp': 10 * rng.standard_normal(K)}


def kl_div(es, eq, ep, lq, lp):
    return ld(lp) - ld(lq) - (ld(es) * (ld(ep) - ld(eq))).sum(-1)


def natural_grad_step(ep, eq, st, lrate):
    return ld(eq) + LD(lrate) * (ld(ep) + ld(st) - ld(eq))


def suffstats(X, cov_type):
    'The oracle\'s statistics in the dtype of X (numpy, one product and a scaling per entry).'
    return orc.SUFFSTATS[cov_type](X)


# ---- errors and bounds ------------------------------------------------------------------------

def nw_blocks(D):
    Q = D * D + D + 2
    return (('vector', slice(0, D)), ('matrix', slice(D, Q - 2)), ('scalar 1', slice(Q - 2, Q - 1)),
            ('scalar 2', slice(Q - 1, Q)))


def ng_blocks(D, iso):
    Q = D + 3 if iso else 2 * D + 2
    return (('vector', slice(0, D)), ('second', slice(D, Q - 2)), ('scalar 1', slice(Q - 2, Q - 1)),
            ('scalar 2', slice(Q - 1, Q)))


WHOLE = (('all', slice(None)),)


def block_err(got, truth):
    'max |got - truth| / max |truth| over one block (longdouble arithmetic).'
    got, truth = ld(got), ld(truth)
    if truth.size == 0:
        return 0.
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - truth).max() / max(np.abs(truth).max(), LD(1e-300)))


def floor64(n):
    'Output rounding plus an n-term sum.'
    return 4 * n * EPS64


def bound64(oracle_err, n, exact_inverse=False):
    '''The float64 bound of a block: max(floor, 16 x the oracle's error at the same inputs); for
    a block that holds the inverse of an exact-family matrix (where LAPACK's inverse breaks down
    and unpivoted elimination is nearly exact) the floor alone, x 8 for the inverse's bit
    growth.'''
    if exact_inverse:
        return 8 * floor64(n)
    if not np.isfinite(oracle_err):
        oracle_err = 0.
    return max(floor64(n), 16 * oracle_err)


def check(got, truth, oracle, n, dtype, group, what, blocks=WHOLE, exact_inverse=(),
          floor_only=()):
    '''Hold `got` [.., Q] to `truth` block by block; `oracle` is the oracle's float64 result at
    the same inputs (None, or a block named in `floor_only`: the floor alone).  float64: block
    error <= bound64; float32: every element within 2^-24 |truth| + bound64 x the block's
    largest |truth|.'''
    got, truth = np.atleast_1d(got), np.atleast_1d(ld(truth))
    assert got.shape == truth.shape, f'{group} {what}: shape {got.shape} != {truth.shape}'
    failures = []
    for name, sl in blocks:
        t, g = truth[..., sl], got[..., sl]
        if t.size == 0:
            continue
        o_err = 0. if oracle is None or name in floor_only else \
            block_err(np.atleast_1d(oracle)[..., sl], t)
        bound = bound64(o_err, n, name in exact_inverse)
        k_err = block_err(g, t) if dtype == 'float64' else None
        if dtype == 'float64':
            ok = k_err <= bound
        else:
            # (what float32 cannot hold is stored as an infinity of its sign: the inverse of
            # a matrix whose determinant is 2^-1280; the rest of the block is held as usual)
            over = np.abs(t) > F32_MAX
            ok = bool((ld(g)[over] == np.sign(t[over]) * np.inf).all())
            g, t = ld(g)[~over], t[~over]
            k_err = block_err(g, t) if t.size else 0.
            if t.size:
                allowed = EPS32 * np.abs(t) + bound * np.abs(t).max()
                ok = ok and bool(np.isfinite(g).all() and (np.abs(g - t) <= allowed).all())
        print(f'EXPFAM | {group} | {what} [{name}] | {dtype} | oracle {o_err:.2e} | '
              f'kernel {k_err:.2e} | bound {bound:.2e} | {"ok" if ok else "FAIL"}')
        if not ok:
            failures.append(f'{what} [{name}] {dtype}: kernel {k_err:.3e}, oracle {o_err:.3e}, '
                            f'bound {bound:.3e}')
    assert not failures, f'{group}: ' + '; '.join(failures)


# ---- the cases of the GPU tests ----------------------------------------------------------------

NW_DIMS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 96, 127, 128)
GENERIC_C = (.2, 1e-2, 1e-4, 1e-5)


def nw_cases():
    '''[(id, kwargs of nw_case)]: every D with K = 7 generic matrices and K = 1 or 7 exact ones
    (diagonal range growing with the case number), K = 512 / 513 on both sides of the
    thread-count switch at D >= 16, and the two determinants outside a double.'''
    cases = []
    for n, D in enumerate(NW_DIMS):
        cases.append((f'generic-K7-D{D}', dict(seed=100 + n, K=7, D=D, family='generic',
                                               c=GENERIC_C[n % 4])))
        cases.append((f'exact-K{1 if n % 2 else 7}-D{D}',
                      dict(seed=200 + n, K=1 if n % 2 else 7, D=D, family='exact',
                           span=1 + n % 3)))
    for n, (K, D, family) in enumerate([(512, 1, 'generic'), (513, 3, 'exact'),
                                        (512, 16, 'generic'), (513, 16, 'exact'),
                                        (512, 17, 'exact'), (513, 17, 'generic'),
                                        (512, 40, 'generic'), (513, 40, 'exact'),
                                        (513, 128, 'exact')]):
        cases.append((f'{family}-K{K}-D{D}', dict(seed=300 + n, K=K, D=D, family=family, c=1e-2,
                                                  span=2)))
    cases.append(('exact-det-2^-1280', dict(seed=400, K=1, D=128, family='exact', span=(-5, -5))))
    cases.append(('exact-det-2^+1280', dict(seed=401, K=1, D=128, family='exact', span=(5, 5))))
    return cases


def nw_inverse_ok(kw):
    'from_natural / nw_update of a generic case factorise every k on their own: D^3 K is capped.'
    return kw['family'] == 'exact' or kw['K'] * kw['D'] ** 3 <= 40e6


NG_SHAPES = [(K, D) for K in (1, 63, 64, 65, 1000) for D in (1, 40, 128)]
DIR_SHAPES = [(S, G) for S in (1, 3, 300) for G in (1, 2, 63, 64, 65, 128, 129, 1000)]
GAMMA_SIZES = (1, 2, 64, 65, 200)
KL_SHAPES = [(K, Q) for K in (1, 300) for Q in (1, 63, 64, 65, 16514)]
NATGRAD_SIZES = (1, 255, 256, 257, 1000003)
LRATES = (0., .3, 1.)
