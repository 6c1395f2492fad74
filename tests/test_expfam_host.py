'''tests/expfam_truth.py tied down without a GPU: its longdouble psi and ln Gamma against mpmath at
40 digits, its formulas against the committed g10 goldens and against the oracle, its exact
matrix family against rational arithmetic -- and the oracle's own float64 error against it at
the inputs of every case group of tests/test_gpu_expfam.py, the quantity the GPU bounds are
built from.'''

from fractions import Fraction

import mpmath
import numpy as np
import pytest

from helpers import load_golden, orc, std_params

import expfam_truth as et

LD = et.LD
# relative to max(|f(x)|, 1): ln Gamma is assembled from two terms of size <= 64 whatever its own
# size, each good to a longdouble ulp of that (2^-63 x 64) -- an eighth of a float64 ulp at 1
SPECIAL_TOL = 2. ** -56
pytestmark = pytest.mark.skipif(np.finfo(LD).nmant < 63,
                                reason='np.longdouble is float64 on this platform')


def _mpf(v):
    'An exact mpmath copy of a longdouble.'
    m, e = np.frexp(LD(v))
    hi = np.float64(m)
    return (mpmath.mpf(float(hi)) + mpmath.mpf(float(np.float64(m - LD(hi))))) * mpmath.mpf(2) ** int(e)


def _argument_grid():
    'Every kind of argument psi / ln Gamma get below: the psi arguments, edges, a log grid.'
    grid = list(et.DIGAMMA_ARGS) + [5e-4, 1.5, 2., 19.999, 20., 20.001, 63.5, 64., 5e6]
    grid += list(np.exp(np.linspace(np.log(1e-6), np.log(2e7), 120)))
    grid += [(D - 1 + 1e-3 + 1 - i) / 2 for D in (1, 16, 128) for i in (1, D)]
    grid += list(np.float32(grid[:40]).astype(np.float64))
    return np.array(grid, dtype=LD)


def test_special_functions_against_mpmath():
    x = _argument_grid()
    psi, lg = et.digamma(x), et.lgamma(x)
    worst = [0., 0.]
    with mpmath.workdps(40):
        for xi, p, g in zip(x, psi, lg):
            for n, (mine, ref) in enumerate(((p, mpmath.digamma(_mpf(xi))),
                                             (g, mpmath.loggamma(_mpf(xi))))):
                err = float(abs(_mpf(mine) - ref) / max(abs(ref), 1))
                worst[n] = max(worst[n], err)
                assert err <= SPECIAL_TOL, f'{("psi", "lgamma")[n]}({float(xi)!r}): {err:.2e}'
    print(f'psi worst {worst[0]:.2e}, ln Gamma worst {worst[1]:.2e} (tolerance {SPECIAL_TOL:.2e})')


def test_constants():
    with mpmath.workdps(40):
        for mine, ref in ((et.PI, mpmath.pi), (et.LOG2, mpmath.log(2)), (et.LOGPI, mpmath.log(mpmath.pi)),
                          (et.LOG2PI, mpmath.log(2 * mpmath.pi))):
            assert abs(_mpf(mine) - ref) / ref < 2. ** -62
    assert abs(float(et.digamma(LD(10.))) - et.PSI_10) < 1e-15


# ---- the g10 goldens ---------------------------------------------------------------------------------

def _close(a, b, tol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f'{what}: {a.shape} != {b.shape}'
    err = np.abs(a - b).max() / np.abs(b).max()
    assert err <= tol, f'{what}: {err:.2e}'


def _nw_all(q):
    mean, scale, W, dof = q
    scale, dof = scale.reshape(-1), dof.reshape(-1)
    Winv, logdet = et.spd_solve(W=W)
    return (et.nw_natural(mean, scale, Winv, dof), et.nw_expected_stats(mean, scale, W, dof, logdet),
            et.nw_log_norm(scale, dof, logdet, mean.shape[1]))


@pytest.mark.parametrize('name', ['nw', 'ng', 'ing', 'dir', 'dirset'])
def test_truth_against_g10_goldens(name):
    g = load_golden('g10_dists')
    q, p = std_params(g, f'{name}.q'), std_params(g, f'{name}.p')
    if name == 'nw':
        (nat, exp, ln), (nat_p, _, ln_p) = _nw_all(q), _nw_all(p)
        back = et.nw_from_natural(np.asarray(nat, dtype=np.float64), q[0].shape[1])[:4]
    elif name in ('ng', 'ing'):
        iso = name == 'ing'
        nat, exp, ln = (f(*q, iso) for f in (et.ng_natural, et.ng_expected_stats, et.ng_log_norm))
        nat_p, ln_p = et.ng_natural(*p, iso), et.ng_log_norm(*p, iso)
        back = et.ng_from_natural(np.asarray(nat, dtype=np.float64), iso)
    else:
        nat, exp, ln = (f(*q) for f in (et.dir_natural, et.dir_expected_stats, et.dir_log_norm))
        nat_p, ln_p = et.dir_natural(*p), et.dir_log_norm(*p)
        back = (et.dir_from_natural(np.asarray(nat, dtype=np.float64)),)
    _close(nat, g[f'{name}.natural'], 1e-12, 'natural')
    _close(exp, g[f'{name}.exp_stats'], 1e-12, 'E[T]')
    _close(ln, g[f'{name}.log_norm'], 1e-12, 'log_norm')
    kl = et.kl_div(exp, nat, nat_p, ln, ln_p)
    _close(kl, g[f'{name}.kl'], 1e-12, 'kl')
    for arr, pn in zip(back, orc.FAMILIES['full']['names'] if name == 'nw' else
                       orc.FAMILIES['diagonal']['names'] if name == 'ng' else
                       orc.FAMILIES['isotropic']['names'] if name == 'ing' else ('concentrations',)):
        ref = g[f'{name}.roundtrip.{pn}']
        # (the golden round trip carries the reference's float64 inverse: 1e-12 is its size)
        _close(np.asarray(arr, dtype=np.float64).reshape(ref.shape), ref, 1e-12, 'roundtrip ' + pn)


def test_truth_against_g10_gamma_and_statistics():
    g = load_golden('g10_dists')
    (a, b), (a_p, b_p) = std_params(g, 'gamma.q'), std_params(g, 'gamma.p')
    _close(et.gamma_natural(a, b), g['gamma.natural'], 1e-12, 'natural')
    _close(et.gamma_expected_stats(a, b), g['gamma.exp_stats'], 1e-12, 'E[T]')
    _close(et.gamma_log_norm(a, b), g['gamma.log_norm'], 1e-12, 'log_norm')
    kl = et.kl_div(et.gamma_expected_stats(a, b), et.gamma_natural(a, b), et.gamma_natural(a_p, b_p),
                   et.gamma_log_norm(a, b), et.gamma_log_norm(a_p, b_p))
    _close(kl, g['gamma.kl'].reshape(()), 1e-12, 'kl')
    shape, rate = et.gamma_from_natural(g['gamma.natural'])
    _close(shape, a, 1e-12, 'shape')
    _close(rate, b, 1e-12, 'rate')
    for cov in ('full', 'diagonal', 'isotropic'):
        assert np.array_equal(et.suffstats(g['X'], cov), g[f'stats.{cov}']) or \
            np.abs(et.suffstats(g['X'], cov) - g[f'stats.{cov}']).max() <= 1e-15
    _close(et.natural_grad_step(g['nw.natural'], g['nw.natural'] * .5, g['nw.exp_stats'], .3),
           orc.natural_grad_update(g['nw.natural'], g['nw.natural'] * .5, g['nw.exp_stats'], .3),
           1e-15, 'natural gradient')


# ---- the oracle on the generic family ------------------------------------------------------------------

@pytest.mark.parametrize('D,c', [(1, .2), (5, .2), (40, 1e-2), (64, 1e-4)])
def test_truth_against_oracle_on_generic_matrices(D, c):
    case = et.nw_case(seed=D, K=7, D=D, family='generic', c=c)
    truth, std = et.nw_truth(case), et.nw_std(case)
    for key, fn in (('exp', orc.nw_expected_stats), ('nat', orc.nw_natural)):
        for name, sl in et.nw_blocks(D):
            err = et.block_err(fn(*std)[:, sl], truth[key][:, sl])
            assert err <= 1e-10, f'{key} [{name}]: {err:.2e}'
    assert et.block_err(orc.nw_log_norm(*std), truth['lnorm']) <= 1e-10
    eta = np.asarray(truth['nat'], dtype=np.float64)
    for mine, ref in zip(et.nw_from_natural(eta, D)[:4], orc.nw_from_natural(eta)):
        assert et.block_err(np.asarray(ref).reshape(mine.shape), mine) <= 1e-9
    # permuted copies: one truth, permuted
    Winv, logdet = et.nw_solve(case)
    direct, logdet_direct = et.spd_solve(W=case['mats'])
    assert et.block_err(Winv, direct) <= 1e-15 * np.linalg.cond(case['base'])
    assert np.abs(logdet - logdet_direct).max() <= 1e-15 * np.linalg.cond(case['base'])


# ---- the exact family ------------------------------------------------------------------------------------

def _exact_spans():
    spans = {(-s, s) for s in (1, 2, 3)} | {(-5, -5), (5, 5)}
    return sorted(spans)


@pytest.mark.parametrize('D', (1, 2, 3, 5))
def test_exact_family_in_rational_arithmetic(D):
    rng = np.random.default_rng(D)
    for lo, hi in _exact_spans():
        L = et.exact_factor(rng, D, lo, hi)[0]
        W = L @ L.T
        Lq = [[Fraction(v) for v in row] for row in L]
        for i in range(D):
            for j in range(D):
                exact = sum(Lq[i][k] * Lq[j][k] for k in range(D))
                assert Fraction(W[i, j]) == exact == Fraction(float(np.float32(W[i, j])))
        # closed-form log-determinant and the inverse against the rational ones
        det = Fraction(1)
        for i in range(D):
            det *= Lq[i][i] ** 2
        Winv, logdet = et.spd_solve(L=L[None])
        with mpmath.workdps(40):
            assert abs(_mpf(logdet[0]) - mpmath.log(mpmath.mpf(det.numerator) / det.denominator)) < 1e-17
        prod = np.asarray(Winv[0] @ et.ld(W), dtype=np.float64)
        assert np.abs(prod - np.eye(D)).max() <= 1e-15


@pytest.mark.parametrize('D', et.NW_DIMS)
def test_exact_family_survives_float32(D):
    rng = np.random.default_rng(D)
    for lo, hi in _exact_spans():
        L = et.exact_factor(rng, D, lo, hi, M=2)
        W = L @ L.transpose(0, 2, 1)
        assert np.array_equal(W.astype(np.float32).astype(np.float64), W)
        assert np.array_equal(W, W.transpose(0, 2, 1))
        # the product itself is exact: longdouble agrees to the last bit
        assert np.array_equal(np.asarray(np.einsum('mik,mjk->mij', et.ld(L), et.ld(L)),
                                         dtype=np.float64), W)


def test_out_of_range_determinants():
    for kw, sign in ((dict(et.nw_cases())['exact-det-2^-1280'], -1),
                     (dict(et.nw_cases())['exact-det-2^+1280'], 1)):
        case = et.nw_case(**kw)
        _, logdet = et.nw_solve(case)
        assert abs(float(logdet[0]) - sign * 1280 * np.log(2.)) < 1e-12
        assert sign * float(logdet[0]) > np.log(np.finfo(np.float64).max)


def test_dyadic_inverse_cases_are_exactly_representable():
    for cid, kw in et.nw_cases():
        if kw['family'] != 'exact' or kw['K'] > 7:
            continue
        case = et.nw_case(**kw, dyadic=True)
        eta = et.inverse_case_eta(case)[:, :-1]
        assert np.array_equal(eta.astype(np.float32).astype(np.float64), eta), cid
        mean, kappa, B, _ = et.nw_inverse_parts(eta_full := et.inverse_case_eta(case), kw['D'])
        assert np.array_equal(np.asarray(B, dtype=np.float64), case['mats'][case['idx']]), cid
        assert eta_full.shape == (kw['K'], kw['D'] ** 2 + kw['D'] + 2)


# ---- the oracle's own error at the inputs of the GPU cases ----------------------------------------------------

def _report(group, errs):
    worst = max(errs.values()) if errs else 0.
    print(f'ORACLE | {group} | ' + ' | '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert np.isfinite(worst)
    return worst


def _merge(into, key, err):
    into[key] = max(into.get(key, 0.), err)


@pytest.mark.parametrize('dtype', ('float64', 'float32'))
def test_oracle_error_normal_wishart(dtype):
    '''The oracle (float64 LAPACK) against the truth at every Normal-Wishart case.  On the
    generic family it is a float64 implementation like any other; on the exact family its
    inverse is reported, not asserted (it breaks down where unpivoted elimination does not).'''
    for family in ('generic', 'exact'):
        errs = {}
        for cid, kw in et.nw_cases():
            if kw['family'] != family or kw['K'] > 7 and kw['D'] > 40:
                continue
            case = et.rounded(et.nw_case(**kw), dtype)
            truth, std = et.nw_truth(case), et.nw_std(case)
            D = kw['D']
            for name, sl in et.nw_blocks(D):
                _merge(errs, f'E[T] {name}', et.block_err(orc.nw_expected_stats(*std)[:, sl],
                                                          truth['exp'][:, sl]))
            _merge(errs, 'log_norm', et.block_err(orc.nw_log_norm(*std), truth['lnorm']))
            with np.errstate(all='ignore'):
                inv = et.block_err(orc.nw_natural(*std)[:, D:D + D * D],
                                   truth['nat'][:, D:D + D * D])
            _merge(errs, 'natural matrix', inv if np.isfinite(inv) else 1.)
        worst = _report(f'NW {family} {dtype}', errs)
        if family == 'generic':
            assert worst <= 1e-9


@pytest.mark.parametrize('dtype', ('float64', 'float32'))
def test_oracle_error_other_families(dtype):
    rnd = lambda a: np.asarray(a).astype(et.NP_DTYPE[dtype]).astype(np.float64)     # noqa: E731
    for iso in (False, True):
        errs, fam = {}, orc.FAMILIES['isotropic' if iso else 'diagonal']
        for K, D in et.NG_SHAPES:
            std = et.ng_std(et.ng_case(1000 * K + D, K, D, iso), dtype)
            for name, sl in et.ng_blocks(D, iso):
                _merge(errs, f'E[T] {name}', et.block_err(fam['exp'](*std)[:, sl],
                                                          et.ng_expected_stats(*std, iso)[:, sl]))
                _merge(errs, f'natural {name}', et.block_err(fam['nat'](*std)[:, sl],
                                                             et.ng_natural(*std, iso)[:, sl]))
            _merge(errs, 'log_norm', et.block_err(fam['lnorm'](*std), et.ng_log_norm(*std, iso)))
        assert _report(f'{"ING" if iso else "NG"} {dtype}', errs) <= 1e-12
    errs = {}
    for S, G in et.DIR_SHAPES:
        conc = rnd(et.dir_case(1000 * S + G, S, G))
        _merge(errs, 'E[T]', et.block_err(orc.dir_expected_stats(conc), et.dir_expected_stats(conc)))
        _merge(errs, 'log_weights', et.block_err(orc.log_weights_set(conc), et.dir_log_weights(conc)))
        _merge(errs, 'log_norm', et.block_err(orc.dir_log_norm(conc), et.dir_log_norm(conc)))
        _merge(errs, 'natural', et.block_err(orc.dir_natural(conc), et.dir_natural(conc)))
    # (log_norm of a row that mixes 1e-3 and 1e7: sum ln Gamma(c) - ln Gamma(sum c) cancels nine
    # digits of terms of size 1e8 G; everything else is at float64's rounding)
    assert errs.pop('log_norm') <= 1e-7
    assert _report(f'Dirichlet {dtype}', errs) <= 1e-12
    errs = {}
    for n in et.GAMMA_SIZES:
        a, b = (rnd(v) for v in et.gamma_case(n, n))
        _merge(errs, 'E[T]', et.block_err(orc.gamma_expected_stats(a, b), et.gamma_expected_stats(a, b)))
        _merge(errs, 'log_norm', et.block_err(orc.gamma_log_norm(a, b), et.gamma_log_norm(a, b)))
    assert _report(f'Gamma {dtype}', errs) <= 1e-12
    errs = {}
    for K, Q in et.KL_SHAPES:
        case = {k: rnd(v) for k, v in et.kl_case(1000 * K + Q, K, Q).items()}
        args = [case[k] for k in ('es', 'eq', 'ep', 'lq', 'lp')]
        _merge(errs, f'Q{Q}', et.block_err(orc.kl_div(*args), et.kl_div(*args)))
    assert _report(f'KL {dtype}', errs) <= 1e-12


def test_oracle_digamma_within_the_recurrence_bound():
    'scipy\'s psi at the isolated arguments sits inside the bound the kernel is held to.'
    from scipy.special import digamma
    x = np.array(et.DIGAMMA_ARGS)
    truth = et.digamma(x)
    err = np.abs(et.ld(digamma(x)) - truth)
    print('ORACLE | digamma | ' + ' '.join(f'{float(e):.1e}' for e in err))
    assert (err <= et.digamma_bound(x, truth)).all()


def test_check_bites():
    'The checker itself: a float32-accumulated result and a missing entry are refused.'
    truth = et.ld(np.linspace(1., 2., 64))
    good = np.asarray(truth, dtype=np.float64)
    et.check(good, truth, good, 1, 'float64', 'self', 'good')
    et.check(good.astype(np.float32), truth, good, 1, 'float32', 'self', 'good')
    with pytest.raises(AssertionError):
        et.check(good.astype(np.float32).astype(np.float64), truth, good, 1, 'float64', 'self', 'f32')
    with pytest.raises(AssertionError):
        et.check((good * (1 + 3e-7)).astype(np.float32), truth, good, 1, 'float32', 'self', '3 ulp')
    bad = good.copy()
    bad[63] = 7.
    with pytest.raises(AssertionError):
        et.check(bad, truth, good, 64, 'float64', 'self', 'sentinel')
