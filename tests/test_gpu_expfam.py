'''The distribution kernels of beer_amd/csrc/expfam.hip, entry point by entry point, against the
longdouble truth of tests/expfam_truth.py at the shapes where their indexing changes: the
thread-count switch and the LDS limit of the Normal-Wishart kernels, the wave and block edges of
the others, determinants outside a double, concentrations from 1e-3 to 1e7 in one row.

Bounds (expfam_truth.check): float64 -- the error of an output block relative to the block's
largest truth entry is at most max(4 n 2^-53, 16 x the oracle's own error at the same inputs),
n the length of the block's sums; blocks that hold the inverse of an exact-family matrix get
8 x 4 n 2^-53.  float32 storage -- every element within 2^-24 |truth| plus that float64 bound,
truth taken at the float32-rounded inputs.  DESIGN.md section 5.4 has the measured figures.'''

import numpy as np
import pytest
import torch

import beer_amd as beer
from beer_amd import _hip
from beer_amd.stats import FrameStats
from helpers import orc

import expfam_truth as et

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
DTYPES = ('float64', 'float32')
DT = {'float64': torch.float64, 'float32': torch.float32}
SENTINEL = 7.


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV, DT[dtype])


def _npy(t):
    return t.detach().cpu().numpy()


def _round(a, dtype):
    return np.asarray(a).astype(et.NP_DTYPE[dtype]).astype(np.float64)


def _new(dtype, *shape):
    return torch.full(shape, SENTINEL, dtype=DT[dtype], device=DEV)


def _call(name, dtype, ints, ins, outs):
    _hip.call(name, _hip.dtype_code(DT[dtype]), *ints, *[_hip.ptr(t) for t in ins],
              *[_hip.ptr(t) for t in outs])
    torch.cuda.synchronize()
    return [_npy(t) for t in outs]


def _ids(cases):
    return [c[0] for c in cases]


def _quiet(fn, *args):
    'The oracle at the same inputs, or None where LAPACK gives up on them.'
    try:
        with np.errstate(all='ignore'):
            return fn(*args)
    except np.linalg.LinAlgError:
        return None


# ---- Normal-Wishart ---------------------------------------------------------------------------

NW_CASES = et.nw_cases()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid,kw', NW_CASES, ids=_ids(NW_CASES))
def test_nw_expected_stats_log_norm_natural(cid, kw, dtype):
    case = et.rounded(et.nw_case(**kw), dtype)
    truth, std = et.nw_truth(case), et.nw_std(case)
    K, D = case['mean'].shape
    Q, blocks = D * D + D + 2, et.nw_blocks(D)
    exact = ('matrix',) if kw['family'] == 'exact' else ()
    ins = [_dev(a, dtype) for a in std]
    group = f'NW {kw["family"]}'

    o_exp, o_ln = _quiet(orc.nw_expected_stats, *std), _quiet(orc.nw_log_norm, *std)
    got, = _call('beer_nw_expected_stats', dtype, (K, D), ins, [_new(dtype, K, Q)])
    et.check(got, truth['exp'], o_exp, D, dtype, group, f'{cid} expected_stats', blocks)
    got, = _call('beer_nw_log_norm', dtype, (K, D), ins, [_new(dtype, K)])
    et.check(got, truth['lnorm'], o_ln, D, dtype, group, f'{cid} log_norm')
    got, ln = _call('beer_nw_expected_stats_log_norm', dtype, (K, D), ins,
                    [_new(dtype, K, Q), _new(dtype, K)])
    et.check(got, truth['exp'], o_exp, D, dtype, group, f'{cid} expected_stats_log_norm E[T]',
             blocks)
    et.check(ln, truth['lnorm'], o_ln, D, dtype, group, f'{cid} expected_stats_log_norm lnorm')
    got, = _call('beer_nw_natural', dtype, (K, D), ins, [_new(dtype, K, Q)])
    et.check(got, truth['nat'], _quiet(orc.nw_natural, *std), D, dtype, group, f'{cid} natural',
             blocks, exact_inverse=exact)


NW_INVERSE_CASES = [c for c in NW_CASES if et.nw_inverse_ok(c[1])]


def _inverse_inputs(kw, dtype):
    '''(eta [K, Q] in float64 holding `dtype` values, truth of from_natural): exact family --
    the matrices are the inverse scale matrices and eta is exactly representable; generic -- eta
    is the rounded truth of `natural` and every k is factorised on its own.'''
    D = kw['D']
    if kw['family'] == 'exact':
        case = et.nw_case(**kw, dyadic=True)
        case['dof'] = _round(case['dof'], dtype)
        eta = et.inverse_case_eta(case)
        assert (_round(eta[:, :-1], 'float32') == eta[:, :-1]).all()       # (nu - D) / 2 aside
        eta = _round(eta, dtype)
        return eta, et.nw_from_natural(eta, D, shared=(et.nw_solve(case), case['idx']))
    case = et.rounded(et.nw_case(**kw), dtype)
    eta = _round(et.nw_truth(case)['nat'], dtype)
    return eta, et.nw_from_natural(eta, D)


def _check_std(got, truth, oracle, D, dtype, group, what, exact):
    'mean, scale, W, dof of a from_natural against truth; `oracle` = orc.nw_from_natural or None.'
    K = len(truth[0])
    for n, (name, size) in enumerate((('mean', 1), ('scale', 1), ('W', D), ('dof', 1))):
        o = None if oracle is None else np.asarray(oracle[n]).reshape(K, -1)
        et.check(got[n].reshape(K, -1), truth[n].reshape(K, -1), o, size, dtype, group,
                 f'{what} {name}', exact_inverse=('all',) if exact and name == 'W' else ())


def _oracle_at_stored(stored, eta, D):
    '''(E[T], log-normaliser, blocks of E[T] left to the floor): the oracle for the parameters an
    update stored.  The truth takes log|W| of the UNROUNDED inverse, so the oracle's two entries
    that hold log|W| (the last of E[T], the log-normaliser) take it as -log|B| from the oracle's
    own float64 Cholesky factor of B = W^-1, formed from eta in float64 -- not from the stored W,
    whose rounding to float32 is another matrix's determinant, nor through LAPACK's inverse,
    which breaks down on the exact family.  The other entries are the oracle's at the stored
    parameters, or the floor where LAPACK refuses the stored W.'''
    mean, kappa, W, nu = stored
    K = len(kappa)
    kappa, nu = kappa.reshape(K, 1), nu.reshape(K, 1)
    k_u = -2 * eta[:, -2]                           # B in float64 as orc.nw_from_natural forms it
    m_u = eta[:, :D] / k_u[:, None]
    B = -2 * eta[:, D:D + D * D].reshape(K, D, D) \
        - k_u[:, None, None] * m_u[:, :, None] * m_u[:, None, :]
    logdet = -orc._chol_logdet(.5 * (B + B.transpose(0, 2, 1)))                     # [K, 1]
    unit = np.broadcast_to(np.eye(D), (K, D, D))                                    # log|I| = 0
    o_ln = orc.nw_log_norm(mean, kappa, unit, nu) + .5 * nu[:, 0] * logdet[:, 0]
    o_exp, rest = _quiet(orc.nw_expected_stats, mean, kappa, W, nu), ()
    if o_exp is None:
        o_exp, rest = np.zeros((K, D * D + D + 2)), ('vector', 'matrix', 'scalar 1')
    o_exp[:, -1] = orc.nw_expected_stats(mean, kappa, unit, nu)[:, -1] + logdet[:, 0]
    return o_exp, o_ln, rest


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cid,kw', NW_INVERSE_CASES, ids=_ids(NW_INVERSE_CASES))
def test_nw_from_natural_and_update(cid, kw, dtype):
    '''`beer_nw_from_natural`, and `beer_nw_update` with and without `moments`: its standard
    parameters against the same truth, its E[T] and log-normaliser against the truth AT the
    parameters it stored (that is what it documents) with log|W| of the unrounded inverse.'''
    K, D = kw['K'], kw['D']
    Q, exact = D * D + D + 2, kw['family'] == 'exact'
    eta, (mean, kappa, W, nu, logdet) = _inverse_inputs(kw, dtype)
    truth = (mean, kappa, W, nu)
    oracle = _quiet(orc.nw_from_natural, eta)
    group = f'NW {kw["family"]}'
    deta = _dev(eta, dtype)
    new_std = lambda: [_new(dtype, K, D), _new(dtype, K), _new(dtype, K, D, D),      # noqa: E731
                       _new(dtype, K)]

    got = _call('beer_nw_from_natural', dtype, (K, D), [deta], new_std())
    _check_std(got, truth, oracle, D, dtype, group, f'{cid} from_natural', exact)

    _, _, B, _ = et.nw_inverse_parts(eta, D)
    blocks = et.nw_blocks(D)
    for with_moments in (True, False):
        outs = new_std() + [_new(dtype, K, Q), _new(dtype, K)]
        mom = _new(dtype, K, D + D * D) if with_moments else None
        _hip.call('beer_nw_update', _hip.dtype_code(DT[dtype]), K, D, _hip.ptr(deta),
                  *[_hip.ptr(t) for t in outs], _hip.ptr(mom))
        torch.cuda.synchronize()
        got = [_npy(t).astype(np.float64) for t in outs]
        what = f'{cid} update{"+moments" if with_moments else ""}'
        _check_std(got, truth, oracle, D, dtype, group, what, exact)
        stored = (got[0], got[1].reshape(K), got[2], got[3].reshape(K))
        if not np.isfinite(got[2]).all():
            # float32 cannot hold the inverse of a determinant of 2^-1280 (checked above to be
            # the infinities it should be): E[T] of such a W is not defined
            assert dtype == 'float32' and np.abs(W).max() > et.F32_MAX
            continue
        t_exp = et.nw_expected_stats(*stored, logdet)
        t_ln = et.nw_log_norm(stored[1], stored[3], logdet, D)
        o_exp, o_ln, rest = _oracle_at_stored(stored, eta, D)
        et.check(got[4], t_exp, o_exp, D, dtype, group, f'{what} E[T]', blocks, floor_only=rest)
        et.check(got[5], t_ln, o_ln, D, dtype, group, f'{what} lnorm')
        if with_moments:
            t_mom = np.concatenate([mean, (B / et.ld(stored[3])[:, None, None]).reshape(K, -1)],
                                   axis=-1)
            _, _, B64, _ = [np.asarray(a, dtype=np.float64)
                            for a in et.nw_inverse_parts(eta, D)]
            o_mom = np.concatenate([np.asarray(mean, dtype=np.float64),
                                    (B64 / stored[3][:, None, None]).reshape(K, -1)], axis=-1)
            et.check(_npy(mom), t_mom, o_mom, 1, dtype, group, f'{what} moments',
                     (('mean', slice(0, D)), ('covariance', slice(D, None))))


# ---- Normal-Gamma, isotropic Normal-Gamma -------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('iso', (False, True), ids=('ng', 'ing'))
@pytest.mark.parametrize('K,D', et.NG_SHAPES)
def test_ng_maps(K, D, iso, dtype):
    prefix, fam = ('ing', orc.FAMILIES['isotropic']) if iso else ('ng', orc.FAMILIES['diagonal'])
    std = et.ng_std(et.ng_case(1000 * K + D, K, D, iso), dtype)
    Q, blocks, group = (D + 3 if iso else 2 * D + 2), et.ng_blocks(D, iso), prefix.upper()
    cid = f'K{K}-D{D}'
    ins = [_dev(a, dtype) for a in std]

    got, = _call(f'beer_{prefix}_expected_stats', dtype, (K, D), ins, [_new(dtype, K, Q)])
    et.check(got, et.ng_expected_stats(*std, iso), fam['exp'](*std), D, dtype, group,
             f'{cid} expected_stats', blocks)
    got, = _call(f'beer_{prefix}_log_norm', dtype, (K, D), ins, [_new(dtype, K)])
    et.check(got, et.ng_log_norm(*std, iso), fam['lnorm'](*std), D, dtype, group,
             f'{cid} log_norm')
    nat = et.ng_natural(*std, iso)
    got, = _call(f'beer_{prefix}_natural', dtype, (K, D), ins, [_new(dtype, K, Q)])
    et.check(got, nat, fam['nat'](*std), D, dtype, group, f'{cid} natural', blocks)

    eta = _round(nat, dtype)
    outs = [_new(dtype, *np.shape(a)) for a in std]
    got = _call(f'beer_{prefix}_from_natural', dtype, (K, D), [_dev(eta, dtype)], outs)
    for g, t, o, name in zip(got, et.ng_from_natural(eta, iso), fam['from_nat'](eta),
                             fam['names']):
        et.check(g, t, np.asarray(o).reshape(t.shape), D, dtype, group,
                 f'{cid} from_natural {name}')


# ---- Dirichlet ----------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('S,G', et.DIR_SHAPES)
def test_dirichlet_maps(S, G, dtype):
    conc = _round(et.dir_case(1000 * S + G, S, G), dtype)
    cid, c = f'S{S}-G{G}', _dev(conc, dtype)
    run = lambda name, *shape: _call(name, dtype, (S, G), [c], [_new(dtype, *shape)])[0]  # noqa: E731

    et.check(run('beer_dirichlet_expected_stats', S, G), et.dir_expected_stats(conc),
             orc.dir_expected_stats(conc), G, dtype, 'Dirichlet', f'{cid} expected_stats')
    et.check(run('beer_dirichlet_log_weights', S, G), et.dir_log_weights(conc),
             orc.log_weights_set(conc), G, dtype, 'Dirichlet', f'{cid} log_weights')
    lw64 = beer.dists.Dirichlet.from_std_parameters(c).log_weights64()   # float64 from any storage
    assert lw64.dtype == torch.float64
    et.check(_npy(lw64), et.dir_log_weights(conc), orc.log_weights_set(conc), G, 'float64',
             'Dirichlet', f'{cid} log_weights64 ({dtype})')
    et.check(run('beer_dirichlet_log_norm', S), et.dir_log_norm(conc), orc.dir_log_norm(conc), G,
             dtype, 'Dirichlet', f'{cid} log_norm')
    nat = et.dir_natural(conc)
    et.check(run('beer_dirichlet_natural', S, G), nat, orc.dir_natural(conc), G, dtype,
             'Dirichlet', f'{cid} natural')
    eta = _round(nat, dtype)
    got, = _call('beer_dirichlet_from_natural', dtype, (S, G), [_dev(eta, dtype)],
                 [_new(dtype, S, G)])
    et.check(got, et.dir_from_natural(eta), orc.dir_from_natural(eta), G, dtype, 'Dirichlet',
             f'{cid} from_natural')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(1,), (65,), (1000,), (3, 129), (300, 64)], ids=str)
def test_dirichlet_class_vector_and_set(shape, dtype):
    'Single-vector and set forms through `beer.dists.Dirichlet`, `log_weights64` included.'
    G = shape[-1]
    conc = _round(et.dir_case(7, int(np.prod(shape[:-1])), G).reshape(shape), dtype)
    d = beer.dists.Dirichlet.from_std_parameters(_dev(conc, dtype))
    name = f'class {shape}'
    et.check(_npy(d.expected_sufficient_statistics()), et.dir_expected_stats(conc),
             orc.dir_expected_stats(conc), G, dtype, 'Dirichlet', f'{name} expected_stats')
    et.check(_npy(d.natural_parameters()), et.dir_natural(conc), orc.dir_natural(conc), G, dtype,
             'Dirichlet', f'{name} natural')
    et.check(_npy(d.log_norm()), et.dir_log_norm(conc), orc.dir_log_norm(conc), G, dtype,
             'Dirichlet', f'{name} log_norm')
    o_lw = orc.log_weights_set(np.atleast_2d(conc)).reshape(shape)
    et.check(_npy(d.log_weights()), et.dir_log_weights(conc), o_lw, G, dtype, 'Dirichlet',
             f'{name} log_weights')
    lw64 = d.log_weights64()
    assert lw64.dtype == torch.float64
    et.check(_npy(lw64), et.dir_log_weights(conc), o_lw, G, 'float64', 'Dirichlet',
             f'{name} log_weights64 ({dtype})')
    back = d.params.from_natural_parameters(d.natural_parameters()).concentrations
    eta = _npy(d.natural_parameters()).astype(np.float64)
    et.check(_npy(back), et.dir_from_natural(eta), orc.dir_from_natural(eta), G, dtype,
             'Dirichlet', f'{name} from_natural')


# ---- Gamma, psi on its own ------------------------------------------------------------------------

GAMMA_BLOCKS = (('mean', slice(0, 1)), ('log', slice(1, 2)))       # of E[T] as [n, 2]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', et.GAMMA_SIZES)
def test_gamma_maps(n, dtype):
    a, b = (_round(v, dtype) for v in et.gamma_case(n, n))
    ins = [_dev(a, dtype), _dev(b, dtype)]
    got, = _call('beer_gamma_expected_stats', dtype, (n,), ins, [_new(dtype, 2 * n)])
    et.check(got.reshape(2, n).T, et.gamma_expected_stats(a, b).reshape(2, n).T,
             orc.gamma_expected_stats(a, b).reshape(2, n).T, 1, dtype, 'Gamma',
             f'n{n} expected_stats', GAMMA_BLOCKS)
    got, = _call('beer_gamma_log_norm', dtype, (n,), ins, [_new(dtype, 1)])
    et.check(got, et.gamma_log_norm(a, b).reshape(1), np.reshape(orc.gamma_log_norm(a, b), 1), n,
             dtype, 'Gamma', f'n{n} log_norm')
    nat = et.gamma_natural(a, b)
    got, = _call('beer_gamma_natural', dtype, (n,), ins, [_new(dtype, 2 * n)])
    et.check(got, nat, orc.gamma_natural(a, b), 1, dtype, 'Gamma', f'n{n} natural')
    eta = _round(nat, dtype)
    got = _call('beer_gamma_from_natural', dtype, (n,), [_dev(eta, dtype)],
                [_new(dtype, n), _new(dtype, n)])
    for g, t, o, name in zip(got, et.gamma_from_natural(eta), orc.gamma_from_natural(eta),
                             ('shape', 'rate')):
        et.check(g, t, o, 1, dtype, 'Gamma', f'n{n} from_natural {name}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_digamma_alone(dtype):
    '''psi(x) through a Gamma E[T] with rate 1 (psi(x) - ln 1) and through the Dirichlet pair
    (x, 1) (psi(x) - psi(1)), every argument held to `expfam_truth.digamma_bound`.'''
    x = _round(np.array(et.DIGAMMA_ARGS), dtype)
    n = len(x)
    psi = et.digamma(x)
    b64 = et.digamma_bound(x, psi)
    eps_t = 0. if dtype == 'float64' else et.EPS32
    got, = _call('beer_gamma_expected_stats', dtype, (n,), [_dev(x, dtype), _dev(np.ones(n), dtype)],
                 [_new(dtype, 2 * n)])
    err = np.abs(et.ld(got[n:]) - psi)
    for xi, e, b, p in zip(x, err, b64, psi):
        print(f'EXPFAM | digamma | Gamma psi({xi:g}) | {dtype} | err {float(e):.2e} | '
              f'bound {float(b + eps_t * abs(p)):.2e}')
    assert (err <= b64 + eps_t * np.abs(psi)).all(), f'psi alone: {err} > {b64}'
    pair = np.stack([x, np.ones(n)], axis=1)
    got, = _call('beer_dirichlet_expected_stats', dtype, (n, 2), [_dev(pair, dtype)],
                 [_new(dtype, n, 2)])
    truth = et.dir_expected_stats(pair)
    b_one = et.digamma_bound(1., et.digamma(1.))
    b_sum = et.digamma_bound(x + 1, et.digamma(x + 1))
    err = np.abs(et.ld(got) - truth)
    assert (err[:, 0] <= b64 + b_one + eps_t * np.abs(truth[:, 0])).all(), f'pair: {err[:, 0]}'
    assert (err[:, 1] <= b_one + b_sum + eps_t * np.abs(truth[:, 1])).all(), f'last: {err[:, 1]}'


# ---- KL, natural-gradient step -----------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K,Q', et.KL_SHAPES)
def test_kl(K, Q, dtype):
    case = {k: _round(v, dtype) for k, v in et.kl_case(1000 * K + Q, K, Q).items()}
    args = [case[k] for k in ('es', 'eq', 'ep', 'lq', 'lp')]
    got, = _call('beer_kl_div', dtype, (K, Q), [_dev(a, dtype) for a in args], [_new(dtype, K)])
    et.check(got, et.kl_div(*args), orc.kl_div(*args), Q, dtype, 'KL', f'K{K}-Q{Q}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lrate', et.LRATES)
@pytest.mark.parametrize('n', et.NATGRAD_SIZES)
def test_natural_grad_step(n, lrate, dtype):
    rng = np.random.default_rng(n)
    ep, eq, st = (_round(rng.standard_normal(n) * np.exp(rng.uniform(-3, 3, n)), dtype)
                  for _ in range(3))
    out = _new(dtype, n + 1)                                  # one element beyond the end
    ins = [_dev(a, dtype) for a in (ep, eq, st)]              # held until the kernel has run
    _hip.call('beer_natural_grad_step', _hip.dtype_code(DT[dtype]), n,
              *[_hip.ptr(t) for t in ins], float(lrate), _hip.ptr(out))
    torch.cuda.synchronize()
    got = _npy(out)
    assert got[n] == SENTINEL
    et.check(got[:n], et.natural_grad_step(ep, eq, st, lrate),
             orc.natural_grad_update(ep, eq, st, lrate), 1, dtype, 'nat-grad',
             f'n{n} lrate {lrate}')
    if lrate == 0.:
        assert (got[:n] == eq.astype(et.NP_DTYPE[dtype])).all()


# ---- sufficient statistics ---------------------------------------------------------------------------

def _check_suffstats(got, X, cov, dtype, what):
    '''Full and diagonal entries, first moments and constants: one product times -1/2, bit-exact
    to numpy in the same dtype; the isotropic sum within D eps of the truth.'''
    T, D = X.shape
    ref = et.suffstats(X, cov)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if cov != 'isotropic':
        assert np.array_equal(got, ref), f'{what}: {int((got != ref).sum())} entries differ'
        return
    rest = [c for c in range(D + 3) if c != D]
    assert np.array_equal(got[:, rest], ref[:, rest]), what
    truth = -(et.ld(X) ** 2).sum(-1) / 2
    eps = et.EPS64 if dtype == 'float64' else et.EPS32
    err = np.abs(et.ld(got[:, D]) - truth)
    print(f'EXPFAM | suffstats | {what} | {dtype} | rel err '
          f'{float((err / np.maximum(np.abs(truth), 1e-300)).max()) if T else 0.:.2e} | '
          f'bound {D * eps:.2e}')
    assert (err <= D * eps * np.abs(truth)).all(), what


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T', (0, 1, 9))
@pytest.mark.parametrize('D', (1, 40))
@pytest.mark.parametrize('cov', ('full', 'diagonal', 'isotropic'))
def test_suffstats_expand(cov, D, T, dtype):
    X = np.random.default_rng(T + D).standard_normal((T, D)).astype(et.NP_DTYPE[dtype])
    Q = orc.stats_dim(cov, D)
    dX = torch.from_numpy(X).to(DEV)
    out = _new(dtype, max(T, 1), Q)
    _hip.call('beer_suffstats_expand', _hip.dtype_code(DT[dtype]), _hip.COV_CODE[cov], T, D,
              _hip.ptr(dX), _hip.ptr(out))
    torch.cuda.synchronize()
    if T == 0:
        assert (_npy(out) == SENTINEL).all()
        return
    _check_suffstats(_npy(out), X, cov, dtype, f'{cov} D{D} T{T}')
    _check_suffstats(_npy(FrameStats(dX, cov).dense()), X, cov, dtype, f'{cov} D{D} T{T} dense()')


@pytest.mark.parametrize('dtype', DTYPES)
def test_suffstats_expand_beyond_one_grid(dtype):
    'T Q = 12000 x 1642 > 65536 x 256: the grid-stride loop takes a second trip.'
    T, D = 12000, 40
    assert T * orc.stats_dim('full', D) > 65536 * 256
    X = np.random.default_rng(5).standard_normal((T, D)).astype(et.NP_DTYPE[dtype])
    got = _npy(FrameStats(torch.from_numpy(X).to(DEV), 'full').dense())
    _check_suffstats(got, X, 'full', dtype, f'full D{D} T{T}')


# ---- through the classes ----------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('single', (False, True), ids=('set', 'single'))
def test_normal_wishart_class(single, dtype):
    '`beer.dists.NormalWishart`: the maps, KL(q || p) and the one-launch M-step.'
    K, D = (1, 17) if single else (7, 40)
    q = et.rounded(et.nw_case(seed=51, K=K, D=D, family='generic', c=1e-2), dtype)
    p = et.rounded(et.nw_case(seed=52, K=K, D=D, family='generic', c=.2), dtype)
    tq, tp = et.nw_truth(q), et.nw_truth(p)

    def build(case):
        mean, scale, W, dof = et.nw_std(case)
        if single:
            mean, scale, W, dof = mean[0], scale[0], W[0], dof[0]
        return beer.dists.NormalWishart.from_std_parameters(
            *[_dev(a, dtype) for a in (mean, scale, W, dof)])
    dq, dp = build(q), build(p)
    std, blocks = et.nw_std(q), et.nw_blocks(D)
    shaped = lambda t, ref: _npy(t).reshape(np.shape(ref))                    # noqa: E731
    et.check(shaped(dq.expected_sufficient_statistics(), tq['exp']), tq['exp'],
             orc.nw_expected_stats(*std), D, dtype, 'classes', 'NW E[T]', blocks)
    et.check(shaped(dq.log_norm(), tq['lnorm']), tq['lnorm'], orc.nw_log_norm(*std), D, dtype,
             'classes', 'NW log_norm')
    et.check(shaped(dq.natural_parameters(), tq['nat']), tq['nat'], orc.nw_natural(*std), D,
             dtype, 'classes', 'NW natural', blocks)
    # KL from the kernel's own (stored) E[T], eta and log-normalisers: the sum alone
    args = [shaped(t, r).astype(np.float64) for t, r in (
        (dq.expected_sufficient_statistics(), tq['exp']), (dq.natural_parameters(), tq['nat']),
        (dp.natural_parameters(), tp['nat']), (dq.log_norm(), tq['lnorm']),
        (dp.log_norm(), tp['lnorm']))]
    et.check(shaped(beer.dists.kl_div(dq, dp), tq['lnorm']), et.kl_div(*args), orc.kl_div(*args),
             D * D + D + 2, dtype, 'classes', 'NW kl_div')
    if single:
        return
    eta = _npy(dq.natural_parameters()).astype(np.float64)
    mean, kappa, W, nu, logdet = et.nw_from_natural(eta, D)
    dq.update_from_natural_parameters(dq.natural_parameters())
    got = [_npy(getattr(dq.params, n)).astype(np.float64).reshape(np.shape(t))
           for n, t in zip(('mean', 'scale', 'scale_matrix', 'dof'), (mean, kappa, W, nu))]
    _check_std(got, (mean, kappa, W, nu), orc.nw_from_natural(eta), D, dtype, 'classes',
               'NW update_from_natural_parameters', False)
    t_exp = et.nw_expected_stats(*got, logdet)
    o_exp, _, rest = _oracle_at_stored(got, eta, D)
    et.check(_npy(dq.expected_sufficient_statistics()), t_exp, o_exp, D, dtype, 'classes',
             'NW E[T] after update', blocks, floor_only=rest)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('iso', (False, True), ids=('ng', 'ing'))
def test_normal_gamma_classes(iso, dtype):
    K, D = 65, 40
    cls = beer.dists.IsotropicNormalGamma if iso else beer.dists.NormalGamma
    fam = orc.FAMILIES['isotropic' if iso else 'diagonal']
    std = et.ng_std(et.ng_case(61, K, D, iso), dtype)
    d = cls.from_std_parameters(*[_dev(a, dtype) for a in std])
    blocks = et.ng_blocks(D, iso)
    et.check(_npy(d.expected_sufficient_statistics()), et.ng_expected_stats(*std, iso),
             fam['exp'](*std), D, dtype, 'classes', f'{cls.__name__} E[T]', blocks)
    et.check(_npy(d.log_norm()), et.ng_log_norm(*std, iso), fam['lnorm'](*std), D, dtype,
             'classes', f'{cls.__name__} log_norm')
    et.check(_npy(d.natural_parameters()), et.ng_natural(*std, iso), fam['nat'](*std), D, dtype,
             'classes', f'{cls.__name__} natural', blocks)
    eta = _npy(d.natural_parameters()).astype(np.float64)
    back = d.params.from_natural_parameters(d.natural_parameters())
    for name, t, o in zip(fam['names'], et.ng_from_natural(eta, iso), fam['from_nat'](eta)):
        et.check(_npy(getattr(back, name)).reshape(t.shape), t, np.asarray(o).reshape(t.shape), D,
                 dtype, 'classes', f'{cls.__name__} from_natural {name}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_gamma_class(dtype):
    a, b = (_round(v, dtype) for v in et.gamma_case(71, 65))
    d = beer.dists.Gamma.from_std_parameters(_dev(a, dtype), _dev(b, dtype))
    et.check(_npy(d.expected_sufficient_statistics()).reshape(2, -1).T,
             et.gamma_expected_stats(a, b).reshape(2, -1).T,
             orc.gamma_expected_stats(a, b).reshape(2, -1).T, 1, dtype, 'classes', 'Gamma E[T]',
             GAMMA_BLOCKS)
    et.check(_npy(d.log_norm()).reshape(1), et.gamma_log_norm(a, b).reshape(1),
             np.reshape(orc.gamma_log_norm(a, b), 1), 65, dtype, 'classes', 'Gamma log_norm')
    et.check(_npy(d.natural_parameters()), et.gamma_natural(a, b), orc.gamma_natural(a, b), 1,
             dtype, 'classes', 'Gamma natural')


# ---- refusals and no-ops -------------------------------------------------------------------------------

def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in tensors)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_come_before_any_launch(dtype):
    code, p = _hip.dtype_code(DT[dtype]), _hip.ptr
    D = 129                                  # D*D fp64 no longer fits a CU's LDS
    Q = D * D + D + 2
    mean, scale, W, dof = (_new(dtype, 1, D), _new(dtype, 1), _new(dtype, 1, D, D),
                           _new(dtype, 1))
    out, ln, mom = _new(dtype, 1, Q), _new(dtype, 1), _new(dtype, 1, D + D * D)
    for name in ('beer_nw_expected_stats', 'beer_nw_log_norm', 'beer_nw_natural'):
        with pytest.raises(_hip.HipInvalid):
            _hip.call(name, code, 1, D, p(mean), p(scale), p(W), p(dof), p(out))
    with pytest.raises(_hip.HipInvalid):
        _hip.call('beer_nw_expected_stats_log_norm', code, 1, D, p(mean), p(scale), p(W), p(dof),
                  p(out), p(ln))
    eta = _new(dtype, 1, Q)
    with pytest.raises(_hip.HipInvalid):
        _hip.call('beer_nw_from_natural', code, 1, D, p(eta), p(mean), p(scale), p(W), p(dof))
    with pytest.raises(_hip.HipInvalid):
        _hip.call('beer_nw_update', code, 1, D, p(eta), p(mean), p(scale), p(W), p(dof), p(out),
                  p(ln), p(mom))
    for name in ('beer_dirichlet_expected_stats', 'beer_dirichlet_natural',
                 'beer_dirichlet_from_natural', 'beer_dirichlet_log_weights',
                 'beer_dirichlet_log_norm'):
        with pytest.raises(_hip.HipInvalid):
            _hip.call(name, code, 1, 0, p(mean), p(out))
    for name in ('beer_gamma_expected_stats', 'beer_gamma_natural', 'beer_gamma_log_norm'):
        with pytest.raises(_hip.HipInvalid):
            _hip.call(name, code, 0, p(mean), p(scale), p(out))
    with pytest.raises(_hip.HipInvalid):
        _hip.call('beer_gamma_from_natural', code, 0, p(eta), p(mean), p(scale))
    assert _untouched(mean, scale, W, dof, out, ln, mom, eta)


@pytest.mark.parametrize('dtype', DTYPES)
def test_empty_sets_touch_nothing(dtype):
    code, p = _hip.dtype_code(DT[dtype]), _hip.ptr
    D = 4
    a, b, c, d, out, out2 = (_new(dtype, 64) for _ in range(6))
    for prefix in ('nw', 'ng', 'ing'):
        for which in ('expected_stats', 'log_norm', 'natural'):
            _hip.call(f'beer_{prefix}_{which}', code, 0, D, p(a), p(b), p(c), p(d), p(out))
        _hip.call(f'beer_{prefix}_from_natural', code, 0, D, p(out), p(a), p(b), p(c), p(d))
    _hip.call('beer_nw_expected_stats_log_norm', code, 0, D, p(a), p(b), p(c), p(d), p(out),
              p(out2))
    _hip.call('beer_nw_update', code, 0, D, p(out), p(a), p(b), p(c), p(d), p(out2), p(out2),
              None)
    for name in ('beer_dirichlet_expected_stats', 'beer_dirichlet_natural',
                 'beer_dirichlet_from_natural', 'beer_dirichlet_log_weights',
                 'beer_dirichlet_log_norm'):
        _hip.call(name, code, 0, D, p(a), p(out))
    _hip.call('beer_kl_div', code, 0, D, p(a), p(b), p(c), p(d), p(out2), p(out))
    _hip.call('beer_natural_grad_step', code, 0, p(a), p(b), p(c), .5, p(out))
    _hip.call('beer_suffstats_expand', code, _hip.FULL, 0, D, p(a), p(out))
    assert _untouched(a, b, c, d, out, out2)
