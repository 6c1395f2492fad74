"""The truth of the posterior-predictive densities (tests/predictive_truth.py) held against an
independent derivation, and the host-side behaviour of the feature -- no GPU.

 * The closed forms against the conjugacy identity ln p(x | eta) = A(eta + phi(x)) - A(eta)
   - D/2 ln 2 pi, through the oracle's natural-parameter maps and sufficient statistics and
   `expfam_truth`'s log-normalisers: 1e-12.
 * D = 1: the density integrates to one.  The quadrature is the trapezoidal rule in theta,
   x = m + s tan(theta): the integrand behaves as cos^(n - 1)(theta) at the ends, n >= 2 the
   Student-t's degrees of freedom, so with 40001 nodes the rule's error is far below the 1e-9 asked.
 * The Gaussian limit: with kappa = a (= nu) = N the value differs from the Gaussian log-density at
   the posterior means by O((D + z^4) / N), z the standardised distance: below 1e-5 at N = 1e8 for
   the frames used (D <= 3, |z| <= 2, so (D + z^4 D) / N <= 6e-7), and ten times less at N = 1e9.
 * Jensen: l_pred >= l_exp entry by entry, l_exp from the oracle's `normal_llh`.
 * What raises NotImplementedError, before any device work; the command line."""

import argparse

import numpy as np
import pytest
import torch

import beer_amd as beer
from beer_amd import kernels
from beer_amd.cli import hmm as hmm_cmds
from helpers import orc

import expfam_truth as et
import predictive_truth as pt


def params(cov, K, D, seed, strength=None):
    '''Standard parameters of K pdfs (float64).  `strength` None: moderate posteriors (kappa in
    .5 .. 5, a in 2 .. 10, nu - D in 1 .. 5); else kappa = a = nu = strength with rates / scale
    matrices scaled so that the expected precision stays of order one.'''
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((K, D))
    kappa = rng.uniform(.5, 5, (K, 1)) if strength is None else np.full((K, 1), float(strength))
    if cov == 'full':
        dof = D + rng.uniform(1, 5, (K, 1)) if strength is None else np.full((K, 1), float(strength))
        cov_m = et.generic_matrices(rng, D, .5, K)                  # E[Lambda]^-1, order one
        W = np.linalg.inv(cov_m) / dof[:, :, None]
        return mean, kappa, .5 * (W + W.transpose(0, 2, 1)), dof
    a = rng.uniform(2, 10, (K, 1)) if strength is None else np.full((K, 1), float(strength))
    var = rng.uniform(.5, 2, (K, 1 if cov == 'isotropic' else D))
    return mean, kappa, a, a * var


def frames(p, T, seed, spread=1.5):
    rng = np.random.default_rng(seed)
    K, D = p[0].shape
    return p[0][rng.integers(0, K, T)] + spread * rng.standard_normal((T, D))


@pytest.mark.parametrize('D', [1, 3, 5])
@pytest.mark.parametrize('cov', pt.COV_TYPES)
def test_closed_form_is_the_conjugacy_identity(cov, D):
    K, T = 3, 4
    p = params(cov, K, D, 10 + D)
    X = frames(p, T, 20 + D)
    l, _ = pt.predictive(cov, X, p)
    worst = 0.
    for k in range(K):
        one = tuple(a[k:k + 1] for a in p)
        for t in range(T):
            ident = pt.conjugacy_identity(cov, X[t], one)
            worst = max(worst, abs(float(l[t, k] - ident)))
    print(f'{cov} D={D}: closed form vs identity {worst:.2e}')
    assert worst <= 1e-12


@pytest.mark.parametrize('cov', pt.COV_TYPES)
def test_integrates_to_one_at_dimension_one(cov):
    for seed in range(3):
        p = params(cov, 1, 1, 30 + seed)
        theta = np.linspace(-np.pi / 2, np.pi / 2, 40001, dtype=et.LD)[1:-1]
        x = et.ld(p[0][0, 0]) + 2 * np.tan(theta)
        l, _ = pt.predictive(cov, x[:, None], p)
        integrand = np.exp(l[:, 0]) * 2 / np.cos(theta) ** 2
        total = integrand.sum() * (theta[1] - theta[0])      # (the end nodes carry zero)
        print(f'{cov} seed {seed}: integral - 1 = {float(total - 1):.2e}')
        assert abs(float(total - 1)) <= 1e-9


def gaussian(cov, X, p):
    'ln N(x; m, E[Lambda]^-1) [T, K] in longdouble.'
    X, m = et.ld(X), et.ld(p[0])
    K, D = m.shape
    y = X[:, None, :] - m[None]
    if cov == 'full':
        prec = et.ld(p[3])[:, :, None] * et.ld(p[2])
        L = et.cholesky(prec)
        logdet = 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
        q = (np.einsum('tkj,kji->tki', y, L) ** 2).sum(-1)
    else:
        prec = np.broadcast_to(et.ld(p[2]) / et.ld(p[3]), (K, D))
        logdet = np.log(prec).sum(-1)
        q = (prec[None] * y * y).sum(-1)
    return (logdet[None] - D * et.LOG2PI - q) / 2


@pytest.mark.parametrize('D', [1, 3])
@pytest.mark.parametrize('cov', pt.COV_TYPES)
def test_tends_to_the_gaussian_at_the_posterior_means(cov, D):
    errs = []
    for strength in (1e8, 1e9):
        p = params(cov, 2, D, 40 + D, strength=strength)
        X = frames(p, 6, 50 + D, spread=.7)
        l, _ = pt.predictive(cov, X, p)
        errs.append(float(np.abs(l - gaussian(cov, X, p)).max()))
    print(f'{cov} D={D}: |l - ln N| = {errs[0]:.2e} (1e8), {errs[1]:.2e} (1e9)')
    assert errs[0] <= 1e-5 and errs[1] <= 1e-6 and errs[1] < errs[0]


@pytest.mark.parametrize('D', [1, 3, 7])
@pytest.mark.parametrize('cov', pt.COV_TYPES)
def test_predictive_is_never_below_the_expected_log_likelihood(cov, D):
    for strength in (None, 50.):
        p = params(cov, 4, D, 60 + D, strength=strength)
        X = frames(p, 25, 70 + D, spread=3.)
        l, _ = pt.predictive(cov, X, p)
        l_exp = orc.normal_llh(orc.SUFFSTATS[cov](X), orc.FAMILIES[cov]['exp'](*p), D)
        gap = np.asarray(l, dtype=np.float64) - l_exp
        print(f'{cov} D={D} strength {strength}: smallest l_pred - l_exp = {gap.min():.3e}')
        assert (gap >= -1e-12 * (1 + np.abs(l_exp))).all()
        assert gap.max() > 0


def test_mixture_level_uses_the_logarithm_of_the_mean_weights():
    conc = np.array([[.5, 2., 7.5], [1e-3, 1., 1e3]])
    lmw = pt.log_mean_weights(conc)
    assert np.allclose(np.asarray(np.exp(lmw).sum(-1), dtype=np.float64), 1., atol=1e-15)
    # E[ln pi] < ln E[pi] (Jensen), strictly
    assert (orc.log_weights_set(conc) < np.asarray(lmw, dtype=np.float64)).all()
    l = np.log(np.array([[.1, .2, .3, .4, .5, .6]]))
    got = pt.mixture(l, lmw, 2, 3)
    want = np.log((np.exp(l).reshape(1, 2, 3) * (conc / conc.sum(-1, keepdims=True))[None]).sum(-1))
    assert np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-15
    assert np.abs(np.asarray(pt.mixture(l, None, 6, 1), dtype=np.float64) - l).max() == 0.


def test_bounds_are_built_from_both_terms():
    l, c = np.array([[-3., 100.]]), np.array([5., 90.])
    assert np.allclose(np.asarray(pt.component_bound(l, c, 1e-5), dtype=np.float64),
                       1e-5 * np.array([[1 + 5 + 8, 1 + 90 + 10]]))
    # a component 40 nats below the state's largest does not widen the state's bound
    l, c = np.array([[0., -50.]]), np.array([1., 1e6])
    assert float(pt.state_bound(l, c, None, 1, 2, 1e-5)[0, 0]) == pytest.approx(1e-5 * 3)


# ---- what is not defined raises, before any device work -------------------------------------------

def _normalset(cov='diagonal', K=4, D=3):
    return beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=K, cov_type=cov)


def test_dense_and_differentiable_statistics_raise():
    table = torch.zeros(4, 2 * 3 + 2)
    with pytest.raises(NotImplementedError, match='dense'):
        kernels.predictive_llh(torch.zeros(5, 2 * 3 + 2), table, 'diagonal')
    with pytest.raises(NotImplementedError, match='differentiable'):
        kernels.predictive_llh(torch.zeros(5, 3, requires_grad=True), table, 'diagonal')
    with pytest.raises(NotImplementedError, match='dense'):
        kernels.mixtureset_predictive(torch.zeros(5, 8), table, None, 2, 2, 'diagonal')
    with pytest.raises(NotImplementedError, match='dense'):
        kernels.predictive_frames(torch.zeros(5, 14), 3, 'full')


def test_tied_emissions_and_vae_say_so():
    tied = beer.TiedMixtureSet.create(3, _normalset())
    with pytest.raises(NotImplementedError, match='TiedMixtureSet'):
        tied.predictive_log_likelihood(torch.zeros(2, 3))
    vae = beer.VAE(beer.Mixture.create(_normalset(D=2)), beer.nnet.ResidualFeedForwardNet(3, 1, 4),
                   beer.nnet.ResidualFeedForwardNet(2, 1, 4))
    with pytest.raises(NotImplementedError, match='VAE'):
        vae.predictive_log_likelihood(torch.zeros(2, 3))


def test_every_emission_model_has_the_method_and_the_searches_the_keyword():
    import inspect
    for cls in (beer.Normal, beer.NormalSet, beer.Mixture, beer.MixtureSet, beer.JointModelSet,
                beer.DynamicallyOrderedModelSet, beer.TiedMixtureSet, beer.VAE):
        assert callable(getattr(cls, 'predictive_log_likelihood'))
    for fn in (beer.HMM.decode, beer.HMM.log_evidence, beer.decode_batch, beer.log_evidence_batch,
               beer.PhoneLoop.decode, beer.BigramPhoneLoop.log_evidence):
        assert inspect.signature(fn).parameters['predictive'].default is False
    for family in (beer.dists.NormalGamma, beer.dists.IsotropicNormalGamma,
                   beer.dists.NormalWishart):
        assert callable(family.predictive_table)


def test_nested_log_mean_weights_multiply_down_to_the_leaves():
    'ln E[pi] of a leaf = the sum of the ln E[pi] of its ancestors: plain host arithmetic.'
    inner = beer.MixtureSet.create(4, _normalset(K=12))             # 4 mixtures of 3 leaves
    outer = beer.MixtureSet.create(2, inner)                        # 2 mixtures of 2 of those
    with torch.no_grad():
        inner.categoricalset.weights.posterior.params.concentrations.copy_(
            torch.arange(1., 13.).view(4, 3))
        outer.categoricalset.weights.posterior.params.concentrations.copy_(
            torch.tensor([[1., 3.], [5., 2.]]))
    lmw = outer.leaf_log_mean_weights()
    assert tuple(lmw.shape) == (2, 6) and lmw.dtype == torch.float64
    wi = np.arange(1., 13.).reshape(4, 3)
    wi /= wi.sum(-1, keepdims=True)
    wo = np.array([[1., 3.], [5., 2.]])
    wo /= wo.sum(-1, keepdims=True)
    want = np.log((wo[:, :, None] * wi.reshape(2, 2, 3)).reshape(2, 6))
    assert np.abs(lmw.numpy() - want).max() <= 1e-6               # (float32 concentrations)
    assert np.allclose(np.exp(lmw.numpy()).sum(-1), 1.)
    top = beer.Mixture.create(outer)
    assert np.allclose(np.exp(top._log_mean_weights().numpy()).sum(), 1.)


def test_command_line_takes_predictive():
    for cmd in (hmm_cmds.score, hmm_cmds.decode):
        parser = argparse.ArgumentParser()
        cmd.setup(parser)
        assert parser.parse_args(['--predictive', 'model', 'data']).predictive is True
        assert parser.parse_args(['model', 'data']).predictive is False
    parser = argparse.ArgumentParser()
    hmm_cmds.decode.setup(parser)
    with pytest.raises(SystemExit):
        hmm_cmds.decode.check(parser.parse_args(['--predictive', '--nbest', '2', 'm', 'd']))
    hmm_cmds.decode.check(parser.parse_args(['--predictive', 'm', 'd']))
