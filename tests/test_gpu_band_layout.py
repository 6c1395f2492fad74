"""The band layout of the full-covariance statistics in the bf16x3 kernels
(estep_tiles.h: band_entry).  Every product x_a x_b of a frame appears exactly once
among the band slabs; the E-step's parameter image, the slab table, the
accumulation's statistic columns and the unpacking all use that one enumeration.  A
pair missing or counted twice in any of them is an O(1) error in a logit or in a
statistic.  Shapes: Dp = 4 ceil(D / 4) with Dp % 8 == 0 and == 4 (a straddling slab
at d = Dp / 2), D not a multiple of 4, and beyond D = 112, where the accumulation keeps
one tile of transposed frames in LDS.  Needs a real MI355X: `pytest -m gpu`."""

import math

import pytest
import torch

from helpers import assert_stats_close

pytestmark = pytest.mark.gpu

import beer_amd as beer                       # noqa: E402
from gpu_helpers import DEV, npy              # noqa: E402

DIMS = [4, 5, 12, 36, 37, 40, 44, 72, 100, 128]
T = 16447                                     # (not a multiple of 64: a partly empty last tile)


def _full_cov_gaussians(X, K, seed):
    '''K full-covariance Gaussians with dense precision matrices: every off-diagonal
    product of a frame carries a parameter of its own in the E-step.'''
    D = X.shape[1]
    ns = beer.NormalSet.create(X.mean(0).cpu(), torch.diag(X.var(0).cpu()), size=K,
                               prior_strength=1., noise_std=.7, cov_type='full')
    post = ns.means_precisions.posterior.params
    g = torch.Generator().manual_seed(seed)
    L = torch.eye(D, dtype=post.scale_matrix.dtype) + \
        torch.randn(K, D, D, generator=g, dtype=post.scale_matrix.dtype).tril(-1) * (.5 / math.sqrt(D))
    s = post.scale_matrix.diagonal(dim1=1, dim2=2).sqrt()
    W = s[:, :, None] * (L @ L.transpose(1, 2)) * s[:, None, :]
    post.scale_matrix.copy_(W.to(post.scale_matrix.device))
    return ns


def _spy(kernels):
    calls = []
    orig = kernels._hip.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    return calls, orig, spy


def _check(ln, acc, ln64, acc64, D):
    # log-normalisers: float32 logits of magnitude up to ~700 here carry a few 1e-6 of
    # relative error (the fp64 kernels' inputs are the same float32 values); a pair missing
    # or doubled in the parameter image moves a logit by ~|Lambda_ab x_a x_b|, O(0.1 .. 10)
    ln_scale = float(ln64.abs().max())
    e_ln = float((ln.double() - ln64).abs().max())
    assert e_ln <= 1e-5 * ln_scale, (e_ln, ln_scale)
    # statistics against the fp64 accumulation of the SAME float32 responsibilities: what is
    # left is the float32 accumulation (~5e-7); a missing or misplaced statistic is O(1)
    assert_stats_close(npy(acc), npy(acc64), D, 5e-6, 'statistics vs the fp64 kernels')


@pytest.mark.parametrize('K', [16, 256, 300])
@pytest.mark.parametrize('D', DIMS)
def test_band_layout_mixture(D, K):
    '''One mixture: the packed E-step -> packed accumulation (K = 16, 256), and for K = 300
    the blocks of a wide mixture (packed sets, the blocks' shares folded in by the
    accumulation) against the fp64 kernels on the same frames.'''
    from beer_amd import _hip, kernels
    torch.manual_seed(D + K)
    X = torch.randn(T, D, dtype=torch.float64, device=DEV) * 1.5 + 3.
    ns = _full_cov_gaussians(X, K, D + K)
    mix = beer.Mixture.create(ns).double().to(DEV)
    E64 = ns.means_precisions.natural_form()
    lw64 = mix._log_weights().view(1, K)
    st64 = beer.FrameStats(X, 'full')
    ln64, _ = kernels.mixtureset_estep(st64, E64, lw64, 1, K, 'full')
    st32 = beer.FrameStats(X.float(), 'full')
    assert _hip.get_f32_mode() == 'bf16x3' and _hip.f32_fast_ok(st32.data)
    calls, orig, spy = _spy(kernels)
    kernels._hip.call = spy
    try:
        if K <= 256:
            assert kernels.packed_path_ok(st32, K, 'full')
            ln, packed = kernels.mixture_estep_packed(st32, E64.float(), lw64.float(), K, 'full')
            acc = kernels.normal_accumulate(st32, packed, None, 1, K, 'full')
            r = packed.unpack()
        else:
            split = kernels.wide_mixture_split(st32, K, 'full')
            assert split is not None
            ln, wr = kernels.wide_mixture_estep(st32, E64.float(), lw64.float(), K, 'full', split)
            acc = kernels.normal_accumulate(st32, wr, None, 1, K, 'full')
            r = wr.dense()
    finally:
        kernels._hip.call = orig
    if K <= 256:
        assert 'beer_mixture_estep_packed' in calls and 'beer_normal_accumulate_packed' in calls
    else:
        assert 'beer_mixtureset_estep_packed' in calls and \
            'beer_mixtureset_accumulate_packed' in calls, calls
    acc64 = kernels.normal_accumulate(st64, r.double(), None, 1, K, 'full')
    _check(ln, acc, ln64, acc64, D)


@pytest.mark.parametrize('D', DIMS)
def test_band_layout_mixture_set_with_state_posteriors(D):
    '''A mixture set (S = 5 states of G = 16 Gaussians): packed responsibilities within
    each state, the state posteriors multiplied in by the accumulation kernel.'''
    from beer_amd import kernels
    S, G = 5, 16
    K = S * G
    torch.manual_seed(D)
    X = torch.randn(T, D, dtype=torch.float64, device=DEV) * 1.5 + 3.
    ns = _full_cov_gaussians(X, K, D)
    mset = beer.MixtureSet.create(S, ns).double().to(DEV)
    E64 = ns.means_precisions.natural_form()
    lw64 = mset._log_weights()
    sr64 = torch.rand(T, S, dtype=torch.float64, device=DEV)
    st64 = beer.FrameStats(X, 'full')
    ln64, _ = kernels.mixtureset_estep(st64, E64, lw64, S, G, 'full')
    st32 = beer.FrameStats(X.float(), 'full')
    assert kernels.packed_sets_ok(st32, S, G, 'full')
    ln, packed = kernels.mixtureset_estep_packed(st32, E64.float(), lw64.float(), S, G, 'full')
    acc = kernels.normal_accumulate(st32, packed, sr64.float(), S, G, 'full')
    acc64 = kernels.normal_accumulate(st64, packed.unpack().double(), sr64.float().double(), S, G,
                                      'full')
    _check(ln, acc, ln64, acc64, D)
