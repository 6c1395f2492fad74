"""The hand-placed instruction stream of the staged full-covariance E-step (llhx_kernel with
BL, estep_bf16.hip): the reads of a slab of A go out a batch ahead of the arithmetic that
uses them, the arithmetic is cut into one unit per batch, and the slab table sits in LDS
with its columns ready-made.  None of that may change a bit: the same products in the same
order per accumulator as the unstaged form, which keeps hipcc's own schedule and the table
as packx_kernel wrote it.  A read that crosses a publish() the wrong way, a unit attached to
the wrong k-step or a column decoded wrongly moves a logit by O(0.1 .. 10).

Shapes: the bf16x3 path starts at 16 384 frames; + 37 gives a ragged last wave and a partial
64-frame tile.  D = 4: one k-step (the odd tail of the loop unrolled by two, the look-ahead
clamped at the table's end); 5: Dp = 8; 37: Dp = 40 with zero dimensions; 40: the benchmark;
44: Dp % 8 == 4, the straddling band slab; 72, 128: the ring does not fit beside the frame
tiles (k1_lds_fits: up to D = 52), the unstaged form runs under either setting.  K = 16 runs
the narrow kernels, 200 and 256 the 256-component ones (200: padded components).
Needs a real MI355X: `pytest -m gpu`."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import beer_amd as beer                                       # noqa: E402
from gpu_helpers import DEV                                   # noqa: E402
from test_gpu_band_layout import _check, _full_cov_gaussians  # noqa: E402

DIMS = [4, 5, 37, 40, 44, 72, 128]
FRAMES = [16384, 16384 + 37]
COMPS = [16, 200, 256]


def _model(D, K, T):
    torch.manual_seed(1000 * D + K + T)
    X = torch.randn(T, D, dtype=torch.float64, device=DEV) * 1.5 + 3.
    ns = _full_cov_gaussians(X, K, D + K)
    mix = beer.Mixture.create(ns).double().to(DEV)
    return X, ns.means_precisions.natural_form(), mix._log_weights().view(1, K)


def _packed_estep(st32, E64, lw64, K, k1_lds=None):
    from beer_amd import _hip, kernels
    assert _hip.get_f32_mode() == 'bf16x3' and _hip.f32_fast_ok(st32.data)
    assert kernels.packed_path_ok(st32, K, 'full')
    calls = []
    orig = kernels._hip.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    old = None if k1_lds is None else _hip.set_option('k1_lds', k1_lds)
    kernels._hip.call = spy
    try:
        ln, packed = kernels.mixture_estep_packed(st32, E64.float(), lw64.float(), K, 'full')
    finally:
        kernels._hip.call = orig
        if old is not None:
            _hip.set_option('k1_lds', old)
    assert 'beer_mixture_estep_packed' in calls, calls
    return ln, packed


@pytest.mark.parametrize('K', COMPS)
@pytest.mark.parametrize('T', FRAMES)
@pytest.mark.parametrize('D', DIMS)
def test_staged_stream_gives_the_bits_of_the_unstaged_form(D, T, K):
    '''`BEER_OPT_K1_LDS` = 1 against = 0: packed responsibilities and log-normalisers equal
    bit for bit.'''
    X, E64, lw64 = _model(D, K, T)
    st32 = beer.FrameStats(X.float(), 'full')
    outs = []
    for mode in (1, 0):
        ln, packed = _packed_estep(st32, E64, lw64, K, k1_lds=mode)
        outs.append((ln.clone(), packed.unpack().clone()))
    assert bool(torch.isfinite(outs[0][0]).all())
    assert torch.equal(outs[0][0], outs[1][0]), 'log-normalisers'
    assert torch.equal(outs[0][1], outs[1][1]), 'responsibilities'


@pytest.mark.parametrize('K', COMPS)
@pytest.mark.parametrize('T', FRAMES)
@pytest.mark.parametrize('D', DIMS)
def test_packed_estep_and_accumulation_against_fp64(D, T, K):
    '''The packed E-step, then the packed accumulation, against the fp64 kernels on the same
    frames (the bounds of test_gpu_band_layout.py).'''
    from beer_amd import kernels
    X, E64, lw64 = _model(D, K, T)
    st64 = beer.FrameStats(X, 'full')
    ln64, _ = kernels.mixtureset_estep(st64, E64, lw64, 1, K, 'full')
    st32 = beer.FrameStats(X.float(), 'full')
    calls = []
    orig = kernels._hip.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    ln, packed = _packed_estep(st32, E64, lw64, K)
    kernels._hip.call = spy
    try:
        acc = kernels.normal_accumulate(st32, packed, None, 1, K, 'full')
    finally:
        kernels._hip.call = orig
    assert 'beer_normal_accumulate_packed' in calls, calls
    acc64 = kernels.normal_accumulate(st64, packed.unpack().double(), None, 1, K, 'full')
    _check(ln, acc, ln64, acc64, D)
