"""`kernels.mixtureset_estep` acts on the library's own answer (`kernels.estep_buffers` over
`beer_estep_route`): one library call per E-step, a responsibilities buffer exactly where the kernels
that run need one, the frame image exactly where the image entry point takes the call.  Inputs and
truth as in tests/test_gpu_estep_routes.py (tests/estep_truth.py: `orc.mixtureset_estep` in float64
on the values the kernel is handed); bounds as there: float64 1e-9 absolute, float32 1e-5 of the
largest |log-normaliser|."""

import numpy as np
import pytest
import torch

import estep_truth as et

pytestmark = pytest.mark.gpu

import beer_amd as beer                                              # noqa: E402
from beer_amd import _hip, kernels                                   # noqa: E402
from gpu_helpers import npy, tt                                      # noqa: E402


def run(monkeypatch, cov, D, S, G, T, dtype, seed):
    'log_norm, truth, responsibilities returned and the library calls made, by name.'
    inp = et.make(cov, D, S, G, T, seed, dtype)
    calls = []
    call = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, *a: (calls.append(name), call(name, *a))[1])
    ln, resps = kernels.mixtureset_estep(beer.FrameStats(tt(inp['X']), cov), tt(inp['E']), tt(inp['lw']),
                                         S, G, cov, want_resps=False)
    torch.cuda.synchronize()
    return npy(ln).astype(np.float64), et.truth(cov, inp, S, G)[0], resps, calls


def bound(dtype, truth):
    return 1e-9 if dtype == np.float64 else 1e-5 * np.abs(truth).max()


# (float32 in exact mode at 96 < D <= 128: the generic kernels -- the shape whose call used to be
#  refused once and repeated with a buffer; float64, G = 3: generic, in a buffer nobody asked for;
#  float64, one mixture of 16: the exact MFMA kernel, no buffer)
@pytest.mark.parametrize('dtype,cov,D,S,G,family', [
    (np.float32, 'diagonal', 100, 3, 4, _hip.ESTEP_GENERIC),
    (np.float64, 'full', 5, 2, 3, _hip.ESTEP_GENERIC),
    (np.float64, 'full', 13, 1, 16, _hip.ESTEP_EXACT_F64)])
def test_one_library_call_with_the_buffer_the_route_asks_for(monkeypatch, dtype, cov, D, S, G, family):
    T = 129
    code = _hip.dtype_code(torch.float32, exact=True) if dtype == np.float32 else _hip.F64
    c = _hip.COV_CODE[cov]
    nws = _hip.lib().beer_estep_workspace_bytes(code, c, D, S, G)
    args = _hip.ARG_LOG_NORM | _hip.ARG_LOG_WEIGHTS
    need, image = kernels.estep_buffers(code, c, D, S, G, args, nws)
    assert (need, image) == (family == _hip.ESTEP_GENERIC, False)
    assert _hip.estep_family(_hip.estep_route(_hip.ESTEP_PLAIN, code, c, D, S, G,
                                              args | (_hip.ARG_RESPS if need else 0), nws)) == family
    with _hip.exact_f32():
        ln, truth, resps, calls = run(monkeypatch, cov, D, S, G, T, dtype, 31)
    err = np.abs(ln - truth).max()
    print(f'{cov} D={D} {S}x{G} {dtype.__name__}: |d log_norm| {err:.3g}, bound {bound(dtype, truth):.3g}')
    assert ln.shape == (T, S) and err <= bound(dtype, truth)
    assert resps is None
    assert calls == ['beer_mixtureset_estep']


def test_log_normalisers_from_the_frame_image(monkeypatch):
    'Enough frames for the bf16x3 kernels, groups of 16, diagonal: the image entry point, once.'
    cov, D, S, G, T = 'diagonal', 13, 5, 16, _hip.FAST_MIN_FRAMES
    assert _hip.get_f32_mode() == 'bf16x3'
    ln, truth, resps, calls = run(monkeypatch, cov, D, S, G, T, np.float32, 32)
    err = np.abs(ln - truth).max()
    print(f'image: |d log_norm| {err:.3g}, bound {bound(np.float32, truth):.3g}')
    assert ln.shape == (T, S) and err <= bound(np.float32, truth)
    assert resps is None
    assert [n for n in calls if n != 'beer_frame_image'] == ['beer_mixtureset_lognorm_image']
