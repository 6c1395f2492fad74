"""The feature kernels of csrc/features.hip where no golden reaches: more frames in one call than
the 4096 workgroups of four waves take in one pass, more elements than the delta kernel's grid,
more than 64 filters or cepstra (lanes stride), FFT lengths 64 and 2048, float32 and mixed inputs,
mean normalisation of empty and one-frame utterances and of more than 256 columns.

Truth: oracle/features_oracle.py, at the tolerances of tests/test_features.py."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import features_oracle as fo          # noqa: E402
from test_features import _close as _project_close   # noqa: E402

pytestmark = pytest.mark.gpu

import beer_amd as beer                           # noqa: E402

WAVES_PER_PASS = 4096 * 4          # features_kernel: at most 4096 workgroups, a frame per wave
DELTA_GRID = 65536 * 256           # deltas_kernel: at most 65536 workgroups of 256 threads


def samples_for(nframes, flen=400, fstep=160, extra=0):
    'Samples of a signal of exactly `nframes` frames (`extra` < fstep more change nothing).'
    return flen + fstep * (nframes - 1) + extra if nframes else 100


def int16_signal(n, seed):
    return (2000 * np.random.RandomState(seed).randn(n)).astype(np.int16)


def _close(a, b, tol=1e-9):
    'The check of tests/test_features.py; the share of its bound that is used is printed.'
    _project_close(a, b, tol)
    if b.size:
        used = float(np.abs(a - b).max()) / (tol * max(1., float(np.abs(b).max())))
        print(f'features {a.shape}: within {used:.3g} of the bound')


def close_deltas(a, b):
    assert a.shape == b.shape
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12), float(np.abs(a - b).max())
    if b.size:
        used = float((np.abs(a - b) / (1e-12 + 1e-12 * np.abs(b))).max())
        print(f'deltas {a.shape}: within {used:.3g} of the bound')


# --- more than 16384 frames in one call --------------------------------------------------------------

LONG = (9000, 0, 7000, 1, 1100)


@functools.lru_cache(maxsize=None)
def long_signals():
    return tuple(int16_signal(samples_for(n, extra=7 * i), 10 + i) for i, n in enumerate(LONG))


@pytest.mark.parametrize('conf', ({}, {'utt_mnorm': True}), ids=('default', 'utt_mnorm'))
def test_a_batch_of_more_frames_than_one_pass_of_the_grid(conf):
    'Every wave takes a second frame, and the last pass is not full.'
    total = sum(LONG)
    assert total == 17101 and WAVES_PER_PASS < total < 2 * WAVES_PER_PASS
    sigs = long_signals()
    batch = beer.features.extract(sigs, conf)
    assert [len(f) for f in batch] == list(LONG)
    for sig, fea in zip(sigs, batch):
        single = beer.features.extract([sig], conf)[0]
        truth = fo.extract(sig, conf)
        assert fea.shape == single.shape == truth.shape and fea.shape[1] == 42
        assert np.array_equal(fea, single)           # frames are independent of each other
        if len(fea):
            assert np.isfinite(fea).all()
            _close(fea, truth)


# --- deltas ------------------------------------------------------------------------------------------

def test_deltas_of_more_elements_than_the_grid():
    T, D = 65600, 256
    assert T * D > DELTA_GRID
    rng = np.random.RandomState(0)
    fea = rng.randn(T, D)
    got = beer.features.add_deltas(fea, winlens=(1,))
    assert got.shape == (T, 2 * D) and np.array_equal(got[:, :D], fea)
    close_deltas(got, fo.add_deltas(fea, (1,)))


@pytest.mark.parametrize('T', (1, 2, 3))
def test_deltas_of_fewer_frames_than_the_window(T):
    rng = np.random.RandomState(T)
    fea = rng.randn(T, 5)
    for winlens in ((4,), (4, 4), (4, 1, 2)):
        close_deltas(beer.features.add_deltas(fea, winlens), fo.add_deltas(fea, winlens))
    sig = int16_signal(samples_for(T), 20 + T)
    conf = {'delta_winlen': 4}
    got = beer.features.extract([sig], conf)[0]
    assert got.shape == (T, 42)
    _close(got, fo.extract(sig, conf))


@pytest.mark.parametrize('order', (0, 1, 3))
def test_delta_orders(order):
    sigs = [int16_signal(n, 30 + n) for n in (3217, 400, 1600)]
    conf = {'delta_order': order}
    for sig, fea in zip(sigs, beer.features.extract(sigs, conf)):
        assert fea.shape[1] == 14 * (1 + order)
        _close(fea, fo.extract(sig, conf))
    sig = sigs[0]
    off = beer.features.extract([sig], {'apply_deltas': False})[0]
    assert np.array_equal(beer.features.extract([sig], {'delta_order': 0})[0], off)


# --- lanes striding over filters and cepstra, FFT lengths, sample rates --------------------------------

SHAPES = {
    # more than 64 filters at FFT 512
    'fft512-70-filters-20-cepstra': ({'nfilters': 70, 'n_dct_coeff': 20}, 512, 21),
    # 70 ms windows: FFT 2048, 147456 B of LDS a workgroup
    'fft2048-130-filters': ({'window_len': .07, 'nfilters': 130, 'apply_dct': False}, 2048, 131),
    'fft2048-80-filters-70-cepstra': ({'window_len': .07, 'nfilters': 80, 'n_dct_coeff': 70},
                                      2048, 71),
    # the log magnitude spectrum itself: 256 columns
    'fft512-spectrum': ({'apply_fbank': False, 'apply_dct': False, 'add_energy': False}, 512, 256),
    # 2 ms windows every millisecond: FFT 64, the smallest
    'fft64': ({'window_len': .002, 'framerate': .001, 'nfilters': 8, 'n_dct_coeff': 5}, 64, 6),
    'srate8000': ({'srate': 8000, 'cutoff_hfreq': 4000, 'nfilters': 12, 'n_dct_coeff': 6}, 256, 7),
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_filter_and_transform_shapes(name):
    conf, fft_len, base = SHAPES[name]
    srate = conf.get('srate', 16000)
    flen = int(srate * conf.get('window_len', .025))
    assert int(2 ** np.floor(np.log2(flen) + 1)) == fft_len
    sigs = [int16_signal(n, 40 + i) for i, n in enumerate((5000, flen, flen - 1, 3001))]
    batch = beer.features.extract(sigs, conf)
    assert len(batch[1]) == 1 and len(batch[2]) == 0          # a window longer than the utterance
    for sig, fea in zip(sigs, batch):
        truth = fo.extract(sig, conf)
        assert fea.shape == truth.shape and fea.shape[1] == 3 * base
        if len(fea):
            assert np.isfinite(truth).all() and np.isfinite(fea).all()
            _close(fea, truth)


# --- inputs ------------------------------------------------------------------------------------------

def test_float32_samples():
    '''The oracle removes the mean in the samples' own type, as the reference's numpy does, the
    kernels in float64; the two are the same function where that subtraction is exact.  Such a
    signal first: integer samples with an integer mean, every partial sum below 2^24.  A general
    float32 signal then: the filter bank (whose reference casts to float32 itself) against the
    oracle, the rest bit for bit against the same samples given as float64.'''
    rng = np.random.RandomState(50)
    half = rng.randint(-2000, 2001, size=2500)
    sig = (np.concatenate([half, -half]) + 3).astype(np.float32)
    assert sig.mean() == 3 and sig.dtype == np.float32
    _close(beer.features.extract([sig])[0], fo.extract(sig))
    _close(beer.features.extract([sig], {'utt_mnorm': True})[0], fo.extract(sig, {'utt_mnorm': True}))
    spec, fft_len = beer.features.short_term_mspec(sig)
    assert fft_len == 512
    _close(spec, fo.short_term_mspec(sig)[0])
    _close(beer.features.fbank(sig), fo.fbank(sig))
    general = (.3 * rng.randn(5000) + .01).astype(np.float32)
    _close(beer.features.fbank(general), fo.fbank(general))
    _close(beer.features.fbank(general, nfilters=70), fo.fbank(general, nfilters=70))
    as64 = general.astype(np.float64)
    assert np.array_equal(beer.features.fbank(general), beer.features.fbank(as64))
    assert np.array_equal(beer.features.short_term_mspec(general)[0],
                          beer.features.short_term_mspec(as64)[0])
    assert np.array_equal(beer.features.extract([general])[0], beer.features.extract([as64])[0])
    _close(beer.features.extract([as64])[0], fo.extract(as64))


def test_a_list_that_mixes_sample_types_and_a_device_tensor():
    a, b = int16_signal(3217, 60), 1000 * np.random.RandomState(61).randn(2000)
    got = beer.features.extract([a, b, a[:100]])
    assert got[2].shape == (0, 42)
    _close(got[0], fo.extract(a))
    _close(got[1], fo.extract(b))
    for sig in (a, b):
        on_device = torch.from_numpy(sig).to('cuda')
        fea = beer.features.extract([on_device])[0]
        assert np.array_equal(fea, beer.features.extract([sig])[0])
        _close(fea, fo.extract(sig))
        kept = beer.features.extract([on_device], as_numpy=False)[0]
        assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), fea)


# --- mean normalisation ------------------------------------------------------------------------------

def test_mean_normalisation_of_empty_and_one_frame_utterances_and_512_columns():
    conf = {'utt_mnorm': True, 'apply_fbank': False, 'apply_dct': False, 'add_energy': False,
            'delta_order': 1}
    sigs = [int16_signal(samples_for(n), 70 + n) for n in (0, 1, 40)]
    got = beer.features.extract(sigs, conf)
    assert [f.shape for f in got] == [(0, 512), (1, 512), (40, 512)]       # 256 threads stride
    assert not any(np.isnan(f).any() for f in got)
    assert not got[1].any()                                   # x - x / 1: exactly 0
    _close(got[2], fo.extract(sigs[2], conf))
    assert np.abs(got[2].mean(0)).max() < 1e-9
    # the default pipeline too, alone and in the batch
    sigs = [int16_signal(samples_for(n), 80 + n) for n in (1, 0, 40, 0)]
    got = beer.features.extract(sigs, {'utt_mnorm': True})
    assert not got[0].any() and not np.isnan(got[2]).any()
    _close(got[2], fo.extract(sigs[2], {'utt_mnorm': True}))
