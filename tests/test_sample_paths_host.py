"""CPU checks of the posterior path sampler: the two C symbols, `beer_hmm_sample_route` against
a Python restatement of the header's formula, the argument errors of the Python entry points
(raised before any device work), and the truth of tests/sample_truth.py itself -- its exact
sampler's state and pair frequencies against the oracle's posteriors."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fb_truth as ft
import sample_truth as st
from helpers import ROOT

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk

F32, F64 = _hip.F32, _hip.F64


def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the query may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype, nsamples):
    return _hip.lib().beer_hmm_sample_route(dtype, ctypes.byref(b) if b is not None else None,
                                            nsamples)


def restated(S, A, dtype, nsamples):
    'The formula of include/beer_hip.h (beer_hmm_sample_route), restated in tests/sample_truth.py.'
    return st.route_formula(S, A, {F32: 4, F64: 8}.get(dtype, 0), nsamples)


def test_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('beer_hmm_sample_paths', 'beer_hmm_sample_route'):
        assert re.search(r'^int %s\(' % name, text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _hip.SIGNATURES
    assert _hip.SIGNATURES['beer_hmm_sample_route'] == [_hip.c_i, _hip.c_p, ctypes.c_int32]
    assert len(_hip.SIGNATURES['beer_hmm_sample_paths']) == 9          # (+ the stream)
    for name, value in (('BEER_SAMPLE_ARCS_LDS', _hip.SAMPLE_ARCS_LDS),
                        ('BEER_SAMPLE_QUAD', _hip.SAMPLE_QUAD)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % name, text).group(1), 16) == value


STATES = (1, 2, 64, 124, 125, 128, 129, 300, 508, 509, 600, 2600, 10231, 10232, 10233, 20000, 32767,
          32768)
ARCS_PER_STATE = (1, 3, 8, 12, 40, 100)
NSAMPLES = (0, 1, 2, 3, 4, 5, 4096, 4 * 65535, 4 * 65535 + 1)


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for deg in ARCS_PER_STATE:
            for A in {S * min(deg, S), max(S * min(deg, S) - 1, 1)}:
                for n in NSAMPLES:
                    for dtype in (F32, F64):
                        want = restated(S, A, dtype, n)
                        assert route(desc(S, A), dtype, n) == want, (S, A, dtype, n)
                        seen.add(want)
    # both sides of every threshold of the formula were on the grid
    forms = {r & 0xFFF for r in seen if r != _hip.EINVAL}
    assert forms == {32 | 0x100 | 0x200, 32 | 0x200, 8 | 0x100 | 0x200, 8 | 0x200, 8 | 0x100, 8,
                     2 | 0x100, 2}
    assert {_hip.sample_waves(r) for r in seen if r != _hip.EINVAL} == {1, 4}
    assert _hip.EINVAL in seen


def test_route_thresholds_sit_where_the_header_says():
    assert _hip.sample_chunk(route(desc(124, 124), F64, 1)) == 32       # 32 rows: 32 KiB
    assert _hip.sample_chunk(route(desc(125, 125), F64, 1)) == 8
    assert _hip.sample_chunk(route(desc(508, 508), F64, 1)) == 8
    assert _hip.sample_chunk(route(desc(509, 509), F64, 1)) == 2
    assert route(desc(128, 128), F64, 1) & _hip.SAMPLE_QUAD
    assert not route(desc(129, 129), F64, 1) & _hip.SAMPLE_QUAD
    assert route(desc(10232, 10232), F64, 1) != _hip.EINVAL             # 16 S + 128 <= 160 KiB
    assert route(desc(10233, 10233), F64, 1) == _hip.EINVAL
    # S = 100, every arc present: 80 KB of arcs in float32
    assert not route(desc(100, 10000), F32, 1) & _hip.SAMPLE_ARCS_LDS
    assert route(desc(100, 300), F32, 1) & _hip.SAMPLE_ARCS_LDS
    for bad in (route(None, F64, 1), route(desc(8, 8), F64, 0), route(desc(8, 8), 7, 1),
                route(desc(0, 8), F64, 1)):
        assert bad == _hip.EINVAL


def test_argument_errors_are_raised_without_a_device():
    'Checked on the host before any device work: these pass on a machine without a GPU.'
    u = torch.rand(7, dtype=torch.float64)
    assert hk.check_sample(False, 7) is None and hk.check_sample(None, 7) is None
    assert hk.check_sample(True, 7) is True and hk.check_sample(u, 7) is u
    with pytest.raises(ValueError):
        hk.check_sample(True, 7, viterbi=True)
    with pytest.raises(ValueError):
        hk.check_sample(u, 7, state_path=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError):
        hk.check_sample(u[:6], 7)
    with pytest.raises(ValueError):
        hk.check_sample(u.float(), 7)
    with pytest.raises(ValueError):
        hk.check_sample([0.5] * 7, 7)
    # through the models and the batched entry point
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2])
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=3, noise_std=1.)
    X = torch.randn(7, 2)
    for model in (beer.HMM.create(graph, ns),):
        stats = torch.zeros(7, 6)           # (the statistics themselves need a device: never read)
        for kwargs in (dict(sample=True, viterbi=True),
                       dict(sample=u, state_path=torch.zeros(7, dtype=torch.int64)),
                       dict(sample=u[:5]), dict(sample=u.float())):
            with pytest.raises(ValueError):
                model.expected_log_likelihood(stats, **kwargs)
            with pytest.raises(ValueError):
                beer.evidence_lower_bound(model, X, **kwargs)
        with pytest.raises(ValueError):
            beer.accumulate_elbo(model, [X], sample=u[:5])
        with pytest.raises(ValueError):
            beer.accumulate_elbo(model, [X], sample=True, viterbi=True)
        with pytest.raises(ValueError):
            beer.accumulate_elbo(model, [X], sample=u, state_paths=[torch.zeros(7)])


# --- the truth itself ---------------------------------------------------------------------------
STAT_S, STAT_T, STAT_N, STAT_BOUND, stat_case = \
    st.STAT_S, st.STAT_T, st.STAT_N, st.STAT_BOUND, st.stat_case


def test_exact_sampler_reproduces_the_posteriors():
    g, llh, U = stat_case()
    paths = st.sample(g, llh, U)
    gam, xi = st.posteriors(g, llh)
    fg, fx = st.path_frequencies(paths, STAT_S)
    dev_g, dev_x = np.abs(fg - gam).max(), np.abs(fx - xi).max()
    print(f'largest deviation: states {dev_g:.4f}, pairs {dev_x:.4f} (bound {STAT_BOUND:.4f})')
    assert dev_g <= STAT_BOUND and dev_x <= STAT_BOUND
    assert all(st.valid_path(g, p) for p in paths)
    # and the stepwise check accepts the exact sampler's paths without the widening
    steps, widened = st.check_paths(g, llh, U[:64], paths[:64], 1e-10)
    assert steps == 64 * STAT_T and widened == 0


def test_forward_values_are_the_oracles_filtering_distribution():
    'exp(trellis) sums to 1 per frame; the last row times exp(final) is gamma_{T-1} up to scale.'
    g, llh, _ = stat_case()
    la = st.forward(g, llh)
    np.testing.assert_allclose(np.exp(la).sum(1), 1., rtol=1e-12)
    gam, _ = st.posteriors(g, llh)
    w = st.last_weights(g, la[-1])
    np.testing.assert_allclose(w / w.sum(), gam[-1], rtol=1e-9, atol=1e-15)


def test_rule_edges():
    w = np.array([0., .25, 0., .5, .25, 0.])
    assert st.choose(w, np.array([0.]))[0] == 1                      # never a term of weight 0
    assert st.choose(w, np.array([.25]))[0] == 3                     # strict: the sum must EXCEED
    assert st.choose(w, np.array([1 - 2. ** -53]))[0] == 4           # the last non-zero term
    assert st.choose(w, np.array([1.]))[0] == 4                      # rounding leaves none
    assert st.choose(np.zeros(4), np.array([.3]))[0] == 0            # total 0: the first term
    assert st.choose(np.array([np.nan, 1.]), np.array([.3]))[0] == 0
    with pytest.raises(AssertionError):
        st.check_paths(dict(init=np.zeros(2), final=np.zeros(2), trans=np.zeros((2, 2))),
                       np.zeros((1, 2)), np.array([[.9]]), np.array([[0]]), 1e-5)
