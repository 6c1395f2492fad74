"""CPU checks of the forward log-evidence: the two C symbols, `beer_hmm_evidence_route` against a
Python restatement of the header's formula on a grid that crosses every boundary of it, the truth
of tests/evidence_truth.py itself against path enumeration and the oracle's `lognorm`, the
argument errors raised before any device work, and the command line's parser."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import evidence_truth as et
import fb_truth as ft
from helpers import ROOT, orc

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main

F32, F64 = _hip.F32, _hip.F64
HAS_GPU = torch.cuda.is_available()


def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the query may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype):
    return _hip.lib().beer_hmm_evidence_route(dtype, ctypes.byref(b) if b is not None else None)


def restated(S, A, dtype):
    return et.route_formula(S, A, {F32: 4, F64: 8}.get(dtype, 0))


def test_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('beer_hmm_log_evidence', 'beer_hmm_evidence_route'):
        assert re.search(r'^int %s\(' % name, text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _hip.SIGNATURES
    assert _hip.SIGNATURES['beer_hmm_evidence_route'] == [_hip.c_i, _hip.c_p]
    assert _hip.SIGNATURES['beer_hmm_log_evidence'] == [_hip.c_i] + [_hip.c_p] * 5   # (+ the stream)
    for name, value in (('BEER_EVIDENCE_WAVE', _hip.EVIDENCE_WAVE),
                        ('BEER_EVIDENCE_BLOCK', _hip.EVIDENCE_BLOCK),
                        ('BEER_EVIDENCE_ARCS_LDS', _hip.EVIDENCE_ARCS_LDS),
                        ('BEER_EVIDENCE_QUAD', _hip.EVIDENCE_QUAD)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % name, text).group(1), 16) == value
        assert getattr(et, name[len('BEER_EVIDENCE_'):]) == value
    assert hk.log_evidence.__name__ in hk.__all__ and hk.evidence_route.__name__ in hk.__all__
    assert 'log_evidence_batch' in beer.inference.batch.__all__ and hasattr(beer, 'log_evidence_batch')


STATES = (1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 300, 509, 600, 2600, 10232, 10233,
          20000, 32767, 32768)


def arc_counts(S, w):
    '''Arc counts on both sides of every threshold in A at this S: the bytes of a wave's slice,
    the 64 KiB of the workgroup form's arcs in LDS.'''
    spl = 1 if S <= 64 else (2 if S <= 128 else 4)
    out = {0, 1, S, 3 * S, 8 * S, 8 * S + 1, 12 * S, min(S * S, 40 * S)}
    for room in (16 * 1024 - 512 * spl, 64 * 1024 - 16 * S - 128):
        a = (room - 4 * (S + 2)) // (4 + w)
        out |= {a, a + 1}
    return sorted(a for a in out if a >= 0)


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 0)):
            for A in arc_counts(S, w or 4):
                want = restated(S, A, dtype)
                assert route(desc(S, A), dtype) == want, (S, A, dtype)
                seen.add(want)
    # both sides of every threshold of the formula were on the grid
    assert seen == {et.WAVE | 1, et.WAVE | 2, et.WAVE | 4, et.BLOCK | et.ARCS_LDS | et.QUAD,
                    et.BLOCK | et.QUAD, et.BLOCK | et.ARCS_LDS, et.BLOCK, _hip.EINVAL}


def test_route_thresholds_sit_where_the_header_says():
    W, B, A, Q = et.WAVE, et.BLOCK, et.ARCS_LDS, et.QUAD
    # states per lane of the wave form
    for S, want in ((1, W | 1), (64, W | 1), (65, W | 2), (128, W | 2), (129, W | 4),
                    (256, W | 4), (257, B | A)):
        assert route(desc(S, 3 * S), F64) == want, S
        assert _hip.evidence_family(want) in (W, B)
    assert _hip.evidence_spl(route(desc(129, 129), F32)) == 4
    # 16 KiB per wave: 512 + 4 (66 + A) + 8 A in float64 at 64 states, 1024 + 4 (130 + A) + 4 A in
    # float32 at 128, 2048 + 4 (258 + A) + 4 A in float32 at 256 states, + 8 A in float64
    assert route(desc(64, 1300), F64) == W | 1
    assert route(desc(64, 1301), F64) == B | A | Q
    assert route(desc(128, 1855), F32) == W | 2
    assert route(desc(128, 1856), F32) == B | A | Q
    assert route(desc(256, 1663), F32) == W | 4
    assert route(desc(256, 1664), F32) == B | A
    assert route(desc(256, 1108), F64) == W | 4
    assert route(desc(256, 1109), F64) == B | A
    # config 3's phone loop (120 states, 1800 arcs with the hub's): 15 912 bytes in float32
    assert route(desc(120, 1800), F32) == W | 2
    assert route(desc(120, 1800), F64) == B | A | Q
    # S = 100, every arc present: 80 KB of arcs in float32
    assert route(desc(100, 10000), F32) == B | Q
    assert route(desc(600, 7200), F32) == B
    # EINVAL exactly where the sampler refuses
    assert route(desc(10232, 10232), F64) != _hip.EINVAL                # 16 S + 128 <= 160 KiB
    assert route(desc(10233, 10233), F64) == _hip.EINVAL
    sample = _hip.lib().beer_hmm_sample_route
    for S in (1, 300, 10232, 10233, 32767, 32768, 0):
        for dtype in (F32, F64, 7):
            b = desc(S, S)
            assert (route(b, dtype) == _hip.EINVAL) == \
                (sample(dtype, ctypes.byref(b), 1) == _hip.EINVAL), (S, dtype)
    assert route(None, F64) == _hip.EINVAL
    # ... and the launch refuses the same batches before it looks at a pointer
    rc = _hip.lib().beer_hmm_log_evidence(F64, ctypes.byref(desc(10233, 10233)), None, None, None,
                                          None)
    assert rc == _hip.EINVAL
    assert _hip.lib().beer_hmm_log_evidence(7, ctypes.byref(desc(8, 8)), None, None, None,
                                            None) == _hip.EINVAL


# --- the truth itself ---------------------------------------------------------------------------
ENUMERATED = ((2, 5, 0), (3, 6, 0), (4, 6, 2), (4, 1, 0), (5, 5, 2))       # (S, T, hub members)


@pytest.mark.parametrize('S,T,hub', ENUMERATED)
def test_truth_is_the_sum_over_all_paths_and_the_oracles_lognorm(S, T, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 40 + S, hub)
    _, (llh,) = ft.inputs(g, [T], np.arange(S), S, 1., 41 + T)
    c, total = et.evidence(g, llh)
    assert c.shape == (T,) and np.isfinite(c).all()
    brute = et.brute_force(g, llh)
    assert abs(total - brute) <= 1e-12 * max(abs(brute), 1.), (total, brute)
    lognorm = orc.posteriors(llh, g['init'], g['final'], g['trans'], True)[-1]
    assert abs(total - float(lognorm)) <= 1e-12 * max(abs(total), 1.), (total, lognorm)


def test_truth_follows_the_inf_rules():
    S = 4
    g = ft.make_graph(S, (0, 1), 3)
    _, (llh,) = ft.inputs(g, [6], np.arange(S), S, 1., 4)
    # scattered -inf, still reachable: enumeration agrees
    holes = llh.copy()
    holes[1, 0] = holes[2, 3] = holes[4, 1] = -np.inf
    c, total = et.evidence(g, holes)
    assert np.isfinite(c).all() and abs(total - et.brute_force(g, holes)) <= 1e-12 * abs(total)
    # a dead frame: -inf from there on
    dead = llh.copy()
    dead[3] = -np.inf
    c, total = et.evidence(g, dead)
    assert np.isfinite(c[:3]).all() and np.isneginf(c[3:]).all() and np.isneginf(total)
    np.testing.assert_array_equal(c[:3], et.evidence(g, llh)[0][:3])
    assert np.isneginf(et.brute_force(g, dead))
    # an unreachable final alone: the frames stay finite
    g2 = dict(g, final=np.full(S, -np.inf))
    c, total = et.evidence(g2, llh)
    assert np.isfinite(c).all() and np.isneginf(total)
    np.testing.assert_array_equal(c, et.evidence(g, llh)[0])
    assert not np.isnan(c).any()


# --- errors raised on the host ----------------------------------------------------------------

def small_model():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2])
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=3, noise_std=1.)
    return beer.HMM.create(graph, ns), graph


def test_wrong_number_of_inference_graphs_is_refused_without_a_device():
    model, graph = small_model()
    X = torch.randn(7, 2)
    for utts, graphs in (([X, X], [graph]), ([X], [graph, graph]), ((torch.cat([X, X]), [7, 7]), []),
                         (iter([X, X]), [graph] * 3)):
        with pytest.raises(ValueError):
            beer.log_evidence_batch(model, utts, inference_graphs=graphs)
        with pytest.raises(ValueError):
            beer.log_evidence_batch(model, utts, inference_graphs=graphs, per_frame=True)


@pytest.mark.skipif(HAS_GPU, reason='checks behaviour on a GPU-less host')
def test_scoring_fails_loudly_without_gpu():
    model, graph = small_model()
    X = torch.randn(7, 2)
    with pytest.raises(_hip.HipUnavailable):
        model.log_evidence(X)
    with pytest.raises(_hip.HipUnavailable):
        model.log_evidence(X, inference_graph=graph, per_frame=True)
    with pytest.raises(_hip.HipUnavailable):
        beer.log_evidence_batch(model, [X, X], inference_graphs=[graph, graph])
    with pytest.raises(_hip.HipUnavailable):
        hk.HmmBatch([graph], [0], [7], torch.float64)


def test_score_is_a_command_and_its_parser_takes_the_options():
    assert hmm_cmds.score in hmm_cmds.COMMANDS
    assert [c.__name__ for c in hmm_cmds.COMMANDS].count('score') == 1
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'score', '-a', 'alis.npz', '-s', '0.5', '-u', 'utts', 'mdl',
                              'ds'])
    assert (args.alis, args.acoustic_scale, args.utts, args.model, args.dataset) == \
        ('alis.npz', .5, 'utts', 'mdl', 'ds')
    assert args.func is hmm_cmds.score.main
    args = parser.parse_args(['hmm', 'score', 'mdl', 'ds'])
    assert (args.alis, args.acoustic_scale, args.utts) == (None, 1., None)
    with pytest.raises(SystemExit):
        parser.parse_args(['hmm', 'score', 'mdl'])
