"""CPU checks of N-best Viterbi: the two C symbols and the header's constants, `beer_hmm_nbest_route`
against a Python restatement of the header's formula on a grid that crosses every boundary of it,
the refusals made before any device work, the truth of tests/nbest_truth.py itself against the
enumeration of all paths and against the oracle's best path, and the command line's options."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fb_truth as ft
import nbest_truth as nt
from helpers import ROOT

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main

F32, F64 = _hip.F32, _hip.F64
HAS_GPU = torch.cuda.is_available()
KS = (1, 2, 3, 5, 8, 16)


def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the query may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype, k):
    return _hip.lib().beer_hmm_nbest_route(dtype, ctypes.byref(b) if b is not None else None, k)


def restated(S, A, dtype, k):
    return nt.route_formula(S, A, {F32: 4, F64: 8}.get(dtype, 0), k)


def test_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('beer_hmm_viterbi_nbest', 'beer_hmm_nbest_route'):
        assert re.search(r'^int %s\(' % name, text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _hip.SIGNATURES
    assert _hip.SIGNATURES['beer_hmm_nbest_route'] == [_hip.c_i, _hip.c_p, ctypes.c_int32]
    assert _hip.SIGNATURES['beer_hmm_viterbi_nbest'] == \
        [_hip.c_i, _hip.c_p, _hip.c_p, ctypes.c_int32, _hip.c_p, _hip.c_p, _hip.c_p, _hip.c_i,
         _hip.c_p]                                                          # (+ the stream)
    assert int(re.search(r'#define\s+BEER_NBEST_MAX\s+(\d+)', text).group(1)) == _hip.NBEST_MAX \
        == nt.NBEST_MAX
    assert int(re.search(r'#define\s+BEER_NBEST_ARCS_LDS\s+(0x[0-9A-Fa-f]+)', text).group(1), 16) \
        == _hip.NBEST_ARCS_LDS == nt.ARCS_LDS
    assert re.search(r'#define\s+BEER_NBEST_CHUNK\(route\)\s+\(\(route\) & 0xFF\)', text)
    assert _hip.nbest_chunk(0x108) == 8
    assert re.search(r'#define\s+BEER_NBEST_LIST\(k\)', text)
    assert [_hip.nbest_list(k) for k in range(1, 17)] == [nt.list_entries(k) for k in range(1, 17)] \
        == [1, 2, 4, 4] + [8] * 4 + [16] * 8
    for name in ('viterbi_nbest', 'nbest_route'):
        assert name in hk.__all__ and callable(getattr(hk, name))
    assert 'decode_nbest_batch' in beer.inference.batch.__all__ and hasattr(beer, 'decode_nbest_batch')
    assert callable(beer.HMM.decode_nbest)
    assert beer.PhoneLoop.decode_nbest is beer.HMM.decode_nbest
    assert beer.BigramPhoneLoop.decode_nbest is beer.HMM.decode_nbest


STATES = (1, 2, 8, 9, 32, 33, 64, 65, 120, 128, 129, 256, 257, 512, 513, 600, 2600, 5000,
          10235, 10236, 32767, 32768)


def arc_counts(S, w, k):
    'Arc counts on both sides of the 64 KiB of the arcs in LDS at this S, k and item size.'
    out = {0, 1, S, 3 * S, 12 * S, min(S * S, 100 * S)}
    row = 4 * S * k
    chunk = 32 if 32 * row <= 16384 else (8 if 8 * row <= 16384 else 2)
    room = 64 * 1024 - (2 * S * k * w + 64 + chunk * row) - 4 * (S + 2)
    out |= {room // (4 + w), room // (4 + w) + 1}
    return sorted(a for a in out if a >= 0)


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 0)):
            for k in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17):
                for A in arc_counts(S, w or 4, max(k, 1)):
                    want = restated(S, A, dtype, k)
                    assert route(desc(S, A), dtype, k) == want, (S, A, dtype, k)
                    seen.add(want)
    # both sides of every threshold of the formula were on the grid
    assert seen == {32, 8, 2, 32 | nt.ARCS_LDS, 8 | nt.ARCS_LDS, 2 | nt.ARCS_LDS, _hip.EINVAL}


def test_route_thresholds_sit_where_the_header_says():
    L = nt.ARCS_LDS
    # the chunk: 32 rows of 4 S k bytes in 16 KiB up to S k = 128, 8 rows up to 512
    for S, k, want in ((128, 1, 32), (129, 1, 8), (64, 2, 32), (65, 2, 8), (8, 16, 32),
                       (9, 16, 8), (512, 1, 8), (513, 1, 2), (32, 16, 8), (33, 16, 2),
                       (120, 1, 32), (120, 4, 8), (120, 16, 2)):
        assert route(desc(S, S), F32, k) == want | L, (S, k)
        assert _hip.nbest_chunk(route(desc(S, 3 * S), F64, k)) == want
    # the arcs, config 3's phone loop (120 states, 1800 arcs): in LDS at every k, in float32
    # 2 * 120 * 16 * 4 + 64 + 2 * 7680 + 4 * 1922 + 4 * 1800 = 45 672 bytes at k = 16
    for k in (1, 4, 16):
        assert route(desc(120, 1800), F32, k) & L
    # ... and on both sides of 64 KiB: base = 8 S + 64 + 128 S at S = 100, k = 1, float32
    base = 2 * 100 * 4 + 64 + 32 * 400
    a = (65536 - base - 4 * 102) // 8
    assert route(desc(100, a), F32, 1) == 32 | L
    assert route(desc(100, a + 1), F32, 1) == 32
    assert route(desc(100, 10000), F32, 1) == 32
    assert route(desc(100, 10000), F32, 2) == 8
    assert route(desc(100, 10000), F32, 8) == 2
    assert route(desc(100, 10000), F32, 16) == 2
    # EINVAL: 2 S k w + 64 + 2 * 4 S k > 160 KiB -- S k > 10236 in float32, > 6824 in float64
    assert route(desc(10236, 10236), F32, 1) == 2
    assert route(desc(10237, 10237), F32, 1) == _hip.EINVAL
    assert route(desc(6824, 6824), F64, 1) == 2
    assert route(desc(6825, 6825), F64, 1) == _hip.EINVAL
    assert route(desc(639, 639), F32, 16) == 2
    assert route(desc(640, 640), F32, 16) == _hip.EINVAL
    assert route(desc(32768, 8), F32, 1) == _hip.EINVAL
    assert route(desc(0, 8), F32, 1) == _hip.EINVAL
    assert route(None, F64, 1) == _hip.EINVAL


def test_bad_k_dtype_and_batch_are_refused_with_no_device_work():
    'NULL pointers everywhere: the entry returns before it looks at one.'
    fn = _hip.lib().beer_hmm_viterbi_nbest
    b = desc(8, 24)
    for dtype, k in ((F32, 0), (F64, 0), (F32, 17), (F64, 17), (F32, -1), (7, 1), (7, 16)):
        assert fn(dtype, ctypes.byref(b), None, k, None, None, None, 0, None) == _hip.EINVAL
        assert route(b, dtype, k) == _hip.EINVAL
    assert fn(F32, None, None, 1, None, None, None, 0, None) == _hip.EINVAL
    assert fn(F32, ctypes.byref(desc(640, 640)), None, 16, None, None, None, 0, None) == _hip.EINVAL
    assert fn(F64, ctypes.byref(desc(32768, 8)), None, 1, None, None, None, 0, None) == _hip.EINVAL
    # the Python faces check k on the host
    for k in (0, 17, -3, 2.5, None, True):
        with pytest.raises(ValueError):
            hk.check_nbest(k, 'test')
        with pytest.raises(ValueError):
            hk.viterbi_nbest(None, None, k)
        with pytest.raises(ValueError):
            hk.nbest_route(None, k)
    model, _ = small_model()
    for k in (0, 17):
        with pytest.raises(ValueError):
            model.decode_nbest(torch.randn(7, 2), k)
        with pytest.raises(ValueError):
            beer.decode_nbest_batch(model, [torch.randn(7, 2)], k)
    assert hk.check_nbest(np.int64(16), 'test') == 16


# --- the truth itself ---------------------------------------------------------------------------
# (S, T, offsets, hub members): S <= 8 and T <= 6, and cases with fewer than k finite paths
ENUMERATED = ((1, 1, 1, 0), (1, 4, 1, 0), (2, 6, 2, 0), (3, 1, 2, 0), (3, 2, 2, 0), (3, 2, 3, 0),
              (4, 5, 3, 0), (5, 6, 2, 0), (6, 5, 3, 2), (8, 5, 3, 0), (8, 6, 2, 0), (8, 4, 8, 3))


@pytest.mark.parametrize('integer', [True, False], ids=['integer', 'real'])
@pytest.mark.parametrize('S,T,nO,hub', ENUMERATED)
def test_truth_is_the_sorted_enumeration_of_all_paths(S, T, nO, hub, integer):
    g = ft.make_graph(S, ft.offsets(nO, S), 60 + S + T, hub, integer=integer)
    if integer:
        (llh,) = ft.viterbi_inputs(S, [T], 61 + S)
    else:
        _, (llh,) = ft.inputs(g, [T], np.arange(S), S, 1., 61 + S)
    all_paths, all_scores = nt.brute_force(g, llh)
    n = len(all_scores)
    assert n >= 1
    short = False
    for k in KS:
        paths, scores = nt.nbest(g, llh, k)
        assert paths.shape == (k, T) and scores.shape == (k,)
        m = min(k, n)
        short |= m < k
        if integer:
            np.testing.assert_array_equal(scores[:m], all_scores[:m])
            np.testing.assert_array_equal(paths[:m], all_paths[:m])
        else:
            np.testing.assert_allclose(scores[:m], all_scores[:m], rtol=0, atol=1e-12)
            # the same paths wherever the enumeration's scores are apart
            apart = np.ones(m, dtype=bool)
            gaps = np.abs(np.diff(all_scores[:m + 1])) > 1e-9
            apart[:len(gaps)] &= gaps[:m]
            apart[1:] &= gaps[:m - 1]
            np.testing.assert_array_equal(paths[:m][apart], all_paths[:m][apart])
        assert np.isneginf(scores[m:]).all() and (paths[m:] == -1).all()
        assert len({tuple(p) for p in paths[:m]}) == m
    if (S, T) in ((1, 1), (1, 4), (3, 1), (3, 2)):
        assert short, 'this case has fewer than 16 finite paths'


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_truth_at_k_1_is_the_oracles_best_path(dtype):
    for S, T, nO, hub in ((3, 9, 2, 0), (8, 33, 3, 0), (20, 17, 4, 5), (1, 3, 1, 0)):
        g = ft.make_graph(S, ft.offsets(nO, S), 70 + S, hub, dtype, integer=True)
        (llh,) = ft.viterbi_inputs(S, [T], 71 + S, dtype)
        paths, scores = nt.nbest(g, llh, 1, dtype)
        np.testing.assert_array_equal(paths[0], np.asarray(ft.best_path(g, llh, dtype)))
        assert scores[0] == nt.path_terms(g, llh, paths[0]).sum()
        # and the first of any k
        for k in (2, 5, 16):
            p2, s2 = nt.nbest(g, llh, k, dtype)
            np.testing.assert_array_equal(p2[0], paths[0])
            assert s2[0] == scores[0]


def test_the_integer_cases_exercise_the_tie_rule():
    ties = []
    for S, T, nO, hub in ENUMERATED:
        if S ** T < 32:
            continue
        g = ft.make_graph(S, ft.offsets(nO, S), 60 + S + T, hub, integer=True)
        (llh,) = ft.viterbi_inputs(S, [T], 61 + S)
        ties.append(int((np.diff(nt.brute_force(g, llh)[1][:16]) == 0).sum()))
    print('ties among the 16 best scores:', ties)
    assert min(ties) >= 3


def test_score_bound():
    assert nt.score_bound([1., -2., 3.], 1e-5) == pytest.approx(7e-5)
    assert nt.score_bound([], 1e-10) == 1e-10


# --- errors raised on the host ------------------------------------------------------------------

def small_model():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2])
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=3, noise_std=1.)
    return beer.HMM.create(graph, ns), graph


@pytest.mark.skipif(HAS_GPU, reason='checks behaviour on a GPU-less host')
def test_nbest_fails_loudly_without_gpu():
    model, graph = small_model()
    X = torch.randn(7, 2)
    with pytest.raises(_hip.HipUnavailable):
        model.decode_nbest(X, 3)
    with pytest.raises(_hip.HipUnavailable):
        beer.decode_nbest_batch(model, [X, X], 2, inference_graphs=[graph, graph])


def test_decode_takes_the_nbest_options_and_refuses_bad_ones(capsys):
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'decode', '--nbest', '3', '--scores', 'sc', '--distinct',
                              '--per-frame', 'mdl', 'ds'])
    assert (args.nbest, args.scores, args.distinct, args.per_frame) == (3, 'sc', True, True)
    hmm_cmds.decode.check(args)
    args = parser.parse_args(['hmm', 'decode', 'mdl', 'ds'])
    assert (args.nbest, args.scores, args.distinct, args.nsamples) == (None, None, False, None)
    hmm_cmds.decode.check(args)
    # refused before the model (a file that does not exist) is read
    for argv in (['--nbest', '3', '--nsamples', '2'], ['--nbest', '0'], ['--nbest', '17'],
                 ['--scores', 'sc'], ['--distinct']):
        args = parser.parse_args(['hmm', 'decode'] + argv + ['no-such-model', 'no-such-dataset'])
        with pytest.raises(SystemExit):
            args.func(args, None)
    with pytest.raises(SystemExit):
        parser.parse_args(['hmm', 'decode', '-h'])
    text = ' '.join(capsys.readouterr().out.split())
    assert 'STATE paths' in text and 'differ only by a boundary frame' in text
    assert hmm_cmds.COMMANDS[-1] is hmm_cmds.boundaries


def test_nbest_lines_skip_missing_ranks_and_keep_distinct_unit_sequences():
    start = {'a': 0, 'b': 3}
    paths = np.array([[0, 1, 3, 4], [0, 0, 3, 4], [3, 4, 4, 4], [-1, -1, -1, -1]])
    scores = np.array([-1., -2., -3., -np.inf])
    lines = hmm_cmds.decode.nbest_lines('u', paths, scores, start)
    assert lines == [('u-1', ['a', 'b'], -1.), ('u-2', ['a', 'b'], -2.), ('u-3', ['b'], -3.)]
    lines = hmm_cmds.decode.nbest_lines('u', paths, scores, start, distinct=True)
    assert lines == [('u-1', ['a', 'b'], -1.), ('u-2', ['b'], -3.)]
    lines = hmm_cmds.decode.nbest_lines('u', paths[:1], scores[:1], start, per_frame=True)
    assert lines == [('u-1', ['a', 'a', 'b', 'b'], -1.)]
