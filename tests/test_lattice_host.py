"""CPU checks of the Viterbi max-marginals: the three C symbols and the Python names,
`beer_hmm_maxmarg_route` against a Python restatement of the header's formula on a grid that
crosses every threshold of it, the refusals of the C entry point, the truth of
tests/lattice_truth.py itself (EXACTLY the enumeration of all paths on integer inputs, within the
derived bound on real ones, a dead utterance, T = 1), the argument errors raised before any device
work, and the `lattice` command's parser and beam."""

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fb_truth as ft
import lattice_truth as lt
from helpers import ROOT

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main

F32, F64 = _hip.F32, _hip.F64
K, L, BL = lt.BLOCK, lt.ARCS_LDS, lt.BINS_LDS


def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the query may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype, n_cat, state=1, frames=0, utt=0):
    return _hip.lib().beer_hmm_maxmarg_route(dtype, ctypes.byref(b) if b is not None else None,
                                             n_cat, state, frames, utt)


def test_symbols_are_declared_exported_and_in_the_ctypes_tables():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name, kind in (('beer_hmm_max_marginals', 'int'), ('beer_hmm_maxmarg_route', 'int'),
                       ('beer_hmm_maxmarg_scratch_doubles', 'size_t')):
        assert re.search(r'^%s %s\(' % (kind, name), text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
    assert _hip.SIGNATURES['beer_hmm_max_marginals'] == \
        [_hip.c_i, _hip.c_p, _hip.c_p, _hip.c_p, _hip.c_i] + [_hip.c_p] * 6       # (+ the stream)
    assert _hip.SIGNATURES['beer_hmm_maxmarg_route'] == [_hip.c_i, _hip.c_p] + [_hip.c_i] * 4
    assert _hip.SIZE_QUERIES['beer_hmm_maxmarg_scratch_doubles'] == [_hip.c_i, _hip.c_p]
    for name, value in (('BEER_MAXMARG_BLOCK', _hip.MAXMARG_BLOCK),
                        ('BEER_MAXMARG_ARCS_LDS', _hip.MAXMARG_ARCS_LDS),
                        ('BEER_MAXMARG_BINS_LDS', _hip.MAXMARG_BINS_LDS)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % name, text).group(1), 16) == value
    assert (K, L, BL) == (_hip.MAXMARG_BLOCK, _hip.MAXMARG_ARCS_LDS, _hip.MAXMARG_BINS_LDS)
    assert _hip.maxmarg_family(K | L | BL) == K
    assert 'max_marginals' in hk.__all__ and 'maxmarg_route' in hk.__all__
    assert 'unit_start_margins_batch' in beer.inference.batch.__all__
    assert hasattr(beer, 'unit_start_margins_batch')
    for cls in (beer.HMM, beer.PhoneLoop, beer.BigramPhoneLoop):
        assert callable(cls.max_marginals) and callable(cls.arc_max_marginals)
    assert beer.PhoneLoop.unit_start_margins is beer.BigramPhoneLoop.unit_start_margins
    assert not hasattr(beer.HMM, 'unit_start_margins')


# --- the route ----------------------------------------------------------------------------------
STATES = (1, 2, 64, 65, 256, 257, 300, 600, 2000, 3900, 6136, 6137, 10232, 10233, 32767, 32768)
CATS = (-3, 0, 1, 7, 2048, 2049, 20000, 1 << 20)
WANTS = [(s, f, u) for s in (0, 1) for f in (0, 1) for u in (0, 1)]


def arc_counts(S, w):
    'Arc counts on both sides of the 64 KiB of the arcs in LDS at this S, and a few besides.'
    out = {0, 1, S, 3 * S, 12 * S, min(S * S, 40 * S)}
    for per_arc in (4 + w, 8 + w):                          # without and with the categories
        a = (64 * 1024 - 16 * S - 128 - 4 * (S + 2) - w) // per_arc
        out |= {a, a + 1}
    return sorted(a for a in out if a >= 0)


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 0)):
            for A in arc_counts(S, w or 4):
                for n_cat in CATS:
                    for wants in WANTS:
                        want = lt.route_formula(S, A, w, n_cat, *wants)
                        assert route(desc(S, A), dtype, n_cat, *wants) == want, \
                            (S, A, dtype, n_cat, wants)
                        seen.add(want)
    # every combination of the two bits, and the refusal
    assert seen == {K | a | b for a in (0, L) for b in (0, BL)} | {_hip.EINVAL}


def test_route_thresholds_sit_where_the_header_says():
    # arcs: 16 S + 128 + 4 (S + 2 + A) + w (A + 1) <= 64 KiB, 4 A more with categories
    assert route(desc(120, 1800), F32, 0) == K | L                         # config 3's loop
    assert route(desc(120, 1800), F32, 40, 1, 1, 0) == K | L | BL
    assert route(desc(120, 1800), F64, 40, 0, 1, 1) == K | L | BL
    assert route(desc(100, 10000), F32, 40, 1, 1) == K | BL                # every arc present
    assert route(desc(300, 4949), F32, 7, 1, 1) == K | L | BL
    assert route(desc(300, 4950), F32, 7, 1, 1) == K | BL
    assert route(desc(300, 4950), F32, 7, 1, 0) == K | L                   # no categories read
    assert route(desc(300, 7424), F32, 0) == K | L
    assert route(desc(300, 7425), F32, 0) == K
    assert route(desc(300, 3712), F64, 7, 0, 0, 1) == K | L | BL
    assert route(desc(300, 3713), F64, 7, 0, 0, 1) == K | BL
    # bins: wanted at all, n_cat <= 2048 ...
    assert route(desc(64, 200), F64, 2048, 1, 1, 1) == K | L | BL
    assert route(desc(64, 200), F64, 2049, 1, 1, 1) == K | L
    assert route(desc(64, 200), F64, 2049, 0, 0, 1) == K | L
    assert route(desc(64, 200), F64, 2048, 1, 0, 0) == K | L
    # ... and rows of at most 96 KiB: 16 S + 128 <= 98304
    assert route(desc(6136, 100000), F64, 1024, 1, 1) == K | BL
    assert route(desc(6137, 100000), F64, 1024, 1, 1) == K
    # EINVAL exactly where the sampler refuses; without an output; categories without a number
    sample = _hip.lib().beer_hmm_sample_route
    for S in (1, 300, 10232, 10233, 32767, 32768, 0):
        for dtype in (F32, F64, 7):
            b = desc(S, S)
            assert (route(b, dtype, 3, 1, 1, 1) == _hip.EINVAL) == \
                (sample(dtype, ctypes.byref(b), 1) == _hip.EINVAL), (S, dtype)
    assert route(None, F64, 3) == _hip.EINVAL
    assert route(desc(8, 8), F64, 3, 0, 0, 0) == _hip.EINVAL
    assert route(desc(8, 8), F64, 0, 1, 1, 0) == _hip.EINVAL
    assert route(desc(8, 8), F64, -4, 0, 0, 1) == _hip.EINVAL
    assert route(desc(8, 8), F64, 0, 1, 0, 0) == K | L


def test_the_entry_point_refuses_before_it_launches():
    call = _hip.lib().beer_hmm_max_marginals
    one = ctypes.c_void_p(16)                # (never dereferenced: every call below is refused)
    good = _hip.ArcMap(one, one, one, one)
    ok = desc(8, 16)

    def rc(dtype, b, n_cat, amap, state, frame, utt, pc=one, ws=one, best=one):
        return call(dtype, ctypes.byref(b) if b is not None else None, pc,
                    ctypes.byref(amap) if amap is not None else None, n_cat, ws, state, frame, utt,
                    best, None)
    assert rc(7, ok, 3, good, one, one, one) == _hip.EINVAL                  # dtype
    assert rc(F64, None, 3, good, one, one, one) == _hip.EINVAL
    assert rc(F64, desc(32768, 8), 3, good, one, one, one) == _hip.EINVAL    # states
    assert rc(F64, desc(10233, 8), 3, good, one, one, one) == _hip.EINVAL    # rows beyond LDS
    assert rc(F64, desc(10233, 8), 0, None, one, None, None) == _hip.EINVAL
    assert rc(F32, ok, 0, good, one, one, one) == _hip.EINVAL                # n_cat < 1 with a map
    assert rc(F32, ok, 0, good, one, None, None) == _hip.EINVAL
    assert rc(F32, ok, 3, None, one, one, None) == _hip.EINVAL               # categories, no map
    assert rc(F32, ok, 3, None, None, None, one) == _hip.EINVAL
    for k in range(4):
        members = [one] * 4
        members[k] = None
        assert rc(F32, ok, 3, _hip.ArcMap(*members), one, one, one) == _hip.EINVAL, k
        assert rc(F32, ok, 3, _hip.ArcMap(*members), one, None, None) == _hip.EINVAL, k
    assert rc(F32, ok, 3, good, None, None, None) == _hip.EINVAL             # no output
    assert rc(F32, ok, 0, None, None, None, None) == _hip.EINVAL
    assert rc(F32, ok, 3, good, one, one, None, pc=None) == _hip.EINVAL
    assert rc(F32, ok, 3, good, None, None, one, ws=None) == _hip.EINVAL
    assert rc(F32, ok, 0, None, one, None, None, best=None) == _hip.EINVAL
    # an empty batch is no error and launches nothing
    empty = desc(8, 16, nutt=0)
    assert rc(F32, empty, 3, good, one, one, None, pc=None, ws=None, best=None) == 0
    assert rc(F64, empty, 0, None, one, None, None, pc=None, ws=None, best=None) == 0
    scratch = _hip.lib().beer_hmm_maxmarg_scratch_doubles
    assert scratch(F64, ctypes.byref(ok)) == 0 and scratch(F64, None) == 0


# --- the truth itself ---------------------------------------------------------------------------
ENUMERATED = ((1, 4, 0), (2, 6, 0), (3, 5, 0), (3, 1, 0), (4, 4, 2), (8, 3, 0), (8, 4, 3),
              (5, 5, 0))                                                   # (S, T, hub)


def both(g, llh, arc_cat, init_cat, n_cat):
    return lt.max_marginals(g, llh, arc_cat, init_cat, n_cat), \
        lt.brute_force(g, llh, arc_cat, init_cat, n_cat)


def holes_in(llh, seed):
    'A copy with a sixth of the entries -inf.'
    out = llh.copy()
    out[np.random.RandomState(seed).rand(*llh.shape) < 1 / 6.] = -np.inf
    return out


@pytest.mark.parametrize('S,T,hub', ENUMERATED)
def test_truth_is_exactly_the_enumeration_on_integer_inputs(S, T, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 60 + S, hub, integer=True)
    (llh,) = ft.viterbi_inputs(S, [T], 61 + T)
    for x in (llh, holes_in(llh, S + T), llh.astype(np.float32)):
        for n_cat, drop in ((1, 0.), (3, .3), (5, .5)):
            arc_cat, init_cat = lt.random_categories(g, n_cat, S + T + n_cat, drop)
            got, want = both(g, x, arc_cat, init_cat, n_cat)
            assert got[0] == want[0]
            for a, b in zip(got[1:], want[1:]):
                assert a.shape == b.shape and np.array_equal(a, b)
            best, mm, frame, utt = got
            assert mm.shape == (T, S) and frame.shape == (T, n_cat) and utt.shape == (n_cat,)
            assert (mm <= 0).all() and (frame <= 0).all() and not np.isnan(mm).any()
            if np.isfinite(best):
                assert (mm.max(1) == 0).all()               # the best path passes every frame
        # gamma categories: the rows are the state max-marginals
        a, i, n = lt.gamma_categories(g)
        _, mm, frame, _ = lt.max_marginals(g, x, a, i, n)
        assert np.array_equal(frame, mm)
        # without categories
        best, mm2, none_f, none_u = lt.max_marginals(g, x)
        assert none_f is None and none_u is None and np.array_equal(mm2, mm)


@pytest.mark.parametrize('S,T,hub', ENUMERATED)
def test_truth_is_the_enumeration_within_the_bound_on_real_inputs(S, T, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 70 + S, hub)
    _, (llh,) = ft.inputs(g, [T], np.arange(S), S, 1., 71 + T)
    for x in (llh, holes_in(llh, S + T)):
        arc_cat, init_cat = lt.random_categories(g, 4, S + T, .3)
        got, want = both(g, x, arc_cat, init_cat, 4)
        tol = 4 * (T + 1) * 2. ** -52 * lt.bound(g, x)
        assert abs(got[0] - want[0]) <= tol
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(np.isfinite(a), np.isfinite(b))
            fin = np.isfinite(a)
            assert np.abs(a[fin] - b[fin]).max(initial=0.) <= tol
        a, i, n = lt.gamma_categories(g)
        _, mm, frame, _ = lt.max_marginals(g, x, a, i, n)
        assert np.array_equal(frame, mm)                    # (bit for bit: rounding is monotone)


def test_truth_of_a_dead_utterance_and_of_one_frame():
    S = 4
    g = ft.make_graph(S, (0, 1), 3)
    _, (llh,) = ft.inputs(g, [6], np.arange(S), S, 1., 4)
    arc_cat, init_cat = lt.random_categories(g, 3, 5)
    dead = llh.copy()
    dead[3] = -np.inf
    for graph, x in ((g, dead), (dict(g, final=np.full(S, -np.inf)), llh)):
        for fn in (lt.max_marginals, lt.brute_force):
            best, mm, frame, utt = fn(graph, x, arc_cat, init_cat, 3)
            assert best == -np.inf and mm.shape == (6, S) and frame.shape == (6, 3)
            assert (mm == -np.inf).all() and (frame == -np.inf).all() and (utt == -np.inf).all()
    # T = 1: init + l + final, states by init_cat alone
    best, mm, frame, utt = lt.max_marginals(g, llh[:1], arc_cat, init_cat, 3)
    score = llh[0] + g['init'] + g['final']
    assert best == score.max() and np.array_equal(mm[0], (llh[0] + g['init']) + g['final'] - best)
    assert mm[0].max() == 0. and (mm[0, 3:] == -np.inf).all()
    for c in range(3):
        assert frame[0, c] == mm[0][init_cat == c].max(initial=-np.inf) and utt[c] == frame[0, c]
    assert lt.bound(g, llh[:1]) >= np.abs(score[np.isfinite(score)]).max()


# --- errors raised on the host ----------------------------------------------------------------

def small_model():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2])
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=3, noise_std=1.)
    return beer.HMM.create(graph, ns), graph, g


class NoDevice(SimpleNamespace):
    'A batch of two graphs that fails the test as soon as anything but its counts is read.'

    def __getattr__(self, name):
        raise AssertionError(f'batch.{name} was read: device work before the arguments were checked')


def test_arguments_are_refused_before_any_device_work():
    batch = NoDevice(n_arcs=[5, 3], n_states=[2, 2])
    arcs = [np.zeros(5, np.int32), np.array([0, 1, -1], np.int32)]
    inits = [np.zeros(2, np.int32), np.array([2, -1], np.int32)]
    with pytest.raises(ValueError, match='none of'):
        hk.max_marginals(batch, None, states=False)
    with pytest.raises(ValueError, match='none of'):
        hk.max_marginals(batch, None, arcs, inits, 3, states=False)
    for kw in (dict(per_frame=True), dict(per_utt=True), dict(states=False, per_utt=True)):
        with pytest.raises(ValueError, match='need arc_cat'):
            hk.max_marginals(batch, None, **kw)
    with pytest.raises(ValueError, match='come together'):
        hk.max_marginals(batch, None, arcs, None, 3)
    for bad_a, bad_i, n_cat in ((arcs, inits, 2), (arcs, inits, 0), (arcs[:1], inits, 3),
                                ([arcs[0], np.array([0, -2, 1])], inits, 3),
                                (arcs, [inits[0], np.zeros(3, np.int32)], 3),
                                (torch.zeros(8), inits, 3)):
        with pytest.raises(ValueError, match='arc_posteriors'):      # (check_arc_categories)
            hk.max_marginals(batch, None, bad_a, bad_i, n_cat, per_frame=True)
        with pytest.raises(ValueError, match='arc_posteriors'):
            hk.max_marginals(batch, None, bad_a, bad_i, n_cat)       # states alone, yet checked


def test_model_arguments_are_refused_without_a_device():
    model, graph, g = small_model()
    X = torch.randn(7, 2)
    A = len(graph.out_arcs()[0])
    ok_a, ok_i = np.zeros(A, np.int32), np.zeros(3, np.int32)
    for arc_cat, init_cat, n_cat in ((ok_a[:-1], ok_i, 2), (ok_a, ok_i[:-1], 2), (ok_a + 2, ok_i, 2),
                                     (ok_a, ok_i - 2, 2), (ok_a, ok_i, 0)):
        with pytest.raises(ValueError):
            model.arc_max_marginals(X, arc_cat, init_cat, n_cat)
        with pytest.raises(ValueError):
            model.arc_max_marginals(X, arc_cat, init_cat, n_cat, inference_graph=graph,
                                    per_frame=False)
    for utts, graphs in (([X, X], [graph]), ([X], [graph, graph]),
                         ((torch.cat([X, X]), [7, 7]), []), (iter([X, X]), [graph] * 3)):
        with pytest.raises(ValueError, match='inference graphs'):
            beer.unit_start_margins_batch(model, utts, inference_graphs=graphs)
    with pytest.raises(ValueError, match='phone loop'):
        beer.unit_start_margins_batch(model, [X])            # a plain HMM has no units


# --- the command line ---------------------------------------------------------------------------

def test_lattice_is_a_command_and_its_parser_takes_the_options():
    assert hmm_cmds.lattice in hmm_cmds.COMMANDS
    assert [c.__name__ for c in hmm_cmds.COMMANDS].count('lattice') == 1
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'lattice', '-a', 'alis.npz', '-s', '0.5', '-u', 'utts',
                              '--beam', '2.5', 'mdl', 'ds', 'out'])
    assert (args.alis, args.acoustic_scale, args.utts, args.beam, args.model, args.dataset,
            args.outdir) == ('alis.npz', .5, 'utts', 2.5, 'mdl', 'ds', 'out')
    assert args.func is hmm_cmds.lattice.main
    args = parser.parse_args(['hmm', 'lattice', 'mdl', 'ds', 'out'])
    assert (args.alis, args.acoustic_scale, args.utts, args.beam) == (None, 1., None, 10.)
    with pytest.raises(SystemExit):
        parser.parse_args(['hmm', 'lattice', 'mdl', 'ds'])


@pytest.mark.parametrize('beam', ['-1', 'nan', 'inf', '-inf', '-0.001'])
def test_a_bad_beam_is_refused_before_any_work(beam, tmp_path):
    out = tmp_path / 'never'
    with pytest.raises(SystemExit, match='--beam'):
        # (the model and the data set do not exist: they are never opened)
        cli_main.main(['hmm', 'lattice', '--beam=' + beam, str(tmp_path / 'no.mdl'),
                       str(tmp_path / 'no.ds'), str(out)])
    assert not out.exists()


def test_lattice_entries_are_the_cells_within_the_beam_sorted():
    m = np.array([[0., -np.inf, -3.], [-10., -2., 0.], [-np.inf, -np.inf, -np.inf], [-2.5, 0., -2.5]])
    frame, unit, margin = hmm_cmds.lattice_entries(m, 2.5)
    assert frame.dtype == np.int32 and unit.dtype == np.int32 and margin.dtype == np.float64
    assert frame.tolist() == [0, 1, 1, 3, 3, 3] and unit.tolist() == [0, 1, 2, 0, 1, 2]
    assert margin.tolist() == [0., -2., 0., -2.5, 0., -2.5]
    frame, unit, margin = hmm_cmds.lattice_entries(m.astype(np.float32), 0.)
    assert list(zip(frame.tolist(), unit.tolist())) == [(0, 0), (1, 2), (3, 1)]
    assert margin.dtype == np.float64 and not margin.any()
