"""CPU checks of the arc posteriors by category: the three C symbols and the Python names,
`beer_hmm_arcs_route` against a Python restatement of the header's formula on a grid that crosses
every threshold of it, the refusals of the C entry point, the truth of tests/arcs_truth.py itself
(against path enumeration, the oracle's per-frame transition posteriors and its state posteriors),
the argument errors raised before any device work, the unit categories of a small phone loop and
of an alignment graph written out by hand, and the command line's parser."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import arcs_truth as at
import fb_truth as ft
from helpers import ROOT, orc

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main
from beer_amd.models.sequence import unit_start_categories

F32, F64 = _hip.F32, _hip.F64
HAS_GPU = torch.cuda.is_available()
K, L, FL, UL = at.BLOCK, at.ARCS_LDS, at.FRAME_LDS, at.UTT_LDS


def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the query may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype, n_cat, want_frames=1):
    return _hip.lib().beer_hmm_arcs_route(dtype, ctypes.byref(b) if b is not None else None,
                                          n_cat, want_frames)


def test_symbols_are_declared_exported_and_in_the_ctypes_tables():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name, kind in (('beer_hmm_arc_posteriors', 'int'), ('beer_hmm_arcs_route', 'int'),
                       ('beer_hmm_arcs_scratch_doubles', 'size_t')):
        assert re.search(r'^%s %s\(' % (kind, name), text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
    assert _hip.SIGNATURES['beer_hmm_arc_posteriors'] == \
        [_hip.c_i, _hip.c_p, _hip.c_p, _hip.c_p, _hip.c_i] + [_hip.c_p] * 4       # (+ the stream)
    assert _hip.SIGNATURES['beer_hmm_arcs_route'] == [_hip.c_i, _hip.c_p, _hip.c_i, _hip.c_i]
    assert _hip.SIZE_QUERIES['beer_hmm_arcs_scratch_doubles'] == [_hip.c_i, _hip.c_p]
    assert 'typedef struct {\n    const int32_t* arc_cat;\n    const int32_t* init_cat;' in text
    assert [f[0] for f in _hip.ArcMap._fields_] == ['arc_cat', 'init_cat', 'arc_off', 'state_off']
    for name, value in (('BEER_ARCS_BLOCK', _hip.ARCS_BLOCK), ('BEER_ARCS_ARCS_LDS', _hip.ARCS_ARCS_LDS),
                        ('BEER_ARCS_FRAME_LDS', _hip.ARCS_FRAME_LDS),
                        ('BEER_ARCS_UTT_LDS', _hip.ARCS_UTT_LDS)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % name, text).group(1), 16) == value
    assert (K, L, FL, UL) == (_hip.ARCS_BLOCK, _hip.ARCS_ARCS_LDS, _hip.ARCS_FRAME_LDS,
                              _hip.ARCS_UTT_LDS)
    assert _hip.arcs_family(K | L | UL) == K
    assert hk.arc_posteriors.__name__ in hk.__all__ and hk.arcs_route.__name__ in hk.__all__
    for name in ('unit_starts_batch', 'unit_counts_batch'):
        assert name in beer.inference.batch.__all__ and hasattr(beer, name)
    for cls in (beer.HMM, beer.PhoneLoop, beer.BigramPhoneLoop):
        assert callable(cls.arc_posteriors)
    assert beer.PhoneLoop.unit_starts is beer.BigramPhoneLoop.unit_starts
    assert not hasattr(beer.HMM, 'unit_starts')
    for cls in (beer.graph.CompiledGraph, beer.graph.SparseGraph, beer.graph.BoundGraph):
        assert callable(cls.out_arcs)


# --- the route ----------------------------------------------------------------------------------
STATES = (1, 2, 64, 65, 256, 257, 300, 600, 2000, 3900, 6136, 6137, 10232, 10233, 32767, 32768)
CATS = (0, 1, 2, 7, 512, 1024, 1025, 4096, 4097, 12000, 20000, 1 << 20)


def arc_counts(S, w):
    'Arc counts on both sides of the 64 KiB of the arcs in LDS at this S, and a few besides.'
    out = {0, 1, S, 3 * S, 12 * S, min(S * S, 40 * S)}
    a = (64 * 1024 - 16 * S - 128 - 4 * (S + 2) - w) // (8 + w)
    out |= {a, a + 1}
    return sorted(a for a in out if a >= 0)


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 0)):
            for A in arc_counts(S, w or 4):
                for n_cat in CATS:
                    for want_frames in (0, 1):
                        want = at.route_formula(S, A, w, n_cat, want_frames)
                        assert route(desc(S, A), dtype, n_cat, want_frames) == want, \
                            (S, A, dtype, n_cat, want_frames)
                        seen.add(want)
    # every combination of the three bits the formula can give (a frame's bins are never in LDS
    # without the utterance's), and the refusal
    assert seen == {K | a | f | u for a in (0, L) for f in (0, FL) for u in (0, UL)
                    if (f, u) != (FL, 0)} | {_hip.EINVAL}


def test_route_thresholds_sit_where_the_header_says():
    # arcs: 16 S + 128 + 4 (S + 2 + 2 A) + w (A + 1) <= 64 KiB
    assert route(desc(120, 1800), F32, 40) == K | L | FL | UL          # config 3's loop
    assert route(desc(120, 1800), F64, 40) == K | L | FL | UL
    assert route(desc(100, 10000), F32, 40) == K | FL | UL             # every arc present: 120 KB
    assert route(desc(300, 4949), F32, 7) == K | L | FL | UL
    assert route(desc(300, 4950), F32, 7) == K | FL | UL
    assert route(desc(300, 3712), F64, 7) == K | L | FL | UL
    assert route(desc(300, 3713), F64, 7) == K | FL | UL
    # a frame's bins: n_cat <= 1024 and wanted at all; the utterance's: n_cat <= 4096
    assert route(desc(64, 200), F64, 1024) == K | L | FL | UL
    assert route(desc(64, 200), F64, 1025) == K | L | UL
    assert route(desc(64, 200), F64, 1024, 0) == K | L | UL
    assert route(desc(64, 200), F64, 4096) == K | L | UL
    assert route(desc(64, 200), F64, 4097) == K | L
    assert route(desc(64, 200), F64, 1 << 20, 0) == K | L
    # ... and rows of at most 96 KiB: 16 S + 128 <= 98304
    assert route(desc(6136, 100000), F64, 1024) == K | FL | UL
    assert route(desc(6137, 100000), F64, 1024) == K
    assert route(desc(6136, 100000), F32, 4096, 0) == K | UL
    assert route(desc(6137, 100000), F32, 1, 0) == K
    # EINVAL exactly where the sampler refuses, and where there is no category
    sample = _hip.lib().beer_hmm_sample_route
    for S in (1, 300, 10232, 10233, 32767, 32768, 0):
        for dtype in (F32, F64, 7):
            b = desc(S, S)
            assert (route(b, dtype, 3) == _hip.EINVAL) == \
                (sample(dtype, ctypes.byref(b), 1) == _hip.EINVAL), (S, dtype)
    assert route(None, F64, 3) == _hip.EINVAL
    assert route(desc(8, 8), F64, 0) == _hip.EINVAL and route(desc(8, 8), F64, -4) == _hip.EINVAL


def test_the_entry_point_refuses_before_it_launches():
    call = _hip.lib().beer_hmm_arc_posteriors
    one = ctypes.c_void_p(16)                # (never dereferenced: every call below is refused)
    good = _hip.ArcMap(one, one, one, one)
    ok = desc(8, 16)

    def rc(dtype, b, n_cat, amap, frame, utt, pc=one, ws=one):
        return call(dtype, ctypes.byref(b) if b is not None else None, pc,
                    ctypes.byref(amap) if amap is not None else None, n_cat, ws, frame, utt, None)
    assert rc(7, ok, 3, good, one, one) == _hip.EINVAL                       # dtype
    assert rc(F64, None, 3, good, one, one) == _hip.EINVAL
    assert rc(F64, desc(32768, 8), 3, good, one, one) == _hip.EINVAL         # states
    assert rc(F64, desc(10233, 8), 3, good, one, one) == _hip.EINVAL         # rows beyond LDS
    assert rc(F32, ok, 0, good, one, one) == _hip.EINVAL                     # n_cat < 1
    assert rc(F32, ok, 3, None, one, one) == _hip.EINVAL                     # no map
    for k in range(4):
        members = [one] * 4
        members[k] = None
        assert rc(F32, ok, 3, _hip.ArcMap(*members), one, one) == _hip.EINVAL, k
    assert rc(F32, ok, 3, good, None, None) == _hip.EINVAL                   # no output
    assert rc(F32, ok, 3, good, one, None, pc=None) == _hip.EINVAL
    assert rc(F32, ok, 3, good, None, one, ws=None) == _hip.EINVAL
    # an empty batch is no error and launches nothing
    assert rc(F32, desc(8, 16, nutt=0), 3, good, one, None, pc=None, ws=None) == 0
    scratch = _hip.lib().beer_hmm_arcs_scratch_doubles
    assert scratch(F64, ctypes.byref(ok)) == 0 and scratch(F64, None) == 0


# --- the truth itself ---------------------------------------------------------------------------
ENUMERATED = ((1, 4, 0), (2, 4, 0), (3, 4, 0), (3, 1, 0), (3, 3, 2), (2, 2, 0))   # (S, T, hub)


@pytest.mark.parametrize('S,T,hub', ENUMERATED)
def test_truth_is_the_enumeration_of_all_paths(S, T, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 60 + S, hub)
    _, (llh,) = ft.inputs(g, [T], np.arange(S), S, 1., 61 + T)
    for n_cat, drop in ((1, 0.), (2, 0.), (3, .3), (5, .5)):
        arc_cat, init_cat = at.random_categories(g, n_cat, S + T + n_cat, drop)
        frame, utt = at.arc_posteriors(g, llh, arc_cat, init_cat, n_cat)
        bf, bu = at.brute_force(g, llh, arc_cat, init_cat, n_cat)
        assert frame.shape == (T, n_cat) and utt.shape == (n_cat,)
        assert np.abs(frame - bf).max() <= 1e-12 and np.abs(utt - bu).max() <= 1e-12 * (T + 1)
        if not drop:
            assert np.abs(frame.sum(1) - 1.).max() <= 1e-12


@pytest.mark.parametrize('S,nO,T,hub', [(3, 2, 4, 0), (8, 3, 9, 0), (12, 3, 6, 4), (64, 8, 5, 0)])
def test_truth_is_the_oracles_xi_and_gamma(S, nO, T, hub):
    g = ft.make_graph(S, ft.offsets(nO, S), 80 + S, hub)
    _, (llh,) = ft.inputs(g, [T], np.arange(S), S, 1., 81 + T)
    src, dst = at.out_arcs(g)
    # one category per arc, no init category: the sparse per-frame xi
    arc_cat = np.arange(len(src), dtype=np.int32)
    frame, utt = at.arc_posteriors(g, llh, arc_cat, -np.ones(S, dtype=np.int32), len(src))
    xi = ft.xi_frames(g, llh)
    assert np.abs(frame[0]).max() == 0.
    assert np.abs(frame[1:] - xi[:, src, dst]).max() <= 1e-12
    assert np.abs(utt - xi.sum(0)[src, dst]).max() <= 1e-12 * (T + 1)
    # arc_cat = dst, init_cat = j: gamma
    gam, _ = at.arc_posteriors(g, llh, dst.astype(np.int32), np.arange(S, dtype=np.int32), S)
    with np.errstate(invalid='ignore', divide='ignore'):
        want = orc.posteriors(llh, g['init'], g['final'], g['trans'], True)[0]
    assert np.abs(gam - want).max() <= 1e-12
    assert np.abs(gam.sum(1) - 1.).max() <= 1e-12


def test_truth_follows_the_zero_rules():
    S = 4
    g = ft.make_graph(S, (0, 1), 3)
    _, (llh,) = ft.inputs(g, [6], np.arange(S), S, 1., 4)
    arc_cat, init_cat = at.random_categories(g, 3, 5)
    holes = llh.copy()
    holes[1, 0] = holes[2, 3] = holes[4, 1] = -np.inf
    frame, utt = at.arc_posteriors(g, holes, arc_cat, init_cat, 3)
    bf, bu = at.brute_force(g, holes, arc_cat, init_cat, 3)
    assert np.abs(frame - bf).max() <= 1e-12 and np.abs(frame.sum(1) - 1.).max() <= 1e-12
    dead = llh.copy()
    dead[3] = -np.inf
    for graph, x in ((g, dead), (dict(g, final=np.full(S, -np.inf)), llh)):
        frame, utt = at.arc_posteriors(graph, x, arc_cat, init_cat, 3)
        assert frame.shape == (6, 3) and not frame.any() and not utt.any()
        bf, bu = at.brute_force(graph, x, arc_cat, init_cat, 3)
        assert not bf.any() and not bu.any()


# --- errors raised on the host ----------------------------------------------------------------

def test_categories_are_checked_on_the_host():
    check = hk.check_arc_categories
    arcs = [np.zeros(5, np.int32), np.array([0, 1, -1], np.int32)]
    inits = [np.zeros(2, np.int32), np.array([2, -1], np.int32)]
    a, i = check([5, 3], [2, 2], arcs, inits, 3)
    assert a.dtype == torch.int32 and a.tolist() == [0] * 5 + [0, 1, -1] and i.tolist() == [0, 0, 2, -1]
    # already concatenated tensors, int64 too
    a2, _ = check([5, 3], [2, 2], torch.cat([torch.from_numpy(x) for x in arcs]).long(),
                  torch.tensor([0, 0, 2, -1]), 3, per_frame=False, per_utt=True)
    assert torch.equal(a2, a)
    with pytest.raises(ValueError, match='neither'):
        check([5, 3], [2, 2], arcs, inits, 3, per_frame=False, per_utt=False)
    with pytest.raises(ValueError, match='categories'):
        check([5, 3], [2, 2], arcs, inits, 0)
    with pytest.raises(ValueError, match='outside'):
        check([5, 3], [2, 2], arcs, inits, 2)                            # 2 >= n_cat
    with pytest.raises(ValueError, match='outside'):
        check([5, 3], [2, 2], [arcs[0], np.array([0, -2, 1])], inits, 3)
    with pytest.raises(ValueError, match='entries'):
        check([5, 4], [2, 2], arcs, inits, 3)
    with pytest.raises(ValueError, match='entries'):
        check([5, 3], [2, 3], arcs, inits, 3)
    with pytest.raises(ValueError, match='distinct graphs'):
        check([5, 3], [2, 2], arcs[:1], inits, 3)
    with pytest.raises(ValueError, match='entries'):
        check([5, 3], [2, 2], torch.zeros(7, dtype=torch.int32), inits, 3)
    with pytest.raises(ValueError, match='integers'):
        check([5, 3], [2, 2], torch.zeros(8), inits, 3)


def small_model():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2])
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=3, noise_std=1.)
    return beer.HMM.create(graph, ns), graph, g


def test_out_arcs_is_the_row_major_order_of_the_finite_transitions():
    _, graph, g = small_model()
    src, dst = graph.out_arcs()
    want = at.out_arcs(g)
    assert src.dtype == np.int32 and dst.dtype == np.int32
    assert src.tolist() == want[0].tolist() and dst.tolist() == want[1].tolist()
    assert (np.diff(src.astype(np.int64) * 3 + dst) > 0).all()


def test_model_arguments_are_refused_without_a_device():
    model, graph, g = small_model()
    X = torch.randn(7, 2)
    A = len(graph.out_arcs()[0])
    ok_a, ok_i = np.zeros(A, np.int32), np.zeros(3, np.int32)
    for arc_cat, init_cat, n_cat in ((ok_a[:-1], ok_i, 2), (ok_a, ok_i[:-1], 2), (ok_a + 2, ok_i, 2),
                                     (ok_a, ok_i - 2, 2), (ok_a, ok_i, 0)):
        with pytest.raises(ValueError):
            model.arc_posteriors(X, arc_cat, init_cat, n_cat)
        with pytest.raises(ValueError):
            model.arc_posteriors(X, arc_cat, init_cat, n_cat, inference_graph=graph, per_frame=False)
    for fn in (beer.unit_starts_batch, beer.unit_counts_batch):
        for utts, graphs in (([X, X], [graph]), ([X], [graph, graph]),
                             ((torch.cat([X, X]), [7, 7]), []), (iter([X, X]), [graph] * 3)):
            with pytest.raises(ValueError, match='inference graphs'):
                fn(model, utts, inference_graphs=graphs)
        with pytest.raises(ValueError, match='phone loop'):
            fn(model, [X])                                   # a plain HMM has no units


@pytest.mark.skipif(HAS_GPU, reason='checks behaviour on a GPU-less host')
def test_arc_posteriors_fail_loudly_without_gpu():
    model, graph, g = small_model()
    A = len(graph.out_arcs()[0])
    with pytest.raises(_hip.HipUnavailable):
        model.arc_posteriors(torch.randn(7, 2), np.zeros(A, np.int32), np.zeros(3, np.int32), 1)


# --- unit categories, written out by hand ---------------------------------------------------

_TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
         {'start_id': 1, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 2, 'trans_prob': .5},
         {'start_id': 2, 'end_id': 3, 'trans_prob': .5}]


def two_state_units(names):
    conf = {'g': {'topology': _TOPO, 'n_normal_per_state': 1, 'prior_strength': 1.,
                  'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}}
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(2), torch.ones(2))
    return units, ems


def test_unit_categories_of_a_small_phone_loop():
    'Three units of two states: pdfs 0 1 | 2 3 | 4 5; a unit is entered at its first state only.'
    names = ['a', 'b', 'c']
    units, ems = two_state_units(names)
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    assert (start, end) == ({'a': 0, 'b': 2, 'c': 4}, {'a': 1, 'b': 3, 'c': 5})
    cg = graph.compile()
    assert [int(i) for i in cg.pdf_id_mapping] == [0, 1, 2, 3, 4, 5]
    src, dst = cg.out_arcs()
    # first states loop and move on; last states loop and leave for every unit's first state
    assert list(zip(src.tolist(), dst.tolist())) == [
        (0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 4), (2, 2), (2, 3), (3, 0), (3, 2), (3, 3),
        (3, 4), (4, 4), (4, 5), (5, 0), (5, 2), (5, 4), (5, 5)]
    arc_cat, init_cat = unit_start_categories(cg, start, end)
    assert arc_cat.dtype == np.int32 and init_cat.dtype == np.int32
    assert arc_cat.tolist() == [-1, -1, 0, -1, 1, 2, -1, -1, 0, 1, -1, 2, -1, -1, 0, 1, 2, -1]
    assert init_cat.tolist() == [0, 0, 1, 1, 2, 2]
    # the units in start_pdf ORDER, whatever their pdf ids
    arc_cat, init_cat = unit_start_categories(cg, {'c': 4, 'a': 0, 'b': 2}, end)
    assert arc_cat.tolist() == [-1, -1, 1, -1, 2, 0, -1, -1, 1, 2, -1, 0, -1, -1, 1, 2, 0, -1]
    assert init_cat.tolist() == [1, 1, 2, 2, 0, 0]


def test_unit_categories_of_an_alignment_graph_with_a_repeated_unit():
    'b a b: five arcs enter a first state from another state, two of them the same unit.'
    names = ['a', 'b', 'c']
    units, _ = two_state_units(names)
    _, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), dict(units))
    gset = beer.graph.compile_alignments([['b', 'a', 'b']], two_state_units(names)[0])
    g = gset[0]
    assert [int(i) for i in g.pdf_id_mapping] == [2, 3, 0, 1, 2, 3]
    src, dst = g.out_arcs()
    assert list(zip(src.tolist(), dst.tolist())) == [
        (0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 5), (5, 5)]
    arc_cat, init_cat = unit_start_categories(g, start, end)
    assert arc_cat.tolist() == [-1, -1, -1, 0, -1, -1, -1, 1, -1, -1, -1]
    assert init_cat.tolist() == [1, 1, 0, 0, 1, 1]


def test_boundaries_is_a_command_and_its_parser_takes_the_options():
    assert hmm_cmds.COMMANDS[-1] is hmm_cmds.boundaries
    assert [c.__name__ for c in hmm_cmds.COMMANDS].count('boundaries') == 1
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'boundaries', '-a', 'alis.npz', '-s', '0.5', '-u', 'utts',
                              '--counts', 'mdl', 'ds', 'out'])
    assert (args.alis, args.acoustic_scale, args.utts, args.counts, args.model, args.dataset,
            args.outdir) == ('alis.npz', .5, 'utts', True, 'mdl', 'ds', 'out')
    assert args.func is hmm_cmds.boundaries.main
    args = parser.parse_args(['hmm', 'boundaries', 'mdl', 'ds', 'out'])
    assert (args.alis, args.acoustic_scale, args.utts, args.counts) == (None, 1., None, False)
    with pytest.raises(SystemExit):
        parser.parse_args(['hmm', 'boundaries', 'mdl', 'ds'])
