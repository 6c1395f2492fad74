"""CPU checks of the unit segment lattices: the truth of tests/segments_truth.py itself (EXACTLY
the enumeration of all paths on integer inputs, within the derived bound on real ones, its row
maximum the start max-marginal of tests/lattice_truth.py), the closures `hk.segment_map` builds,
the four C symbols and the Python names, `beer_hmm_segments_route` against a Python restatement of
the header's formula on a grid that crosses its thresholds, the refusals of the C entry points, the
argument errors raised before any device work, and the `lattice` command's new options."""

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fb_truth as ft
import lattice_truth as lt
import segments_truth as st
from helpers import ROOT

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main

F32, F64 = _hip.F32, _hip.F64
K, L, BL = st.BLOCK, st.ARCS_LDS, st.BINS_LDS


# --- the truth itself ---------------------------------------------------------------------------
ENUMERATED = ((1, 4, 0), (2, 6, 0), (3, 5, 0), (3, 1, 0), (4, 4, 2), (5, 5, 0), (3, 6, 0),
              (4, 5, 0))                                                   # (S, T, hub)


def holes_in(llh, seed):
    'A copy with a sixth of the entries -inf.'
    out = llh.copy()
    out[np.random.RandomState(seed).rand(*llh.shape) < 1 / 6.] = -np.inf
    return out


@pytest.mark.parametrize('S,T,hub', ENUMERATED)
def test_truth_is_exactly_the_enumeration_on_integer_inputs(S, T, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 80 + S, hub, integer=True)
    (llh,) = ft.viterbi_inputs(S, [T], 81 + T)
    for x in (llh, holes_in(llh, S + T), llh.astype(np.float32)):
        for n_cat, drop in ((1, .5), (2, .6), (3, .3), (5, .5), (2, 0.)):
            arc_cat, init_cat = lt.random_categories(g, n_cat, S + T + n_cat, drop)
            for max_dur in (1, 2, T, T + 2):
                got = st.segments(g, x, arc_cat, init_cat, n_cat, max_dur)
                want = st.brute_force(g, x, arc_cat, init_cat, n_cat, max_dur)
                assert got.shape == (T, n_cat, max_dur) and np.array_equal(got, want)
                assert (got <= 0).all() and not np.isnan(got).any()
                # nothing runs past the utterance
                for s in range(T):
                    assert (got[s, :, T - s:] == -np.inf).all()
            # the best segment of a start is the start's max-marginal
            best, _, frame, _ = lt.max_marginals(g, x, arc_cat, init_cat, n_cat)
            assert np.array_equal(got.max(2), frame)
            # cutting max_dur cuts columns and changes nothing else
            assert np.array_equal(st.segments(g, x, arc_cat, init_cat, n_cat, 2), got[:, :, :2])
            # where the best path has a boundary with a label, its segment has no margin
            assert not np.isfinite(best) or ((frame == 0) == (got.max(2) == 0)).all()


@pytest.mark.parametrize('S,T,hub', ENUMERATED)
def test_truth_is_the_enumeration_within_the_bound_on_real_inputs(S, T, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 90 + S, hub)
    _, (llh,) = ft.inputs(g, [T], np.arange(S), S, 1., 91 + T)
    for x in (llh, holes_in(llh, S + T)):
        arc_cat, init_cat = lt.random_categories(g, 3, S + T, .4)
        got = st.segments(g, x, arc_cat, init_cat, 3, T)
        want = st.brute_force(g, x, arc_cat, init_cat, 3, T)
        tol = float(st.tolerance(st.bound(g, x), T, 0.))
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        fin = np.isfinite(got)
        assert np.abs(got[fin] - want[fin]).max(initial=0.) <= tol
        frame = lt.max_marginals(g, x, arc_cat, init_cat, 3)[2]
        assert np.array_equal(np.isfinite(got.max(2)), np.isfinite(frame))
        fin = np.isfinite(frame)
        assert np.abs(got.max(2)[fin] - frame[fin]).max(initial=0.) <= tol


def test_truth_of_a_dead_utterance_one_frame_and_no_boundary():
    S = 4
    g = ft.make_graph(S, (0, 1), 3, integer=True)
    (llh,) = ft.viterbi_inputs(S, [6], 4)
    arc_cat, init_cat = lt.random_categories(g, 3, 5)
    dead = llh.copy()
    dead[3] = -np.inf
    for fn in (st.segments, st.brute_force):
        assert (fn(g, dead, arc_cat, init_cat, 3, 6) == -np.inf).all()
        # T = 1: the segment (init_cat[j], 0, 0) of every state
        one = fn(g, llh[:1], arc_cat, init_cat, 3, 4)
        score = (llh[0] + g['init']) + g['final']
        for c in range(3):
            want = score[init_cat == c].max(initial=-np.inf) - score.max()
            assert one[0, c, 0] == (want if np.isfinite(want) else -np.inf)
        assert (one[:, :, 1:] == -np.inf).all()
        # no arc ends a segment: one segment from frame 0 to the end, of the first state's unit
        whole = fn(g, llh, np.full(len(arc_cat), -1), init_cat, 3, 6)
        assert (whole[1:] == -np.inf).all() and (whole[0, :, :5] == -np.inf).all()
        assert whole[0, :, 5].max() == 0.


# --- closures -----------------------------------------------------------------------------------

def triple(g):
    src, dst = st.out_arcs(g)
    return src, dst, g['S']


def check_map(smap, graphs, cats, n_cat):
    'Every array of a SegmentMap against the graphs it was built from.'
    total = 0
    for gi, (g, (arc_cat, init_cat)) in enumerate(zip(graphs, cats)):
        src, dst = st.out_arcs(g)
        want = st.closures(g, arc_cat, init_cat, n_cat)
        for c in range(n_cat):
            k = gi * n_cat + c
            m0, m1 = smap.mem_ptr[k], smap.mem_ptr[k + 1]
            members = smap.members[m0:m1]
            assert np.array_equal(members, want[c]) and np.array_equal(smap.closure(gi, c), want[c])
            assert np.array_equal(smap.mem_init[m0:m1], init_cat[members] == c)
            total = max(total, len(members))
            stays, enters = set(), set()
            for m in range(m0, m1):
                for a in range(smap.in_ptr[m], smap.in_ptr[m + 1]):
                    arc = smap.in_arc[a]
                    assert arc_cat[arc] == -1 and dst[arc] == smap.members[m]
                    assert members[smap.in_src[a]] == src[arc]
                    stays.add(int(arc))
                for a in range(smap.ent_ptr[m], smap.ent_ptr[m + 1]):
                    arc = smap.ent_arc[a]
                    assert arc_cat[arc] == c and dst[arc] == smap.members[m]
                    assert smap.ent_src[a] == src[arc]
                    enters.add(int(arc))
            inside = np.isin(src, members)
            assert stays == set(np.nonzero((arc_cat == -1) & inside)[0].tolist())
            assert enters == set(np.nonzero(arc_cat == c)[0].tolist())
    assert smap.max_closure == total
    assert len(smap.mem_ptr) == len(graphs) * n_cat + 1
    assert len(smap.in_ptr) == len(smap.members) + 1 == len(smap.ent_ptr)
    for name in hk.SegmentMap.FIELDS:
        assert getattr(smap, name).dtype == np.int32


def test_closures_of_a_phone_loop_are_the_units_own_states():
    g, arc_cat, init_cat = st.loop_graph([3, 3, 3])
    smap = hk.segment_map([triple(g)], [arc_cat], [init_cat], 3)
    for c in range(3):
        assert smap.closure(0, c).tolist() == [3 * c, 3 * c + 1, 3 * c + 2]
    assert smap.max_closure == 3 and smap.n_cat == 3 and smap.n_graphs == 1
    check_map(smap, [g], [(arc_cat, init_cat)], 3)


def test_closures_of_an_alignment_graph_join_the_instances_of_a_repeated_unit():
    g, arc_cat, init_cat = st.chain_graph([1, 0, 1, 2, 1], 2)
    loop = st.loop_graph([3] * 4)
    smap = hk.segment_map([triple(g), triple(loop[0])], [arc_cat, loop[1]], [init_cat, loop[2]], 4)
    assert smap.closure(0, 1).tolist() == [0, 1, 4, 5, 8, 9]
    assert smap.closure(0, 0).tolist() == [2, 3] and smap.closure(0, 2).tolist() == [6, 7]
    # a category with no member: unit 3 is not in the transcription
    assert smap.closure(0, 3).tolist() == []
    assert smap.closure(1, 3).tolist() == [9, 10, 11]
    assert smap.max_closure == 6
    check_map(smap, [g, loop[0]], [(arc_cat, init_cat), loop[1:]], 4)


def test_closures_of_random_categories_and_of_none():
    for S, seed in ((1, 0), (5, 1), (8, 2), (13, 3)):
        g = ft.make_graph(S, ft.offsets(3, S), seed)
        for n_cat, drop in ((1, .9), (3, .5), (6, .8), (2, 0.)):
            arc_cat, init_cat = lt.random_categories(g, n_cat, seed + n_cat, drop)
            smap = hk.segment_map([triple(g)], [arc_cat], [init_cat], n_cat)
            check_map(smap, [g], [(arc_cat, init_cat)], n_cat)
    g = ft.make_graph(4, (0, 1), 5)
    A = len(st.out_arcs(g)[0])
    smap = hk.segment_map([triple(g)], [np.full(A, -1)], [np.full(4, -1)], 2)
    assert smap.max_closure == 0 and len(smap.members) == 0 and smap.mem_ptr.tolist() == [0, 0, 0]
    assert hk.segment_map([], [], [], 2).mem_ptr.tolist() == [0]


# --- symbols and names --------------------------------------------------------------------------

def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the queries may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype, n_cat, max_closure=0):
    return _hip.lib().beer_hmm_segments_route(dtype, ctypes.byref(b) if b is not None else None,
                                              n_cat, max_closure)


def test_symbols_are_declared_exported_and_in_the_ctypes_tables():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name, kind in (('beer_hmm_segment_trellis', 'int'), ('beer_hmm_segment_margins', 'int'),
                       ('beer_hmm_segments_route', 'int'),
                       ('beer_hmm_segments_scratch_doubles', 'size_t')):
        assert re.search(r'^%s %s\(' % (kind, name), text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
    p, i = _hip.c_p, _hip.c_i
    assert _hip.SIGNATURES['beer_hmm_segment_trellis'] == [i, p, p, p, i] + [p] * 6
    assert _hip.SIGNATURES['beer_hmm_segment_margins'] == \
        [i, p, p, p, i] + [p] * 6 + [_hip.c_l, i, p, p]
    assert _hip.SIGNATURES['beer_hmm_segments_route'] == [i, p, i, i]
    assert _hip.SIZE_QUERIES['beer_hmm_segments_scratch_doubles'] == [i, p]
    assert 'beer_seg_map;' in text
    fields = re.search(r'typedef struct \{([^}]*)\} beer_seg_map;', text).group(1)
    assert re.findall(r'(\w+);', fields) == [f[0] for f in _hip.SegMap._fields_]
    for name, value in (('BEER_SEGMENTS_BLOCK', _hip.SEGMENTS_BLOCK),
                        ('BEER_SEGMENTS_ARCS_LDS', _hip.SEGMENTS_ARCS_LDS),
                        ('BEER_SEGMENTS_BINS_LDS', _hip.SEGMENTS_BINS_LDS)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % name, text).group(1), 16) == value
    assert (K, L, BL) == (_hip.SEGMENTS_BLOCK, _hip.SEGMENTS_ARCS_LDS, _hip.SEGMENTS_BINS_LDS)
    assert _hip.segments_family(K | L | 5) == K and _hip.segments_team(K | L | 5) == 32
    for name in ('segment_map', 'segment_margins', 'segments_route'):
        assert name in hk.__all__ and callable(getattr(hk, name))
    assert 'unit_segments_batch' in beer.inference.batch.__all__
    assert hasattr(beer, 'unit_segments_batch')
    assert beer.PhoneLoop.unit_segments is beer.BigramPhoneLoop.unit_segments
    assert not hasattr(beer.HMM, 'unit_segments')


# --- the route ----------------------------------------------------------------------------------
STATES = (1, 2, 64, 256, 257, 300, 2000, 4095, 4096, 6136, 6137, 10232, 10233, 32767, 32768)
CATS = (-3, 0, 1, 7, 2048, 2049, 1 << 20)


def arc_counts(S, w):
    a = (64 * 1024 - 16 * S - 128 - 4 * (S + 2) - w) // (8 + w)
    return sorted(v for v in {0, 1, S, 12 * S, a, a + 1} if v >= 0)


def closure_sizes(S):
    return sorted({v for v in (-1, 0, 1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40, 64, 65, 128, 129, 256, 257, 300, 4095,
                               4096, S, S + 1) if v <= S + 1})


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 0)):
            for A in arc_counts(S, w or 4):
                for n_cat in CATS:
                    for M in closure_sizes(S):
                        want = st.route_formula(S, A, w, n_cat, M)
                        assert route(desc(S, A), dtype, n_cat, M) == want, (S, A, dtype, n_cat, M)
                        seen.add(want)
    # every combination of the two bits with every team size, and the refusal
    assert {r & ~0xF for r in seen if r != _hip.EINVAL} == {K | a | b for a in (0, L) for b in (0, BL)}
    assert {_hip.segments_team(r) for r in seen if r != _hip.EINVAL} == {4, 8, 16, 32, 64, 128, 256}
    assert _hip.EINVAL in seen


def test_route_thresholds_sit_where_the_header_says():
    assert route(desc(120, 1800), F32, 40, 3) == K | L | BL | 2           # config 3's loop
    assert route(desc(9, 30), F64, 3, 4) == K | L | BL | 2
    assert route(desc(9, 30), F64, 3, 5) == K | L | BL | 3
    assert route(desc(300, 900), F64, 3, 64) == K | L | BL | 6
    assert route(desc(300, 900), F64, 3, 65) == K | L | BL | 7
    assert route(desc(300, 900), F64, 3, 256) == K | L | BL | 8
    assert route(desc(300, 900), F64, 3, 300) == K | L | BL | 8            # strided lanes
    assert route(desc(300, 900), F64, 3, 301) == _hip.EINVAL               # more than the graph
    assert route(desc(300, 900), F64, 3, -1) == _hip.EINVAL
    assert route(desc(5000, 900), F64, 3, 4095) == K | BL | 8
    assert route(desc(5000, 900), F64, 3, 4096) == _hip.EINVAL             # two rows above 64 KiB
    # the trellis kernel's form is max_marginals' with the frames asked for
    mm = _hip.lib().beer_hmm_maxmarg_route
    for S, A in ((120, 1800), (300, 4949), (300, 4950), (100, 10000), (6136, 9), (6137, 9),
                 (10232, 9), (10233, 9), (32768, 9), (0, 0)):
        for dtype in (F32, F64, 7):
            for n_cat in (0, 1, 2048, 2049):
                b = desc(S, A)
                got, want = route(b, dtype, n_cat), mm(dtype, ctypes.byref(b), n_cat, 0, 1, 0)
                if want == _hip.EINVAL:
                    assert got == _hip.EINVAL, (S, A, dtype, n_cat)
                else:
                    assert got == (want & 0xF00) | K | 2, (S, A, dtype, n_cat)
    assert route(None, F64, 3) == _hip.EINVAL
    scratch = _hip.lib().beer_hmm_segments_scratch_doubles
    assert scratch(F64, ctypes.byref(desc(256, 9, nutt=5))) == 0
    assert scratch(F32, ctypes.byref(desc(257, 9, nutt=5))) == 5 * 257
    assert scratch(F64, ctypes.byref(desc(10233, 9, nutt=5))) == 0 and scratch(F64, None) == 0


def test_the_entry_points_refuse_before_they_launch():
    lib = _hip.lib()
    one = ctypes.c_void_p(16)                # (never dereferenced: every call below is refused)
    good = _hip.ArcMap(one, one, one, one)
    ok = desc(8, 16)

    def trellis(dtype, b, n_cat, amap, d=one, x=one, ws=one, frame=one, best=one, pc=one):
        return lib.beer_hmm_segment_trellis(dtype, ctypes.byref(b) if b is not None else None, pc,
                                            ctypes.byref(amap) if amap is not None else None,
                                            n_cat, d, x, ws, frame, best, None)
    assert trellis(7, ok, 3, good) == _hip.EINVAL
    assert trellis(F64, None, 3, good) == _hip.EINVAL
    assert trellis(F64, desc(32768, 8), 3, good) == _hip.EINVAL
    assert trellis(F64, desc(10233, 8), 3, good) == _hip.EINVAL
    assert trellis(F32, ok, 0, good) == _hip.EINVAL
    assert trellis(F32, ok, 3, None) == _hip.EINVAL
    for k in range(4):
        members = [one] * 4
        members[k] = None
        assert trellis(F32, ok, 3, _hip.ArcMap(*members)) == _hip.EINVAL, k
    for kw in ('d', 'x', 'frame', 'best', 'pc'):
        assert trellis(F32, ok, 3, good, **{kw: None}) == _hip.EINVAL, kw
    assert trellis(F32, desc(300, 16), 3, good, ws=None) == _hip.EINVAL
    empty = desc(8, 16, nutt=0)
    assert trellis(F32, empty, 3, good, d=None, x=None, ws=None, frame=None, best=None, pc=None) == 0

    def smap(max_closure, **null):
        return _hip.SegMap(*[None if f in null else one for f in hk.SegmentMap.FIELDS],
                           max_closure, 0)

    def margins(dtype, b, n_cat, sm, n_entries=5, max_dur=4, **null):
        args = {k: None if k in null else one
                for k in ('pc', 'd', 'x', 'best', 'frame', 'cat', 'off', 'out')}
        return lib.beer_hmm_segment_margins(
            dtype, ctypes.byref(b) if b is not None else None, args['pc'],
            ctypes.byref(sm) if sm is not None else None, n_cat, args['d'], args['x'],
            args['best'], args['frame'], args['cat'], args['off'], n_entries, max_dur, args['out'],
            None)
    assert margins(7, ok, 3, smap(3)) == _hip.EINVAL
    assert margins(F64, None, 3, smap(3)) == _hip.EINVAL
    assert margins(F64, ok, 3, None) == _hip.EINVAL
    assert margins(F64, ok, 0, smap(3)) == _hip.EINVAL
    assert margins(F64, ok, 3, smap(9)) == _hip.EINVAL                       # more than max_states
    assert margins(F64, ok, 3, smap(-1)) == _hip.EINVAL
    assert margins(F64, desc(5000, 9), 3, smap(4096)) == _hip.EINVAL
    assert margins(F64, ok, 3, smap(3), n_entries=-1) == _hip.EINVAL
    assert margins(F64, ok, 3, smap(3), max_dur=0) == _hip.EINVAL
    for f in hk.SegmentMap.FIELDS:
        assert margins(F64, ok, 3, smap(3, **{f: 1})) == _hip.EINVAL, f
    for k in ('pc', 'd', 'x', 'best', 'frame', 'cat', 'off', 'out'):
        assert margins(F64, ok, 3, smap(3), **{k: 1}) == _hip.EINVAL, k
    # no entry, or no utterance: no error, nothing launched
    assert margins(F64, ok, 3, smap(3), n_entries=0, pc=1, out=1) == 0
    assert margins(F32, empty, 3, smap(3), pc=1, out=1) == 0


# --- errors raised on the host ----------------------------------------------------------------

class NoDevice(SimpleNamespace):
    'A batch of two graphs that fails the test as soon as anything but its counts is read.'

    def __getattr__(self, name):
        raise AssertionError(f'batch.{name} was read: device work before the arguments were checked')


def test_arguments_are_refused_before_any_device_work():
    batch = NoDevice(n_arcs=[5, 3], n_states=[2, 2])
    arcs = [np.zeros(5, np.int32), np.array([0, 1, -1], np.int32)]
    inits = [np.zeros(2, np.int32), np.array([2, -1], np.int32)]
    for beam in (-1., float('nan'), -1e-9, float('-inf')):
        with pytest.raises(ValueError, match='beam'):
            hk.segment_margins(batch, None, arcs, inits, 3, beam, 5)
    for max_dur in (0, -3, 2.5, None):
        with pytest.raises(ValueError, match='max_dur'):
            hk.segment_margins(batch, None, arcs, inits, 3, 10., max_dur)
    for bad_a, bad_i, n_cat in ((arcs, inits, 2), (arcs, inits, 0), (arcs[:1], inits, 3),
                                ([arcs[0], np.array([0, -2, 1])], inits, 3),
                                (arcs, [inits[0], np.zeros(3, np.int32)], 3),
                                (torch.zeros(8), inits, 3)):
        with pytest.raises(ValueError, match='arc_posteriors'):      # (check_arc_categories)
            hk.segment_margins(batch, None, bad_a, bad_i, n_cat, 10., 5)
        with pytest.raises(ValueError):
            hk.segment_map([(np.zeros(5, int), np.zeros(5, int), 2),
                            (np.zeros(3, int), np.zeros(3, int), 2)], bad_a, bad_i, n_cat)
    assert hk.check_segments(float('inf'), 7) == (float('inf'), 7)
    assert hk.check_segments(0, None) == (0., None)


def small_model():
    g, _, _ = st.loop_graph([2, 2])
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2, 3])
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=4, noise_std=1.)
    return beer.HMM.create(graph, ns), graph


def test_model_arguments_are_refused_without_a_device():
    model, graph = small_model()
    X = torch.randn(7, 2)
    loop = NoDevice()                        # (a phone loop of which nothing may be read)
    for kw in (dict(beam=-1.), dict(beam=float('nan')), dict(max_dur=0), dict(max_dur=-2)):
        with pytest.raises(ValueError, match='unit_segments'):
            beer.PhoneLoop.unit_segments(loop, X, **kw)
        with pytest.raises(ValueError, match='unit_segments_batch'):
            beer.unit_segments_batch(loop, [X], **kw)
    for utts, graphs in (([X, X], [graph]), ([X], [graph, graph]),
                         ((torch.cat([X, X]), [7, 7]), []), (iter([X, X]), [graph] * 3)):
        with pytest.raises(ValueError, match='inference graphs'):
            beer.unit_segments_batch(model, utts, inference_graphs=graphs)
    with pytest.raises(ValueError, match='phone loop'):
        beer.unit_segments_batch(model, [X])                 # a plain HMM has no units


# --- the command line ---------------------------------------------------------------------------

def test_the_lattice_parser_takes_the_segment_options():
    assert hmm_cmds.COMMANDS[-1] is hmm_cmds.boundaries
    assert [c.__name__ for c in hmm_cmds.COMMANDS].count('lattice') == 1
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'lattice', '--segments', '--max-dur', '25', '--beam', '2.5',
                              'mdl', 'ds', 'out'])
    assert (args.segments, args.max_dur, args.beam) == (True, 25, 2.5)
    assert args.func is hmm_cmds.lattice.main
    args = parser.parse_args(['hmm', 'lattice', 'mdl', 'ds', 'out'])
    assert (args.segments, args.max_dur, args.beam) == (False, 100, 10.)
    with pytest.raises(SystemExit):
        parser.parse_args(['hmm', 'lattice', '--max-dur', '2.5', 'mdl', 'ds', 'out'])


@pytest.mark.parametrize('max_dur', ['0', '-1'])
def test_a_bad_max_dur_is_refused_before_the_model_is_opened(max_dur, tmp_path):
    out = tmp_path / 'never'
    for more in ([], ['--segments']):
        with pytest.raises(SystemExit, match='--max-dur'):
            # (the model and the data set do not exist: they are never opened)
            cli_main.main(['hmm', 'lattice', '--max-dur=' + max_dur, *more,
                           str(tmp_path / 'no.mdl'), str(tmp_path / 'no.ds'), str(out)])
    assert not out.exists()
