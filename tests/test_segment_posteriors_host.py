"""CPU checks of the segment posteriors: the truth of tests/segposts_truth.py itself (its recursion
against the enumeration of all paths within 1e-12, its two identities, the duration histogram),
the C symbols and the Python names, `beer_hmm_segposts_route` against a Python restatement of the
header's formula on a grid that crosses its thresholds, the refusals of the C entry points, the
argument errors raised before any device work, and the `segments` command's refusals."""

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arcs_truth as at
import evidence_truth as et
import segposts_truth as sp
from helpers import ROOT

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main

F32, F64 = _hip.F32, _hip.F64
K, L, BL = sp.BLOCK, sp.ARCS_LDS, sp.BINS_LDS


# --- the truth itself ---------------------------------------------------------------------------

def holes(g, arc_cat, init_cat, seed):
    'The graph with an arc, an initial and a final state removed (-inf), and its categories.'
    rng = np.random.RandomState(seed)
    src, dst = sp.out_arcs(g)
    gone = rng.randint(len(src))
    trans = g['trans'].copy()
    trans[src[gone], dst[gone]] = -np.inf
    init, final = g['init'].copy(), g['final'].copy()
    fin = np.nonzero(np.isfinite(init))[0]
    if len(fin) > 1:
        init[fin[rng.randint(len(fin))]] = -np.inf
    fin = np.nonzero(np.isfinite(final))[0]
    if len(fin) > 1:
        final[fin[rng.randint(len(fin))]] = -np.inf
    return dict(g, trans=trans, init=init, final=final), np.delete(arc_cat, gone), init_cat


def enumerated():
    'Graphs of at most 5 states with their lengths (at most 6 frames): (name, graph, cats, n_cat, T).'
    out = []
    for T in (1, 2, 5):
        out.append((f'loop221-T{T}', *split(sp.loop_graph([2, 2, 1], seed=T, open_end=True, real=True)), 3, T))
    out.append(('loop131-skip', *split(sp.loop_graph([1, 3, 1], seed=4, skips=(1, 2), real=True)), 3, 6))
    out.append(('loop23-holes', *split(holes(*sp.loop_graph([2, 3], seed=5, open_end=True, real=True), 6)), 2, 5))
    out.append(('loop1111-holes', *split(holes(*sp.loop_graph([1, 1, 1, 1], seed=7, real=True), 8)), 4, 6))
    # a unit that repeats: the closure of category 1 is the union of its two instances
    out.append(('chain101', *split(sp.chain_graph([1, 0, 1], 1, seed=2, real=True)), 2, 6))
    out.append(('chain1012', *split(sp.chain_graph([1, 0, 1, 2], 1, seed=3, real=True)), 3, 6))
    out.append(('chain10-2', *split(sp.chain_graph([1, 0], 2, seed=3, real=True)), 2, 1))     # dead: T = 1
    return out


def split(built):
    return built[0], (built[1], built[2])


ENUMERATED = enumerated()


def inputs(g, T, seed, with_holes=True):
    rng = np.random.RandomState(seed)
    llh = rng.randn(T, g['S']) * 2.5
    if with_holes and T > 2:
        llh[rng.rand(T, g['S']) < .12] = -np.inf
    return llh


@pytest.mark.parametrize('name,g,cats,n_cat,T', ENUMERATED, ids=[e[0] for e in ENUMERATED])
def test_the_recursion_is_the_enumeration(name, g, cats, n_cat, T):
    assert g['S'] <= 5 and T <= 6
    llh = inputs(g, T, len(name))
    worst = 0.
    for max_dur in (1, 2, T, T + 2):
        post, starts, evidence = sp.segment_posteriors(g, llh, *cats, n_cat, max_dur)
        bpost, bstarts, bevidence = sp.brute_force(g, llh, *cats, n_cat, max_dur)
        assert post.shape == (T, n_cat, max_dur) and not np.isnan(post).any()
        worst = max(worst, np.abs(post - bpost).max(), np.abs(starts - bstarts).max())
        if np.isfinite(bevidence):
            worst = max(worst, abs(evidence - bevidence) / (1. + abs(bevidence)))
            assert abs(evidence - et.brute_force(g, llh)) <= 1e-12 * (1. + abs(bevidence))
        else:
            assert evidence == -np.inf and not post.any() and not starts.any()
        # the start posteriors are those of the arc posteriors' own truth
        assert np.abs(starts - at.arc_posteriors(g, llh, *cats, n_cat)[0]).max() <= 1e-12
    print(f'{name}: the recursion within {worst:.2e} of the enumeration')
    assert worst <= 1e-12


def test_the_enumerated_cases_hold_what_they_should():
    names = [e[0] for e in ENUMERATED]
    assert {e[4] for e in ENUMERATED} >= {1, 2, 5, 6}
    g, cats = ENUMERATED[names.index('loop23-holes')][1:3]
    assert np.isinf(g['init']).any() and np.isinf(g['final']).any()
    g, cats, n_cat = ENUMERATED[names.index('chain101')][1:4]
    assert [len(c) for c in sp.closures(g, *cats, n_cat)] == [1, 2]      # the union of two instances
    dead = ENUMERATED[names.index('chain10-2')]
    assert sp.segment_posteriors(dead[1], inputs(dead[1], 1, 0), *dead[2], 2, 3)[2] == -np.inf


@pytest.mark.parametrize('sizes,T', [((3, 3, 3), 17), ((1, 2, 5), 12), ((2, 2), 1), ((4, 1, 2), 2)])
def test_the_two_identities_and_the_histogram(sizes, T):
    g, arc_cat, init_cat = sp.loop_graph(list(sizes), seed=T, skips=(1, 2), open_end=True, real=True)
    n_cat = len(sizes)
    llh = inputs(g, T, 3 * T)
    post, starts, evidence = sp.segment_posteriors(g, llh, arc_cat, init_cat, n_cat, T)
    assert np.isfinite(evidence)
    # sum_e post(c, s, e) is the start posterior; every frame is covered with probability 1 (every
    # initial state of a phone loop has a category)
    assert np.abs(post.sum(2) - starts).max() <= 1e-12
    mass, count = sp.coverage(post)
    assert np.abs(mass - 1.).max() <= 1e-12 and (count >= 1).all()
    assert abs(evidence - et.evidence(g, llh)[1]) <= 1e-12 * (1. + abs(evidence))
    # the rows of the duration histogram sum to the expected unit counts
    hist = sp.durations(post)
    assert hist.shape == (n_cat, T)
    assert np.abs(hist.sum(1) - at.arc_posteriors(g, llh, arc_cat, init_cat, n_cat)[1]).max() <= 1e-12
    # a shorter max_dur cuts columns and nothing else
    for max_dur in (1, 2, T + 2):
        cut = sp.segment_posteriors(g, llh, arc_cat, init_cat, n_cat, max_dur)[0]
        k = min(max_dur, T)
        assert np.array_equal(cut[:, :, :k], post[:, :, :k]) and not cut[:, :, k:].any()


# --- the symbols --------------------------------------------------------------------------------

def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the queries may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def route(b, dtype, n_cat, max_closure=0):
    return _hip.lib().beer_hmm_segposts_route(dtype, ctypes.byref(b) if b is not None else None,
                                              n_cat, max_closure)


def test_symbols_are_declared_exported_and_in_the_ctypes_tables():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('beer_hmm_segpost_trellis', 'beer_hmm_segment_posteriors', 'beer_hmm_segposts_route'):
        assert re.search(r'^int %s\(' % name, text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
    p, i = _hip.c_p, _hip.c_i
    assert _hip.SIGNATURES['beer_hmm_segpost_trellis'] == [i, p, p, p, i] + [p] * 6
    assert _hip.SIGNATURES['beer_hmm_segment_posteriors'] == \
        [i, p, p, p, i] + [p] * 7 + [_hip.c_l, i, p, p]
    assert _hip.SIGNATURES['beer_hmm_segposts_route'] == [i, p, i, i]
    for name, value in (('BEER_SEGPOSTS_BLOCK', _hip.SEGPOSTS_BLOCK),
                        ('BEER_SEGPOSTS_ARCS_LDS', _hip.SEGPOSTS_ARCS_LDS),
                        ('BEER_SEGPOSTS_BINS_LDS', _hip.SEGPOSTS_BINS_LDS)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % name, text).group(1), 16) == value
    assert (K, L, BL) == (_hip.SEGPOSTS_BLOCK, _hip.SEGPOSTS_ARCS_LDS, _hip.SEGPOSTS_BINS_LDS)
    assert _hip.segposts_family(K | L | 5) == K and _hip.segposts_team(K | L | 5) == 32
    for name in ('segment_posteriors', 'segposts_route', 'segments_above', 'check_segment_posteriors'):
        assert name in hk.__all__ and callable(getattr(hk, name))
    for name in ('unit_segment_posteriors_batch', 'unit_durations_batch'):
        assert name in beer.inference.batch.__all__ and hasattr(beer, name)
    for name in ('unit_segment_posteriors', 'unit_durations'):
        assert getattr(beer.PhoneLoop, name) is getattr(beer.BigramPhoneLoop, name)
        assert not hasattr(beer.HMM, name)


# --- the route ----------------------------------------------------------------------------------
STATES = (1, 2, 64, 256, 257, 300, 2000, 2046, 2047, 4096, 6136, 6137, 10232, 10233, 32767, 32768)
CATS = (-3, 0, 1, 7, 1024, 1025, 1 << 20)


def arc_counts(S, w):
    a = (64 * 1024 - 16 * S - 128 - 4 * (S + 2) - w) // (8 + w)
    return sorted(v for v in {0, 1, S, 12 * S, a, a + 1} if v >= 0)


def closure_sizes(S):
    return sorted({v for v in (-1, 0, 1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40, 64, 65, 128, 129, 256, 257, 300,
                               510, 511, 1022, 1023, 2046, 2047, S, S + 1) if v <= S + 1})


def test_route_is_the_headers_formula():
    seen = set()
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 0)):
            for A in arc_counts(S, w or 4):
                for n_cat in CATS:
                    for M in closure_sizes(S):
                        want = sp.route_formula(S, A, w, n_cat, M)
                        assert route(desc(S, A), dtype, n_cat, M) == want, (S, A, dtype, n_cat, M)
                        seen.add(want)
    # every combination of the two bits with every team size, and the refusal
    assert {r & ~0xF for r in seen if r != _hip.EINVAL} == {K | a | b for a in (0, L) for b in (0, BL)}
    assert {_hip.segposts_team(r) for r in seen if r != _hip.EINVAL} == {4, 8, 16, 32, 64, 128, 256}
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
    # the team's LDS: (256 / L) (32 max_closure + 64) bytes within 64 KiB
    assert route(desc(5000, 900), F64, 3, 2046) == K | BL | 8
    assert route(desc(5000, 900), F64, 3, 2047) == _hip.EINVAL
    assert route(desc(5000, 900), F64, 3, 128) == K | BL | 7              # 2 teams x 4160 bytes
    # the trellis kernel's form is arc_posteriors' with the frames asked for
    arcs = _hip.lib().beer_hmm_arcs_route
    for S, A in ((120, 1800), (300, 4949), (300, 4950), (100, 10000), (6136, 9), (6137, 9),
                 (10232, 9), (10233, 9), (32768, 9), (0, 0)):
        for dtype in (F32, F64, 7):
            for n_cat in (0, 1, 1024, 1025):
                b = desc(S, A)
                got, want = route(b, dtype, n_cat), arcs(dtype, ctypes.byref(b), n_cat, 1)
                if want == _hip.EINVAL:
                    assert got == _hip.EINVAL, (S, A, dtype, n_cat)
                else:
                    assert got == (want & (_hip.ARCS_ARCS_LDS | _hip.ARCS_FRAME_LDS)) | K | 2, \
                        (S, A, dtype, n_cat)
    assert route(None, F64, 3) == _hip.EINVAL


def test_the_entry_points_refuse_before_they_launch():
    lib = _hip.lib()
    one = ctypes.c_void_p(16)                # (never dereferenced: every call below is refused)
    good = _hip.ArcMap(one, one, one, one)
    ok = desc(8, 16)

    def trellis(dtype, b, n_cat, amap, **null):
        a = {k: None if k in null else one for k in ('pc', 'alpha', 'y', 'norm', 'frame', 'evidence')}
        return lib.beer_hmm_segpost_trellis(dtype, ctypes.byref(b) if b is not None else None, a['pc'],
                                            ctypes.byref(amap) if amap is not None else None,
                                            n_cat, a['alpha'], a['y'], a['norm'], a['frame'],
                                            a['evidence'], None)
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
    for kw in ('pc', 'alpha', 'y', 'norm', 'frame', 'evidence'):
        assert trellis(F32, ok, 3, good, **{kw: 1}) == _hip.EINVAL, kw
    empty = desc(8, 16, nutt=0)
    assert trellis(F32, empty, 3, good, pc=1, alpha=1, y=1, norm=1, frame=1, evidence=1) == 0

    def smap(max_closure, **null):
        return _hip.SegMap(*[None if f in null else one for f in hk.SegmentMap.FIELDS],
                           max_closure, 0)

    names = ('pc', 'alpha', 'y', 'norm', 'evidence', 'frame', 'cat', 'off', 'out')

    def expand(dtype, b, n_cat, sm, n_entries=5, max_dur=4, **null):
        a = {k: None if k in null else one for k in names}
        return lib.beer_hmm_segment_posteriors(
            dtype, ctypes.byref(b) if b is not None else None, a['pc'],
            ctypes.byref(sm) if sm is not None else None, n_cat, a['alpha'], a['y'], a['norm'],
            a['evidence'], a['frame'], a['cat'], a['off'], n_entries, max_dur, a['out'], None)
    assert expand(7, ok, 3, smap(3)) == _hip.EINVAL
    assert expand(F64, None, 3, smap(3)) == _hip.EINVAL
    assert expand(F64, ok, 3, None) == _hip.EINVAL
    assert expand(F64, ok, 0, smap(3)) == _hip.EINVAL
    assert expand(F64, ok, 3, smap(9)) == _hip.EINVAL                        # more than max_states
    assert expand(F64, ok, 3, smap(-1)) == _hip.EINVAL
    assert expand(F64, desc(5000, 9), 3, smap(2047)) == _hip.EINVAL          # the team's LDS
    assert expand(F64, ok, 3, smap(3), n_entries=-1) == _hip.EINVAL
    assert expand(F64, ok, 3, smap(3), max_dur=0) == _hip.EINVAL
    for f in hk.SegmentMap.FIELDS:
        assert expand(F64, ok, 3, smap(3, **{f: 1})) == _hip.EINVAL, f
        assert expand(F64, ok, 3, smap(3, **{f: 1}), n_entries=0) == _hip.EINVAL, f
    for k in names:
        assert expand(F64, ok, 3, smap(3), **{k: 1}) == _hip.EINVAL, k
    # no entry, or no utterance: no error, nothing launched
    assert expand(F64, ok, 3, smap(3), n_entries=0, pc=1, out=1) == 0
    assert expand(F32, empty, 3, smap(3), pc=1, out=1) == 0


# --- errors raised on the host ----------------------------------------------------------------

class NoDevice(SimpleNamespace):
    'A batch of two graphs that fails the test as soon as anything but its counts is read.'

    def __getattr__(self, name):
        raise AssertionError(f'batch.{name} was read: device work before the arguments were checked')


def test_arguments_are_refused_before_any_device_work():
    batch = NoDevice(n_arcs=[5, 3], n_states=[2, 2], n_frames=20)
    arcs = [np.zeros(5, np.int32), np.array([0, 1, -1], np.int32)]
    inits = [np.zeros(2, np.int32), np.array([2, -1], np.int32)]
    for min_post in (-1., float('nan'), -1e-9, 1.0001, float('inf')):
        with pytest.raises(ValueError, match='min_post'):
            hk.segment_posteriors(batch, None, arcs, inits, 3, min_post, 5)
    for max_dur in (0, -3, 2.5, None):
        with pytest.raises(ValueError, match='max_dur'):
            hk.segment_posteriors(batch, None, arcs, inits, 3, .1, max_dur)
    for bad_a, bad_i, n_cat in ((arcs, inits, 2), (arcs, inits, 0), (arcs[:1], inits, 3),
                                ([arcs[0], np.array([0, -2, 1])], inits, 3),
                                (arcs, [inits[0], np.zeros(3, np.int32)], 3),
                                (torch.zeros(8), inits, 3)):
        with pytest.raises(ValueError, match='arc_posteriors'):      # (check_arc_categories)
            hk.segment_posteriors(batch, None, bad_a, bad_i, n_cat, .1, 5)
    graphs = [(np.array([0, 0, 1, 1, 1]), np.array([0, 1, 0, 1, 1]), 2),
              (np.array([0, 0, 1]), np.array([0, 1, 1]), 2)]
    with pytest.raises(ValueError, match='segment map'):
        hk.segment_posteriors(batch, None, arcs, inits, 3, .1, 5,
                              seg_map=hk.segment_map(graphs, arcs, inits, 4))
    with pytest.raises(ValueError, match='segment map'):
        hk.segment_posteriors(batch, None, arcs, inits, 3, .1, 5,
                              seg_map=hk.segment_map(graphs[:1], arcs[:1], inits[:1], 3))
    smap = hk.segment_map(graphs, arcs, inits, 3)
    for frames, cats, why in (([3, 2], [0, 0], 'sorted'), ([0, 20], [0, 0], 'outside'),
                              ([-1, 2], [0, 0], 'outside'), ([0, 2], [0, 3], 'outside'),
                              ([0, 2], [-1, 0], 'outside'), ([0, 2], [0], 'one length'),
                              ([0., 2.], [0, 0], 'integers')):
        with pytest.raises(ValueError, match=why):
            hk.segment_posteriors(batch, None, arcs, inits, 3, .1, 5, seg_map=smap,
                                  entries=(torch.tensor(frames), torch.tensor(cats)))
    with pytest.raises(ValueError, match='pair'):
        hk.segment_posteriors(batch, None, arcs, inits, 3, .1, 5, seg_map=smap,
                              entries=torch.zeros(3, dtype=torch.int64))
    assert hk.check_segment_posteriors(1, 7) == (1., 7)
    assert hk.check_segment_posteriors(0, None) == (0., None)


def test_model_arguments_are_refused_without_a_device():
    g, _, _ = sp.loop_graph([2, 2])
    tt = torch.from_numpy
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2, 3])
    model = beer.HMM.create(graph, beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=4,
                                                         noise_std=1.))
    X = torch.randn(7, 2)
    loop = NoDevice()                        # (a phone loop of which nothing may be read)
    for kw in (dict(min_post=-1.), dict(min_post=float('nan')), dict(min_post=1.5), dict(max_dur=0),
               dict(max_dur=-2)):
        with pytest.raises(ValueError, match='unit_segment_posteriors'):
            beer.PhoneLoop.unit_segment_posteriors(loop, X, **kw)
        with pytest.raises(ValueError, match='unit_segment_posteriors_batch'):
            beer.unit_segment_posteriors_batch(loop, [X], **kw)
    for max_dur in (0, -2, 2.5, None):
        with pytest.raises(ValueError, match='unit_durations_batch'):
            beer.unit_durations_batch(loop, [X], max_dur)
    with pytest.raises(ValueError, match='unit_durations'):
        beer.PhoneLoop.unit_durations(loop, X, max_dur=0)
    for utts, graphs in (([X, X], [graph]), ([X], [graph, graph]),
                         ((torch.cat([X, X]), [7, 7]), []), (iter([X, X]), [graph] * 3)):
        with pytest.raises(ValueError, match='inference graphs'):
            beer.unit_segment_posteriors_batch(model, utts, inference_graphs=graphs)
        with pytest.raises(ValueError, match='inference graphs'):
            beer.unit_durations_batch(model, utts, 5, inference_graphs=graphs)
    with pytest.raises(ValueError, match='phone loop'):
        beer.unit_segment_posteriors_batch(model, [X])       # a plain HMM has no units
    with pytest.raises(ValueError, match='phone loop'):
        beer.unit_durations_batch(model, [X], 5)


# --- the command line ---------------------------------------------------------------------------

def test_the_segments_parser():
    assert [c.__name__ for c in hmm_cmds.COMMANDS].count('segments') == 1
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'segments', '--min-post', '0.05', '--max-dur', '25', '--durations',
                              'd.npy', '-s', '0.5', 'mdl', 'ds', 'out'])
    assert (args.min_post, args.max_dur, args.durations, args.acoustic_scale) == (.05, 25, 'd.npy', .5)
    assert args.func is hmm_cmds.segments.main
    args = parser.parse_args(['hmm', 'segments', 'mdl', 'ds', 'out'])
    assert (args.min_post, args.max_dur, args.durations, args.alis, args.utts) == (1e-3, None, None, None, None)
    with pytest.raises(SystemExit):
        parser.parse_args(['hmm', 'segments', '--max-dur', '2.5', 'mdl', 'ds', 'out'])
    # `lattice` stays as it is
    args = parser.parse_args(['hmm', 'lattice', 'mdl', 'ds', 'out'])
    assert (args.segments, args.max_dur, args.beam) == (False, 100, 10.)


@pytest.mark.parametrize('bad,flag', [(['--max-dur=0'], '--max-dur'), (['--max-dur=-1'], '--max-dur'),
                                      (['--min-post=-0.1'], '--min-post'), (['--min-post=1.5'], '--min-post'),
                                      (['--min-post=nan'], '--min-post'),
                                      (['--durations=d.npy'], '--durations')])
def test_bad_values_are_refused_before_the_model_is_opened(bad, flag, tmp_path):
    out = tmp_path / 'never'
    with pytest.raises(SystemExit, match=flag):
        # (the model and the data set do not exist: they are never opened)
        cli_main.main(['hmm', 'segments', *bad, str(tmp_path / 'no.mdl'), str(tmp_path / 'no.ds'),
                       str(out)])
    assert not out.exists() and not (tmp_path / 'd.npy').exists()
