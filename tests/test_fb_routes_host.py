"""CPU checks of the forward-backward dispatch: `beer_hmm_fb_route` on hand-built descriptors on
both sides of every boundary, the case tables of tests/test_gpu_fb_routes.py (every kernel family
named, every case's expected route what the generator's graph gives, enough Viterbi ties), and
the truth of tests/fb_truth.py against the identities it must satisfy."""

import ctypes
import os
import re

import numpy as np
import pytest

import fb_truth as ft
from helpers import ROOT
import test_gpu_fb_routes as table
from test_gpu_fb_routes import BIG, GENERAL, LOWDEG, WAVE, wave

from beer_amd import _hip

F32, F64 = _hip.F32, _hip.F64


def desc(max_states, max_degree=3, all_lowdeg=1, max_hubs=0, members=0, max_arcs=None,
         max_segs=None, nutt=3):
    'A beer_batch with only its scalar fields filled: all the query may read.'
    arcs = max_arcs if max_arcs is not None else max_states * max(max_degree, 1)
    return _hip.Batch(nutt, max_states, max(arcs, 1), max(max_segs or max_states, 1), all_lowdeg, 1,
                      None, None, None, None, None, None, max_degree, max_hubs, members, 0, None)


def route(b, dtype=F64, want_xi=0, have_flow=None):
    have_flow = want_xi if have_flow is None else have_flow
    return _hip.lib().beer_hmm_fb_route(dtype, ctypes.byref(b) if b is not None else None,
                                        want_xi, have_flow)


BOUNDARIES = [
    # states: 64|65, 128|129, 256|257, 512|513
    (dict(max_states=1), wave(1, 4)), (dict(max_states=64), wave(1, 4)),
    (dict(max_states=65), wave(2, 4)), (dict(max_states=128), wave(2, 4)),
    (dict(max_states=129), wave(4, 4)), (dict(max_states=256), wave(4, 4)),
    (dict(max_states=257), LOWDEG | 512), (dict(max_states=512), LOWDEG | 512),
    (dict(max_states=513), GENERAL),
    # degree: 2|3, 4|5, 8|9; 0 is "unknown" and a graph of 9 arcs a state has no image at all
    (dict(max_states=64, max_degree=1), wave(1, 2)), (dict(max_states=64, max_degree=2), wave(1, 2)),
    (dict(max_states=64, max_degree=3), wave(1, 4)), (dict(max_states=64, max_degree=4), wave(1, 4)),
    (dict(max_states=64, max_degree=5), wave(1, 8)), (dict(max_states=64, max_degree=8), wave(1, 8)),
    (dict(max_states=64, max_degree=9), LOWDEG | 128), (dict(max_states=64, max_degree=0), LOWDEG | 128),
    (dict(max_states=64, max_degree=9, all_lowdeg=0), GENERAL),
    (dict(max_states=256, max_degree=8), wave(4, 8)), (dict(max_states=256, max_degree=9), LOWDEG | 256),
    # one hub of 64|65 members a side; a second hub
    (dict(max_states=130, max_hubs=1, members=64), wave(4, 4)),
    (dict(max_states=130, max_hubs=1, members=65), LOWDEG | 256),
    (dict(max_states=130, max_hubs=2, members=3), LOWDEG | 256),
    # the workgroup of the one-thread-per-state kernel: 128|129, 256|257 states
    (dict(max_states=128, max_hubs=1, members=65), LOWDEG | 128),
    (dict(max_states=129, max_hubs=1, members=65), LOWDEG | 256),
    (dict(max_states=256, max_hubs=1, members=65), LOWDEG | 256),
    (dict(max_states=257, max_hubs=1, members=65), LOWDEG | 512),
    (dict(max_states=512, max_hubs=1, members=65), LOWDEG | 512),
    (dict(max_states=513, max_hubs=1, members=65), GENERAL),
    # without a low-degree image for every graph: the general kernel at any size
    (dict(max_states=1, all_lowdeg=0), GENERAL), (dict(max_states=64, all_lowdeg=0), GENERAL),
    (dict(max_states=257, all_lowdeg=0), GENERAL), (dict(max_states=700, all_lowdeg=0), GENERAL),
    # arc lists beyond a CU's LDS (a dense graph of 100 states), per-state arrays beyond it
    (dict(max_states=100, all_lowdeg=0, max_degree=0, max_arcs=10000, max_segs=1300), BIG),
    (dict(max_states=3000, all_lowdeg=0, max_degree=0, max_arcs=200000, max_segs=30000), BIG),
    (dict(max_states=32767, all_lowdeg=0, max_degree=0, max_arcs=100000, max_segs=40000), _hip.EINVAL),
    (dict(max_states=0), _hip.EINVAL), (dict(max_states=32768, all_lowdeg=0), _hip.EINVAL),
    (dict(max_states=64, nutt=-1), _hip.EINVAL),
]


@pytest.mark.parametrize('fields,want', BOUNDARIES, ids=[str(i) for i in range(len(BOUNDARIES))])
def test_route_on_both_sides_of_every_boundary(fields, want):
    for dtype in (F32, F64):
        for want_xi in (0, 1):
            assert route(desc(**fields), dtype, want_xi) == want, (fields, dtype, want_xi)
    assert route(desc(**fields), 7) == _hip.EINVAL
    # an empty batch launches nothing but is routed like any other
    if want != _hip.EINVAL:
        assert route(desc(**dict(fields, nutt=0))) == want


def test_route_values_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    values = {m.group(1): int(m.group(2), 16)
              for m in re.finditer(r'#define\s+BEER_FB_(\w+)\s+(0x[0-9A-Fa-f]+)', text)}
    assert values == dict(WAVE=_hip.FB_WAVE, LOWDEG=_hip.FB_LOWDEG, GENERAL=_hip.FB_GENERAL,
                          GENERAL_BIG=_hip.FB_GENERAL_BIG)
    assert re.search(r'#define\s+BEER_FB_FAMILY\(route\)\s+\(\(route\) & 0xF000\)', text)
    assert _hip.fb_family(wave(4, 8)) == WAVE and _hip.fb_family(LOWDEG | 512) == LOWDEG
    assert _hip.SIGNATURES['beer_hmm_fb_route'] == [_hip.c_i, _hip.c_p, _hip.c_i, _hip.c_i]


def test_route_without_hub_flow_leaves_the_factorised_kernels():
    'Transition posteriors through a hub have nowhere to go without `hub_flow`: the general kernel.'
    for S in (64, 300):
        assert _hip.fb_family(route(desc(S), F64, 1, 1)) in (WAVE, LOWDEG)
        assert route(desc(S), F64, 1, 0) == GENERAL
        assert _hip.fb_family(route(desc(S), F64, 0, 0)) in (WAVE, LOWDEG)
    assert route(None) == _hip.EINVAL


def test_general_kernel_moves_its_arc_lists_out_of_lds_by_precision():
    '''513 states of 8 arcs: the lists fit a CU's LDS in float32 without the transition
    posteriors, not in float64 with them -- the same graph, two kernels.'''
    b = desc(513, 8, all_lowdeg=1, max_arcs=513 * 8, max_segs=513)
    assert route(b, F32, 0) == GENERAL
    assert route(b, F64, 1) == BIG


def test_route_agrees_with_the_scratch_query():
    for fields, want in BOUNDARIES:
        for dtype in (F32, F64):
            for want_xi in (0, 1):
                b = desc(**fields)
                n = _hip.lib().beer_hmm_fb_scratch_doubles(dtype, ctypes.byref(b), want_xi)
                if route(b, dtype, want_xi) == BIG:
                    assert n > 0
                elif _hip.fb_family(route(b, dtype, want_xi)) == GENERAL:
                    assert n == 0


def test_case_table_names_every_family():
    routes = {c.route for c in table.CASES}
    for spl in (1, 2, 4):
        for deg in (2, 4, 8):
            assert wave(spl, deg) in routes
    for threads in (128, 256, 512):
        assert LOWDEG | threads in routes
    assert GENERAL in routes and BIG in routes
    assert 150 <= len(table.CASES) <= 300
    waves = [c for c in table.CASES if _hip.fb_family(c.route) == WAVE]
    # the fused launch: all three ways back to pdf ids, 512 and 513 columns, both scales
    assert {table.out_mode(c) for c in waves} == {0, 1, 2}
    assert {512, 513} <= {c.S_total for c in waves}
    assert {(c.flavour, c.scale) for c in waves} >= {(f, s) for f in ft.FLAVOURS for s in (1., .7)}
    assert {c.nutt for c in table.CASES} == {1, 5, 9}
    assert {c.S for c in table.CASES} >= {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513}
    assert {c.nO for c in table.CASES} >= {1, 2, 3, 4, 5, 8, 9}
    assert {c.hub for c in table.CASES} == {0, 1, 2, 64, 65}
    for nutt in (1, 5, 9):
        lens = [T for seed in range(40) for T in ft.lengths(nutt, seed)]
        assert set(lens) == set(ft.LENGTHS)
        assert all(len(ft.lengths(nutt, seed)) == nutt for seed in range(10))


@pytest.mark.parametrize('case', table.CASES, ids=table.case_id)
def test_case_route_is_what_its_graph_gives(case):
    '''The descriptor `HmmBatch` fills for the case's graph (DeviceGraph._lowdeg: degrees of the
    CSR without the hub block, an image only up to 8 arcs a state), built here by hand.'''
    g = ft.make_graph(case.S, table.case_offsets(case), case.seed, case.hub)
    finite = np.isfinite(g['trans'])
    src, dst = ft.lowdeg_arcs(g)
    keep = np.zeros_like(finite)
    keep[src, dst] = True
    deg = max(1, int(keep.sum(0).max()), int(keep.sum(1).max()))
    if not case.hub:
        assert deg == ft.degree(case.S, table.case_offsets(case))
        assert (finite.sum(0) == deg).all() and (finite.sum(1) == deg).all()
    lowdeg = deg <= _hip.SEG
    segs = int(np.ceil(finite.sum(0) / _hip.SEG).sum())
    b = desc(case.S, deg if lowdeg else 0, int(lowdeg), int(bool(case.hub)) if lowdeg else 0,
             case.hub if lowdeg else 0, max_arcs=int(finite.sum()), max_segs=segs, nutt=case.nutt)
    for dtype in (F32, F64):
        for want_xi in (0, 1):
            assert route(b, dtype, want_xi) == case.route
    assert np.isfinite(g['init']).sum() == min(case.S, 3) and np.isfinite(g['final']).all()
    assert np.isfinite(np.diag(g['trans'])).all()
    # the longest utterance (9 frames) puts mass on the last state -- the one past a boundary --
    # and, from 8 arcs a state on, on every state (3 starting states and d arcs a state reach at
    # most 3 + 8 (d - 1) states in 9 frames: 11 of them at degree 2, wherever the arcs point)
    reach = np.isfinite(g['init'])
    for _ in range(max(ft.LENGTHS) - 1):
        reach = reach | (finite[reach].any(0) if reach.any() else reach)
    if deg >= 2 or case.hub:
        assert reach[case.S - 1]
    if deg >= 8:
        assert reach.all()
    if case.hub:
        E, a, B, c = g['hub']
        np.testing.assert_array_equal(g['trans'][np.ix_(E, B)], a[:, None] + c[None, :])
        f32 = ft.make_graph(case.S, table.case_offsets(case), case.seed, case.hub, np.float32)
        E, a, B, c = f32['hub']
        np.testing.assert_array_equal(f32['trans'][np.ix_(E, B)], a[:, None] + c[None, :])


SELF_CHECK = [c for c in table.CASES if c.S <= 130][::6]


@pytest.mark.parametrize('case', SELF_CHECK, ids=table.case_id)
def test_truth_satisfies_its_identities(case):
    g = ft.make_graph(case.S, table.case_offsets(case), case.seed, case.hub)
    ids = ft.pdf_ids(case.S, case.flavour, case.S_total, case.seed)
    lens = ft.lengths(case.nutt, case.seed) + [1]
    pc_all, llhs = ft.inputs(g, lens, ids, case.S_total, case.scale, case.seed)
    assert pc_all.shape == (sum(lens), case.S_total) and [len(l) for l in llhs] == lens
    np.testing.assert_array_equal(llhs[0], case.scale * pc_all[:lens[0]][:, ids])
    t = ft.truth(g, llhs, ids, case.S_total, case.scale)
    dense = ft.truth(g, llhs, ids, case.S_total, case.scale, factored_hub=False)
    for gam in t['gamma']:
        np.testing.assert_allclose(gam.sum(1), 1., rtol=0, atol=1e-12)
    assert np.isfinite(t['lognorm']).all()                 # (the last utterance has one frame)
    before_last = sum(gam[:-1].sum(0) for gam in t['gamma'])
    np.testing.assert_allclose(t['xi_dense'].sum(1), before_last, rtol=0, atol=1e-11)
    np.testing.assert_allclose(t['xi_dense'].sum(0), sum(gam[1:].sum(0) for gam in t['gamma']),
                               rtol=0, atol=1e-11)
    np.testing.assert_array_equal(dense['xi_sum'], t['xi_dense'])
    assert not dense['hub_flow'].any()
    # the factored report loses nothing: matrix + flow through the hub = all arrivals
    np.testing.assert_allclose(t['xi_sum'].sum(0) + t['hub_flow'], t['xi_dense'].sum(0), rtol=0,
                               atol=1e-11)
    np.testing.assert_allclose(t['arc_counts'].sum() + t['hub_flow'].sum(), t['xi_dense'].sum(),
                               rtol=0, atol=1e-10)
    # every state is left once per frame: by an arc, through the hub, or at the utterance's end
    exits = np.zeros(case.S)
    np.add.at(exits, ft.lowdeg_arcs(g)[0], t['arc_counts'])
    np.testing.assert_allclose(exits + t['src_flow'], sum(gam.sum(0) for gam in t['gamma']),
                               rtol=0, atol=1e-11)
    np.testing.assert_allclose(t['state_resps'].sum(1), case.scale, rtol=0, atol=1e-12)
    np.testing.assert_allclose(t['utt_llh'].sum(), t['frame_llh'].sum(), rtol=1e-13)
    u = int(np.argmax(lens))
    xi = ft.xi_frames(g, llhs[u])
    assert xi.shape == (lens[u] - 1, case.S, case.S)
    np.testing.assert_allclose(xi.sum((1, 2)), 1., rtol=0, atol=1e-12)


# --- Viterbi -----------------------------------------------------------------------------------

@pytest.mark.parametrize('vc', table.VCASES, ids=lambda vc: f'S{vc.S}-O{vc.nO}')
def test_viterbi_cases_are_exact_in_float32_and_full_of_ties(vc):
    '''Integer inputs: the float32 and float64 oracle paths are identical, and -- a condition on
    the table, not a measurement of the code -- at least 5 % of the reachable cells of the long
    utterances have their maximum attained by more than one source.'''
    g = table.vcase_graph(vc)
    lens = list(ft.VITERBI_LENGTHS)
    llhs = ft.viterbi_inputs(vc.S, lens, vc.seed)
    tied = reach = 0
    for T, l in zip(lens, llhs):
        assert set(np.unique(l)) <= set(range(-4, 1))
        np.testing.assert_array_equal(ft.best_path(g, l), ft.best_path(g, l, np.float32))
        if T >= 31:
            a, b = ft.tie_share(g, l)
            assert vc.S < 2 or 20 * a >= b, f'T={T}: {a} tied cells of {b}'
            tied, reach = tied + a, reach + b
    for k in ('init', 'final', 'trans'):
        fin = g[k][np.isfinite(g[k])]
        assert (fin == np.round(fin)).all() and fin.min() >= -3
    print(f'tied cells: {tied} of {reach} ({100. * tied / max(reach, 1):.1f} %)')


def test_viterbi_table_covers_the_thread_schemes():
    sizes = {vc.S for vc in table.VCASES}
    assert sizes >= {1, 2, 7, 64, 128, 129, 256, 257, 300}
    assert {vc.nO for vc in table.VCASES} >= {2, 3, 5, 8, 12}
    assert set(ft.VITERBI_LENGTHS) == {1, 2, 31, 32, 33, 64, 65}
    # arc lists that do not fit beside the trellis in 64 KiB of LDS (beer_hmm_viterbi), both dtypes
    for elem in (4, 8):
        S, A = 130, 130 * 130
        assert 2 * S * elem + 32 * S * 4 + (S + 2 + A) * 4 + A * elem > 64 * 1024
    for k, S in enumerate(table.VMIXED_SIZES):
        g = ft.make_graph(S, ft.offsets(5, S), 2000 + k, 0, np.float64, integer=True)
        for u, (T, kk) in enumerate(zip(table.VMIXED_LENS, table.VMIXED_GIDS)):
            if kk == k and T >= 31:
                a, b = ft.tie_share(g, ft.viterbi_inputs(S, [T], 2100 + u)[0])
                assert 20 * a >= b


# --- argument validation of every beer_hmm_* entry point of csrc/hmm.hip --------------------------
# Rows that return before any HIP call, so they run without a GPU; the codes are literals.

_SCRATCH = ctypes.create_string_buffer(64)
P = ctypes.cast(_SCRATCH, ctypes.c_void_p)          # "some buffer": never reached by these rows


def _cmap(arc_cat=P, last_cat=P, arc_off=P, state_off=P):
    return _hip.CatMap(arc_cat, last_cat, arc_off, state_off)


# name -> the argument list (without the stream) from: dtype, batch, every buffer, S_total,
# atomic_out, category map, element / frame count, hub_ws alone
ENTRY_ARGS = {
    'gather': lambda d, b, p, S, a, m, n, h: (d, b, S, p, 1., p),
    'scatter': lambda d, b, p, S, a, m, n, h: (d, b, S, p, p, 1., p, p, p),
    'forward_backward': lambda d, b, p, S, a, m, n, h: (d, b, p, p, h, p, p, p, p, p),
    'fb_log_count': lambda d, b, p, S, a, m, n, h: (b, h, p),
    'posteriors_fused': lambda d, b, p, S, a, m, n, h: (d, b, S, p, 1., p, h, p, a, p, p, p, p),
    'posteriors_fused_counts':
        lambda d, b, p, S, a, m, n, h: (d, b, S, p, 1., p, h, p, a, p, p, p, p, p, p),
    'forward_backward_counts': lambda d, b, p, S, a, m, n, h: (d, b, p, p, h, p, p, p, p, p, p),
    'last_frame_sum': lambda d, b, p, S, a, m, n, h: (d, b, p, p),
    'refresh_weights': lambda d, b, p, S, a, m, n, h: (d, n, p, p, p, p),
    'posteriors_fused_cat':
        lambda d, b, p, S, a, m, n, h: (d, b, S, p, 1., p, h, p, a, p, p, p, m, p),
    'forward_backward_cat': lambda d, b, p, S, a, m, n, h: (d, b, p, p, h, p, p, m, p, p),
    'path_counts_cat': lambda d, b, p, S, a, m, n, h: (b, p, m, p),
    'trans_posteriors': lambda d, b, p, S, a, m, n, h: (d, n, S, p, p, p, p, p),
    'viterbi': lambda d, b, p, S, a, m, n, h: (d, b, p, p, p, 0),
    'path_posteriors': lambda d, b, p, S, a, m, n, h: (d, b, p, p, p, p),
}
WITH_BATCH = [n for n in ENTRY_ARGS if n not in ('refresh_weights', 'trans_posteriors')]
FUSED = ['posteriors_fused', 'posteriors_fused_counts', 'posteriors_fused_cat']
WAVE_ONLY = FUSED + ['forward_backward_counts', 'fb_log_count']
CAT = ['posteriors_fused_cat', 'forward_backward_cat']
CHECKS_STATES = FUSED + ['forward_backward', 'forward_backward_counts', 'forward_backward_cat',
                         'viterbi']
DENSE = dict(all_lowdeg=0, max_degree=0)


def _two_graphs():
    b = desc(64)
    b.n_graphs = 2
    return b


def validation_rows():
    'Rows (what, entry point, keyword arguments of `validate`, expected code).'
    rows = []

    def add(what, names, want, **kw):
        rows.extend((what, n, kw, want) for n in names)

    add('null batch', WITH_BATCH, -100000, b=None)
    add('negative nutt', WITH_BATCH, -100000, b=desc(64, nutt=-1))
    add('empty batch, null buffers', [n for n in WITH_BATCH if n != 'fb_log_count'], 0,
        b=desc(64, nutt=0), p=None, h=None, m=None)
    add('empty batch, null count', ['fb_log_count'], -100000, b=desc(64, nutt=0), p=None, h=None)
    add('empty batch, null hub_ws', ['fb_log_count'], 0, b=desc(64, nutt=0), h=None)
    add('no elements / one frame', ['refresh_weights', 'trans_posteriors'], 0, n=0, p=None)
    add('one frame', ['trans_posteriors'], 0, n=1, p=None)
    add('negative count', ['refresh_weights', 'trans_posteriors'], -100000, n=-1)
    add('no state', ['trans_posteriors'], -100000, S=0)
    add('null buffers', ['refresh_weights', 'trans_posteriors'], -100000, n=2, p=None)
    add('null buffers', WAVE_ONLY + ['last_frame_sum', 'forward_backward_cat', 'path_counts_cat'],
        -100000, p=None, h=None)
    # dtype 99: the two entry points that look at the batch first take an empty one
    by_dtype = [n for n in ENTRY_ARGS if n not in ('fb_log_count', 'path_counts_cat')]
    add('dtype 99, empty batch', [n for n in by_dtype if n not in ('viterbi', 'path_posteriors')],
        -100000, d=99, b=desc(64, nutt=0), n=0)
    add('dtype 99, empty batch', ['viterbi', 'path_posteriors'], 0, d=99, b=desc(64, nutt=0))
    add('dtype 99', by_dtype, -100000, d=99)
    add('no states', CHECKS_STATES, -100000, b=desc(0))
    add('32768 states', ['forward_backward', 'forward_backward_cat', 'viterbi'], -100000,
        b=desc(32768, **DENSE))
    add('not a one-wave descriptor', WAVE_ONLY, -100000, b=desc(300))
    add('no low-degree image', WAVE_ONLY, -100000, b=desc(64, all_lowdeg=0))
    add('two graphs', ['posteriors_fused_counts', 'forward_backward_counts', 'last_frame_sum',
                       'path_posteriors'], -100000, b=_two_graphs())
    add('a hub', CAT, -100000, b=desc(64, max_hubs=1, members=3))
    add('null map', CAT + ['path_counts_cat'], -100000, m=None)
    for member in ('arc_cat', 'last_cat', 'arc_off', 'state_off'):
        add(f'null {member}', CAT + ['path_counts_cat'], -100000, m=_cmap(**{member: None}))
    add('no pdf column', FUSED + ['gather', 'scatter'], -100000, S=0)
    add('no pdf column, empty batch', FUSED + ['gather', 'scatter'], -100000, S=0,
        b=desc(64, nutt=0))
    add('rows of 513 columns through LDS', FUSED, -100000, S=513, a=2)
    # the general kernel: per-state arrays beyond a CU's LDS; per-arc scratch without `hub_ws`
    add('beyond LDS', ['forward_backward', 'forward_backward_cat'], -100000,
        b=desc(32767, max_arcs=100000, max_segs=40000, **DENSE))
    add('arc lists beyond LDS, null hub_ws', ['forward_backward', 'forward_backward_cat'],
        -100000, b=desc(100, max_arcs=10000, max_segs=1300, **DENSE), h=None)
    return rows


def validate(name, d=F32, b=None, p=P, S=5, a=0, m=_cmap(), n=2, h=P):
    args = ENTRY_ARGS[name](d, ctypes.byref(b) if b is not None else None, p, S, a,
                            ctypes.byref(m) if m is not None else None, n, h)
    return getattr(_hip.lib(), 'beer_hmm_' + name)(*args, None)


VALIDATION = validation_rows()


@pytest.mark.parametrize('what,name,kw,want', VALIDATION,
                         ids=[f'{r[1]}-{r[0].replace(" ", "_")}' for r in VALIDATION])
def test_entry_points_validate_their_arguments(what, name, kw, want):
    kw = dict(kw)
    if 'b' not in kw and name in WITH_BATCH:
        kw['b'] = desc(64)
    assert validate(name, **kw) == want


def test_validation_table_names_every_entry_point_of_the_file():
    text = open(os.path.join(ROOT, 'beer_amd', 'csrc', 'hmm.hip')).read()
    defined = set(re.findall(r'^(?:int|size_t) beer_hmm_(\w+)\(', text, re.M))
    host_only = {'fb_route', 'fb_scratch_doubles'}          # (no stream; see below and above)
    assert defined == set(ENTRY_ARGS) | host_only
    assert {r[1] for r in VALIDATION} == set(ENTRY_ARGS)
    scratch = _hip.lib().beer_hmm_fb_scratch_doubles
    big = desc(100, max_arcs=10000, max_segs=1300, **DENSE)
    assert scratch(F64, None, 1) == 0 and scratch(99, ctypes.byref(big), 1) == 0
    assert scratch(F64, ctypes.byref(desc(100, nutt=0, max_arcs=10000, **DENSE)), 1) == 0
    assert scratch(F64, ctypes.byref(big), 1) == 3 * (2 * 10000 + 1300)
    assert route(None) == -100000 and route(desc(64), 99) == -100000
    assert route(desc(64, nutt=0), 99) == -100000 and route(desc(64, nutt=0)) == 0x1014
