"""CPU checks of the bigram kernel's launch rule: `beer_hmm_bigram_route` on hand-built
descriptors on both sides of every boundary, the case tables of tests/test_gpu_bigram_routes.py
(all 15 SPL x DEG forms and every wave count named, every case's stated form what its generated
graph gives), the conditions that keep a case from passing emptily, and the vectorised truth of
tests/bigram_truth.py pinned to the oracle."""

import ctypes
import os
import re

import numpy as np
import pytest

import bigram_truth as bt
import fb_truth as ft
from helpers import ROOT, orc
import test_gpu_bigram_routes as table

from beer_amd import _hip

F32, F64 = _hip.F32, _hip.F64
N_CU = 256                      # the compute units of an MI355X: what the tables' wave counts assume
ALL_CASES = table.FORMS + table.WAVES


def desc(S, P=5, max_degree=2):
    'A beer_bigram with only its scalar fields filled: all the query may read.'
    return _hip.Bigram(S, P, max_degree, 0, *([None] * 14))


def route(b, dtype=F64, nutt=3, n_cu=N_CU):
    return _hip.lib().beer_hmm_bigram_route(dtype, ctypes.byref(b) if b is not None else None,
                                            nutt, n_cu)


def form(spl, deg, waves=1):
    return table.route_value(spl, deg, waves)


BOUNDARIES = [
    # states: 64|65, 128|129, 256|257, 320|321, 512|513
    (dict(S=1), {}, form(1, 2)), (dict(S=64), {}, form(1, 2)), (dict(S=65), {}, form(2, 2)),
    (dict(S=128), {}, form(2, 2)), (dict(S=129), {}, form(4, 2)), (dict(S=256), {}, form(4, 2)),
    (dict(S=257), {}, form(5, 2)), (dict(S=320), {}, form(5, 2)), (dict(S=321), {}, form(8, 2)),
    (dict(S=512), {}, form(8, 2)), (dict(S=513), {}, _hip.EINVAL), (dict(S=0), {}, _hip.EINVAL),
    # residual arcs a state: 0, 2|3, 4|5, 8|9
    (dict(S=64, max_degree=0), {}, form(1, 2)), (dict(S=64, max_degree=1), {}, form(1, 2)),
    (dict(S=64, max_degree=2), {}, form(1, 2)), (dict(S=64, max_degree=3), {}, form(1, 4)),
    (dict(S=64, max_degree=4), {}, form(1, 4)), (dict(S=64, max_degree=5), {}, form(1, 8)),
    (dict(S=64, max_degree=8), {}, form(1, 8)), (dict(S=64, max_degree=9), {}, _hip.EINVAL),
    (dict(S=64, max_degree=-1), {}, _hip.EINVAL), (dict(S=512, max_degree=8), {}, form(8, 8)),
    (dict(S=300, max_degree=3), {}, form(5, 4)),
    # phones: 1, 128|129
    (dict(S=300, P=1), {}, form(5, 2)), (dict(S=300, P=128), {}, form(5, 2)),
    (dict(S=300, P=129), {}, _hip.EINVAL), (dict(S=300, P=0), {}, _hip.EINVAL),
    # utterances on 256 compute units: 1 -> 2 waves at 256|257, 7 -> 8 at 1792|1793, then 8
    (dict(S=300), dict(nutt=1), form(5, 2, 1)), (dict(S=300), dict(nutt=256), form(5, 2, 1)),
    (dict(S=300), dict(nutt=257), form(5, 2, 2)), (dict(S=300), dict(nutt=1792), form(5, 2, 7)),
    (dict(S=300), dict(nutt=1793), form(5, 2, 8)), (dict(S=300), dict(nutt=4096), form(5, 2, 8)),
    (dict(S=300), dict(nutt=1 << 30), form(5, 2, 8)),
    # ... on other devices
    (dict(S=300), dict(nutt=9, n_cu=1), form(5, 2, 8)), (dict(S=300), dict(nutt=9, n_cu=4), form(5, 2, 3)),
    (dict(S=300), dict(nutt=305, n_cu=304), form(5, 2, 2)),
    # what the LDS holds behind W: 128 phones leave 31 KiB of the 160
    (dict(S=512, P=128), dict(nutt=4096), form(8, 2, 3)), (dict(S=128, P=128), dict(nutt=4096), form(2, 2, 7)),
    (dict(S=64, P=128), dict(nutt=4096), form(1, 2, 8)), (dict(S=320, P=128), dict(nutt=4096), form(5, 2, 4)),
    (dict(S=512, P=128), dict(nutt=513), form(8, 2, 3)), (dict(S=512, P=128), dict(nutt=512), form(8, 2, 2)),
    (dict(S=512, P=100), dict(nutt=4096), form(8, 2, 8)),
    # no utterance: nothing is launched, the form is that of one wave
    (dict(S=300), dict(nutt=0), form(5, 2, 1)), (dict(S=300), dict(nutt=-1), _hip.EINVAL),
]


@pytest.mark.parametrize('fields,kw,want', BOUNDARIES, ids=[str(i) for i in range(len(BOUNDARIES))])
def test_route_on_both_sides_of_every_boundary(fields, kw, want):
    for dtype in (F32, F64):
        assert route(desc(**fields), dtype, **kw) == want, (fields, kw, dtype)
    assert route(desc(**fields), 7, **kw) == _hip.EINVAL
    assert route(None, F64, **kw) == _hip.EINVAL


def test_route_refuses_where_the_entry_point_does():
    '''Every descriptor of the boundary table through `beer_hmm_posteriors_bigram` with buffers
    it never reaches: the rows the query refuses are refused before anything is launched, and an
    empty batch of the others is accepted.'''
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    entry = _hip.lib().beer_hmm_posteriors_bigram
    for fields, kw, want in BOUNDARIES:
        nutt = kw.get('nutt', 3)
        if want != _hip.EINVAL:
            nutt = 0
        for dtype in (F32, F64, 7):
            rc = entry(dtype, ctypes.byref(desc(**fields)), nutt, 0, buf, None, 5, buf, 1., buf, buf,
                       buf, 0, buf, buf, None)
            assert rc == (_hip.EINVAL if want == _hip.EINVAL or dtype == 7 else 0), (fields, kw, dtype)


def test_route_asks_the_device_when_no_cu_count_is_given():
    'n_cu <= 0: the current device, or 256 without one -- either way a valid form of the same kernel.'
    for n_cu in (0, -1):
        r = route(desc(300), F64, 4096, n_cu)
        assert r & 0xFFFF == form(5, 2, 0) and 1 <= r >> 16 <= 8


def test_route_is_declared_in_the_header_and_bound():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    assert re.search(r'int beer_hmm_bigram_route\(int dtype, const beer_bigram\* graph, int32_t nutt,'
                     r'\s+int32_t n_cu\);', text)
    assert _hip.SIGNATURES['beer_hmm_bigram_route'] == [_hip.c_i, _hip.c_p, ctypes.c_int32,
                                                        ctypes.c_int32]
    assert (_hip.BIGRAM_MAX_PHONES, _hip.BIGRAM_MAX_STATES, _hip.SEG) == (128, 512, 8)


def test_case_tables_name_every_form():
    forms = {(c.spl, c.deg) for c in table.FORMS}
    assert forms == {(spl, deg) for spl in (1, 2, 4, 5, 8) for deg in (2, 4, 8)}
    assert {c.waves for c in ALL_CASES} == {1, 2, 3, 7, 8}
    assert {c.S for c in table.FORMS} >= {s for s, _ in table.SPL_BANDS}
    # each form at the smallest and at the largest size of its band (one band below 65 states)
    for spl in (2, 4, 5, 8):
        lo, hi = [s for s, k in table.SPL_BANDS if k == spl]
        for deg in (2, 4, 8):
            assert {c.S for c in table.FORMS if (c.spl, c.deg) == (spl, deg)} >= {lo, hi}
    assert {c.P for c in table.FORMS} >= set(table.BLOCK_SIZES)
    assert {c.d for c in table.FORMS} == {0, 1, 2, 3, 4, 5, 8}
    assert {c.placement for c in table.FORMS} == {'disjoint', 'overlap', 'identical'}
    assert {(c.flavour, c.scale) for c in table.FORMS} >= {(f, s) for f in bt.FLAVOURS for s in (1., .8)}
    assert any(c.neg for c in table.FORMS) and any(c.deep for c in table.FORMS)
    assert {c.deep for c in table.FORMS if c.P > 64} == {False, True}
    assert all(c.waves == 1 and c.per_cu == 0 and c.lens == bt.LENGTHS for c in table.FORMS)
    # the wave cases: S <= 64 and T <= 9 at n + 1, 7 n + 1 and 8 n + 3 utterances, then the two
    # that the LDS limits
    assert [(c.per_cu, c.extra, c.waves) for c in table.WAVES] == \
        [(1, 1, 2), (7, 1, 8), (8, 3, 8), (6, 1, 7), (2, 1, 3)]
    assert all(c.S <= 64 and max(c.lens) <= 9 for c in table.WAVES[:3])
    assert [(c.P, c.S) for c in table.WAVES[3:]] == [(128, 128), (128, 512)]
    assert max(table.WAVES[4].lens) <= 3
    assert len({table.case_id(c) for c in ALL_CASES}) == len(ALL_CASES) <= 60


@pytest.fixture(scope='module')
def truths():
    'The float64 truth of every case on a device of N_CU compute units, computed once.'
    memo = {}

    def get(c):
        if c not in memo:
            g, ids, lens, pc_all, llhs = table.case_inputs(c, N_CU)
            memo[c] = (g, ids, lens, pc_all, llhs,
                       bt.truth(g, llhs, ids, c.S_total, c.scale, vectorised=True))
        return memo[c]
    return get


@pytest.mark.parametrize('c', ALL_CASES, ids=table.case_id)
def test_case_form_is_what_its_graph_gives(c):
    '`BigramImage`\'s degree rule restated on the host arrays, in either dtype.'
    for dtype in (np.float64, np.float32):
        g = table.case_graph(c, dtype)
        trans, src, dst = g['trans'], g['src'], g['dst']
        assert len(src) == len(dst) == c.P and len(set(src)) == len(set(dst)) == c.P
        keep = trans > -np.inf
        keep[np.ix_(src, dst)] = False
        assert g['max_degree'] == int(max(keep.sum(0).max(), keep.sum(1).max())) == c.d
        nutt = table.case_nutt(c, N_CU) + (not c.per_cu)
        for code in (F32, F64):
            assert route(desc(c.S, c.P, g['max_degree']), code, nutt) == form(c.spl, c.deg, c.waves)
        # the circulant arcs outside the block are all there; every row and column of the block
        # keeps an entry; the placement is what the case says
        mask = ft.circulant_mask(c.S, ft.offsets(c.d, c.S) if c.d else ())
        mask[np.ix_(src, dst)] = False
        np.testing.assert_array_equal(keep, mask)
        block = np.isfinite(g['block'])
        assert block.any(0).all() and block.any(1).all()
        assert bool((~block).any()) == bool(c.neg and c.P > 1)
        both = set(src) & set(dst)
        assert {'disjoint': not both, 'reversed': not both, 'identical': both == set(src),
                'overlap': (0 < len(both) < c.P) or c.P == 1}[c.placement]
        if c.deep:
            assert np.exp(g['block'][block].max().astype(np.float32)) == 0.
            assert np.exp(g['block'][block].min().astype(np.float64)) > 0.
        assert np.isfinite(g['init']).sum() == min(3, c.P - 64 if c.P > 64 else c.P)
        assert set(np.nonzero(np.isfinite(g['init']))[0]) <= set(src)


@pytest.mark.parametrize('c', ALL_CASES, ids=table.case_id)
def test_no_case_passes_emptily(c, truths):
    g, ids, lens, pc_all, llhs, t = truths(c)
    assert len(lens) == table.case_nutt(c, N_CU) + (not c.per_cu)
    assert set(lens) == set(c.lens) | ({0} if not c.per_cu else set())
    assert lens.count(0) == (not c.per_cu)
    gam = np.concatenate(t['gamma'])
    assert gam.shape == (sum(lens), c.S)
    np.testing.assert_allclose(gam.sum(1), 1., rtol=0, atol=1e-12)
    np.testing.assert_allclose(t['state_resps'].sum(1), c.scale, rtol=0, atol=1e-12)
    # the block carries posterior mass in every utterance long enough to show it
    long = [u for u, T in enumerate(lens) if T >= 3]
    assert long and t['utt_counts'][long].min() > .05
    np.testing.assert_allclose(t['counts'].sum(), t['utt_counts'].sum(), rtol=1e-12)
    if c.P > 64:        # ... and in the second chunk of the member loop
        assert 1. - t['counts'][:64, :64].sum() / t['counts'].sum() >= .2
    if c.spl >= 2:      # the states that a wrong lane mask or states-per-lane count loses
        assert gam[:, -64:].sum() >= .2 * gam.sum()
    if c.deep:
        assert t['counts'].sum() > 0
    if c.per_cu:        # every utterance different: waves reading each other's LDS cannot agree
        assert len({l.tobytes() for l in llhs}) == len(llhs)
    # pdf ids: what `posteriors_bigram` turns into atomic adds or plain stores
    assert len(set(ids)) < c.S if c.flavour == 'repeat' and c.S > 1 else len(set(ids)) == c.S
    assert (set(ids) == set(range(c.S_total))) == (c.flavour == 'perm')


PINNED = [c for c in ALL_CASES if c.S <= 130][::4] + [table.WAVES[0]]


@pytest.mark.parametrize('c', PINNED, ids=table.case_id)
def test_vectorised_truth_is_the_oracles(c, truths):
    '`bigram_truth.batch_posteriors` against `orc.posteriors`, utterance by utterance, to 1e-12.'
    g, ids, lens, pc_all, llhs, t = truths(c)
    pick = list(range(len(lens)))[:12]
    sub = [llhs[u] for u in pick]
    want = bt.truth(g, sub, ids, c.S_total, c.scale)
    got = bt.truth(g, sub, ids, c.S_total, c.scale, vectorised=True)
    for key in ('state_resps', 'counts', 'utt_llh', 'utt_counts'):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=1e-12, err_msg=key)
    for u, k in enumerate(pick):
        np.testing.assert_allclose(t['gamma'][k], want['gamma'][u], rtol=0, atol=1e-12)
        np.testing.assert_allclose(t['utt_llh'][k], want['utt_llh'][u], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(t['utt_counts'][k], want['utt_counts'][u], rtol=1e-12, atol=1e-12)
    # the oracle's own outputs, restated: rows of xi sum to the posteriors they leave
    u = int(np.argmax([len(l) for l in sub]))
    init, final, trans = (g[k].astype(np.float64) for k in ('init', 'final', 'trans'))
    with np.errstate(invalid='ignore', divide='ignore'):
        gam, xi, _ = orc.posteriors(sub[u].astype(np.float64), init, final, trans, True)
    np.testing.assert_allclose(xi.sum(2), gam[:-1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(xi.sum(1), gam[1:], rtol=0, atol=1e-12)


def test_fallback_twins_sit_on_either_side_of_the_kernels_limit():
    '''The linear-domain column of the twin at frame 1, restated in float64 logarithms: its
    largest entry relative to the frame's best state is what the kernel holds against 2^-800.'''
    limit = -800 * np.log(2.)
    for gap, inside in [(500., True), (700., False)]:
        for dtype in (np.float64, np.float32):
            g, ids, lens, pc_all, llhs = table.fallback_batch(gap, dtype)
            assert g['max_degree'] == 2 and lens[2] == 3
            assert g['src'] == [4, 5] and g['dst'] == [0, 1]
            assert list(np.nonzero(np.isfinite(g['init']))[0]) == [0, 1, 2]
            l = llhs[2].astype(np.float64)
            init, trans = g['init'].astype(np.float64), g['trans'].astype(np.float64)
            a0 = l[0] + init
            a0 -= a0.max()                                     # the column in [1/2, 1) up to a factor 2
            with np.errstate(divide='ignore'):
                col = orc.logsumexp(a0[:, None] + trans, 0) + l[1] - l[1].max()
            assert set(np.nonzero(np.isfinite(col))[0]) == {0, 1, 2, 3}
            assert (col.max() > limit + 40.) == inside and (col.max() < limit - 40.) == (not inside)
            t = bt.truth(g, llhs, ids, table.FALLBACK_S, 1.)
            assert t['counts'].sum() > .05 and t['utt_counts'][2] == 0.
            np.testing.assert_allclose(np.concatenate(t['gamma']).sum(1), 1., rtol=0, atol=1e-12)
