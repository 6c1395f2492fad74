"""CPU checks of the arc posteriors under explicit durations: the truth of
tests/hsmm_arcs_truth.py pinned four ways (the count-down HMM under lifted categories and the
geometric equivalence against the plain HMM's arc truth, enumeration of every segmentation, the
begin / end posteriors that `hsmm_truth.posteriors` implies), the route and the workspace size
against restatements of the header's text, the refusals made before any launch, and the
bigram categories i P + j against the unit-start categories."""

import ctypes

import numpy as np
import pytest

import arcs_truth as at
import fb_truth as ft
import hsmm_arcs_truth as hat
import hsmm_truth as ht
from test_durations_host import _graph, desc

from beer_amd import _hip, hmm_kernels as hk
from beer_amd.models.sequence import unit_start_categories

PIN = 1e-12
GRAPHS = ((1, 0), (3, 0), (8, 0), (12, 4))


# --- the truth, pinned -------------------------------------------------------------------------

@pytest.mark.parametrize('S,hub', GRAPHS)
@pytest.mark.parametrize('D', [1, 3, 4])
def test_the_count_down_hmm_under_lifted_categories(S, hub, D):
    g = ft.make_graph(S, ft.offsets(3, S), 6, hub)
    rng = np.random.RandomState(S * D)
    ld, lw = rng.uniform(-3, 0, size=(S, D)), rng.uniform(0, 1, size=S)
    n_cat = 5
    arc_cat, init_cat = hat.random_categories(g, n_cat, 11 + S, drop=.25)
    eg, e_arc, e_init = hat.lifted_categories(g, ld, lw, arc_cat, init_cat)
    live = 0
    for T in ft.LENGTHS:
        l = rng.randn(T, S) * 3
        frame, utt = hat.arc_posteriors(g, ld, lw, l, arc_cat, init_cat, n_cat)
        want, want_utt = at.arc_posteriors(eg, np.repeat(l, D, axis=1), e_arc, e_init, n_cat)
        assert np.abs(frame - want).max() <= PIN and np.abs(utt - want_utt).max() <= PIN * T
        live += bool(frame.any())
    assert live >= (1 if S == 1 else len(ft.LENGTHS))


@pytest.mark.parametrize('S,D,T', [(2, 2, 4), (3, 3, 5), (3, 2, 3), (1, 3, 2), (2, 1, 3), (3, 5, 1),
                                   (1, 2, 5)])
def test_enumeration_of_every_segmentation(S, D, T):
    g = ft.make_graph(S, ft.offsets(3, S), 7, 0)
    rng = np.random.RandomState(S * D + T)
    ld, lw, l = rng.uniform(-3, 0, size=(S + 2, D)), rng.uniform(0, 1, size=S + 2), \
        rng.randn(T, S) * 3
    ld[0, 0] = -np.inf
    ids = rng.choice(S + 2, size=S, replace=False)
    n_cat = 4
    arc_cat, init_cat = hat.random_categories(g, n_cat, 3 * S + T, drop=.2)
    frame, utt = hat.arc_posteriors(g, ld, lw, l, arc_cat, init_cat, n_cat, ids)
    want, want_utt = hat.brute_force(g, ld, lw, l, arc_cat, init_cat, n_cat, ids)
    assert np.abs(frame - want).max() <= PIN and np.abs(utt - want_utt).max() <= PIN
    if not np.isfinite(ht.posteriors(g, ld, lw, l, ids)['Z']):
        assert not frame.any() and not utt.any()


@pytest.mark.parametrize('S,hub', GRAPHS)
def test_geometric_duration_laws_give_the_hmms_rows_on_the_other_arcs(S, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 5, hub)
    src, dst = at.out_arcs(g)
    n_cat = 6
    arc_cat, init_cat = hat.random_categories(g, n_cat, 17 + S, drop=.25)
    off_diagonal = np.where(src != dst, arc_cat, -1)
    for T in ft.LENGTHS:
        l = np.random.RandomState(T).randn(T, S) * 3
        frame, utt = hat.arc_posteriors(g, ht.geometric_log_dur(g, T), None, l, arc_cat, init_cat,
                                        n_cat)
        want, want_utt = at.arc_posteriors(g, l, off_diagonal, init_cat, n_cat)
        assert np.abs(frame - want).max() <= PIN and np.abs(utt - want_utt).max() <= PIN * T


@pytest.mark.parametrize('S,hub', GRAPHS[1:])
@pytest.mark.parametrize('D', [2, 5])
def test_rows_sum_to_the_begin_posterior(S, hub, D):
    '''By destination the rows are B_t(j), by source E_{t-1}(i): their sums over the frames are
    entry_sum, row 0 is gamma0_sum, and B_t(j) - E_{t-1}(j) = gamma_t(j) - gamma_{t-1}(j).'''
    g = ft.make_graph(S, ft.offsets(3, S), 8, hub)
    rng = np.random.RandomState(S + D)
    ld, lw = rng.uniform(-3, 0, size=(S, D)), rng.uniform(0, 1, size=S)
    src, dst = at.out_arcs(g)
    for T in ft.LENGTHS:
        l = rng.randn(T, S) * 3
        p = ht.posteriors(g, ld, lw, l)
        by_dst, _ = hat.arc_posteriors(g, ld, lw, l, dst, np.arange(S), S)
        by_src, _ = hat.arc_posteriors(g, ld, lw, l, src, np.full(S, -1), S)
        one, _ = hat.arc_posteriors(g, ld, lw, l, np.zeros(len(src), dtype=int), np.zeros(S, dtype=int), 1)
        assert np.abs(by_dst[0] - p['gamma0_sum']).max() <= PIN
        assert np.abs(by_dst[1:].sum(0) - p['entry_sum']).max() <= PIN * T
        assert np.abs(one[:, 0] - by_dst.sum(1)).max() <= PIN       # B_t: the row sum
        assert abs(one[0, 0] - 1.) <= PIN and (one <= 1 + PIN).all()
        if T > 1:
            assert np.abs(by_dst[1:].sum(1) - by_src[1:].sum(1)).max() <= PIN
            assert np.abs((by_dst[1:] - by_src[1:]) - np.diff(p['gamma'], axis=0)).max() <= PIN
        # a self-loop given a category counts nothing: the diagonal arcs are in the CSR
        assert (src == dst).any()


# --- route and workspace -----------------------------------------------------------------------

def test_route_is_the_header_formula():
    lib = _hip.lib()
    seen = set()
    for S in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 96, 120, 128, 129, 150, 256, 257, 1024,
              2048):
        for D in (1, 2, 3, 5, 9, 16, 17, 33, 64, 65, 128):
            for code, size in ((_hip.F32, 4), (_hip.F64, 8)):
                for n_cat in (1, 24, 25, 48, 49, 1024, 1025, 1600, 4096, 4097, 20000):
                    for want in (0, 1):
                        # (the low-degree fields of the batch change nothing)
                        b = desc(S, 3, 1, 8, 4)
                        got = lib.beer_hsmm_arcs_route(code, ctypes.byref(b), D, n_cat, want)
                        assert got == hat.route_formula(S, D, size, n_cat, want), \
                            (S, D, size, n_cat, want)
                        assert not got & ht.LOWDEG
                        seen.add(got)
                for nutt in (0, 3, 513):
                    b = desc(S, nutt)
                    assert lib.beer_hsmm_arcs_scratch_doubles(code, ctypes.byref(b), D) == \
                        hat.scratch_formula(S, D, size, nutt) == \
                        lib.beer_hsmm_scratch_doubles(code, ctypes.byref(b), D)
    assert {r & 0xF for r in seen} == set(range(7))
    bits = hat.FRAME_LDS | hat.UTT_LDS | ht.RING_LDS
    assert {r & bits for r in seen} >= {0, ht.RING_LDS, bits, hat.UTT_LDS, hat.FRAME_LDS | hat.UTT_LDS,
                                        ht.RING_LDS | hat.UTT_LDS, ht.RING_LDS | hat.FRAME_LDS}
    # the ring of S = 150, D = 64 leaves 384 bytes: 48 bins
    assert hat.route_formula(150, 64, 8, 48, 1) & bits == ht.RING_LDS | hat.FRAME_LDS
    assert hat.route_formula(150, 64, 8, 24, 1) & bits == bits
    assert hat.route_formula(150, 64, 8, 49, 1) & bits == ht.RING_LDS


def test_refusals_before_any_launch():
    lib = _hip.lib()
    good = desc(8)
    for code, b, D, n_cat in ((_hip.F64, good, 0, 3), (_hip.F64, good, _hip.HSMM_MAX_DUR + 1, 3),
                              (2, good, 4, 3), (_hip.F64, desc(0), 4, 3),
                              (_hip.F64, desc(_hip.HSMM_MAX_STATES + 1), 4, 3),
                              (_hip.F64, desc(8, nutt=-1), 4, 3), (_hip.F64, good, 4, 0),
                              (_hip.F64, good, 4, -2)):
        assert lib.beer_hsmm_arcs_route(code, ctypes.byref(b), D, n_cat, 1) == _hip.EINVAL
        assert hat.route_formula(b.max_states, D, 8 if code == _hip.F64 else 4, n_cat, 1) == \
            ht.EINVAL or code == 2 or b.nutt < 0
    assert lib.beer_hsmm_arcs_route(_hip.F64, None, 4, 3, 1) == _hip.EINVAL
    # the entry point: no device is touched.  (A pointer that is only compared with NULL)
    some = ctypes.c_void_p(8)
    amap = _hip.ArcMap(8, 8, 8, 8)
    fn = lib.beer_hsmm_arc_posteriors

    def call(b=good, D=4, S_total=8, m=ctypes.byref(amap), n_cat=3, outs=(some, None, None)):
        return fn(_hip.F64, ctypes.byref(b), None, None, None, D, S_total, m, n_cat, None, None,
                  None, None, None, None, *outs, None)
    assert call(D=0) == _hip.EINVAL and call(n_cat=0) == _hip.EINVAL
    assert call(S_total=0) == _hip.EINVAL and call(m=None) == _hip.EINVAL
    assert call(outs=(None, None, None)) == _hip.EINVAL
    for hole in range(4):
        members = [8, 8, 8, 8]
        members[hole] = None
        assert call(m=ctypes.byref(_hip.ArcMap(*members))) == _hip.EINVAL
    # with utterances in the batch the NULL inputs are refused too; without, nothing is done
    assert call() == _hip.EINVAL
    assert call(b=desc(8, nutt=0)) == 0
    for outs in ((None, some, None), (None, None, some)):
        assert call(b=desc(8, nutt=0), outs=outs) == 0


def test_the_python_layer_checks_before_the_device():
    with pytest.raises(ValueError, match='neither'):
        hk.check_arc_categories([2], [2], [np.zeros(2, int)], [np.zeros(2, int)], 3, False, False)
    assert _hip.HSMM_ARCS_FRAME_LDS == hat.FRAME_LDS and _hip.HSMM_ARCS_UTT_LDS == hat.UTT_LDS


# --- the categories a bigram loop would count by -------------------------------------------------

def test_bigram_categories_fold_to_the_unit_starts():
    '''On the categories i P + j of the arcs end_i -> start_j (-1 elsewhere, the states
    included) the truth's [P, P] has column sums equal to the unit-start counts without the init
    row.'''
    P, n_states, D = 4, 3, 5
    cg, start, end, _ = _graph(n_units=P, n_states=n_states)
    g = dict(S=cg.n_states, init=cg.init_log_probs.double().numpy(), hub=None,
             final=cg.final_log_probs.double().numpy(), trans=cg.trans_log_probs.double().numpy())
    src, dst = at.out_arcs(g)
    a_src, a_dst = (np.asarray(a) for a in cg.out_arcs())
    assert (a_src == src).all() and (a_dst == dst).all()
    ends, starts = list(end.values()), list(start.values())
    arc_cat = np.asarray([ends.index(i) * P + starts.index(j) if i in ends and j in starts and i != j
                          else -1 for i, j in zip(src, dst)], dtype=np.int32)
    init_cat = np.full(cg.n_states, -1, dtype=np.int32)
    assert (np.sort(arc_cat[arc_cat >= 0]) == np.arange(P * P)).all()
    rng = np.random.RandomState(3)
    ld = rng.uniform(-3, 0, size=(cg.n_states, D))
    lw = -np.log1p(-np.exp(np.diagonal(g['trans'])))
    u_arc, u_init = unit_start_categories(cg, start, end)
    for T in (3, 7, 40):                 # (a unit of three states cannot be crossed in fewer)
        l = rng.randn(T, cg.n_states) * 2
        frame, total = hat.arc_posteriors(g, ld, lw, l, arc_cat, init_cat, P * P)
        units, _ = hat.arc_posteriors(g, ld, lw, l, u_arc, u_init, P)
        assert not frame[0].any()
        assert np.abs(total.reshape(P, P).sum(0) - units[1:].sum(0)).max() <= PIN * T
        assert abs(units[0].sum() - 1.) <= PIN
        p = ht.posteriors(g, ld, lw, l)
        assert np.abs(units.sum(0) - (p['gamma0_sum'] + p['entry_sum'])[starts]).max() <= PIN * T
