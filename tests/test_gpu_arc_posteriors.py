"""The arc posteriors by category (csrc/hmm_arcs.hip) against the float64 truth of
tests/arcs_truth.py, on graphs that sit on the boundaries of the route.

Tolerances, `tol` = 1e-10 (float64) / 1e-5 (float32), the project's:
 * frame_out: |frame_out - truth| <= tol, absolute -- its entries are probabilities;
 * utt_out:   |utt_out[u] - truth| <= tol * (T_u + 1): every row sums to at most 1.

 * One static table: each case names the route `beer_hmm_arcs_route` must report for it in either
   precision, and the table as a whole reaches every value the route can take.
 * Guards around both outputs and the workspace, `pc_llhs` unchanged, either output alone.
 * Categories: a random third -1, everything in one category (rows of 1), arc_cat = dst (gamma,
   also against `hk.forward_backward`), one category per arc (the sparse xi).
 * Graphs of different sizes in one launch, long utterances, a per-frame shift of +-3e4, the
   -inf edges, T = 1.
 * The model level: `HMM.arc_posteriors`, `unit_starts`, `unit_starts_batch` /
   `unit_counts_batch` (against the phone counts of the training E-step too), bound alignment
   graphs, `beer hmm boundaries`."""

import ctypes
import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import arcs_truth as at
import fb_truth as ft
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
K, L, FL, UL = at.BLOCK, at.ARCS_LDS, at.FRAME_LDS, at.UTT_LDS
ALL = K | L | FL | UL
GUARD, SENTINEL = 5, -12345.678

LONG = tuple(ft.VITERBI_LENGTHS) + (7, 8, 9, 3)

# S, offsets, hub members, utterances (a number: fb_truth.lengths; 'long': LONG), the categories
# (a number: drawn, a third of them -1 in every other case; 'gamma': arc_cat = dst, init_cat = j;
# 'arc': one per arc, no init category), the route in float64 and in float32
Case = namedtuple('Case', 'S nO hub nutt cats f64 f32 seed')
CASES = []


def add(S, nO, cats, f64, f32=None, hub=0, nutt=None):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, nutt or (1, 5, 9)[i % 3], cats, f64,
                      f64 if f32 is None else f32, 900 + i))


add(1, 2, 1, ALL)
add(1, 2, 2, ALL, nutt=5)
add(3, 2, 2, ALL)
add(3, 3, 'arc', ALL)
add(8, 2, 7, ALL, nutt='long')
add(8, 8, 'arc', ALL)                    # every arc present
add(8, 3, 'gamma', ALL)
add(64, 12, 'gamma', ALL)
add(64, 2, 1024, ALL)                    # the last n_cat with a frame's bins in LDS ...
add(64, 2, 1025, K | L | UL)             # ... and the first without
add(64, 3, 4096, K | L | UL, hub=8)      # the last n_cat with the utterance's bins in LDS ...
add(64, 3, 4097, K | L)                  # ... and the first without
add(65, 3, 7, ALL)
add(128, 8, 'arc', ALL, nutt='long')     # 1024 arcs
add(129, 8, 'arc', K | L | UL)           # 1032 arcs
add(100, 3, 7, ALL, hub=30)
add(120, 3, 40, ALL, hub=40)             # the shape of config 3's loop
add(256, 3, 'gamma', ALL)
add(257, 3, 2, ALL)
add(509, 3, 7, ALL, nutt='long')
add(256, 12, 'gamma', ALL)
# arcs that no longer fit LDS
add(300, 3, 7, K | FL | UL, hub=100)     # rows of 100 + 3 arcs
add(300, 3, 'gamma', K | FL | UL, hub=100, nutt=5)
add(600, 12, 'arc', K)                   # 7200 arcs, as many categories
add(600, 12, 1025, K | UL)
add(100, 100, 4096, K | UL, nutt=5)      # every arc present at 100 states: 10 000 arcs
add(100, 100, 7, K | FL | UL, nutt=5)


def case_id(c):
    return f'{c.seed}-S{c.S}-O{c.nO}-hub{c.hub}-n{c.nutt}-{c.cats}'


def test_the_cases_reach_every_value_of_the_route():
    forms = {c.f64 for c in CASES} | {c.f32 for c in CASES}
    assert forms == {K | a | f | u for a in (0, L) for f in (0, FL) for u in (0, UL)
                     if (f, u) != (FL, 0)}
    assert {1, 3, 8, 64, 65, 128, 129, 256, 257, 300, 509, 600} <= {c.S for c in CASES}
    assert {2, 3, 8, 12, 100} <= {c.nO for c in CASES}
    assert {1, 2, 7, 'gamma', 'arc', 1024, 1025, 4096, 4097} <= {c.cats for c in CASES}


def packed(llhs):
    return torch.cat([tt(l).reshape(-1) for l in llhs])


def compiled(g, ids=None):
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in (range(g['S']) if ids is None else ids)])
    if g['hub'] is not None:
        E, a, B_, c = g['hub']
        graph.set_hub(E, tt(a), B_, tt(c))
    return graph


def categories(g, kind, seed, drop=0.):
    '(arc_cat, init_cat, n_cat) of a case.'
    src, dst = at.out_arcs(g)
    if kind == 'gamma':
        return dst.astype(np.int32), np.arange(g['S'], dtype=np.int32), g['S']
    if kind == 'arc':
        return np.arange(len(src), dtype=np.int32), -np.ones(g['S'], dtype=np.int32), len(src)
    return at.random_categories(g, kind, seed, drop) + (kind,)


def guarded_call(batch, flat, arc_cats, init_cats, n_cat, per_frame=True, per_utt=True):
    '''beer_hmm_arc_posteriors into the middle of sentinel-filled buffers (both outputs and the
    workspace): (frame or None, utt or None) after the guards were checked.  `arc_cats` /
    `init_cats`: one array per distinct graph of the batch.'''
    n, f = batch.nutt, batch.n_frames
    dev = 'cuda'
    fbuf = torch.full(((f + 2 * GUARD) * n_cat,), SENTINEL, dtype=batch.dtype, device=dev)
    ubuf = torch.full(((n + 2 * GUARD) * n_cat,), SENTINEL, dtype=torch.float64, device=dev)
    n_ws = f + batch.n_elems + _hip.lib().beer_hmm_arcs_scratch_doubles(
        _hip.dtype_code(batch.dtype), batch.ref())
    wbuf = torch.full((n_ws + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    frame = fbuf[GUARD * n_cat:(GUARD + f) * n_cat]
    utt = ubuf[GUARD * n_cat:(GUARD + n) * n_cat]
    arcs = tt(np.concatenate(arc_cats).astype(np.int32))
    inits = tt(np.concatenate(init_cats).astype(np.int32))
    arc_off = tt(np.concatenate([[0], np.cumsum([len(a) for a in arc_cats])[:-1]]).astype(np.int64))
    state_off = tt(np.concatenate([[0], np.cumsum([len(a) for a in init_cats])[:-1]]).astype(np.int64))
    amap = _hip.ArcMap(arcs.data_ptr(), inits.data_ptr(), arc_off.data_ptr(), state_off.data_ptr())
    _hip.call('beer_hmm_arc_posteriors', _hip.dtype_code(batch.dtype), batch.ref(), _hip.ptr(flat),
              ctypes.byref(amap), n_cat, _hip.ptr(wbuf[GUARD:]),
              _hip.ptr(frame) if per_frame else None, _hip.ptr(utt) if per_utt else None)
    torch.cuda.synchronize()
    for what, buf, lo, hi, used in (('frame_out', fbuf, GUARD * n_cat, (GUARD + f) * n_cat, per_frame),
                                    ('utt_out', ubuf, GUARD * n_cat, (GUARD + n) * n_cat, per_utt),
                                    ('ws', wbuf, GUARD, GUARD + n_ws, True)):
        if used:
            assert (buf[:lo] == SENTINEL).all() and (buf[hi:] == SENTINEL).all(), \
                f'a guard element of {what} was written'
        else:
            assert (buf == SENTINEL).all(), f'{what} = NULL, yet something was written'
    return (frame.clone().view(f, n_cat) if per_frame else None,
            utt.clone().view(n, n_cat) if per_utt else None)


def truths_of(g_of, llhs, cats_of, n_cat):
    return [at.arc_posteriors(g_of[u], llhs[u], cats_of[u][0], cats_of[u][1], n_cat)
            for u in range(len(llhs))]


def hold(truths, lens, frame, utt, tol, what):
    '''Both outputs of a batch against the truth: (largest frame error, largest ratio of an
    utterance's error to its bound).'''
    ferr = uerr = 0.
    if frame is not None:
        frame = npy(frame).astype(np.float64)
        assert not np.isnan(frame).any(), f'{what}: NaN in frame_out'
        want = np.concatenate([f for f, _ in truths])
        assert frame.shape == want.shape
        ferr = float(np.abs(frame - want).max()) if want.size else 0.
        print(f'{what}: frame_out off by {ferr:.3e} (bound {tol:.0e})')
        assert ferr <= tol, f'{what}: frame_out off by {ferr:.3e} > {tol:.1e}'
    if utt is not None:
        utt = npy(utt)
        assert utt.dtype == np.float64 and not np.isnan(utt).any(), f'{what}: NaN in utt_out'
        for u, (_, total) in enumerate(truths):
            d = float(np.abs(utt[u] - total).max())
            bound = tol * (lens[u] + 1)
            uerr = max(uerr, d / bound)
            assert d <= bound, f'{what} utterance {u}: utt_out off by {d:.3e} > {bound:.3e}'
        print(f'{what}: utt_out within {uerr:.3e} of its bounds')
    return ferr, uerr


def close_to(a, b, lens, tol, rows):
    'Two runs of the kernel agree within the tolerance (the order of the atomic adds is free).'
    d = np.abs(npy(a).astype(np.float64) - npy(b).astype(np.float64))
    if rows:
        assert d.max(initial=0.) <= tol
    else:
        assert (d.max(axis=1) <= tol * (np.asarray(lens) + 1)).all()


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_arc_posteriors_are_the_truth(case, dtype):
    tol = TOL[dtype]
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype])
    graph = compiled(g)
    lens = list(LONG) if case.nutt == 'long' else ft.lengths(case.nutt, case.seed)
    _, llhs = ft.inputs(g, lens, np.arange(case.S), case.S, 1., case.seed, NP[dtype])
    arc_cat, init_cat, n_cat = categories(g, case.cats, case.seed, (case.seed % 2) / 3.)
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    want = case.f64 if dtype == torch.float64 else case.f32
    route = hk.arcs_route(batch, n_cat, True)
    assert route == want, f'route {route:#x}, the table says {want:#x}'
    for per_frame in (True, False):
        assert hk.arcs_route(batch, n_cat, per_frame) == at.route_formula(
            case.S, batch.struct.max_arcs, tt(llhs[0]).element_size(), n_cat, per_frame)
    src, dst = graph.out_arcs()
    assert batch.n_arcs == [len(src)]
    assert np.array_equal(src, at.out_arcs(g)[0]) and np.array_equal(dst, at.out_arcs(g)[1])
    flat = packed(llhs)
    before = flat.clone()
    frame, utt = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat)
    truths = truths_of([g] * len(lens), llhs, [(arc_cat, init_cat)] * len(lens), n_cat)
    hold(truths, lens, frame, utt, tol, case_id(case))
    assert torch.equal(flat, before), 'pc_llhs was written'
    if case.cats == 'gamma' or (isinstance(case.cats, int) and case.seed % 2 == 0):
        rows = npy(frame).astype(np.float64).sum(1)
        assert np.abs(rows - 1.).max() <= tol * n_cat, 'a row without -1 does not sum to 1'
    if case.cats == 'gamma':
        gamma = hk.forward_backward(batch, flat)[0].view(sum(lens), case.S)
        assert np.abs(npy(gamma).astype(np.float64) - npy(frame).astype(np.float64)).max() <= 2 * tol
    # either output alone: another form of the launch, the same numbers
    f_only, none = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat, per_utt=False)
    assert none is None
    close_to(f_only, frame, lens, tol, True)
    none, u_only = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat, per_frame=False)
    assert none is None
    close_to(u_only, utt, lens, tol, False)
    hold(truths, lens, f_only, u_only, tol, case_id(case) + ' alone')
    # and through the Python face
    f2, u2 = hk.arc_posteriors(batch, flat, [arc_cat], [init_cat], n_cat, per_frame=True, per_utt=True)
    assert f2.dtype == dtype and f2.shape == (sum(lens), n_cat) and f2.is_cuda
    assert u2.dtype == torch.float64 and u2.shape == (len(lens), n_cat)
    hold(truths, lens, f2, u2, tol, case_id(case) + ' hk')
    f3, none = hk.arc_posteriors(batch, flat, tt(arc_cat), tt(init_cat), n_cat)
    assert none is None
    close_to(f3, frame, lens, tol, True)


@DTYPES
def test_every_arc_in_one_category_gives_rows_of_one(dtype):
    S = 65
    g = ft.make_graph(S, ft.offsets(3, S), 77, 0, NP[dtype])
    lens = [9, 1, 33]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 78, NP[dtype])
    A = len(at.out_arcs(g)[0])
    batch = hk.HmmBatch([compiled(g)], [0] * 3, lens, dtype)
    # init_cat = -1: row 0 of every utterance stays 0, every other row is 1
    frame, utt = guarded_call(batch, packed(llhs), [np.zeros(A, np.int32)], [-np.ones(S, np.int32)], 1)
    want = np.ones(sum(lens))
    want[[0, 9, 10]] = 0.
    assert np.abs(npy(frame)[:, 0] - want).max() <= TOL[dtype]
    assert (np.abs(npy(utt)[:, 0] - (np.asarray(lens) - 1)) <= TOL[dtype] * (np.asarray(lens) + 1)).all()


MIXED_LENS, MIXED_GIDS = [33, 65, 32, 2, 64, 1], [0, 1, 2, 0, 2, 1]


@DTYPES
@pytest.mark.parametrize('sizes,want', [((7, 65, 129), ALL), ((7, 65, 300), ALL)], ids=['129', '300'])
def test_graphs_of_different_sizes_in_one_launch(sizes, want, dtype):
    'Alignment-graph style: the form follows the largest graph, every utterance its own categories.'
    arrays = [ft.make_graph(S, ft.offsets(3, S), 2300 + k, 0, NP[dtype]) for k, S in enumerate(sizes)]
    graphs = [compiled(g) for g in arrays]
    n_cat = 11
    cats = [at.random_categories(g, n_cat, 40 + k, 1 / 3.) for k, g in enumerate(arrays)]
    rng = np.random.RandomState(5)
    llhs = [(rng.randn(T, sizes[k]) * 3).astype(NP[dtype]) for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert hk.arcs_route(batch, n_cat) == want
    frame, utt = guarded_call(batch, packed(llhs), [c[0] for c in cats], [c[1] for c in cats], n_cat)
    truths = truths_of([arrays[k] for k in MIXED_GIDS], llhs, [cats[k] for k in MIXED_GIDS], n_cat)
    hold(truths, MIXED_LENS, frame, utt, TOL[dtype], str(sizes))
    f2, u2 = hk.arc_posteriors(batch, packed(llhs), [c[0] for c in cats], [c[1] for c in cats],
                               n_cat, per_utt=True)
    hold(truths, MIXED_LENS, f2, u2, TOL[dtype], str(sizes) + ' hk')
    with pytest.raises(ValueError):
        hk.arc_posteriors(batch, packed(llhs), [c[0] for c in cats][:2], [c[1] for c in cats], n_cat)


# --- length: drift and range ---------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize('S,T', [(16, 4096), (300, 1000)], ids=['S16', 'S300'])
def test_long_utterances(S, T, dtype):
    g = ft.make_graph(S, ft.offsets(3, S), 31, 0, NP[dtype])
    _, llhs = ft.inputs(g, [T], np.arange(S), S, 1., 32, NP[dtype])
    arc_cat, init_cat = at.random_categories(g, 5, 33)
    batch = hk.HmmBatch([compiled(g)], [0], [T], dtype)
    assert hk.arcs_route(batch, 5) == ALL
    frame, utt = hk.arc_posteriors(batch, packed(llhs), [arc_cat], [init_cat], 5, per_utt=True)
    truths = truths_of([g], llhs, [(arc_cat, init_cat)], 5)
    hold(truths, [T], frame, utt, TOL[dtype], f'S={S} T={T}')
    assert np.abs(npy(frame).astype(np.float64).sum(1) - 1.).max() <= 5 * TOL[dtype]


@DTYPES
@pytest.mark.parametrize('S,nO', [(16, 3), (300, 3)], ids=['S16', 'S300'])
def test_a_per_frame_shift_leaves_the_posteriors(S, nO, dtype):
    '''k_t in +-3e4 added to every entry of row t changes no posterior.  The log-likelihoods and
    the shifts are multiples of 1/64 (below 2^24 / 64): the shifted rows are exact in float32.'''
    tol = TOL[dtype]
    g = ft.make_graph(S, ft.offsets(nO, S), 51, 0, NP[dtype])
    lens = [200, 1, 9, 33]
    rng = np.random.RandomState(52)
    base = [(rng.randint(-512, 513, size=(T, S)) / 64.).astype(NP[dtype]) for T in lens]
    ks = [rng.randint(-30000 * 64, 30000 * 64 + 1, size=T) / 64. for T in lens]
    shifted = [(l.astype(np.float64) + k[:, None]).astype(NP[dtype]) for l, k in zip(base, ks)]
    for l, s, k in zip(base, shifted, ks):
        assert (s.astype(np.float64) - l.astype(np.float64) == k[:, None]).all()
    arc_cat, init_cat = at.random_categories(g, 7, 53, 1 / 3.)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    f0, u0 = hk.arc_posteriors(batch, packed(base), [arc_cat], [init_cat], 7, per_utt=True)
    f1, u1 = hk.arc_posteriors(batch, packed(shifted), [arc_cat], [init_cat], 7, per_utt=True)
    truths = truths_of([g] * len(lens), base, [(arc_cat, init_cat)] * len(lens), 7)
    hold(truths, lens, f0, u0, tol, 'unshifted')
    hold(truths, lens, f1, u1, tol, 'shifted')
    close_to(f1, f0, lens, tol, True)
    close_to(u1, u0, lens, tol, False)


# --- edges -----------------------------------------------------------------------------------
EDGE_GRAPHS = pytest.mark.parametrize('S', [8, 300])


def edge_graph(S, dtype, last_only=False):
    'Self-loop and step to the next state; `last_only`: only the last state may end an utterance.'
    g = ft.make_graph(S, (0, 1), 5, 0, NP[dtype])
    if last_only:
        g['final'][:] = -np.inf
        g['final'][S - 1] = 0.
    return g


def edge_run(g, llhs, lens, dtype, what, n_cat=6):
    arc_cat, init_cat = at.random_categories(g, n_cat, 11, 1 / 3.)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    flat = packed(llhs)
    before = flat.clone()
    frame, utt = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat)
    assert torch.equal(flat, before), 'pc_llhs was written'
    truths = truths_of([g] * len(lens), llhs, [(arc_cat, init_cat)] * len(lens), n_cat)
    hold(truths, lens, frame, utt, TOL[dtype], what)
    # the global-bin variants take the same edges
    big = 4097
    f2, u2 = guarded_call(batch, flat, [arc_cat], [init_cat], big)
    assert not npy(f2)[:, n_cat:].any() and not npy(u2)[:, n_cat:].any()
    close_to(f2[:, :n_cat], frame, lens, TOL[dtype], True)
    close_to(u2[:, :n_cat], utt, lens, TOL[dtype], False)
    return npy(frame).astype(np.float64), npy(utt), truths


@DTYPES
@EDGE_GRAPHS
def test_scattered_inf_entries_that_leave_the_utterance_reachable(S, dtype):
    g = edge_graph(S, dtype)
    lens = [12, 1, 5, 30]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 6, NP[dtype])
    rng = np.random.RandomState(7)
    for l in llhs:
        holes = rng.random_sample(l.shape) < .3
        holes[:, 0] = False                             # state 0 and its self-loop stay
        l[holes] = -np.inf
    frame, utt, truths = edge_run(g, llhs, lens, dtype, f'holes S={S}')
    assert all(f.any() for f, _ in truths)


@DTYPES
@EDGE_GRAPHS
def test_a_dead_frame_in_one_utterance_of_five(S, dtype):
    g = edge_graph(S, dtype)
    lens = [6, 5, 7, 4, 9]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 8, NP[dtype])
    f0, u0, _ = edge_run(g, llhs, lens, dtype, f'alive S={S}')
    llhs[2][3] = -np.inf                                # nothing explains frame 3 of utterance 2
    f1, u1, truths = edge_run(g, llhs, lens, dtype, f'dead frame S={S}')
    off = np.concatenate([[0], np.cumsum(lens)])
    assert not f1[off[2]:off[3]].any() and not u1[2].any(), 'a dead utterance is all zeros'
    keep = np.setdiff1d(np.arange(off[-1]), np.arange(off[2], off[3]))
    assert np.abs(f1[keep] - f0[keep]).max() <= TOL[dtype]
    assert f0[off[2]:off[3]].any()


@DTYPES
@EDGE_GRAPHS
def test_an_unreachable_final_gives_zeros(S, dtype):
    '''Only the last state may end an utterance; utterances shorter than S - 3 frames cannot
    reach it from the three initial states.'''
    g = edge_graph(S, dtype, last_only=True)
    lens = [1, 2, S + 4, 5]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 9, NP[dtype])
    frame, utt, truths = edge_run(g, llhs, lens, dtype, f'unreachable final S={S}')
    assert not utt[0].any() and not utt[1].any() and utt[2].any()
    assert bool(utt[3].any()) == (5 >= S - 2)
    assert not frame[:3].any()


@DTYPES
@pytest.mark.parametrize('S', [8, 65, 300])
def test_one_frame(S, dtype):
    g = ft.make_graph(S, ft.offsets(3, S), 9, 0, NP[dtype])
    _, llhs = ft.inputs(g, [1], np.arange(S), S, 1., 9, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0], [1], dtype)
    A = len(at.out_arcs(g)[0])
    frame, utt = guarded_call(batch, packed(llhs), [np.zeros(A, np.int32)], [np.arange(S, dtype=np.int32)], S)
    # gamma_0 over the three initial states, weighted by the final term
    a = sum(v[:3].astype(np.float64) for v in (g['init'], llhs[0][0], g['final']))
    want = np.zeros(S)
    want[:3] = np.exp(a - a.max()) / np.exp(a - a.max()).sum()
    assert np.abs(npy(frame)[0] - want).max() <= TOL[dtype]
    assert np.abs(npy(utt)[0] - want).max() <= 2 * TOL[dtype]


def test_an_utterance_of_no_frames_and_an_empty_batch():
    g = ft.make_graph(8, ft.offsets(3, 8), 3)
    lens = [4, 0, 3]
    _, llhs = ft.inputs(g, lens, np.arange(8), 8, 1., 4)
    arc_cat, init_cat = at.random_categories(g, 3, 5)
    batch = hk.HmmBatch([compiled(g)], [0] * 3, lens, torch.float64)
    frame, utt = guarded_call(batch, packed(llhs), [arc_cat], [init_cat], 3)
    truths = [at.arc_posteriors(g, llhs[0], arc_cat, init_cat, 3), (np.zeros((0, 3)), np.zeros(3)),
              at.arc_posteriors(g, llhs[2], arc_cat, init_cat, 3)]
    hold(truths, lens, frame, utt, 1e-10, 'no frames')
    assert not npy(utt)[1].any()
    empty = hk.HmmBatch([compiled(g)], [], [], torch.float64)
    f, u = hk.arc_posteriors(empty, torch.zeros(0, dtype=torch.float64, device='cuda'), [arc_cat],
                             [init_cat], 3, per_utt=True)
    assert f.shape == (0, 3) and u.shape == (0, 3)


def test_arguments_are_checked():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    graph = compiled(g)
    batch = hk.HmmBatch([graph], [0], [4], torch.float64)
    flat = torch.zeros(12, dtype=torch.float64, device='cuda')
    A = len(graph.out_arcs()[0])
    a, i = np.zeros(A, np.int32), np.zeros(3, np.int32)
    for bad in ((a[:-1], i, 2), (a, i[:-1], 2), (a + 2, i, 2), (a, i - 2, 2), (a, i, 0)):
        with pytest.raises(ValueError):
            hk.arc_posteriors(batch, flat, [bad[0]], [bad[1]], bad[2])
    with pytest.raises(ValueError):
        hk.arc_posteriors(batch, flat, [a], [i], 2, per_frame=False, per_utt=False)
    with pytest.raises(_hip.HipInvalid):
        hk.arcs_route(batch, 0)


# --- model level -----------------------------------------------------------------------------------

_TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
         {'start_id': 1, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 2, 'trans_prob': .5},
         {'start_id': 2, 'end_id': 3, 'trans_prob': .5}, {'start_id': 3, 'end_id': 3, 'trans_prob': .5},
         {'start_id': 3, 'end_id': 4, 'trans_prob': .5}]
D = 4


def make_model(kind):
    torch.manual_seed(3)
    conf = {'g': {'topology': _TOPO, 'n_normal_per_state': 2, 'prior_strength': 1.,
                  'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(4)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(D), torch.ones(D))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    if kind == 'hmm':
        model = beer.HMM.create(graph.compile(), ems)
    elif kind == 'bigram':
        model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet2')
        assert isinstance(model, beer.BigramPhoneLoop)
    else:
        model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet')
        assert type(model) is beer.PhoneLoop
    return model.double().to('cuda')


def utterances(lens, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randn(T, D) * 1.5).to('cuda') for T in lens]


def dense_arrays(graph):
    return dict(S=graph.n_states, init=npy(graph.init_log_probs), final=npy(graph.final_log_probs),
                trans=npy(graph.trans_log_probs))


def model_llh(model, X, ids, scale):
    'Per-state log-likelihoods from the per-pdf ones the model itself computes, read back.'
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    return scale * npy(pc_all).astype(np.float64)[:, np.asarray([int(i) for i in ids])]


def unit_categories_by_hand(arrays, ids, start_pdf, end_pdf):
    'The unit-start categories from state pairs, restated: no code of the package.'
    ids = [int(i) for i in ids]
    firsts = [int(start_pdf[u]) for u in start_pdf]
    src, dst = at.out_arcs(arrays)
    arc_cat = np.asarray([firsts.index(ids[j]) if i != j and ids[j] in firsts else -1
                          for i, j in zip(src, dst)], dtype=np.int32)
    init_cat = -np.ones(len(ids), dtype=np.int32)
    for k, u in enumerate(start_pdf):
        for j, p in enumerate(ids):
            if int(start_pdf[u]) <= p <= int(end_pdf[u]):
                init_cat[j] = k
    return arc_cat, init_cat


def hold_one(got, want, T, per_frame, what):
    assert got.is_cuda and not torch.isnan(got).any()
    d = np.abs(npy(got).astype(np.float64) - want).max(initial=0.)
    bound = 1e-10 if per_frame else 1e-10 * (T + 1)
    assert got.shape == want.shape and d <= bound, f'{what}: off by {d:.3e} > {bound:.1e}'


@pytest.mark.parametrize('kind', ['hmm', 'phoneloop', 'bigram'])
def test_model_arc_posteriors_and_unit_starts_are_the_truth(kind):
    model = make_model(kind)
    arrays = dense_arrays(model.graph)
    ids = model.graph.pdf_id_mapping
    arc_cat, init_cat = at.random_categories(arrays, 5, 21, 1 / 3.)
    for X, scale in zip(utterances([57, 1, 23], 1), (1., 1., .7)):
        llh = model_llh(model, X, ids, scale)
        frame, utt = at.arc_posteriors(arrays, llh, arc_cat, init_cat, 5)
        got = model.arc_posteriors(X, arc_cat, init_cat, 5, scale=scale)
        assert got.dtype == torch.float64
        hold_one(got, frame, len(X), True, kind)
        got = model.arc_posteriors(X, torch.from_numpy(arc_cat), init_cat, 5, scale=scale,
                                   inference_graph=model.graph, per_frame=False)
        assert got.dtype == torch.float64
        hold_one(got, utt, len(X), False, kind)
        if kind == 'hmm':
            assert not hasattr(model, 'unit_starts')
            continue
        hand = unit_categories_by_hand(arrays, ids, model.start_pdf, model.end_pdf)
        frame, utt = at.arc_posteriors(arrays, llh, hand[0], hand[1], len(model.start_pdf))
        got = model.unit_starts(X, scale=scale)
        hold_one(got, frame, len(X), True, kind + ' unit_starts')
        if len(X) > 1:
            # (one frame cannot reach the end of a left-to-right unit: zeros)
            assert abs(float(got[0].sum()) - 1.) <= 1e-10 and float(got.sum()) >= 1.


def test_unit_counts_are_the_phone_counts_of_the_training_estep():
    '''On a free phone loop the only arcs that enter a unit's first state from another state are
    the hub's: the expected unit counts are the phone counts the E-step accumulates.'''
    model = make_model('phoneloop')
    lens = [23, 40, 9, 31, 5]
    utts = utterances(lens, 3)
    counts = beer.unit_counts_batch(model, utts)
    assert counts.shape == (len(lens), 4) and counts.dtype == torch.float64 and counts.is_cuda
    elbo = beer.accumulate_elbo(model, utts)
    wparam = model.categorical.mean_field_factorization()[0][0]
    trained = npy(elbo._acc_stats[wparam]).astype(np.float64).reshape(-1)
    assert trained.shape == (4,)
    # the statistics of the weights hold the counts' sum in their last entry
    # (CategoricalLikelihood.sufficient_statistics): undo that
    trained[-1] -= trained[:-1].sum()
    d = np.abs(npy(counts).sum(0) - trained).max()
    bound = 1e-10 * sum(T + 1 for T in lens)
    print(f'unit counts against the E-step phone counts: off by {d:.3e} (bound {bound:.3e})')
    assert d <= bound
    assert trained.sum() > len(lens)


@pytest.mark.parametrize('kind', ['phoneloop', 'bigram'])
def test_batch_functions_are_unit_starts_per_utterance(kind):
    model = make_model(kind)
    lens = [23, 40, 9, 31, 1]
    utts = utterances(lens, 3)
    one_by_one = [model.unit_starts(X, scale=.9) for X in utts]
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        starts = beer.unit_starts_batch(model, utts, scale=.9, max_frames=max_frames)
        counts = beer.unit_counts_batch(model, utts, scale=.9, max_frames=max_frames)
        assert [tuple(s.shape) for s in starts] == [(T, 4) for T in lens]
        assert counts.shape == (len(lens), 4) and counts.dtype == torch.float64 and counts.is_cuda
        for u, want in enumerate(one_by_one):
            assert starts[u].dtype == torch.float64
            assert np.abs(npy(starts[u]) - npy(want)).max() <= 1e-10, (max_frames, u)
            assert np.abs(npy(counts[u]) - npy(want).sum(0)).max() <= 1e-10 * (lens[u] + 1)
    packed_in = (torch.cat(utts), lens)
    again = beer.unit_counts_batch(model, packed_in, scale=.9)
    assert np.abs(npy(again) - npy(counts)).max() <= 1e-10 * (max(lens) + 1)


def test_bound_alignment_graphs_after_the_posterior_moved():
    'E[ln a] of the CURRENT posterior is on the arcs: the bound image is refreshed by the call.'
    from aligned_truth import CategoryMap, alignment_set, expected_log_probs, loop_model
    model, units = loop_model(torch.float64, seed=3)
    model = model.to('cuda')
    seqs = [['s0'], ['s0', 'n0', 's0', 's0'], ['s1', 's0', 'n0', 's2', 's0']]
    gset = alignment_set(units, seqs)
    bound = model.bind_alignment_graphs(gset)
    lens = [7, 40, 61]
    rng = np.random.RandomState(4)
    utts = [torch.from_numpy(rng.randn(T, 4) * 1.5).to('cuda') for T in lens]
    stale = [npy(model.unit_starts(X, inference_graph=bound[i])) for i, X in enumerate(utts)]
    gen = torch.Generator().manual_seed(1)
    for p in model.transitions.parameters_of_groups():
        conc = p.posterior.params.concentrations
        conc.add_(torch.rand(conc.shape, generator=gen, dtype=torch.float64).to(conc) * 3)
    model._on_transitions_update()
    tmap, log_a = CategoryMap(model), expected_log_probs(model.transitions)
    n_units = len(model.start_pdf)
    names = list(model.start_pdf)
    truths = []
    for i, X in enumerate(utts):
        dense = gset[i].to_dense()
        src, dst, cats, last = tmap.arcs(seqs[i], dense)
        trans = np.full((len(last), len(last)), -np.inf)
        trans[src, dst] = log_a[cats]
        arrays = dict(S=len(last), init=dense.init_log_probs.double().numpy(),
                      final=dense.final_log_probs.double().numpy(), trans=trans)
        hand = unit_categories_by_hand(arrays, dense.pdf_id_mapping, model.start_pdf, model.end_pdf)
        llh = model_llh(model, X, dense.pdf_id_mapping, .8)
        truths.append(at.arc_posteriors(arrays, llh, hand[0], hand[1], n_units))
        got = model.unit_starts(X, inference_graph=bound[i], scale=.8)
        hold_one(got, truths[-1][0], lens[i], True, f'bound graph {i}')
        if len(seqs[i]) > 1:            # (one unit begins at frame 0, whatever the weights)
            moved = npy(model.unit_starts(X, inference_graph=bound[i]))
            assert np.abs(moved - stale[i]).max() > 1e-6
        # a chain: every unit of the transcription begins exactly once
        want = np.asarray([seqs[i].count(n) for n in names], dtype=np.float64)
        assert np.abs(truths[-1][1] - want).max() <= 1e-9
    starts = beer.unit_starts_batch(model, utts, inference_graphs=list(bound), scale=.8, max_frames=50)
    counts = beer.unit_counts_batch(model, utts, inference_graphs=list(bound), scale=.8, max_frames=50)
    for i, (frame, utt) in enumerate(truths):
        hold_one(starts[i], frame, lens[i], True, f'batched bound graph {i}')
        hold_one(counts[i], utt, lens[i], False, f'batched bound graph {i}')
    with pytest.raises(ValueError):
        beer.unit_starts_batch(model, utts, inference_graphs=list(bound)[:2])


def run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_boundaries(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    run(['dataset', 'create', str(tmp_path), feats, ds])
    out_dir = tmp_path / 'starts'
    out = run(['hmm', 'boundaries', '--counts', mdl, ds, str(out_dir)]).strip().split('\n')
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    n_units = len(model.start_pdf)
    want = beer.unit_counts_batch(model, utts).cpu().numpy()
    starts = beer.unit_starts_batch(model, utts)
    assert sorted(os.listdir(out_dir)) == [f'{u}.npy' for u in ids]
    assert [l.split()[0] for l in out] == ids
    for u, line, T in zip(range(3), out, (35, 50, 41)):
        post = np.load(out_dir / f'{ids[u]}.npy')
        assert post.shape == (T, n_units)
        assert np.abs(post - npy(starts[u])).max() <= TOL[starts[u].dtype]
        printed = np.asarray([float(v) for v in line.split()[1:]])
        assert printed.shape == (n_units,)
        assert np.abs(printed - want[u]).max() <= 1e-6          # (%.6f of the same float64)
        assert np.abs(post.sum(0) - want[u]).max() <= TOL[starts[u].dtype] * (T + 1)
    # without --counts nothing is printed; a scale and a list of utterances
    (tmp_path / 'utts').write_text('utt2\n')
    out2 = tmp_path / 'two'
    assert run(['hmm', 'boundaries', '-s', '0.5', '-u', str(tmp_path / 'utts'), mdl, ds, str(out2)]) == ''
    assert os.listdir(out2) == ['utt2.npy']
    half = beer.unit_starts_batch(model, [utts[2]], scale=.5)[0]
    assert np.abs(np.load(out2 / 'utt2.npy') - npy(half)).max() <= TOL[half.dtype]
