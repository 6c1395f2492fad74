"""The Viterbi max-marginals (csrc/hmm_lattice.hip) against the float64 truth of
tests/lattice_truth.py, on graphs that sit on the boundaries of the route.

Tolerance, derived: every output of utterance u is a float64 sum of at most 2 T_u + 2 terms whose
partial sums are bounded by B_u (`lattice_truth.bound`), compared with a truth that sums the same
terms:  |out - truth| <= 4 (T_u + 1) 2^-52 B_u + r |truth|,  r = 0 for the float64 outputs and
2^-23 for the float32-stored `state_out` / `frame_out`; -inf must match -inf exactly.

 * One static table: each case names the route `beer_hmm_maxmarg_route` must report for it, and
   the table as a whole reaches every value the route can take.
 * Guards around all four outputs and the workspace, `pc_llhs` unchanged, each output alone (the
   states with a NULL map), two calls bit for bit the same, 'gamma' categories bit for bit the
   states.
 * Integer inputs: every output exactly the truth, mm <= 0, mm == 0 along `hk.viterbi`'s path,
   `best` and the second-best score against `hk.viterbi_nbest`.
 * Graphs of different sizes in one launch, a long utterance, a per-frame shift of +-3e4, the
   -inf edges, an utterance of no frames.
 * The model level: `HMM.max_marginals`, `arc_max_marginals`, `unit_start_margins`,
   `unit_start_margins_batch`, bound alignment graphs, `beer hmm lattice`."""

import ctypes
import functools
import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import fb_truth as ft
import lattice_truth as lt
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
R = {torch.float64: 0., torch.float32: 2. ** -23}       # rounding of the stored per-frame outputs
EPS = {torch.float64: 2. ** -53, torch.float32: 2. ** -24}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
K, L, BL = lt.BLOCK, lt.ARCS_LDS, lt.BINS_LDS
ALL = K | L | BL
GUARD, SENTINEL = 5, -12345.678

LONG = tuple(ft.VITERBI_LENGTHS) + (7, 8, 9, 3)

# S, offsets, hub members, utterances (a number: fb_truth.lengths; 'long': LONG), the categories
# (a number: drawn, a third of them -1 in every other case; 'gamma': arc_cat = dst, init_cat = j;
# 'arc': one per arc, no init category), the route with every output asked for (the same in
# both precisions at these shapes)
Case = namedtuple('Case', 'S nO hub nutt cats route seed')
CASES = []


def add(S, nO, cats, route, hub=0, nutt=None):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, nutt or (1, 5, 9)[i % 3], cats, route, 700 + i))


add(1, 2, 1, ALL)
add(1, 2, 2, ALL, nutt=5)
add(3, 2, 2, ALL)
add(3, 3, 'arc', ALL)
add(8, 2, 7, ALL, nutt='long')
add(8, 8, 'arc', ALL)                    # every arc present
add(8, 3, 'gamma', ALL)
add(64, 12, 'gamma', ALL)
add(64, 2, 2048, ALL)                    # the last n_cat with the bins in LDS ...
add(64, 2, 2049, K | L)                  # ... and the first with the bins in the output rows
add(64, 48, 'arc', K | L, nutt=5)        # rows of 48 arcs: 3072 arcs, as many categories
add(65, 3, 7, ALL, hub=8)
add(128, 8, 'arc', ALL, nutt='long')     # 1024 arcs
add(129, 8, 'arc', ALL)                  # 1032 arcs
add(100, 3, 7, ALL, hub=30)
add(120, 3, 40, ALL, hub=40)             # the shape of config 3's loop
add(256, 3, 'gamma', ALL)                # the last S with a state per thread ...
add(257, 3, 2, ALL)                      # ... and the first without
add(509, 3, 7, ALL, nutt='long')
add(256, 12, 'arc', K | L, nutt=5)       # 3072 arcs in LDS, their bins in the output rows
# arcs that no longer fit LDS
add(300, 3, 7, K | BL, hub=100)          # rows of 100 + 3 arcs
add(300, 3, 'gamma', K | BL, hub=100, nutt=5)
add(600, 12, 'arc', K)                   # 7200 arcs, as many categories
add(600, 12, 2048, K | BL, nutt=5)
add(100, 100, 2049, K, nutt=5)           # every arc present at 100 states: 10 000 arcs
add(100, 100, 7, K | BL, nutt=5)


def case_id(c):
    return f'{c.seed}-S{c.S}-O{c.nO}-hub{c.hub}-n{c.nutt}-{c.cats}'


def test_the_cases_reach_every_value_of_the_route():
    assert {c.route for c in CASES} == {K | a | b for a in (0, L) for b in (0, BL)}
    assert {1, 3, 8, 64, 65, 128, 129, 256, 257, 300, 509, 600} <= {c.S for c in CASES}
    assert {2, 3, 8, 12, 48, 100} <= {c.nO for c in CASES}
    assert {1, 2, 7, 'gamma', 'arc', 2048, 2049} <= {c.cats for c in CASES}
    assert {1, 5, 9, 'long'} <= {c.nutt for c in CASES}


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
    if kind == 'gamma':
        return lt.gamma_categories(g)
    if kind == 'arc':
        return lt.arc_categories(g)
    return lt.random_categories(g, kind, seed, drop) + (kind,)


def guarded_call(batch, flat, arc_cats, init_cats, n_cat, states=True, per_frame=True,
                 per_utt=True):
    '''beer_hmm_max_marginals into the middle of sentinel-filled buffers (the four outputs and the
    workspace): (best, state or None, frame or None, utt or None) after the guards were checked.
    `arc_cats` / `init_cats`: one array per distinct graph of the batch, or None: a NULL map.'''
    n, f, m = batch.nutt, batch.n_frames, batch.n_elems
    dev = 'cuda'
    sbuf = torch.full((m + 2 * GUARD,), SENTINEL, dtype=batch.dtype, device=dev)
    fbuf = torch.full(((f + 2 * GUARD) * max(n_cat, 1),), SENTINEL, dtype=batch.dtype, device=dev)
    ubuf = torch.full(((n + 2 * GUARD) * max(n_cat, 1),), SENTINEL, dtype=torch.float64, device=dev)
    bbuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    n_ws = m + _hip.lib().beer_hmm_maxmarg_scratch_doubles(_hip.dtype_code(batch.dtype), batch.ref())
    wbuf = torch.full((n_ws + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    state = sbuf[GUARD:GUARD + m]
    frame = fbuf[GUARD * n_cat:(GUARD + f) * n_cat]
    utt = ubuf[GUARD * n_cat:(GUARD + n) * n_cat]
    amap = None
    if arc_cats is not None:
        arcs = tt(np.concatenate(arc_cats).astype(np.int32))
        inits = tt(np.concatenate(init_cats).astype(np.int32))
        arc_off = tt(np.concatenate([[0], np.cumsum([len(a) for a in arc_cats])[:-1]]).astype(np.int64))
        state_off = tt(np.concatenate([[0], np.cumsum([len(a) for a in init_cats])[:-1]]).astype(np.int64))
        amap = ctypes.byref(_hip.ArcMap(arcs.data_ptr(), inits.data_ptr(), arc_off.data_ptr(),
                                        state_off.data_ptr()))
    _hip.call('beer_hmm_max_marginals', _hip.dtype_code(batch.dtype), batch.ref(), _hip.ptr(flat),
              amap, n_cat, _hip.ptr(wbuf[GUARD:]), _hip.ptr(state) if states else None,
              _hip.ptr(frame) if per_frame else None, _hip.ptr(utt) if per_utt else None,
              _hip.ptr(bbuf[GUARD:]))
    torch.cuda.synchronize()
    for what, buf, lo, hi, used in (('state_out', sbuf, GUARD, GUARD + m, states),
                                    ('frame_out', fbuf, GUARD * n_cat, (GUARD + f) * n_cat, per_frame),
                                    ('utt_out', ubuf, GUARD * n_cat, (GUARD + n) * n_cat, per_utt),
                                    ('best', bbuf, GUARD, GUARD + n, True),
                                    ('ws', wbuf, GUARD, GUARD + n_ws, True)):
        if used:
            assert (buf[:lo] == SENTINEL).all() and (buf[hi:] == SENTINEL).all(), \
                f'a guard element of {what} was written'
        else:
            assert (buf == SENTINEL).all(), f'{what} = NULL, yet something was written'
    return (bbuf[GUARD:GUARD + n].clone(), state.clone() if states else None,
            frame.clone().view(f, n_cat) if per_frame else None,
            utt.clone().view(n, n_cat) if per_utt else None)


def truths_of(g_of, llhs, cats_of, n_cat):
    'Per utterance: (best, mm, frame, utt) and the bound B_u.'
    return [lt.max_marginals(g_of[u], llhs[u], *(cats_of[u] if cats_of else (None, None)), n_cat) +
            (lt.bound(g_of[u], llhs[u]),) for u in range(len(llhs))]


def share(got, want, B, T, r, what):
    '''|got - want| <= 4 (T + 1) 2^-52 B + r |want|, -inf exactly where the truth has it, no NaN:
    the largest share of the bound that is used.'''
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f'{what}: shape {got.shape}, not {want.shape}'
    assert not np.isnan(got).any(), f'{what}: NaN'
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), f'{what}: -inf in other places than the truth'
    assert (got[~fin] == -np.inf).all(), f'{what}: +inf'
    tol = lt.tolerance(B, T, want, r)
    d = np.abs(got[fin] - want[fin])
    worst = float((d / np.broadcast_to(tol, want.shape)[fin]).max(initial=0.))
    assert worst <= 1., f'{what}: off by {d.max():.3e}, {worst:.3f} of the bound'
    return worst


def hold(truths, lens, sizes, out, dtype, what, exact=False):
    '''The outputs of a batch (best, state, frame, utt; None: not asked) against the truth,
    utterance by utterance: the largest share of the bound.  `exact`: equality.'''
    best, state, frame, utt = (None if o is None else npy(o) for o in out)
    assert best.dtype == np.float64 and (utt is None or utt.dtype == np.float64)
    worst, f0, e0 = 0., 0, 0
    for u, (tb, tmm, tframe, tutt, B) in enumerate(truths):
        T, S = lens[u], sizes[u]
        pairs = [('best', best[u], tb, 0.)]
        if state is not None:
            pairs.append(('state_out', state[e0:e0 + T * S].reshape(T, S), tmm, R[dtype]))
        if frame is not None:
            pairs.append(('frame_out', frame[f0:f0 + T], tframe, R[dtype]))
        if utt is not None:
            pairs.append(('utt_out', utt[u], tutt if T else np.full(utt.shape[1], -np.inf), 0.))
        for name, got, want, r in pairs:
            if exact:
                assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want)), \
                    f'{what} utterance {u}: {name} is not exactly the truth'
            else:
                worst = max(worst, share(got, want, B, T, r, f'{what} utterance {u}: {name}'))
        f0, e0 = f0 + T, e0 + T * S
    if not exact:
        print(f'{what}: within {worst:.3f} of the bound')
    return worst


def same_bits(a, b, what):
    for name, x, y in zip(('best', 'state_out', 'frame_out', 'utt_out'), a, b):
        if x is not None and y is not None:
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), \
                f'{what}: {name} differs in its bits'


@functools.lru_cache(maxsize=None)
def case_data(case, dtype, integer):
    'Graph, lengths, inputs, categories and truths of a case: computed once, never changed.'
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype], integer)
    lens = list(LONG) if case.nutt == 'long' else ft.lengths(case.nutt, case.seed)
    if integer:
        llhs = ft.viterbi_inputs(case.S, lens, case.seed, NP[dtype])
    else:
        _, llhs = ft.inputs(g, lens, np.arange(case.S), case.S, 1., case.seed, NP[dtype])
    arc_cat, init_cat, n_cat = categories(g, case.cats, case.seed, (case.seed % 2) / 3.)
    truths = truths_of([g] * len(lens), llhs, [(arc_cat, init_cat)] * len(lens), n_cat)
    return g, lens, llhs, arc_cat, init_cat, n_cat, truths


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_max_marginals_are_the_truth(case, dtype):
    g, lens, llhs, arc_cat, init_cat, n_cat, truths = case_data(case, dtype, False)
    graph = compiled(g)
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    route = hk.maxmarg_route(batch, n_cat, True, True, True)
    assert route == case.route, f'route {route:#x}, the table says {case.route:#x}'
    w = tt(llhs[0]).element_size()
    for wants in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)):
        assert hk.maxmarg_route(batch, n_cat, *wants) == lt.route_formula(
            case.S, batch.struct.max_arcs, w, n_cat, *wants)
    src, dst = graph.out_arcs()
    assert batch.n_arcs == [len(src)]
    assert np.array_equal(src, lt.out_arcs(g)[0]) and np.array_equal(dst, lt.out_arcs(g)[1])
    flat = packed(llhs)
    before = flat.clone()
    sizes = [case.S] * len(lens)
    out = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat)
    hold(truths, lens, sizes, out, dtype, case_id(case))
    assert torch.equal(flat, before), 'pc_llhs was written'
    if case.cats == 'gamma':
        same_bits((None, out[1].view(-1), None, None), (None, out[2].reshape(-1), None, None),
                  'gamma categories: frame_out against state_out')
    # folding by maximum has no order: the same bits again
    same_bits(out, guarded_call(batch, flat, [arc_cat], [init_cat], n_cat), 'a second call')
    # each output alone (the states with a NULL map): other forms of the launch, the same bits
    alone = guarded_call(batch, flat, None, None, 0, per_frame=False, per_utt=False)
    assert alone[2] is None and alone[3] is None
    same_bits(out, alone, 'state_out alone')
    alone = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat, states=False, per_utt=False)
    assert alone[1] is None and alone[3] is None
    same_bits(out, alone, 'frame_out alone')
    alone = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat, states=False, per_frame=False)
    assert alone[1] is None and alone[2] is None
    same_bits(out, alone, 'utt_out alone')
    # and through the Python face
    py = hk.max_marginals(batch, flat, [arc_cat], [init_cat], n_cat, per_frame=True, per_utt=True)
    assert py[0].dtype == torch.float64 and py[0].shape == (len(lens),) and py[0].is_cuda
    assert py[1].dtype == dtype and py[1].shape == (batch.n_elems,)
    assert py[2].dtype == dtype and py[2].shape == (sum(lens), n_cat)
    assert py[3].dtype == torch.float64 and py[3].shape == (len(lens), n_cat)
    same_bits(out, (py[0], py[1], py[2], py[3]), 'hk.max_marginals')
    py = hk.max_marginals(batch, flat)
    assert py[2] is None and py[3] is None
    same_bits(out, py, 'hk.max_marginals, states alone')
    py = hk.max_marginals(batch, flat, tt(arc_cat), tt(init_cat), n_cat, states=False, per_utt=True)
    assert py[1] is None and py[2] is None
    same_bits(out, py, 'hk.max_marginals, utt alone, categories on the device')


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_integer_inputs_are_exact(case, dtype):
    g, lens, llhs, arc_cat, init_cat, n_cat, truths = case_data(case, dtype, True)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    flat = packed(llhs)
    out = guarded_call(batch, flat, [arc_cat], [init_cat], n_cat)
    hold(truths, lens, [case.S] * len(lens), out, dtype, case_id(case), exact=True)
    best, mm = npy(out[0]), npy(out[1]).astype(np.float64)
    assert (mm <= 0).all() and (npy(out[2]) <= 0).all() and (npy(out[3]) <= 0).all()
    path = npy(hk.viterbi(batch, flat))
    _, scores = hk.viterbi_nbest(batch, flat, 2)
    scores = npy(scores)
    e0 = f0 = 0
    for u, T in enumerate(lens):
        rows = mm[e0:e0 + T * case.S].reshape(T, case.S).copy()
        p = path[f0:f0 + T]
        assert np.isfinite(best[u]) and best[u] == scores[u, 0]
        assert (rows[np.arange(T), p] == 0).all(), f'utterance {u}: mm != 0 on the Viterbi path'
        rows[np.arange(T), p] = -np.inf
        # the second-best path leaves the best somewhere (one path only: -inf on both sides)
        second = scores[u, 1] - scores[u, 0] if np.isfinite(scores[u, 1]) else -np.inf
        assert rows.max() == second, f'utterance {u}: {rows.max()} off the path, {second} second'
        e0, f0 = e0 + T * case.S, f0 + T


MIXED_LENS, MIXED_GIDS = [33, 65, 32, 2, 64, 1], [0, 1, 2, 0, 2, 1]


@DTYPES
@pytest.mark.parametrize('sizes,want', [((7, 65, 129), ALL), ((7, 65, 300), ALL)], ids=['129', '300'])
def test_graphs_of_different_sizes_in_one_launch(sizes, want, dtype):
    'Alignment-graph style: the form follows the largest graph, every utterance its own categories.'
    arrays = [ft.make_graph(S, ft.offsets(3, S), 2300 + k, 0, NP[dtype]) for k, S in enumerate(sizes)]
    graphs = [compiled(g) for g in arrays]
    n_cat = 11
    cats = [lt.random_categories(g, n_cat, 40 + k, 1 / 3.) for k, g in enumerate(arrays)]
    rng = np.random.RandomState(5)
    llhs = [(rng.randn(T, sizes[k]) * 3).astype(NP[dtype]) for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert hk.maxmarg_route(batch, n_cat, True, True, True) == want
    out = guarded_call(batch, packed(llhs), [c[0] for c in cats], [c[1] for c in cats], n_cat)
    truths = truths_of([arrays[k] for k in MIXED_GIDS], llhs, [cats[k] for k in MIXED_GIDS], n_cat)
    hold(truths, MIXED_LENS, [sizes[k] for k in MIXED_GIDS], out, dtype, str(sizes))
    py = hk.max_marginals(batch, packed(llhs), [c[0] for c in cats], [c[1] for c in cats], n_cat,
                          per_frame=True, per_utt=True)
    same_bits(out, py, 'hk.max_marginals')
    with pytest.raises(ValueError):
        hk.max_marginals(batch, packed(llhs), [c[0] for c in cats][:2], [c[1] for c in cats], n_cat)


@DTYPES
def test_a_long_utterance(dtype):
    S, T = 8, 4096
    g = ft.make_graph(S, ft.offsets(3, S), 31, 0, NP[dtype])
    _, llhs = ft.inputs(g, [T], np.arange(S), S, 1., 32, NP[dtype])
    arc_cat, init_cat = lt.random_categories(g, 5, 33)
    batch = hk.HmmBatch([compiled(g)], [0], [T], dtype)
    out = hk.max_marginals(batch, packed(llhs), [arc_cat], [init_cat], 5, per_frame=True, per_utt=True)
    hold(truths_of([g], llhs, [(arc_cat, init_cat)], 5), [T], [S], out, dtype, f'S={S} T={T}')
    assert float(out[1].view(T, S).max(1).values.abs().max()) <= \
        float(lt.tolerance(lt.bound(g, llhs[0]), T, 0.))      # the best path passes every frame


@DTYPES
@pytest.mark.parametrize('S,nO', [(16, 3), (300, 3)], ids=['S16', 'S300'])
def test_a_per_frame_shift_moves_best_and_leaves_the_margins(S, nO, dtype):
    '''k_t in +-3e4 added to every entry of row t moves `best` by sum_t k_t and no max-marginal.
    The log-likelihoods and the shifts are multiples of 1/64 (below 2^24 / 64): the shifted rows
    are exact in float32.'''
    g = ft.make_graph(S, ft.offsets(nO, S), 51, 0, NP[dtype])
    lens = [200, 1, 9, 33]
    rng = np.random.RandomState(52)
    base = [(rng.randint(-512, 513, size=(T, S)) / 64.).astype(NP[dtype]) for T in lens]
    ks = [rng.randint(-30000 * 64, 30000 * 64 + 1, size=T) / 64. for T in lens]
    shifted = [(l.astype(np.float64) + k[:, None]).astype(NP[dtype]) for l, k in zip(base, ks)]
    for l, s, k in zip(base, shifted, ks):
        assert (s.astype(np.float64) - l.astype(np.float64) == k[:, None]).all()
    arc_cat, init_cat = lt.random_categories(g, 7, 53, 1 / 3.)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    kw = dict(per_frame=True, per_utt=True)
    out0 = hk.max_marginals(batch, packed(base), [arc_cat], [init_cat], 7, **kw)
    out1 = hk.max_marginals(batch, packed(shifted), [arc_cat], [init_cat], 7, **kw)
    cats = [(arc_cat, init_cat)] * len(lens)
    t0, t1 = truths_of([g] * len(lens), base, cats, 7), truths_of([g] * len(lens), shifted, cats, 7)
    hold(t0, lens, [S] * len(lens), out0, dtype, 'unshifted')
    hold(t1, lens, [S] * len(lens), out1, dtype, 'shifted')
    # shifted against unshifted: the two bounds added; best moved by the shifts
    e0 = f0 = 0
    for u, T in enumerate(lens):
        B0, B1 = t0[u][4], t1[u][4]
        for a, b, want, r, lo, hi in ((out0[1], out1[1], t0[u][1], R[dtype], e0, e0 + T * S),
                                      (out0[2].reshape(-1), out1[2].reshape(-1), t0[u][2], R[dtype],
                                       f0 * 7, (f0 + T) * 7),
                                      (out0[3][u], out1[3][u], t0[u][3], 0., 0, 7)):
            x, y = npy(a)[lo:hi].astype(np.float64), npy(b)[lo:hi].astype(np.float64)
            want = want.reshape(-1)
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(x), fin) and np.array_equal(np.isfinite(y), fin)
            tol = lt.tolerance(B0, T, want, r) + lt.tolerance(B1, T, want, r)
            assert (np.abs(x[fin] - y[fin]) <= np.broadcast_to(tol, want.shape)[fin]).all()
        moved = float(out1[0][u] - out0[0][u])
        assert abs(moved - ks[u].sum()) <= float(lt.tolerance(B0 + B1, T, 0.))
        e0, f0 = e0 + T * S, f0 + T


# --- edges -----------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize('S', [8, 65, 300])
def test_a_column_of_minus_infinity_and_an_unreachable_final(S, dtype):
    g = ft.make_graph(S, ft.offsets(3, S), 9, 0, NP[dtype])
    lens = [6, 1, 9, 4]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 9, NP[dtype])
    llhs = [l.copy() for l in llhs]
    llhs[0][:, 1] = -np.inf                                  # a state that is never there
    llhs[2][4] = -np.inf                                     # a frame without a state: dead
    llhs[3][1, ::2] = -np.inf
    arc_cat, init_cat = lt.random_categories(g, 4, 10, 1 / 3.)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    cats = [(arc_cat, init_cat)] * len(lens)
    out = guarded_call(batch, packed(llhs), [arc_cat], [init_cat], 4)
    hold(truths_of([g] * len(lens), llhs, cats, 4), lens, [S] * len(lens), out, dtype, f'-inf S={S}')
    assert float(out[0][2]) == -np.inf and (out[3][2] == -np.inf).all()
    assert (out[1][(6 + 1) * S:(6 + 1 + 9) * S] == -np.inf).all()
    assert (out[1][:6 * S].view(6, S)[:, 1] == -np.inf).all()
    # no state may end: everything -inf, no NaN
    dead = dict(g, final=np.full(S, -np.inf, dtype=NP[dtype]))
    batch = hk.HmmBatch([compiled(dead)], [0] * len(lens), lens, dtype)
    out = guarded_call(batch, packed(llhs), [arc_cat], [init_cat], 4)
    hold(truths_of([dead] * len(lens), llhs, cats, 4), lens, [S] * len(lens), out, dtype, 'no final')
    for o in out:
        assert (o == -np.inf).all()


def test_an_utterance_of_no_frames_and_an_empty_batch():
    g = ft.make_graph(8, ft.offsets(3, 8), 3)
    lens = [4, 0, 3]
    _, llhs = ft.inputs(g, lens, np.arange(8), 8, 1., 4)
    arc_cat, init_cat = lt.random_categories(g, 3, 5)
    batch = hk.HmmBatch([compiled(g)], [0] * 3, lens, torch.float64)
    out = guarded_call(batch, packed(llhs), [arc_cat], [init_cat], 3)
    none = (-np.inf, np.zeros((0, 8)), np.zeros((0, 3)), np.full(3, -np.inf), 1.)
    truths = truths_of([g] * 2, [llhs[0], llhs[2]], [(arc_cat, init_cat)] * 2, 3)
    hold([truths[0], none, truths[1]], lens, [8] * 3, out, torch.float64, 'no frames')
    assert float(out[0][1]) == -np.inf and (out[3][1] == -np.inf).all()
    empty = hk.HmmBatch([compiled(g)], [], [], torch.float64)
    out = hk.max_marginals(empty, torch.zeros(0, dtype=torch.float64, device='cuda'), [arc_cat],
                           [init_cat], 3, per_frame=True, per_utt=True)
    assert [tuple(o.shape) for o in out] == [(0,), (0,), (0, 3), (0, 3)]


def test_arguments_are_checked():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    graph = compiled(g)
    batch = hk.HmmBatch([graph], [0], [4], torch.float64)
    flat = torch.zeros(12, dtype=torch.float64, device='cuda')
    A = len(graph.out_arcs()[0])
    a, i = np.zeros(A, np.int32), np.zeros(3, np.int32)
    for bad in ((a[:-1], i, 2), (a, i[:-1], 2), (a + 2, i, 2), (a, i - 2, 2), (a, i, 0)):
        with pytest.raises(ValueError):
            hk.max_marginals(batch, flat, [bad[0]], [bad[1]], bad[2], per_frame=True)
    with pytest.raises(ValueError):
        hk.max_marginals(batch, flat, [a], [i], 2, states=False)
    with pytest.raises(ValueError):
        hk.max_marginals(batch, flat, per_utt=True)
    with pytest.raises(_hip.HipInvalid):
        hk.maxmarg_route(batch, 0, True, True, False)
    with pytest.raises(_hip.HipInvalid):
        hk.maxmarg_route(batch, 3, False, False, False)


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
    pc = npy(pc_all)
    return (pc.dtype.type(scale) * pc)[:, np.asarray([int(i) for i in ids])]


def unit_categories_by_hand(arrays, ids, start_pdf, end_pdf):
    'The unit-start categories from state pairs, restated: no code of the package.'
    ids = [int(i) for i in ids]
    firsts = [int(start_pdf[u]) for u in start_pdf]
    src, dst = lt.out_arcs(arrays)
    arc_cat = np.asarray([firsts.index(ids[j]) if i != j and ids[j] in firsts else -1
                          for i, j in zip(src, dst)], dtype=np.int32)
    init_cat = -np.ones(len(ids), dtype=np.int32)
    for k, u in enumerate(start_pdf):
        for j, p in enumerate(ids):
            if int(start_pdf[u]) <= p <= int(end_pdf[u]):
                init_cat[j] = k
    return arc_cat, init_cat


def decoded_starts(path, start_pdf):
    '(frame, unit) at which the pdf path of `decode` begins a unit, the units in start_pdf order.'
    firsts = [int(start_pdf[u]) for u in start_pdf]
    path = [int(p) for p in path]
    return [(t, firsts.index(p)) for t, p in enumerate(path)
            if t >= 1 and p in firsts and path[t - 1] != p]


def decode_slack(B, T, dtype):
    '''How far below the best score the path of `decode` may lie: it is the best in sums made in
    the model's precision, 2 T + 2 additions each off by at most eps B -- twice that, once for
    the path it takes and once for the one it leaves -- and the max-marginal's own bound.'''
    return 2 * (2 * T + 2) * EPS[dtype] * B + float(lt.tolerance(B, T, 0.))


@pytest.mark.parametrize('kind', ['hmm', 'phoneloop', 'bigram'])
def test_model_max_marginals_and_unit_start_margins_are_the_truth(kind):
    model = make_model(kind)
    arrays = dense_arrays(model.graph)
    ids = model.graph.pdf_id_mapping
    S = arrays['S']
    arc_cat, init_cat = lt.random_categories(arrays, 5, 21, 1 / 3.)
    dt = torch.float64
    for X, scale in zip(utterances([57, 1, 23], 1), (1., 1., .7)):
        T = len(X)
        llh = model_llh(model, X, ids, scale)
        truth = lt.max_marginals(arrays, llh, arc_cat, init_cat, 5) + (lt.bound(arrays, llh),)
        best, mm = model.max_marginals(X, scale=scale)
        assert best.dtype == torch.float64 and best.dim() == 0 and mm.shape == (T, S) and mm.is_cuda
        hold([truth], [T], [S], (best.view(1), mm.reshape(-1), None, None), dt, kind)
        best, frame = model.arc_max_marginals(X, arc_cat, init_cat, 5, scale=scale)
        assert frame.shape == (T, 5) and frame.dtype == torch.float64
        hold([truth], [T], [S], (best.view(1), None, frame, None), dt, kind)
        best, utt = model.arc_max_marginals(X, torch.from_numpy(arc_cat), init_cat, 5, scale=scale,
                                            inference_graph=model.graph, per_frame=False)
        assert utt.shape == (5,) and utt.dtype == torch.float64
        hold([truth], [T], [S], (best.view(1), None, None, utt.view(1, 5)), dt, kind)
        # decode's path has no margin (one frame cannot reach the end of a left-to-right unit:
        # no path at all)
        slack = decode_slack(truth[4], T, dt)
        alive = np.isfinite(truth[0])
        assert float(mm.max()) <= slack
        path = model.decode(X, scale=scale)
        on_path = npy(mm)[np.arange(T), [list(map(int, ids)).index(int(p)) for p in path]]
        assert not alive or (on_path >= -slack).all()
        if kind == 'hmm':
            assert not hasattr(model, 'unit_start_margins')
            continue
        n_units = len(model.start_pdf)
        hand = unit_categories_by_hand(arrays, ids, model.start_pdf, model.end_pdf)
        truth = lt.max_marginals(arrays, llh, hand[0], hand[1], n_units) + (truth[4],)
        best, got = model.unit_start_margins(X, scale=scale)
        assert got.shape == (T, n_units)
        hold([truth], [T], [S], (best.view(1), None, got, None), dt, kind + ' unit_start_margins')
        got = npy(got)
        if not alive:
            assert (got == -np.inf).all()
            continue
        # (0 up to the rounding of sums that are not exact, on either side)
        assert got.max() <= slack and got[0].max() >= -slack
        for t, u in decoded_starts(path, model.start_pdf):
            assert got[t, u] >= -slack, (t, u)


@pytest.mark.parametrize('kind', ['phoneloop', 'bigram'])
def test_the_batch_function_is_unit_start_margins_per_utterance(kind):
    model = make_model(kind)
    lens = [23, 40, 9, 31, 1]
    utts = utterances(lens, 3)
    one_by_one = [model.unit_start_margins(X, scale=.9) for X in utts]
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        best, margins = beer.unit_start_margins_batch(model, utts, scale=.9, max_frames=max_frames)
        assert best.shape == (len(lens),) and best.dtype == torch.float64 and best.is_cuda
        assert [tuple(m.shape) for m in margins] == [(T, 4) for T in lens]
        for u, (b, want) in enumerate(one_by_one):
            # (the same kernel on the same inputs: the same bits)
            assert float(best[u]) == float(b) and torch.equal(margins[u], want), (max_frames, u)
    again = beer.unit_start_margins_batch(model, (torch.cat(utts), lens), scale=.9)
    assert torch.equal(again[0], best) and all(torch.equal(a, b) for a, b in zip(again[1], margins))


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
    stale = [float(model.unit_start_margins(X, inference_graph=bound[i])[0]) for i, X in enumerate(utts)]
    gen = torch.Generator().manual_seed(1)
    for p in model.transitions.parameters_of_groups():
        conc = p.posterior.params.concentrations
        conc.add_(torch.rand(conc.shape, generator=gen, dtype=torch.float64).to(conc) * 3)
    model._on_transitions_update()
    tmap, log_a = CategoryMap(model), expected_log_probs(model.transitions)
    n_units = len(model.start_pdf)
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
        truths.append(lt.max_marginals(arrays, llh, hand[0], hand[1], n_units) +
                      (lt.bound(arrays, llh),))
        best, got = model.unit_start_margins(X, inference_graph=bound[i], scale=.8)
        hold([truths[-1]], [lens[i]], [len(last)], (best.view(1), None, got, None), torch.float64,
             f'bound graph {i}')
        assert float(model.unit_start_margins(X, inference_graph=bound[i])[0]) != stale[i]
        # a chain: the first unit of the transcription begins at frame 0 on every path
        first = list(model.start_pdf).index(seqs[i][0])
        assert abs(float(got[0, first])) <= float(lt.tolerance(truths[-1][4], lens[i], 0.))
        assert (npy(got)[0, np.arange(n_units) != first] == -np.inf).all()
    best, margins = beer.unit_start_margins_batch(model, utts, inference_graphs=list(bound), scale=.8,
                                                  max_frames=50)
    for i, truth in enumerate(truths):
        hold([truth], [lens[i]], [truth[1].shape[1]], (best[i:i + 1], None, margins[i], None),
             torch.float64, f'batched bound graph {i}')
    with pytest.raises(ValueError):
        beer.unit_start_margins_batch(model, utts, inference_graphs=list(bound)[:2])


def run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_lattice(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    run(['dataset', 'create', str(tmp_path), feats, ds])
    out_dir = tmp_path / 'lat'
    out = run(['hmm', 'lattice', mdl, ds, str(out_dir)]).strip().split('\n')
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    names = [str(u) for u in model.start_pdf]
    best, margins = beer.unit_start_margins_batch(model, utts)
    paths = beer.decode_batch(model, utts)
    dtype = margins[0].dtype
    arrays, pdf = dense_arrays(model.graph), model.graph.pdf_id_mapping
    assert sorted(os.listdir(out_dir)) == [f'{u}.npz' for u in ids]
    assert [l.split()[0] for l in out] == ids
    zero_dir = tmp_path / 'zero'
    run(['hmm', 'lattice', '--beam', '0', mdl, ds, str(zero_dir)])
    for u, line, T in zip(range(3), out, (35, 50, 41)):
        lat = np.load(out_dir / f'{ids[u]}.npz')
        assert sorted(lat.files) == ['frame', 'margin', 'score', 'unit', 'units']
        frame, unit, margin = lat['frame'], lat['unit'], lat['margin']
        assert frame.dtype == np.int32 and unit.dtype == np.int32 and margin.dtype == np.float64
        assert lat['units'].tolist() == names and float(lat['score']) == float(best[u])
        full = npy(margins[u]).astype(np.float64)
        assert full.shape == (T, len(names))
        # the cells within the beam, all of them, by frame and then by unit
        want = np.argwhere(full >= -10.)
        assert np.array_equal(np.stack([frame, unit], 1), want)
        assert (np.diff(frame.astype(np.int64) * len(names) + unit) > 0).all()
        assert np.array_equal(margin, full[frame, unit]) and (margin >= -10.).all()
        assert line.split() == [ids[u], '%.6f' % float(best[u]), str(len(frame)), str(T)]
        # the Viterbi segmentation is in it
        B = lt.bound(arrays, model_llh(model, utts[u].to('cuda'), pdf, 1.))
        slack = decode_slack(B, T, dtype)
        assert slack < 10.
        kept = set(zip(frame.tolist(), unit.tolist()))
        starts = decoded_starts(paths[u].cpu(), model.start_pdf)
        assert all(s in kept for s in starts)
        assert all(full[t, k] >= -slack for t, k in starts)
        assert any(t == 0 and m >= -slack for t, m in zip(frame, margin))
        # --beam 0: the starts of the best segmentation and whatever ties them
        zero = np.load(zero_dir / f'{ids[u]}.npz')
        assert np.array_equal(np.stack([zero['frame'], zero['unit']], 1), np.argwhere(full >= 0.))
        assert not zero['margin'].any() and zero['frame'][0] == 0
        # (a start is entered on the best path or not at all: as many as the best path has units)
        assert len(zero['frame']) >= 1 + sum(full[t, k] == 0. for t, k in starts)
    # a scale, a beam and a list of utterances
    (tmp_path / 'utts').write_text('utt2\n')
    out2 = tmp_path / 'two'
    line = run(['hmm', 'lattice', '-s', '0.5', '--beam', '3', '-u', str(tmp_path / 'utts'), mdl, ds,
                str(out2)]).split()
    assert os.listdir(out2) == ['utt2.npz']
    b2, m2 = beer.unit_start_margins_batch(model, [utts[2]], scale=.5)
    lat = np.load(out2 / 'utt2.npz')
    assert np.array_equal(np.stack([lat['frame'], lat['unit']], 1), np.argwhere(npy(m2[0]) >= -3.))
    assert line == ['utt2', '%.6f' % float(b2[0]), str(len(lat['frame'])), '41']
