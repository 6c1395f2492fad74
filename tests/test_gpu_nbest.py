"""N-best Viterbi (csrc/hmm_nbest.hip) against the truth of tests/nbest_truth.py, on graphs that
sit on the boundaries of its forms.

 * One static table: each case names the route `beer_hmm_nbest_route` must report for it in
   either precision; the table as a whole reaches every value the route can take, every number of
   list entries a thread keeps (k = 1, 2, 3, 8, 16) and both sides of every boundary in S: the
   workgroup's 64 / 65 and 256 / 257 states, the chunk's S k = 128 / 129 and 512 / 513.
 * Integer inputs (every sum exact in float32): paths and scores ARE the truth's, ties included,
   and rank 0 is `hk.viterbi`'s path element for element, with and without `map_pdf`.
 * Real inputs, `tol` = 1e-10 (float64) / 1e-5 (float32), the project's flat tolerances: scores
   non-increasing, paths pairwise distinct, every path rescored in float64 within
   `score_bound` = tol * (sum of |terms| along the path + 1) of its reported score, and the sorted
   scores within that bound of the truth's (a float32 near-tie that swaps two ranks passes).
 * Guards around `paths`, `scores` and `bt_ws`; `pc_llhs` unchanged bit for bit.
 * Edges: fewer than k paths, an all -inf final vector, T = 1, 4096 frames beside short ones.
 * The model level: `HMM.decode_nbest`, `decode_nbest_batch`, `beer hmm decode --nbest`."""

import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import fb_truth as ft
import nbest_truth as nt
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
L = nt.ARCS_LDS
GUARD = 7
P_SENTINEL, S_SENTINEL, B_SENTINEL = -777, -12345.678, -555

# around the back-pointer chunks of 32, 8 and 2 frames
LONG = tuple(ft.VITERBI_LENGTHS) + (7, 8, 9, 3, 16, 17)

# S, offsets, hub members, k, utterances (a number: fb_truth.lengths; 'long': LONG), pdf-id
# flavour, the route in float64 and in float32
Case = namedtuple('Case', 'S nO hub k nutt flavour f64 f32 seed')
CASES = []


def add(S, nO, k, f64, f32=None, hub=0, nutt=None):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, k, nutt or (1, 5, 9)[i % 3], ft.FLAVOURS[i % 3], f64,
                      f64 if f32 is None else f32, 900 + i))


# chunks of 32 frames: S k <= 128
add(1, 2, 3, 32 | L)                       # one path, three asked for
add(3, 2, 2, 32 | L)
add(3, 3, 16, 32 | L)
add(8, 2, 1, 32 | L, nutt='long')
add(8, 3, 8, 32 | L, nutt='long')
add(8, 8, 16, 32 | L)                      # every arc present; S k = 128
add(64, 3, 2, 32 | L)                      # one wave; S k = 128
add(65, 3, 1, 32 | L)                      # two waves
add(128, 3, 1, 32 | L, nutt='long')        # S k = 128
add(120, 3, 1, 32 | L, hub=40)             # a phone loop's rows of 40 + 3 arcs
add(100, 100, 1, 32, nutt=5)               # every arc present: 80 KB of arcs stay in global memory
# chunks of 8: S k <= 512
add(16, 3, 16, 8 | L, nutt='long')
add(17, 3, 16, 8 | L)
add(129, 3, 1, 8 | L, nutt='long')         # S k = 129
add(64, 3, 3, 8 | L)
add(65, 3, 3, 8 | L)
add(128, 3, 2, 8 | L)
add(256, 3, 1, 8 | L, nutt='long')         # the last size with a thread per state
add(257, 3, 1, 8 | L, nutt='long')         # threads stride over the states
add(120, 3, 3, 8 | L, hub=40, nutt='long')
add(256, 3, 2, 8 | L)                      # S k = 512
add(64, 3, 8, 8 | L, hub=8)                # S k = 512
add(100, 100, 2, 8, nutt=5)
# chunks of 2
add(257, 4, 3, 2 | L)
add(513, 3, 1, 2 | L, nutt='long')         # S k = 513
add(65, 3, 16, 2 | L, nutt='long')
add(120, 3, 16, 2, 2 | L, hub=40)          # 61 KiB of columns and chunk in float64
add(509, 3, 8, 2)
# arcs that no longer fit LDS: 7200 at 600 states, every arc present at 100
add(600, 12, 1, 2)
add(600, 12, 2, 2, nutt='long')
add(100, 100, 8, 2, nutt=5)
add(100, 100, 16, 2, nutt=5)


def case_id(c):
    return f'{c.seed}-S{c.S}-O{c.nO}-hub{c.hub}-k{c.k}-n{c.nutt}-{c.flavour}'


def test_the_cases_reach_every_value_of_the_route():
    forms = {c.f64 for c in CASES} | {c.f32 for c in CASES}
    assert forms == {32 | L, 8 | L, 2 | L, 32, 8, 2}
    assert {1, 3, 8, 64, 65, 120, 256, 257, 600} <= {c.S for c in CASES}
    assert {1, 2, 3, 8, 16} == {c.k for c in CASES}
    assert {nt.list_entries(c.k) for c in CASES} == {1, 2, 4, 8, 16}
    assert {128, 129, 512, 513} <= {c.S * c.k for c in CASES}       # both sides of a chunk size
    assert any(c.S == 120 and c.hub == 40 for c in CASES)
    assert set(ft.FLAVOURS) == {c.flavour for c in CASES}
    for chunk in (32, 8, 2):                    # lengths on both sides of every chunk
        assert {chunk - 1, chunk, chunk + 1} <= set(LONG) | {0}
        assert any(_hip.nbest_chunk(c.f64) == chunk and c.nutt == 'long' for c in CASES)


def packed(llhs):
    return torch.cat([tt(l).reshape(-1) for l in llhs])


def compiled(g, ids=None):
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in (range(g['S']) if ids is None else ids)])
    if g['hub'] is not None:
        E, a, B_, c = g['hub']
        graph.set_hub(E, tt(a), B_, tt(c))
    return graph


def guarded_call(batch, flat, k, map_pdf=False):
    '''beer_hmm_viterbi_nbest into the middle of sentinel-filled buffers: (paths [k, n_frames],
    scores [nutt, k]) as numpy arrays after the guards were checked.'''
    n, f, e = batch.nutt, batch.n_frames, batch.n_elems
    pbuf = torch.full((k * f + 2 * GUARD,), P_SENTINEL, dtype=torch.int64, device='cuda')
    sbuf = torch.full((n * k + 2 * GUARD,), S_SENTINEL, dtype=torch.float64, device='cuda')
    bbuf = torch.full((k * e + 2 * GUARD,), B_SENTINEL, dtype=torch.int32, device='cuda')
    paths, scores, bt = pbuf[GUARD:GUARD + k * f], sbuf[GUARD:GUARD + n * k], bbuf[GUARD:GUARD + k * e]
    _hip.call('beer_hmm_viterbi_nbest', _hip.dtype_code(batch.dtype), batch.ref(), _hip.ptr(flat),
              k, _hip.ptr(bt), _hip.ptr(paths), _hip.ptr(scores), 1 if map_pdf else 0)
    torch.cuda.synchronize()
    for buf, sentinel, size, what in ((pbuf, P_SENTINEL, k * f, 'paths'),
                                      (sbuf, S_SENTINEL, n * k, 'scores'),
                                      (bbuf, B_SENTINEL, k * e, 'bt_ws')):
        assert (buf[:GUARD] == sentinel).all() and (buf[GUARD + size:] == sentinel).all(), \
            f'a guard element of {what} was written'
    assert (paths != P_SENTINEL).all() and (scores != S_SENTINEL).all(), 'an output was left out'
    return npy(paths).reshape(k, f), npy(scores).reshape(n, k)


def setup(case, dtype, integer):
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype],
                      integer=integer)
    S_total = case.S if case.flavour == 'perm' else case.S + 3
    ids = ft.pdf_ids(case.S, case.flavour, S_total, case.seed)
    graph = compiled(g, ids)
    lens = list(LONG) if case.nutt == 'long' else ft.lengths(case.nutt, case.seed)
    if integer:
        llhs = ft.viterbi_inputs(case.S, lens, case.seed, NP[dtype])
    else:
        _, llhs = ft.inputs(g, lens, np.arange(case.S), case.S, 1., case.seed, NP[dtype])
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    want = case.f64 if dtype == torch.float64 else case.f32
    route = hk.nbest_route(batch, case.k)
    assert route == want, f'route {route:#x}, the table says {want:#x}'
    assert route == nt.route_formula(case.S, batch.struct.max_arcs, tt(llhs[0]).element_size(),
                                     case.k)
    return g, ids, lens, llhs, batch


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_integer_inputs_give_the_truth_exactly(case, dtype):
    g, ids, lens, llhs, batch = setup(case, dtype, True)
    k = case.k
    flat = packed(llhs)
    before = flat.clone()
    paths, scores = guarded_call(batch, flat, k)
    assert torch.equal(flat, before), 'pc_llhs was written'
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, l in enumerate(llhs):
        want_p, want_s = nt.nbest(g, l, k, NP[dtype])
        np.testing.assert_array_equal(scores[u], want_s, err_msg=f'utterance {u}')
        np.testing.assert_array_equal(paths[:, off[u]:off[u + 1]], want_p, err_msg=f'utterance {u}')
    # rank 0 is the Viterbi path, as states and as pdf ids
    assert np.isfinite(scores[:, 0]).all()
    np.testing.assert_array_equal(paths[0], npy(hk.viterbi(batch, flat)))
    mapped, scores2 = guarded_call(batch, flat, k, map_pdf=True)
    np.testing.assert_array_equal(scores2, scores)
    np.testing.assert_array_equal(mapped[0], npy(hk.viterbi(batch, flat, map_pdf=True)))
    np.testing.assert_array_equal(mapped, np.where(paths >= 0, np.asarray(ids)[paths], -1))
    # and through the Python face
    p3, s3 = hk.viterbi_nbest(batch, flat, k)
    assert p3.dtype == torch.int64 and p3.is_cuda and p3.shape == (k, sum(lens))
    assert s3.dtype == torch.float64 and s3.is_cuda and s3.shape == (len(lens), k)
    np.testing.assert_array_equal(npy(p3), paths)
    np.testing.assert_array_equal(npy(s3), scores)


def hold_real(g, l, paths, scores, k, tol, what):
    '''The properties of one utterance's result on real inputs; returns the largest ratio of an
    error to its bound (rescoring, truth).'''
    want_p, want_s = nt.nbest(g, l.astype(np.float64), k)
    n = int(np.isfinite(want_s).sum())
    assert np.isfinite(scores[:n]).all() and np.isneginf(scores[n:]).all(), what
    assert (paths[n:] == -1).all() and (paths[:n] >= 0).all(), what
    assert (np.diff(scores[:n]) <= 0).all(), f'{what}: scores increase'
    assert len({tuple(p) for p in paths[:n]}) == n, f'{what}: a path twice'
    worst = 0.
    for r in range(n):
        terms = nt.path_terms(g, l, paths[r])
        d, bound = abs(terms.sum() - scores[r]), nt.score_bound(terms, tol)
        assert d <= bound, f'{what} rank {r}: rescored {terms.sum()} for {scores[r]}'
        d2, bound2 = abs(want_s[r] - scores[r]), nt.score_bound(nt.path_terms(g, l, want_p[r]), tol)
        assert d2 <= bound2, f'{what} rank {r}: {scores[r]} for the truth\'s {want_s[r]}'
        worst = max(worst, d / bound, d2 / bound2)
    return worst


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_real_inputs_hold_the_properties(case, dtype):
    g, ids, lens, llhs, batch = setup(case, dtype, False)
    k = case.k
    flat = packed(llhs)
    before = flat.clone()
    paths, scores = guarded_call(batch, flat, k)
    assert torch.equal(flat, before), 'pc_llhs was written'
    off = np.concatenate([[0], np.cumsum(lens)])
    worst = 0.
    for u, l in enumerate(llhs):
        worst = max(worst, hold_real(g, l, paths[:, off[u]:off[u + 1]], scores[u], k, TOL[dtype],
                                     f'{case_id(case)} utterance {u}'))
    print(f'{case_id(case)}: scores within {worst:.3e} of their bounds (tol {TOL[dtype]:.0e})')
    # rank 0 is the Viterbi path here too: the same operations in the same order
    np.testing.assert_array_equal(paths[0], npy(hk.viterbi(batch, flat)))


MIXED_LENS, MIXED_GIDS = [33, 65, 32, 2, 64, 1], [0, 1, 2, 0, 2, 1]


@DTYPES
@pytest.mark.parametrize('sizes,k,want', [((7, 65, 129), 2, 8 | L), ((7, 65, 300), 5, 2 | L)],
                         ids=['S129', 'S300'])
def test_graphs_of_different_sizes_in_one_launch(sizes, k, want, dtype):
    'Alignment-graph style: the form follows the largest graph, every utterance its own.'
    arrays = [ft.make_graph(S, ft.offsets(3, S), 2300 + i, 0, NP[dtype], integer=True)
              for i, S in enumerate(sizes)]
    graphs = [compiled(g) for g in arrays]
    llhs = [ft.viterbi_inputs(sizes[i], [T], 40 + u, NP[dtype])[0]
            for u, (T, i) in enumerate(zip(MIXED_LENS, MIXED_GIDS))]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert hk.nbest_route(batch, k) == want
    flat = packed(llhs)
    paths, scores = guarded_call(batch, flat, k)
    off = np.concatenate([[0], np.cumsum(MIXED_LENS)])
    for u, l in enumerate(llhs):
        want_p, want_s = nt.nbest(arrays[MIXED_GIDS[u]], l, k, NP[dtype])
        np.testing.assert_array_equal(scores[u], want_s)
        np.testing.assert_array_equal(paths[:, off[u]:off[u + 1]], want_p)
    np.testing.assert_array_equal(paths[0], npy(hk.viterbi(batch, flat)))


# --- edges -----------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize('map_pdf', [False, True], ids=['states', 'pdf'])
def test_fewer_than_k_paths_give_inf_and_minus_one(map_pdf, dtype):
    '''One state: one path whatever the length.  Three states and one frame: at most three paths;
    two frames on self-loop-and-step: at most six.'''
    for S, nO, lens, k in ((1, 1, [1, 5, 33], 3), (3, 2, [1, 2, 1], 8), (3, 2, [2, 1, 2], 16)):
        g = ft.make_graph(S, ft.offsets(nO, S), 11, 0, NP[dtype], integer=True)
        ids = [5 + 2 * j for j in range(S)]
        llhs = ft.viterbi_inputs(S, lens, 12, NP[dtype])
        batch = hk.HmmBatch([compiled(g, ids)], [0] * len(lens), lens, dtype)
        paths, scores = guarded_call(batch, packed(llhs), k, map_pdf=map_pdf)
        off = np.concatenate([[0], np.cumsum(lens)])
        for u, l in enumerate(llhs):
            want_p, want_s = nt.nbest(g, l, k, NP[dtype])
            n = int(np.isfinite(want_s).sum())
            assert 1 <= n < k and n == len(nt.brute_force(g, l)[1])
            if map_pdf:
                want_p = np.where(want_p >= 0, np.asarray(ids)[want_p], -1)
            np.testing.assert_array_equal(scores[u], want_s)
            np.testing.assert_array_equal(paths[:, off[u]:off[u + 1]], want_p)
            assert np.isneginf(scores[u, n:]).all() and (paths[n:, off[u]:off[u + 1]] == -1).all()


@DTYPES
@pytest.mark.parametrize('S,k', [(8, 3), (300, 16)])
def test_an_all_inf_final_vector_leaves_no_path(S, k, dtype):
    g = ft.make_graph(S, ft.offsets(3, S), 13, 0, NP[dtype])
    lens = [6, 1, 9, 40]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 14, NP[dtype])
    live = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    paths, scores = guarded_call(live, packed(llhs), k)
    assert np.isfinite(scores[:, 0]).all() and (paths[0] >= 0).all()
    g['final'][:] = -np.inf
    dead = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    for map_pdf in (False, True):
        paths, scores = guarded_call(dead, packed(llhs), k, map_pdf=map_pdf)
        assert np.isneginf(scores).all() and (paths == -1).all()
    # one unreachable utterance among reachable ones: only the third state may end an utterance
    g = ft.make_graph(S, (0, 1), 15, 0, NP[dtype])
    g['final'][:] = -np.inf
    g['final'][min(S - 1, 5)] = 0.
    mixed = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    paths, scores = guarded_call(mixed, packed(llhs), k)
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, l in enumerate(llhs):
        want_p, want_s = nt.nbest(g, l.astype(np.float64), k)
        assert (np.isfinite(scores[u]) == np.isfinite(want_s)).all()
        assert ((paths[:, off[u]:off[u + 1]] >= 0).all(1) == np.isfinite(want_s)).all()
    assert np.isneginf(scores[1]).all() and np.isfinite(scores[3, 0])


@DTYPES
def test_one_frame(dtype):
    for S, k in ((8, 3), (120, 16), (300, 2)):
        g = ft.make_graph(S, ft.offsets(3, S), 16, 0, NP[dtype], integer=True)
        lens = [1, 1, 1]
        llhs = ft.viterbi_inputs(S, lens, 17, NP[dtype])
        batch = hk.HmmBatch([compiled(g)], [0] * 3, lens, dtype)
        paths, scores = guarded_call(batch, packed(llhs), k)
        for u, l in enumerate(llhs):
            want_p, want_s = nt.nbest(g, l, k, NP[dtype])
            np.testing.assert_array_equal(scores[u], want_s)
            np.testing.assert_array_equal(paths[:, u:u + 1], want_p)
            assert np.isfinite(scores[u, :min(k, 3)]).all() and np.isneginf(scores[u, 3:]).all()


@DTYPES
@pytest.mark.parametrize('S,k,chunk', [(8, 3, 32), (40, 8, 8), (120, 16, 2)])
def test_a_long_utterance_beside_short_ones(S, k, chunk, dtype):
    'Integer inputs: -7 a frame at worst, 4096 frames stay exact in float32.'
    g = ft.make_graph(S, ft.offsets(3, S), 18, 0, NP[dtype], integer=True)
    lens = [3, 4096, 1, 33]
    llhs = ft.viterbi_inputs(S, lens, 19, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    assert _hip.nbest_chunk(hk.nbest_route(batch, k)) == chunk
    flat = packed(llhs)
    paths, scores = guarded_call(batch, flat, k)
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, l in enumerate(llhs):
        want_p, want_s = nt.nbest(g, l, k, NP[dtype])
        np.testing.assert_array_equal(scores[u], want_s)
        np.testing.assert_array_equal(paths[:, off[u]:off[u + 1]], want_p)
    np.testing.assert_array_equal(paths[0], npy(hk.viterbi(batch, flat)))


def test_refusals_on_the_device():
    g = ft.make_graph(4, ft.offsets(2, 4), 20)
    batch = hk.HmmBatch([compiled(g)], [0], [4], torch.float64)
    flat = torch.zeros(16, dtype=torch.float64, device='cuda')
    for k in (0, 17):
        with pytest.raises(ValueError):
            hk.viterbi_nbest(batch, flat, k)
        rc = _hip.lib().beer_hmm_viterbi_nbest(_hip.F64, batch.ref(), _hip.ptr(flat), k, None, None,
                                               None, 0, None)
        assert rc == _hip.EINVAL
    rc = _hip.lib().beer_hmm_viterbi_nbest(_hip.F64, batch.ref(), _hip.ptr(flat), 2, None, None,
                                           None, 0, None)
    assert rc == _hip.EINVAL                                            # NULL outputs
    big = ft.make_graph(700, (0, 1), 21)
    batch = hk.HmmBatch([compiled(big)], [0], [2], torch.float32)
    assert hk.nbest_route(batch, 8) == 2
    with pytest.raises(_hip.HipInvalid, match='160 KB'):
        hk.nbest_route(batch, 16)
    with pytest.raises(_hip.HipInvalid):
        hk.viterbi_nbest(batch, torch.zeros(1400, device='cuda'), 16)


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


def hold_model(model, X, arrays, ids, scale, paths, scores, k, what):
    'A model-level result against the truth on the log-likelihoods the model itself computes.'
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    llh = scale * npy(pc_all).astype(np.float64)[:, np.asarray(ids)]
    want_p, want_s = nt.nbest(arrays, llh, k)
    paths, scores = npy(paths), npy(scores)
    assert paths.shape == (k, len(X)) and scores.shape == (k,)
    n = int(np.isfinite(want_s).sum())
    assert np.isfinite(scores[:n]).all() and np.isneginf(scores[n:]).all(), what
    for r in range(n):
        bound = nt.score_bound(nt.path_terms(arrays, llh, want_p[r]), 1e-10)
        assert abs(scores[r] - want_s[r]) <= bound, (what, r)
        # the truth's own path wherever its score stands clear of its neighbours'
        gaps = np.abs(want_s[r] - np.delete(want_s[:n], r))
        if n == 1 or gaps.min() > 4 * bound:
            np.testing.assert_array_equal(paths[r], np.asarray(ids)[want_p[r]], err_msg=what)
    assert (paths[n:] == -1).all()


@pytest.mark.parametrize('kind', ['hmm', 'phoneloop', 'bigram'])
def test_model_decode_nbest(kind):
    model = make_model(kind)
    arrays = dense_arrays(model.graph)
    ids = model.graph.pdf_id_mapping
    for X, scale, k in zip(utterances([57, 1, 23], 1), (1., 1., .7), (5, 3, 16)):
        paths, scores = model.decode_nbest(X, k, scale=scale)
        assert not paths.is_cuda and paths.dtype == torch.int64 and scores.dtype == torch.float64
        hold_model(model, X, arrays, ids, scale, paths, scores, k, kind)
        # k = 1 is `decode`, and so is the first of any k
        best = model.decode(X, scale=scale)
        one, s1 = model.decode_nbest(X, 1, scale=scale)
        if torch.isfinite(s1[0]):
            assert torch.equal(one[0], best) and torch.equal(paths[0], best)
            assert s1[0] == scores[0]
        else:                           # (one frame cannot reach the end of a left-to-right unit)
            assert len(X) == 1 and (one == -1).all()
        # the model's own graph handed in as an inference graph: the same launch
        again = model.decode_nbest(X, k, inference_graph=model.graph, scale=scale)
        assert torch.equal(again[0], paths) and torch.equal(again[1], scores)


@pytest.mark.parametrize('kind', ['phoneloop', 'bigram'])
def test_decode_nbest_batch_is_decode_nbest_per_utterance(kind):
    '''The batched call computes the emissions with the shard's E-step kernels, the model's call
    with the per-call ones: scores within the float64 bound, the same paths.'''
    model = make_model(kind)
    lens = [23, 40, 9, 31, 1]
    utts = utterances(lens, 3)
    k = 4
    one_by_one = [model.decode_nbest(X, k, scale=.9) for X in utts]
    results = []
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        paths, scores = beer.decode_nbest_batch(model, utts, k, scale=.9, max_frames=max_frames)
        assert scores.shape == (len(lens), k) and scores.dtype == torch.float64 and scores.is_cuda
        assert [tuple(p.shape) for p in paths] == [(k, T) for T in lens]
        assert all(p.dtype == torch.int64 and p.is_cuda for p in paths)
        for u, (p1, s1) in enumerate(one_by_one):
            fin = torch.isfinite(s1)
            assert torch.equal(torch.isfinite(scores[u]).cpu(), fin)
            a, b = scores[u].cpu()[fin], s1[fin]
            assert (torch.abs(a - b) <= 1e-10 * (b.abs() * lens[u] + 1.)).all(), (max_frames, u)
            assert torch.equal(paths[u].cpu(), p1), (max_frames, u)
        results.append((paths, scores))
    # invariant under the split into sub-batches, bit for bit
    assert torch.equal(results[0][1], results[1][1])
    assert all(torch.equal(a, b) for a, b in zip(results[0][0], results[1][0]))
    # packed input; rank 0 is decode_batch
    p2, s2 = beer.decode_nbest_batch(model, (torch.cat(utts), lens), k, scale=.9)
    assert torch.equal(s2, results[0][1]) and all(torch.equal(a, b) for a, b in zip(p2, results[0][0]))
    best = beer.decode_batch(model, utts, scale=.9)
    for u, p in enumerate(best):
        if torch.isfinite(s2[u, 0]):
            assert torch.equal(p2[u][0], p)


def test_alignment_graphs_plain_and_bound():
    from aligned_truth import alignment_set, loop_model
    model, units = loop_model(torch.float64, seed=3)
    model = model.to('cuda')
    seqs = [['s0'], ['s0', 'n0', 's0', 's0'], ['s1', 's0', 'n0', 's2', 's0']]
    gset = alignment_set(units, seqs)
    bound = model.bind_alignment_graphs(gset)
    lens = [7, 40, 61]
    rng = np.random.RandomState(4)
    utts = [torch.from_numpy(rng.randn(T, 4) * 1.5).to('cuda') for T in lens]
    k = 5
    for graphs, what in (([gset[i] for i in range(3)], 'plain'), (list(bound), 'bound')):
        single = [model.decode_nbest(X, k, inference_graph=graphs[i], scale=.8)
                  for i, X in enumerate(utts)]
        for i, X in enumerate(utts):
            p, s = single[i]
            n = int(torch.isfinite(s).sum())
            assert n >= 1 and (torch.diff(s[:n]) <= 0).all(), what
            assert len({tuple(r.tolist()) for r in p[:n]}) == n
            assert torch.equal(p[0], model.decode(X, inference_graph=graphs[i], scale=.8)), what
            # every path is one of the alignment's: the pdfs of its states, each path rescored
            # by the first one's arcs would need the set's own weights -- the kernel-level tests
            # hold the scores; here the paths must stay inside the graph's pdf ids
            assert set(p[:n].reshape(-1).tolist()) <= set(int(j) for j in graphs[i].pdf_id_mapping)
        paths, scores = beer.decode_nbest_batch(model, utts, k, inference_graphs=graphs, scale=.8,
                                                max_frames=50)
        for i, (p, s) in enumerate(single):
            fin = torch.isfinite(s)
            assert torch.equal(torch.isfinite(scores[i]).cpu(), fin), what
            assert (torch.abs(scores[i].cpu()[fin] - s[fin]) <=
                    1e-10 * (s[fin].abs() * lens[i] + 1.)).all(), what
            assert torch.equal(paths[i].cpu(), p), (what, i)
    # ranks without a path: -1 rows beyond the finite scores, whatever their number
    p, s = model.decode_nbest(utts[0], 16, inference_graph=gset[0])
    n = int(torch.isfinite(s).sum())
    assert n >= 1 and torch.isneginf(s[n:]).all()
    assert (p[n:] == -1).all() and (p[:n] >= 0).all()


def run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_decode_nbest(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    run(['dataset', 'create', str(tmp_path), feats, ds])
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    paths, scores = beer.decode_nbest_batch(model, utts, 3)
    scores = scores.cpu().numpy()
    units = [[hmm_cmds.phones_of_path(p, model.start_pdf) for p in ps.cpu().numpy()] for ps in paths]
    assert np.isfinite(scores).all()
    # --nbest 3 with --scores
    sc = tmp_path / 'scores'
    out = run(['hmm', 'decode', '--nbest', '3', '--scores', str(sc), mdl, ds])
    want = [f'{u}-{r + 1} ' + ' '.join(units[i][r]) for i, u in enumerate(ids) for r in range(3)]
    assert out == '\n'.join(want) + '\n'
    assert sc.read_text() == ''.join(f'{u}-{r + 1} {scores[i, r]:.6f}\n'
                                     for i, u in enumerate(ids) for r in range(3))
    # --per-frame: one unit per frame
    per_frame = run(['hmm', 'decode', '--nbest', '3', '--per-frame', mdl, ds]).strip().split('\n')
    assert [len(l.split()) - 1 for l in per_frame] == [35] * 3 + [50] * 3 + [41] * 3
    # --distinct: the best path of each unit sequence, renumbered
    big_p, big_s = beer.decode_nbest_batch(model, utts, 16)
    want, want_scores = [], []
    for i, u in enumerate(ids):
        seen = []
        for p, s in zip(big_p[i].cpu().numpy(), big_s[i].cpu().numpy()):
            seq = hmm_cmds.phones_of_path(p, model.start_pdf)
            if seq not in seen:
                seen.append(seq)
                want.append(f'{u}-{len(seen)} ' + ' '.join(seq))
                want_scores.append(f'{u}-{len(seen)} {s:.6f}\n')
    out = run(['hmm', 'decode', '--nbest', '16', '--distinct', '--scores', str(sc), mdl, ds])
    assert out == '\n'.join(want) + '\n' and len(want) < 48
    assert sc.read_text() == ''.join(want_scores)
    # refused together with --nsamples, and outside 1 .. 16
    for argv in (['--nbest', '3', '--nsamples', '2'], ['--nbest', '0'], ['--nbest', '17']):
        with pytest.raises(SystemExit):
            run(['hmm', 'decode'] + argv + [mdl, ds])
    # plain decode prints what it printed before: the Viterbi path's units, one line an utterance
    plain = run(['hmm', 'decode', mdl, ds])
    best = beer.decode_batch(model, utts)
    assert plain == ''.join(f'{u} ' + ' '.join(hmm_cmds.phones_of_path(p.cpu().numpy(),
                                                                        model.start_pdf)) + '\n'
                            for u, p in zip(ids, best))
    assert plain == ''.join(f'{u} ' + ' '.join(units[i][0]) + '\n' for i, u in enumerate(ids))
