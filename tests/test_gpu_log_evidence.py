"""The forward log-evidence (csrc/hmm_score.hip) against the float64 truth of
tests/evidence_truth.py, on graphs that sit on the boundaries of its forms.

Tolerances, `tol` = 1e-10 (float64) / 1e-5 (float32), the path sampler's:
 * per frame: helpers.rel_err(frame_evidence, c) <= tol over the batch;
 * per utterance: |utt_evidence[u] - total_u| <= tol * (sum_t |c_t| + |tail_u| + 1)
   (evidence_truth.total_bound; a relative bound on the total alone is ill-conditioned).
A pure float32 restatement of the recursion misses the truth by 1.5e-7 .. 9.8e-7 per frame and
1e-9 .. 3e-9 on the total at T = 1000 .. 4096: the bounds leave a factor of 10 over float32.

 * One static table: each case names the route `beer_hmm_evidence_route` must report for it in
   either precision, and the table as a whole reaches every value the route can take.
 * Guards around both outputs, `pc_llhs` unchanged, `frame_evidence = NULL` bit for bit.
 * Long utterances, a per-frame shift of +-3e4, the -inf edges, T = 1.
 * Consistency with the forward-backward `lognorm` and the Viterbi score.
 * The model level: `HMM.log_evidence`, `log_evidence_batch`, `beer hmm score`."""

import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import evidence_truth as et
import fb_truth as ft
from helpers import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
W, B, A, Q = et.WAVE, et.BLOCK, et.ARCS_LDS, et.QUAD
GUARD, SENTINEL = 5, -12345.678

LONG = tuple(ft.VITERBI_LENGTHS) + (7, 8, 9, 3)

# S, offsets, hub members, utterances (a number: fb_truth.lengths; 'long': LONG), pdf-id flavour,
# the route in float64 and in float32
Case = namedtuple('Case', 'S nO hub nutt flavour f64 f32 seed')
CASES = []


def add(S, nO, f64, f32=None, hub=0, nutt=None):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, nutt or (1, 5, 9)[i % 3], ft.FLAVOURS[i % 3], f64,
                      f64 if f32 is None else f32, 700 + i))


# one wave per utterance, one state a lane: up to 64 states, 16 KiB of LDS a wave
add(1, 2, W | 1)
add(3, 2, W | 1)
add(3, 3, W | 1)
add(8, 2, W | 1, nutt='long')
add(8, 3, W | 1)
add(8, 8, W | 1)                       # every arc present
add(64, 2, W | 1)
add(64, 8, W | 1)
add(64, 3, W | 1, hub=8)               # rows of 8 + 3 arcs walked by one lane
add(64, 12, W | 1)
# two states a lane
add(65, 3, W | 2)
add(128, 3, W | 2, nutt='long')
add(128, 8, W | 2)
add(128, 12, B | A | Q, W | 2)          # 1536 arcs: 20 KiB in float64, 14 KiB in float32
add(100, 3, W | 2, hub=30)             # rows of 30 + 3 arcs walked by one lane
# four states a lane, up to 256 states and 16 KiB a wave
add(129, 3, W | 4)
add(200, 4, W | 4, nutt='long')
add(256, 3, W | 4)
add(256, 5, B | A, W | 4)              # 1280 arcs: 18 KiB in float64, 13 KiB in float32
add(256, 8, B | A)
# beyond: a workgroup, one thread a state, strided beyond 256
add(257, 3, B | A)
add(509, 3, B | A, nutt='long')
add(600, 12, B)                        # 7200 arcs no longer fit LDS
# hubs: a phone start has an arc from every phone end -- rows of 40 / 64 / 100 (+ degree) arcs
add(120, 3, B | A | Q, hub=40)
add(256, 3, B | A, hub=64)
add(300, 3, B, hub=100)
# every arc present at 100 states: 80 KB of arcs in float32
add(100, 100, B | Q, nutt=5)


def case_id(c):
    return f'{c.seed}-S{c.S}-O{c.nO}-hub{c.hub}-n{c.nutt}-{c.flavour}'


def test_the_cases_reach_every_value_of_the_route():
    forms = {c.f64 for c in CASES} | {c.f32 for c in CASES}
    assert forms == {W | 1, W | 2, W | 4, B | A | Q, B | Q, B | A, B}
    assert {1, 3, 8, 64, 65, 128, 129, 256, 257, 509, 600} <= {c.S for c in CASES}
    assert {0, 8, 30, 40, 64, 100} <= {c.hub for c in CASES}
    assert set(ft.FLAVOURS) == {c.flavour for c in CASES}


def packed(llhs):
    return torch.cat([tt(l).reshape(-1) for l in llhs])


def compiled(g, ids=None):
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in (range(g['S']) if ids is None else ids)])
    if g['hub'] is not None:
        E, a, B_, c = g['hub']
        graph.set_hub(E, tt(a), B_, tt(c))
    return graph


def guarded_call(batch, flat, per_frame=True):
    '''beer_hmm_log_evidence into the middle of two sentinel-filled buffers: (utt, frame or None)
    after the guards were checked.'''
    n, f = batch.nutt, batch.n_frames
    ubuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device='cuda')
    fbuf = torch.full((f + 2 * GUARD,), SENTINEL, dtype=torch.float64, device='cuda')
    utt, frame = ubuf[GUARD:GUARD + n], fbuf[GUARD:GUARD + f]
    _hip.call('beer_hmm_log_evidence', _hip.dtype_code(batch.dtype), batch.ref(), _hip.ptr(flat),
              _hip.ptr(utt), _hip.ptr(frame) if per_frame else None)
    torch.cuda.synchronize()
    assert (ubuf[:GUARD] == SENTINEL).all() and (ubuf[GUARD + n:] == SENTINEL).all(), \
        'a guard element of utt_evidence was written'
    if per_frame:
        assert (fbuf[:GUARD] == SENTINEL).all() and (fbuf[GUARD + f:] == SENTINEL).all(), \
            'a guard element of frame_evidence was written'
    else:
        assert (fbuf == SENTINEL).all(), 'frame_evidence = NULL, yet something was written'
    return utt.clone(), (frame.clone() if per_frame else None)


def hold(g_of, llhs, lens, utt, frame, tol, what, truths=None):
    '''Both outputs of a batch against the truth: (largest frame error relative to the largest
    |c_t|, largest ratio of a total's error to its bound).  `g_of[u]`: the graph arrays of u.'''
    utt, frame = npy(utt), npy(frame)
    assert utt.dtype == np.float64 and frame.dtype == np.float64
    assert not np.isnan(utt).any() and not np.isnan(frame).any(), f'{what}: NaN'
    truths = truths or [et.evidence(g_of[u], llhs[u]) for u in range(len(lens))]
    c_all = np.concatenate([c for c, _ in truths])
    err = rel_err(frame, c_all)
    print(f'{what}: per-frame rel_err {err:.3e} (bound {tol:.0e})')
    assert err <= tol, f'{what}: per-frame rel_err {err:.3e} > {tol:.1e}'
    worst = 0.
    for u, (c, total) in enumerate(truths):
        if not np.isfinite(total):
            assert utt[u] == total, f'{what} utterance {u}: {utt[u]} for {total}'
            continue
        bound = et.total_bound(c, total, tol)
        d = abs(utt[u] - total)
        worst = max(worst, d / bound)
        assert d <= bound, f'{what} utterance {u}: total off by {d:.3e} > {bound:.3e}'
    print(f'{what}: totals within {worst:.3e} of their bounds')
    return err, worst


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_evidence_is_the_truth(case, dtype):
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype])
    S_total = case.S if case.flavour == 'perm' else case.S + 3
    ids = ft.pdf_ids(case.S, case.flavour, S_total, case.seed)
    graph = compiled(g, ids)
    lens = list(LONG) if case.nutt == 'long' else ft.lengths(case.nutt, case.seed)
    pc_all, llhs = ft.inputs(g, lens, ids, S_total, 1., case.seed, NP[dtype])
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    want = case.f64 if dtype == torch.float64 else case.f32
    route = hk.evidence_route(batch)
    assert route == want, f'route {route:#x}, the table says {want:#x}'
    assert route == et.route_formula(case.S, batch.struct.max_arcs, tt(llhs[0]).element_size())
    # the gather of the product path makes the packed log-likelihoods from the pdf ids
    flat = hk.gather(batch, tt(pc_all), 1.)
    assert torch.equal(flat, packed(llhs))
    before = flat.clone()
    utt, frame = guarded_call(batch, flat)
    hold([g] * len(lens), llhs, lens, utt, frame, TOL[dtype], case_id(case))
    assert torch.equal(flat, before), 'pc_llhs was written'
    # without the per-frame output: the same totals, bit for bit
    alone, _ = guarded_call(batch, flat, per_frame=False)
    assert torch.equal(alone, utt)
    # and through the Python face
    u2, f2 = hk.log_evidence(batch, flat, per_frame=True)
    u3, none = hk.log_evidence(batch, flat)
    assert none is None and torch.equal(u2, utt) and torch.equal(f2, frame) and torch.equal(u3, utt)
    assert u2.dtype == torch.float64 and u2.is_cuda and f2.shape == (sum(lens),)


MIXED_LENS, MIXED_GIDS = [33, 65, 32, 2, 64, 1], [0, 1, 2, 0, 2, 1]


@DTYPES
@pytest.mark.parametrize('sizes,want', [((7, 65, 129), W | 4), ((7, 65, 300), B | A)],
                         ids=['wave', 'block'])
def test_graphs_of_different_sizes_in_one_launch(sizes, want, dtype):
    'Alignment-graph style: the form follows the largest graph, every utterance its own.'
    arrays = [ft.make_graph(S, ft.offsets(3, S), 2100 + k, 0, NP[dtype]) for k, S in enumerate(sizes)]
    graphs = [compiled(g) for g in arrays]
    rng = np.random.RandomState(5)
    llhs = [(rng.randn(T, sizes[k]) * 3).astype(NP[dtype]) for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert hk.evidence_route(batch) == want
    utt, frame = guarded_call(batch, packed(llhs))
    hold([arrays[k] for k in MIXED_GIDS], llhs, MIXED_LENS, utt, frame, TOL[dtype], str(sizes))


# --- length: drift and range ---------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize('S,T,want', [(16, 4096, W | 1), (300, 1000, B | A)], ids=['S16', 'S300'])
def test_long_utterances(S, T, want, dtype):
    g = ft.make_graph(S, ft.offsets(3, S), 31, 0, NP[dtype])
    _, llhs = ft.inputs(g, [T], np.arange(S), S, 1., 32, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0], [T], dtype)
    assert hk.evidence_route(batch) == want
    utt, frame = hk.log_evidence(batch, packed(llhs), per_frame=True)
    hold([g], llhs, [T], utt, frame, TOL[dtype], f'S={S} T={T}')


# --- shift -----------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize('S,nO,want', [(16, 3, W | 1), (300, 3, B | A)], ids=['wave', 'block'])
def test_a_per_frame_shift_moves_the_evidence_by_the_shift(S, nO, want, dtype):
    '''k_t in +-3e4 added to every entry of row t: c_t moves by k_t, the total by sum_t k_t.  The
    log-likelihoods and the shifts are multiples of 1/64 (below 2^24 / 64), so the shifted rows are
    exact in float32 too; every bound is sized with the magnitudes of the run it holds.'''
    tol = TOL[dtype]
    g = ft.make_graph(S, ft.offsets(nO, S), 51, 0, NP[dtype])
    lens = [200, 1, 9, 33]
    rng = np.random.RandomState(52)
    base = [(rng.randint(-512, 513, size=(T, S)) / 64.).astype(NP[dtype]) for T in lens]
    ks = [rng.randint(-30000 * 64, 30000 * 64 + 1, size=T) / 64. for T in lens]
    shifted = [(l.astype(np.float64) + k[:, None]).astype(NP[dtype]) for l, k in zip(base, ks)]
    for l, s, k in zip(base, shifted, ks):
        assert (s.astype(np.float64) - l.astype(np.float64) == k[:, None]).all()
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    assert hk.evidence_route(batch) == want
    u0, f0 = hk.log_evidence(batch, packed(base), per_frame=True)
    u1, f1 = hk.log_evidence(batch, packed(shifted), per_frame=True)
    t0 = [et.evidence(g, l) for l in base]
    t1 = [et.evidence(g, l) for l in shifted]
    hold([g] * len(lens), base, lens, u0, f0, tol, 'unshifted', t0)
    hold([g] * len(lens), shifted, lens, u1, f1, tol, 'shifted', t1)
    # the truth itself moves by the shift, and so do the kernel's values within both runs' bounds
    k_all = np.concatenate(ks)
    c0, c1 = np.concatenate([c for c, _ in t0]), np.concatenate([c for c, _ in t1])
    np.testing.assert_allclose(c1 - c0, k_all, rtol=0, atol=1e-10 * np.abs(c1).max())
    d = np.abs(npy(f1) - npy(f0) - k_all).max()
    bound = tol * (np.abs(c0).max() + np.abs(c1).max())
    print(f'frames move by k_t within {d:.3e} (bound {bound:.3e})')
    assert d <= bound
    for u, k in enumerate(ks):
        bound = et.total_bound(*t0[u], tol) + et.total_bound(*t1[u], tol)
        d = abs(float(u1[u]) - float(u0[u]) - k.sum())
        assert d <= bound, f'utterance {u}: total moves by sum k_t within {d:.3e} > {bound:.3e}'


# --- edges -----------------------------------------------------------------------------------
EDGE_GRAPHS = pytest.mark.parametrize('S,want', [(8, W | 1), (300, B | A)], ids=['wave', 'block'])


def edge_graph(S, dtype, last_only=False):
    'Self-loop and step to the next state; `last_only`: only the last state may end an utterance.'
    g = ft.make_graph(S, (0, 1), 5, 0, NP[dtype])
    if last_only:
        g['final'][:] = -np.inf
        g['final'][S - 1] = 0.
    return g


@DTYPES
@EDGE_GRAPHS
def test_scattered_inf_entries_that_leave_the_utterance_reachable(S, want, dtype):
    g = edge_graph(S, dtype)
    lens = [12, 1, 5, 30]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 6, NP[dtype])
    rng = np.random.RandomState(7)
    for l in llhs:
        holes = rng.random_sample(l.shape) < .3
        holes[:, 0] = False                             # state 0 and its self-loop stay
        l[holes] = -np.inf
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    assert hk.evidence_route(batch) == want
    utt, frame = guarded_call(batch, packed(llhs))
    assert torch.isfinite(utt).all() and torch.isfinite(frame).all()
    hold([g] * len(lens), llhs, lens, utt, frame, TOL[dtype], f'holes S={S}')


@DTYPES
@EDGE_GRAPHS
def test_a_dead_frame_in_one_utterance_of_five(S, want, dtype):
    g = edge_graph(S, dtype)
    lens = [6, 5, 7, 4, 9]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 8, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    assert hk.evidence_route(batch) == want
    u0, f0 = guarded_call(batch, packed(llhs))
    llhs[2][3] = -np.inf                                # nothing explains frame 3 of utterance 2
    u1, f1 = guarded_call(batch, packed(llhs))
    hold([g] * len(lens), llhs, lens, u1, f1, TOL[dtype], f'dead frame S={S}')
    off = np.concatenate([[0], np.cumsum(lens)])
    dead = np.arange(off[2] + 3, off[3])
    f0, f1, u0, u1 = npy(f0), npy(f1), npy(u0), npy(u1)
    assert np.isneginf(f1[dead]).all() and np.isneginf(u1[2])
    # the other four utterances: as without it, bit for bit; the frames before the dead one
    # within the bound (the one-wave form starts such an utterance again in log space)
    keep = np.setdiff1d(np.arange(off[-1]), np.arange(off[2], off[3]))
    np.testing.assert_array_equal(f1[keep], f0[keep])
    early = np.arange(off[2], off[2] + 3)
    assert np.abs(f1[early] - f0[early]).max() <= 2 * TOL[dtype] * np.abs(f0[early]).max()
    np.testing.assert_array_equal(np.delete(u1, 2), np.delete(u0, 2))
    assert np.isfinite(f0).all() and np.isfinite(u0).all()


@DTYPES
@EDGE_GRAPHS
def test_an_unreachable_final_leaves_the_frames_finite(S, want, dtype):
    '''Only the last state may end an utterance; utterances shorter than S - 3 frames cannot
    reach it from the three initial states: finite frames, a total of -inf.'''
    g = edge_graph(S, dtype, last_only=True)
    lens = [1, 2, S + 4, 5]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 9, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    assert hk.evidence_route(batch) == want
    utt, frame = guarded_call(batch, packed(llhs))
    hold([g] * len(lens), llhs, lens, utt, frame, TOL[dtype], f'unreachable final S={S}')
    utt = npy(utt)
    assert torch.isfinite(frame).all()
    assert np.isneginf(utt[[0, 1]]).all() and np.isfinite(utt[2])
    assert np.isneginf(utt[3]) == (5 < S - 2)


@DTYPES
def test_what_the_scaled_pass_cannot_hold_is_redone_in_log_space(dtype):
    '''The one-wave form runs on scaled probabilities.  Utterance 0: the only path that survives
    frame 1 carries exp(-2000) of frame 0's mass -- 0 in fp64; utterance 2's graph has an arc of
    weight -100, exp of which float32 cannot hold.  Both come out of log space, finite and within
    the bounds; utterances 1 and 3 are ordinary.'''
    S = 8
    g = edge_graph(S, dtype)
    thin = edge_graph(S, dtype)
    thin['trans'][1, 2] = -100.
    lens = [3, 6, 7, 5]
    gids = [0, 0, 1, 1]
    arrays = [g, thin]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 10, NP[dtype])
    llhs[0][:] = -np.inf
    llhs[0][0, 0], llhs[0][0, 1] = 0., -2000.
    llhs[0][1, 2] = 0.
    llhs[0][2, 2] = llhs[0][2, 3] = -1.
    batch = hk.HmmBatch([compiled(g), compiled(thin)], gids, lens, dtype)
    assert hk.evidence_route(batch) == W | 1
    utt, frame = guarded_call(batch, packed(llhs))
    assert torch.isfinite(utt).all() and torch.isfinite(frame).all()
    hold([arrays[k] for k in gids], llhs, lens, utt, frame, TOL[dtype], 'redone in log space')
    assert float(utt[0]) < -1999.


@DTYPES
@pytest.mark.parametrize('S,want', [(8, W | 1), (65, W | 2), (300, B | A)])
def test_one_frame(S, want, dtype):
    g = ft.make_graph(S, ft.offsets(3, S), 9, 0, NP[dtype])
    _, llhs = ft.inputs(g, [1], np.arange(S), S, 1., 9, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0], [1], dtype)
    assert hk.evidence_route(batch) == want
    utt, frame = guarded_call(batch, packed(llhs))
    hold([g], llhs, [1], utt, frame, TOL[dtype], f'T=1 S={S}')
    # c_0 = ln sum_j exp(init_j + l_0(j)) over the three initial states
    a = g['init'][:3].astype(np.float64) + llhs[0][0, :3].astype(np.float64)
    assert abs(float(frame[0]) - np.log(np.exp(a).sum())) <= TOL[dtype] * abs(float(frame[0]))


def test_arguments_are_checked():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    batch = hk.HmmBatch([compiled(g)], [0], [4], torch.float64)
    flat = torch.zeros(12, dtype=torch.float64, device='cuda')
    utt = torch.zeros(1, dtype=torch.float64, device='cuda')
    lib = _hip.lib()
    assert lib.beer_hmm_log_evidence(_hip.F64, batch.ref(), None, _hip.ptr(utt), None, None) == _hip.EINVAL
    assert lib.beer_hmm_log_evidence(_hip.F64, batch.ref(), _hip.ptr(flat), None, None, None) == _hip.EINVAL
    assert lib.beer_hmm_log_evidence(7, batch.ref(), _hip.ptr(flat), _hip.ptr(utt), None, None) == _hip.EINVAL


# --- consistency with what the parent computes -------------------------------------------------

@DTYPES
@pytest.mark.parametrize('S,nO,hub', [(8, 3, 0), (120, 3, 40), (300, 3, 0)])
def test_agrees_with_the_forward_backward_lognorm_and_bounds_the_viterbi_score(S, nO, hub, dtype):
    '''`lognorm_mean` of beer_hmm_forward_backward is this number, stored in the dtype and held by
    its own tests to 1e-5 / 1e-10 of its size: the two agree within this kernel's bound plus that.'''
    tol = TOL[dtype]
    g = ft.make_graph(S, ft.offsets(nO, S), 61, hub, NP[dtype])
    graph = compiled(g)
    lens = [40, 1, 9, 17]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 62, NP[dtype])
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    flat = packed(llhs)
    utt = npy(hk.log_evidence(batch, flat)[0])
    lognorm = npy(hk.forward_backward(batch, flat, want_lognorm=True)[3]).astype(np.float64)
    for u, l in enumerate(llhs):
        c, total = et.evidence(g, l)
        slack = et.total_bound(c, total, tol) + tol * abs(total)
        assert abs(utt[u] - lognorm[u]) <= slack, (u, utt[u], lognorm[u])
        one = float(graph.posteriors(tt(l))[1])
        assert abs(utt[u] - one) <= slack, (u, utt[u], one)
        # the best path is one of the paths the evidence sums over
        path = ft.best_path(g, l)
        f64 = {k: g[k].astype(np.float64) for k in ('init', 'final', 'trans')}
        score = f64['init'][path[0]] + l.astype(np.float64)[np.arange(len(l)), path].sum() + \
            f64['trans'][path[:-1], path[1:]].sum() + f64['final'][path[-1]]
        assert utt[u] >= score - et.total_bound(c, total, tol), (u, utt[u], score)


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


def model_truth(model, X, arrays, ids, scale):
    'The truth from the per-pdf log-likelihoods the model itself computes, read back.'
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    return et.evidence(arrays, scale * npy(pc_all).astype(np.float64)[:, np.asarray(ids)])


def hold_model(value, frame, truth, what):
    c, total = truth
    assert value.dim() == 0 and value.dtype == torch.float64 and value.is_cuda
    if np.isfinite(total):
        assert abs(float(value) - total) <= et.total_bound(c, total, 1e-10), what
    else:                               # (one frame cannot reach the end of a left-to-right unit)
        assert float(value) == total, what
    if frame is not None:
        assert frame.shape == c.shape and frame.dtype == torch.float64
        assert rel_err(npy(frame), c) <= 1e-10, what


@pytest.mark.parametrize('kind', ['hmm', 'phoneloop', 'bigram'])
def test_model_log_evidence_is_the_truth(kind):
    model = make_model(kind)
    arrays = dense_arrays(model.graph)
    for X, scale in zip(utterances([57, 1, 23], 1), (1., 1., .7)):
        truth = model_truth(model, X, arrays, model.graph.pdf_id_mapping, scale)
        value, frame = model.log_evidence(X, scale=scale, per_frame=True)
        hold_model(value, frame, truth, kind)
        assert torch.equal(model.log_evidence(X, scale=scale), value)
        # the model's own graph handed in as an inference graph: the same launch
        assert torch.equal(model.log_evidence(X, inference_graph=model.graph, scale=scale), value)


def test_learned_transitions_on_bound_alignment_graphs():
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
    stale = [float(model.log_evidence(X, inference_graph=bound[i])) for i, X in enumerate(utts)]
    # move the posterior away from the prior AFTER the graphs were bound and used
    gen = torch.Generator().manual_seed(1)
    for p in model.transitions.parameters_of_groups():
        conc = p.posterior.params.concentrations
        conc.add_(torch.rand(conc.shape, generator=gen, dtype=torch.float64).to(conc) * 3)
    model._on_transitions_update()
    tmap, log_a = CategoryMap(model), expected_log_probs(model.transitions)
    truths = []
    for i, X in enumerate(utts):
        dense = gset[i].to_dense()
        src, dst, cats, last = tmap.arcs(seqs[i], dense)
        trans = np.full((len(last), len(last)), -np.inf)
        trans[src, dst] = log_a[cats]
        arrays = dict(S=len(last), init=dense.init_log_probs.double().numpy(),
                      final=dense.final_log_probs.double().numpy(), trans=trans)
        truths.append(model_truth(model, X, arrays, dense.pdf_id_mapping, .8))
        value, frame = model.log_evidence(X, inference_graph=bound[i], scale=.8, per_frame=True)
        hold_model(value, frame, truths[-1], f'bound graph {i}')
        assert float(model.log_evidence(X, inference_graph=bound[i])) != stale[i]
    # batched, every utterance with its own graph, in sub-batches
    got, frames = beer.log_evidence_batch(model, utts, inference_graphs=list(bound), scale=.8,
                                          per_frame=True, max_frames=50)
    for i, (c, total) in enumerate(truths):
        assert abs(float(got[i]) - total) <= et.total_bound(c, total, 1e-10)
        assert rel_err(npy(frames[i]), c) <= 1e-10
    with pytest.raises(ValueError):
        beer.log_evidence_batch(model, utts, inference_graphs=list(bound)[:2])


@pytest.mark.parametrize('kind', ['phoneloop', 'bigram'])
def test_log_evidence_batch_is_log_evidence_per_utterance(kind):
    '''The batched call computes the emissions with the shard's E-step kernels, the model's call
    with the per-call ones: the same numbers within the float64 bounds, not bit for bit.'''
    model = make_model(kind)
    lens = [23, 40, 9, 31, 1]
    utts = utterances(lens, 3)
    one_by_one = [model.log_evidence(X, scale=.9, per_frame=True) for X in utts]
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        got, frames = beer.log_evidence_batch(model, utts, scale=.9, per_frame=True,
                                              max_frames=max_frames)
        assert got.shape == (len(lens),) and got.dtype == torch.float64 and got.is_cuda
        assert [tuple(f.shape) for f in frames] == [(T,) for T in lens]
        for u, (value, frame) in enumerate(one_by_one):
            c = npy(frame)
            if torch.isfinite(value):
                assert abs(float(got[u]) - float(value)) <= \
                    et.total_bound(c, float(value), 1e-10), (max_frames, u)
            else:                       # (one frame cannot reach the end of a left-to-right unit)
                assert lens[u] == 1 and float(got[u]) == float(value)
            assert rel_err(npy(frames[u]), c) <= 1e-10
        assert torch.equal(beer.log_evidence_batch(model, utts, scale=.9, max_frames=max_frames), got)
    # packed input
    packed_in = (torch.cat(utts), lens)
    assert torch.equal(beer.log_evidence_batch(model, packed_in, scale=.9), got)


def run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_score(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    run(['dataset', 'create', str(tmp_path), feats, ds])
    out = run(['hmm', 'score', mdl, ds]).strip().split('\n')
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    want = beer.log_evidence_batch(model, utts).cpu().tolist()
    assert out == [f'{u} {v:.6f} {len(x)}' for u, v, x in zip(ids, want, utts)]
    assert [int(l.split()[2]) for l in out] == [35, 50, 41]
    # a scale and a list of utterances
    (tmp_path / 'utts').write_text('utt2\nutt0\n')
    out = run(['hmm', 'score', '-s', '0.5', '-u', str(tmp_path / 'utts'), mdl, ds]).strip().split('\n')
    want = beer.log_evidence_batch(model, [utts[2], utts[0]], scale=.5).cpu().tolist()
    assert out == [f'utt2 {want[0]:.6f} 41', f'utt0 {want[1]:.6f} 35']
