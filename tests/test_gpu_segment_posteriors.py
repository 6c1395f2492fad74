"""The segment posteriors (csrc/hmm_segposts.hip) against the float64 truth of
tests/segposts_truth.py, on the smallest shapes at which each form of the two kernels can go wrong.

Tolerances, the project's `tol` = 1e-10 (float64) / 1e-5 (float32), absolute on probabilities, as
tests/test_gpu_arc_posteriors.py and DESIGN section 8 have it:
 * `seg` and `starts` within tol of the truth, every cell of every case; `evidence` within
   evidence_truth.total_bound, as tests/test_gpu_log_evidence.py holds utt_evidence;
 * `starts` within 2 tol of `hk.arc_posteriors`' frame_out (each is within tol of the truth);
 * with max_dur >= T a row of `seg` sums to its entry's start posterior within tol (max_dur + 1):
   max_dur cells and the start posterior itself, each within tol;
 * with min_post = 0 the segments that cover a frame sum to 1 within tol x their number;
 * a constant added to every log-likelihood of a frame (its own, in +-1e4) leaves everything but
   `evidence` within 2 tol (the inputs are multiples of 1/64, so the shifted ones are exact in
   float32 too).

 * One table of cases: each names the form `beer_hmm_segposts_route` must report (team size, arcs
   in LDS, bins in LDS); together they reach every team size, 4 .. 256, strided lanes,
   S > 256, arcs read from global memory, bins in the output rows, graphs of different sizes in one
   launch, an alignment chain with a repeated unit, T = 1, 2 and 17, and a ragged batch with an
   utterance of no frames, a dead frame, an unreachable final and scattered -inf.
 * max_dur 1, 2, T, T + 2 with min_post 0 and 0.05; `entries=` twice the same bits; the entries
   of `hk.segment_margins`; guards around every buffer the two kernels write.
 * The model level: `unit_segment_posteriors`, `unit_durations`, their batch forms, bound
   alignment graphs, `beer hmm segments`."""

import ctypes
import functools
import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import arcs_truth as at
import evidence_truth as et
import segposts_truth as sp
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
K, L, BL = sp.BLOCK, sp.ARCS_LDS, sp.BINS_LDS
GUARD, SENTINEL = 5, -12345.678

# graphs: (builder, arguments) of every distinct graph; gids, lens: the utterances; route: what
# beer_hmm_segposts_route must report in both precisions; edits: per utterance what is done to its
# log-likelihoods ('holes': scattered -inf, 'frame': a frame of all -inf)
Case = namedtuple('Case', 'name graphs gids lens n_cat route edits')
OPEN = dict(open_end=True)
CHAIN = ('chain', ([1, 0, 1, 2, 1], 2), {})
CASES = [
    Case('loop3x3', [('loop', ([3, 3, 3],), OPEN)], [0] * 3, [1, 2, 17], 3, K | L | BL | 2, {}),
    Case('loop125', [('loop', ([1, 2, 5],), dict(skips=(1, 2), open_end=True))], [0] * 2, [17, 9], 3,
         K | L | BL | 3, {1: 'holes'}),
    Case('loop12', [('loop', ([12, 3],), dict(skips=(1, 3), open_end=True))], [0], [9], 2,
         K | L | BL | 4, {}),
    Case('u20', [('loop', ([20, 3],), dict(skips=(1, 4), open_end=True))], [0], [9], 2,
         K | L | BL | 5, {}),
    Case('u40', [('loop', ([40, 3],), dict(skips=(1, 6), open_end=True))], [0], [9], 2,
         K | L | BL | 6, {0: 'holes'}),
    # (a unit that repeats: the closure of unit 1 is the union of three instances; 1 and 2 frames
    #  cannot cross the chain's 10 states: dead utterances before a live one)
    Case('chain', [CHAIN], [0] * 3, [1, 2, 17], 3, K | L | BL | 3, {}),
    Case('ninety', [('loop', ([3] * 90,), OPEN)], [0], [9], 90, K | BL | 2, {}),
    Case('u70', [('loop', ([70],), dict(skips=(1, 9), open_end=True))], [0] * 2, [12, 5], 1,
         K | L | BL | 7, {}),
    Case('u130', [('loop', ([130],), dict(skips=(1, 17), open_end=True))], [0], [12], 1,
         K | L | BL | 8, {}),
    Case('u200', [('loop', ([200],), dict(skips=(1, 29), open_end=True))], [0], [11], 1,
         K | L | BL | 8, {0: 'holes'}),
    Case('big', [('loop', ([300, 3],), dict(skips=(1, 7, 50), open_end=True))], [0] * 2, [9, 2], 2,
         K | L | BL | 8, {}),
    Case('arcs', [('loop', ([3] * 72,), OPEN)], [0] * 2, [9, 4], 72, K | BL | 2, {}),
    Case('bins', [('loop', ([3, 3, 3],), dict(open_end=True, labels=[0, 500, 1024]))], [0] * 2,
         [7, 12], 1025, K | L | 2, {}),
    # no frames; T = 1; a frame of all -inf; a chain too short to reach its final; ordinary ones
    Case('ragged', [('loop', ([3, 3, 3],), OPEN), ('chain', ([1, 0, 1], 3), {}),
                    ('loop', ([5] * 3,), OPEN)], [0, 2, 0, 1, 0, 1, 2], [0, 1, 8, 5, 17, 12, 6], 3,
         K | L | BL | 3, {2: 'frame', 4: 'holes', 5: 'holes'}),
]
IDS = [c.name for c in CASES]


def test_the_cases_reach_every_form():
    assert {_hip.segposts_team(c.route) for c in CASES} == {4, 8, 16, 32, 64, 128, 256}
    assert {c.route & 0xF00 for c in CASES} >= {L | BL, BL, L}
    for name in ('loop3x3', 'chain'):
        assert {1, 2, 17} <= set(CASES[IDS.index(name)].lens)
    assert {0, 1} <= set(CASES[IDS.index('ragged')].lens)


def packed(llhs, dtype):
    if not llhs:
        return torch.zeros(0, dtype=dtype, device='cuda')
    return torch.cat([tt(np.asarray(l, dtype=NP[dtype])).reshape(-1) for l in llhs])


def compiled(g):
    return beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                    [int(i) for i in range(g['S'])])


Truth = namedtuple('Truth', 'post starts evidence c')


def truth_of(g, llh, arc_cat, init_cat, n_cat, max_dur):
    post, starts, evidence = sp.segment_posteriors(g, llh, arc_cat, init_cat, n_cat, max_dur)
    c = et.evidence(g, llh)[0] if len(llh) else np.zeros(0)
    return Truth(post, starts, evidence, c)


@functools.lru_cache(maxsize=None)
def case_data(name):
    '''(arrays, cats, llhs, truths) of a case, computed once, never changed and shared by both
    precisions: the weights and the log-likelihoods are multiples of 1/64, exact in float32.  The
    truth of an utterance has T + 2 columns: a smaller max_dur cuts columns and nothing else
    (tests/test_segment_posteriors_host.py).'''
    case = CASES[IDS.index(name)]
    built = [(sp.loop_graph if kind == 'loop' else sp.chain_graph)(*args, seed=3 + k, real=True, **kw)
             for k, (kind, args, kw) in enumerate(case.graphs)]
    arrays, cats = [b[0] for b in built], [b[1:] for b in built]
    rng = np.random.RandomState(len(name))
    llhs = []
    for u, (T, gid) in enumerate(zip(case.lens, case.gids)):
        S = arrays[gid]['S']
        llh = np.round(rng.randn(T, S) * 3 * 64) / 64
        if case.edits.get(u) == 'holes':
            llh[rng.rand(T, S) < .1] = -np.inf
        if case.edits.get(u) == 'frame':
            llh[T // 2] = -np.inf
        llhs.append(llh)
    truths = [truth_of(arrays[gid], llh, *cats[gid], case.n_cat, len(llh) + 2)
              for llh, gid in zip(llhs, case.gids)]
    return arrays, cats, llhs, truths


def run(case, arrays, cats, llhs, dtype, min_post, max_dur, **kw):
    batch = hk.HmmBatch([compiled(g) for g in arrays], case.gids, case.lens, dtype)
    flat = packed(llhs, dtype)
    out = hk.segment_posteriors(batch, flat, [c[0] for c in cats], [c[1] for c in cats], case.n_cat,
                                min_post, max_dur, **kw)
    return batch, flat, out


def columns(post, max_dur):
    'The truth [T, n_cat, D] cut or padded with zeros to max_dur columns.'
    if max_dur <= post.shape[2]:
        return post[:, :, :max_dur]
    return np.concatenate([post, np.zeros(post.shape[:2] + (max_dur - post.shape[2],))], 2)


def clean(got, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f'{what}: NaN or inf'
    return got


def hold(out, truths, lens, n_cat, min_post, max_dur, dtype, what, entries=None):
    '''Every output of every utterance against the truth; the entries are the cells of the returned
    `starts` that are >= min_post and > 0, row-major (or `entries`).  Returns the largest error as
    a fraction of its bound.'''
    tol = TOL[dtype]
    evidence, starts, entry_frame, entry_cat, seg = out
    assert evidence.dtype == torch.float64 and evidence.shape == (len(lens),)
    assert starts.dtype == dtype and starts.shape == (sum(lens), n_cat)
    assert entry_frame.dtype == torch.int64 and entry_cat.dtype == torch.int32
    assert seg.dtype == dtype and seg.shape == (len(entry_frame), max_dur)
    evidence, entry_frame, entry_cat = npy(evidence), npy(entry_frame), npy(entry_cat)
    starts, seg = clean(npy(starts), what + ': starts'), clean(npy(seg), what + ': seg')
    assert not np.isnan(evidence).any() and (evidence < np.inf).all()
    assert (seg >= 0).all() and (starts >= 0).all()
    if entries is None:
        at_ = np.argwhere((starts >= NP[dtype](min_post)) & (starts > 0))
        assert np.array_equal(entry_frame, at_[:, 0]) and np.array_equal(entry_cat, at_[:, 1]), \
            f'{what}: the entries are not the cells of starts that are >= min_post'
    else:
        assert np.array_equal(entry_frame, entries[0]) and np.array_equal(entry_cat, entries[1])
    worst, f0 = 0., 0
    for u, t in enumerate(truths):
        T = lens[u]
        tag = f'{what} utterance {u}'
        if np.isfinite(t.evidence):
            bound = et.total_bound(t.c, t.evidence, tol)
            worst = max(worst, abs(evidence[u] - t.evidence) / bound)
            assert abs(evidence[u] - t.evidence) <= bound, f'{tag}: evidence {evidence[u]} for {t.evidence}'
        else:
            assert evidence[u] == t.evidence, f'{tag}: evidence {evidence[u]} for {t.evidence}'
        mine = (entry_frame >= f0) & (entry_frame < f0 + T)
        if T:
            d = np.abs(starts[f0:f0 + T] - t.starts).max()
            assert d <= tol, f'{tag}: starts off by {d:.3e}'
            worst = max(worst, d / tol)
            want = columns(t.post, max_dur)[entry_frame[mine] - f0, entry_cat[mine]]
            d = np.abs(seg[mine] - want).max(initial=0.)
            assert d <= tol, f'{tag}: seg off by {d:.3e}'
            worst = max(worst, d / tol)
            # the rows sum to the start posteriors once nothing is cut
            if max_dur >= T:
                d = np.abs(seg[mine].sum(1) - starts[entry_frame[mine], entry_cat[mine]]).max(initial=0.)
                assert d <= tol * (max_dur + 1), f'{tag}: a row sums to its start posterior within {d:.3e}'
                worst = max(worst, d / (tol * (max_dur + 1)))
        if not np.isfinite(t.evidence):
            assert not starts[f0:f0 + T].any(), f'{tag}: dead, yet it has start posteriors'
            assert entries is not None or not mine.any(), f'{tag}: dead, yet it has entries'
            assert not seg[mine].any()
        elif min_post == 0. and entries is None and max_dur >= T and T:
            # every frame is covered with probability 1 (every initial state has a category)
            mass, count = np.zeros(T), np.zeros(T)
            for s, row in zip(entry_frame[mine] - f0, seg[mine]):
                for k in np.nonzero(row)[0]:
                    mass[s:s + k + 1] += row[k]
                    count[s:s + k + 1] += 1
            d = np.abs(mass - 1.) / (tol * np.maximum(count, 1))
            assert d.max() <= 1., f'{tag}: coverage off by {np.abs(mass - 1.).max():.3e}'
            worst = max(worst, d.max())
        f0 += T
    print(f'{what}: within {worst:.3f} of the bound')
    return worst


@DTYPES
@pytest.mark.parametrize('name', IDS)
def test_segment_posteriors_are_the_truth(name, dtype):
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name)
    arc_cats, init_cats = [c[0] for c in cats], [c[1] for c in cats]
    T = max(case.lens)
    batch, flat, out = run(case, arrays, cats, llhs, dtype, 0., T)
    smap = hk.segment_map(batch.source_graphs, arc_cats, init_cats, case.n_cat)
    route = hk.segposts_route(batch, case.n_cat, smap.max_closure)
    assert route == case.route, f'route {route:#x}, the table says {case.route:#x}'
    assert route == sp.route_formula(batch.struct.max_states, batch.struct.max_arcs,
                                     flat.element_size(), case.n_cat, smap.max_closure)
    before = flat.clone()
    hold(out, truths, case.lens, case.n_cat, 0., T, dtype, name)
    assert torch.equal(flat, before), 'pc_llhs was written'
    # the project's own kernel: the same start posteriors
    frame = hk.arc_posteriors(batch, flat, arc_cats, init_cats, case.n_cat)[0]
    d = float((out[1].double() - frame.double()).abs().max()) if frame.numel() else 0.
    print(f'{name}: starts within {d / (2 * TOL[dtype]):.3f} of 2 tol of arc_posteriors')
    assert d <= 2 * TOL[dtype]
    # every max_dur, with and without a threshold, also with a map built beforehand
    for max_dur in (1, 2, T + 2):
        for min_post in (0., .05):
            _, _, small = run(case, arrays, cats, llhs, dtype, min_post, max_dur, seg_map=smap)
            hold(small, truths, case.lens, case.n_cat, min_post, max_dur, dtype,
                 f'{name} max_dur {max_dur} min_post {min_post}')
    # the same entries: the same bits, whatever the order of the atomic adds made of `starts`
    fixed = (out[2], out[3])
    a = hk.segment_posteriors(batch, flat, arc_cats, init_cats, case.n_cat, 0., T, entries=fixed)
    b = hk.segment_posteriors(batch, flat, arc_cats, init_cats, case.n_cat, .5, T, seg_map=smap,
                              entries=fixed)
    for x, y in ((a[4], b[4]), (a[4], out[4]), (a[0], b[0]), (a[2], out[2]), (a[3], out[3])):
        assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8),
                                                  y.contiguous().view(torch.uint8)), 'the bits differ'


@DTYPES
@pytest.mark.parametrize('name', ['loop3x3', 'loop125', 'chain', 'u130', 'big', 'ragged'])
def test_a_constant_per_frame_moves_the_evidence_alone(name, dtype):
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name)
    T = max(case.lens)
    _, _, out = run(case, arrays, cats, llhs, dtype, 0., T)
    rng = np.random.RandomState(5)
    shifts = [rng.randint(-10000, 10001, size=len(l)).astype(np.float64) for l in llhs]
    moved = [l + k[:, None] for l, k in zip(llhs, shifts)]
    for l in moved:
        assert np.array_equal(l.astype(np.float32).astype(np.float64), l)   # exact in float32
    _, _, got = run(case, arrays, cats, moved, dtype, 0., T, entries=(out[2], out[3]))
    for o in got:
        assert not torch.isnan(o.double()).any()
    assert torch.isfinite(got[1]).all() and torch.isfinite(got[4]).all()
    tol = TOL[dtype]
    d = max(float((got[k].double() - out[k].double()).abs().max()) if out[k].numel() else 0. for k in (1, 4))
    print(f'{name}: the shifted outputs within {d / (2 * tol):.3f} of 2 tol')
    assert d <= 2 * tol
    for u, (k, t) in enumerate(zip(shifts, truths)):
        if np.isfinite(t.evidence):
            bound = 2 * et.total_bound(t.c, t.evidence, tol) + tol * np.abs(k).sum()
            assert abs(float(got[0][u]) - float(out[0][u]) - k.sum()) <= bound
        else:
            assert float(got[0][u]) == float(out[0][u]) == t.evidence


@DTYPES
@pytest.mark.parametrize('name', ['loop3x3', 'loop125', 'chain', 'ragged'])
def test_the_entries_of_segment_margins_get_their_posteriors(name, dtype):
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name)
    arc_cats, init_cats = [c[0] for c in cats], [c[1] for c in cats]
    T = max(case.lens)
    batch, flat, out = run(case, arrays, cats, llhs, dtype, 0., T)
    _, _, frame, cat, margin = hk.segment_margins(batch, flat, arc_cats, init_cats, case.n_cat, 5., T)
    assert len(frame) > 0
    got = hk.segment_posteriors(batch, flat, arc_cats, init_cats, case.n_cat, 0., T, entries=(frame, cat))
    hold(got, truths, case.lens, case.n_cat, 0., T, dtype, name + ' lattice entries',
         entries=(npy(frame), npy(cat)))
    # the same cells of the min_post = 0 run (a cell it does not have is a row of zeros)
    dense = torch.zeros(sum(case.lens), case.n_cat, T, dtype=dtype, device='cuda')
    dense[out[2], out[3].long()] = out[4]
    d = float((dense[frame, cat.long()].double() - got[4].double()).abs().max())
    assert d <= TOL[dtype]
    # a segment within the beam is a possible one: its posterior is not 0 in the truth
    f0s = np.concatenate([[0], np.cumsum(case.lens)])
    utt = np.searchsorted(f0s[1:], npy(frame), side='right')
    fin = np.isfinite(npy(margin).astype(np.float64))
    for n in range(len(utt)):
        want = columns(truths[utt[n]].post, T)[npy(frame)[n] - f0s[utt[n]], npy(cat)[n]]
        assert (want[fin[n]] > 0).all()


@DTYPES
@pytest.mark.parametrize('name', ['loop3x3', 'u70', 'big', 'bins', 'ragged'])
def test_nothing_is_written_beside_the_outputs(name, dtype):
    'The two entry points on sentinel-guarded buffers; entries out of range get rows of zeros.'
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name)
    batch = hk.HmmBatch([compiled(g) for g in arrays], case.gids, case.lens, dtype)
    flat, dev, n_cat = packed(llhs, dtype), 'cuda', case.n_cat
    dcode = _hip.dtype_code(dtype)
    arc_cats, init_cats = [c[0] for c in cats], [c[1] for c in cats]
    smap = hk.segment_map(batch.source_graphs, arc_cats, init_cats, n_cat)
    arcs, inits = tt(np.concatenate(arc_cats).astype(np.int32)), tt(np.concatenate(init_cats).astype(np.int32))
    arc_off = tt(np.concatenate([[0], np.cumsum([len(a) for a in arc_cats])[:-1]]).astype(np.int64))
    state_off = tt(np.concatenate([[0], np.cumsum([len(a) for a in init_cats])[:-1]]).astype(np.int64))
    amap = _hip.ArcMap(arcs.data_ptr(), inits.data_ptr(), arc_off.data_ptr(), state_off.data_ptr())
    m, f, n = batch.n_elems, batch.n_frames, batch.nutt

    def guarded(size, dt):
        buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=dt, device=dev)
        return buf, buf[GUARD:GUARD + size]
    bufs = {k: guarded(size, dt) for k, size, dt in (
        ('alpha', m, torch.float64), ('y', m, torch.float64), ('norm', f, torch.float64),
        ('starts', f * n_cat, dtype), ('evidence', n, torch.float64))}
    _hip.call('beer_hmm_segpost_trellis', dcode, batch.ref(), _hip.ptr(flat), ctypes.byref(amap),
              n_cat, *[_hip.ptr(bufs[k][1]) for k in ('alpha', 'y', 'norm', 'starts', 'evidence')])
    torch.cuda.synchronize()
    want = hk.segment_posteriors(batch, flat, arc_cats, init_cats, n_cat, 0., 7)
    assert torch.equal(bufs['evidence'][1], want[0])
    assert float((bufs['starts'][1].view(f, n_cat).double() - want[1].double()).abs().max()) <= TOL[dtype]
    # the entries of the library's own call, and two that the last utterance cannot have: a
    # category out of range, and a frame of an utterance before it
    assert n > 1 and case.lens[-1] > 0
    first = next(u for u, T in enumerate(case.lens) if T)
    assert first < n - 1
    entry_frame = torch.cat([want[2], torch.tensor([f - 1, int(batch.bufs['frame_off'][first])],
                                                   dtype=torch.int64, device=dev)])
    entry_cat = torch.cat([want[3], torch.tensor([n_cat, 0], dtype=torch.int32, device=dev)])
    entry_off = torch.searchsorted(want[2], batch.bufs['frame_off'])
    entry_off[-1] += 2
    ne = len(entry_frame)
    bufs['seg'] = guarded(ne * 7, dtype)
    _hip.call('beer_hmm_segment_posteriors', dcode, batch.ref(), _hip.ptr(flat),
              ctypes.byref(smap.struct(torch.device('cuda', torch.cuda.current_device()))), n_cat,
              *[_hip.ptr(bufs[k][1]) for k in ('alpha', 'y', 'norm', 'evidence')],
              _hip.ptr(entry_frame), _hip.ptr(entry_cat), _hip.ptr(entry_off), ne, 7,
              _hip.ptr(bufs['seg'][1]))
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + view.numel():] == SENTINEL).all(), \
            f'a guard element of {k} was written'
    seg = bufs['seg'][1].view(ne, 7)
    assert torch.equal(seg[:-2], want[4]) and (seg[-2:] == 0).all()


def test_no_utterance_no_category_and_the_refusals():
    g, arc_cat, init_cat = sp.loop_graph([3, 3], seed=1, open_end=True)
    case = Case('none', None, [], [], 2, None, {})
    _, _, out = run(case, [g], [(arc_cat, init_cat)], [], torch.float32, .1, 4)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 2), (0,), (0,), (0, 4)]
    assert out[1].dtype == out[4].dtype == torch.float32 and out[2].dtype == torch.int64
    none = (np.full(len(arc_cat), -1, np.int32), np.full(6, -1, np.int32))
    case = Case('none', None, [0], [5], 2, None, {})
    batch, flat, out = run(case, [g], [none], [np.zeros((5, 6))], torch.float64, 0., 5)
    assert np.isfinite(float(out[0][0])) and not out[1].any() and out[4].shape == (0, 5)
    with pytest.raises(ValueError, match='min_post'):
        hk.segment_posteriors(batch, flat, [arc_cat], [init_cat], 2, -1., 5)
    with pytest.raises(ValueError, match='sorted'):
        hk.segment_posteriors(batch, flat, [arc_cat], [init_cat], 2, 0., 5,
                              entries=(torch.tensor([3, 1]), torch.tensor([0, 0])))
    with pytest.raises(_hip.HipInvalid):
        hk.segposts_route(batch, 0)
    with pytest.raises(_hip.HipInvalid):
        hk.segposts_route(batch, 2, 7)                       # more than the graph's states


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
    model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet2' if kind == 'bigram' else 'dirichlet')
    return model.double().to('cuda')


def utterances(lens, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randn(T, D) * 1.5).to('cuda') for T in lens]


def dense_arrays(graph):
    return dict(S=graph.n_states, init=npy(graph.init_log_probs), final=npy(graph.final_log_probs),
                trans=npy(graph.trans_log_probs))


def model_llh(model, X, ids, scale):
    'Per-state log-likelihoods from the per-pdf ones the model itself computes, read back.'
    pc = npy(model._emissions().expected_log_likelihood(model.sufficient_statistics(X)))
    return (pc.dtype.type(scale) * pc)[:, np.asarray([int(i) for i in ids])]


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


MODEL_TOL = 1e-10                                            # (the models are float64)


def hold_segments(got, arrays, llh, hand, n_units, min_post, max_dur, what):
    '''(log_evidence, start, end, unit, post) of `unit_segment_posteriors` against the truth: every
    segment the truth has clearly above min_post is there, none that is clearly below, every
    posterior within tol; the order and the types.  Returns the truth.'''
    evidence, start, end, unit, post = got
    assert evidence.dtype == torch.float64 and evidence.dim() == 0 and post.dtype == torch.float64
    assert start.dtype == end.dtype == unit.dtype == torch.int32 and start.is_cuda
    evidence, start, end, unit, post = float(evidence), npy(start), npy(end), npy(unit), npy(post)
    T = len(llh)
    t = truth_of(arrays, llh, hand[0], hand[1], n_units, max_dur)
    if not np.isfinite(t.evidence):
        assert evidence == t.evidence and len(start) == 0
        return t
    assert abs(evidence - t.evidence) <= et.total_bound(t.c, t.evidence, MODEL_TOL)
    assert (post >= min_post).all() and (post > 0).all()
    assert (end >= start).all() and (end - start < max_dur).all() and (end < T).all()
    key = (start.astype(np.int64) * n_units + unit) * (T + 1) + end
    assert (np.diff(key) > 0).all(), f'{what}: not sorted by (start, unit, end)'
    d = np.abs(post - t.post[start, unit, end - start]).max(initial=0.)
    print(f'{what}: {len(start)} segments within {d / MODEL_TOL:.3f} of tol')
    assert d <= MODEL_TOL
    sure = np.argwhere((t.post >= min_post + MODEL_TOL) & (t.post > MODEL_TOL))
    have = set(zip(start.tolist(), unit.tolist(), (end - start).tolist()))
    assert all((s, c, k) in have for s, c, k in sure.tolist()), f'{what}: a segment is missing'
    assert len(have) <= ((t.post >= min_post - MODEL_TOL) & (t.post > 0)).sum()
    return t


@pytest.mark.parametrize('kind', ['phoneloop', 'bigram'])
def test_unit_segment_posteriors_durations_and_the_batch_functions(kind):
    model = make_model(kind)
    arrays, ids = dense_arrays(model.graph), model.graph.pdf_id_mapping
    n_units = len(model.start_pdf)
    hand = unit_categories_by_hand(arrays, ids, model.start_pdf, model.end_pdf)
    lens = [23, 40, 9, 31, 3]
    utts = utterances(lens, 3)
    hist_sum = np.zeros((n_units, 12))
    for X, (min_post, max_dur) in zip(utts, ((1e-3, None), (.05, 12), (0., None), (.3, 40), (1e-3, None))):
        got = model.unit_segment_posteriors(X, min_post=min_post, max_dur=max_dur, scale=.9)
        llh = model_llh(model, X, ids, .9)
        t = hold_segments(got, arrays, llh, hand, n_units, min_post, max_dur or len(X), kind)
        assert len(got[1]) >= 1 or len(X) < 4     # (3 frames cannot cross a unit: no path at all)
        # the expected duration histogram, cut at 12 frames and whole
        for dur in (12, None):
            hist = model.unit_durations(X, max_dur=dur, scale=.9)
            want = sp.durations(truth_of(arrays, llh, hand[0], hand[1], n_units, dur or len(X)).post)
            assert hist.dtype == torch.float64 and hist.is_cuda and hist.shape == want.shape
            assert np.abs(npy(hist) - want).max() <= MODEL_TOL * len(X)
            if dur is None and np.isfinite(t.evidence):
                counts = npy(model.unit_starts(X, scale=.9)).sum(0)
                assert np.abs(npy(hist).sum(1) - counts).max() <= MODEL_TOL * len(X) * (len(X) + 1)
            elif dur is not None:
                hist_sum += want
    one_by_one = [model.unit_segment_posteriors(X, min_post=.01, scale=.9) for X in utts]
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        evidence, segs = beer.unit_segment_posteriors_batch(model, utts, min_post=.01, scale=.9,
                                                            max_frames=max_frames)
        assert evidence.shape == (len(lens),) and evidence.dtype == torch.float64 and len(segs) == len(lens)
        for u, want in enumerate(one_by_one):
            assert float(evidence[u]) == float(want[0])      # (the trellises have no atomics)
            for a, b in zip(segs[u][:3], want[1:4]):
                assert a.dtype == b.dtype and torch.equal(a, b), u
            # (the threshold reads `starts`, whose bins take atomic adds: the cells are the same
            #  here, and each is its entry's row, which has the same bits)
            assert torch.equal(segs[u][3], want[4])
        hist = beer.unit_durations_batch(model, utts, 12, scale=.9, max_frames=max_frames)
        assert hist.dtype == torch.float64 and hist.shape == (n_units, 12)
        assert np.abs(npy(hist) - hist_sum).max() <= MODEL_TOL * sum(lens)
    again = beer.unit_segment_posteriors_batch(model, (torch.cat(utts), lens), min_post=.01, scale=.9,
                                               max_dur=50)
    assert all(torch.equal(a, b) for u in range(len(lens)) for a, b in zip(again[1][u], segs[u]))


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
    stale = [float(model.unit_segment_posteriors(X, inference_graph=bound[i])[0]) for i, X in enumerate(utts)]
    gen = torch.Generator().manual_seed(1)
    for p in model.transitions.parameters_of_groups():
        conc = p.posterior.params.concentrations
        conc.add_(torch.rand(conc.shape, generator=gen, dtype=torch.float64).to(conc) * 3)
    model._on_transitions_update()
    tmap, log_a = CategoryMap(model), expected_log_probs(model.transitions)
    n_units = len(model.start_pdf)
    singles, total = [], np.zeros((n_units, 30))
    for i, X in enumerate(utts):
        dense = gset[i].to_dense()
        src, dst, cats, last = tmap.arcs(seqs[i], dense)
        trans = np.full((len(last), len(last)), -np.inf)
        trans[src, dst] = log_a[cats]
        arrays = dict(S=len(last), init=dense.init_log_probs.double().numpy(),
                      final=dense.final_log_probs.double().numpy(), trans=trans)
        hand = unit_categories_by_hand(arrays, dense.pdf_id_mapping, model.start_pdf, model.end_pdf)
        llh = model_llh(model, X, dense.pdf_id_mapping, .8)
        got = model.unit_segment_posteriors(X, min_post=.02, inference_graph=bound[i], scale=.8)
        t = hold_segments(got, arrays, llh, hand, n_units, .02, lens[i], f'bound graph {i}')
        assert float(model.unit_segment_posteriors(X, inference_graph=bound[i])[0]) != stale[i]
        # a chain: every path begins with the first unit of the transcription, and the counts of
        # the units are those of the transcription
        first = list(model.start_pdf).index(seqs[i][0])
        assert (npy(got[3])[npy(got[1]) == 0] == first).all()
        counts = npy(model.unit_durations(X, inference_graph=bound[i], scale=.8)).sum(1)
        want = np.bincount([list(model.start_pdf).index(u) for u in seqs[i]], minlength=n_units)
        assert np.abs(counts - want).max() <= MODEL_TOL * lens[i] * (lens[i] + 1)
        total += sp.durations(columns(t.post, 30))
        singles.append(got)
    evidence, segs = beer.unit_segment_posteriors_batch(model, utts, min_post=.02,
                                                        inference_graphs=list(bound), scale=.8,
                                                        max_frames=50)
    for i, want in enumerate(singles):
        assert float(evidence[i]) == float(want[0])
        assert all(torch.equal(a, b) for a, b in zip(segs[i], want[1:])), i
    hist = beer.unit_durations_batch(model, utts, 30, inference_graphs=list(bound), scale=.8, max_frames=50)
    assert np.abs(npy(hist) - total).max() <= MODEL_TOL * sum(lens)


def cli(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_segments(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    cli(['dataset', 'create', str(tmp_path), feats, ds])
    hist_file = str(tmp_path / 'durations.npy')
    out = cli(['hmm', 'segments', '--min-post', '0.01', '--max-dur', '30', '--durations', hist_file,
               mdl, ds, str(tmp_path / 'seg')]).strip().split('\n')
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    n_units = len(model.start_pdf)
    evidence, segs = beer.unit_segment_posteriors_batch(model, utts, min_post=.01, max_dur=30)
    scores = beer.log_evidence_batch(model, utts)
    assert sorted(os.listdir(tmp_path / 'seg')) == [f'{u}.npz' for u in ids]
    tol = TOL[model.graph.init_log_probs.dtype]
    total = 0
    for u, T in zip(range(3), (35, 50, 41)):
        new = np.load(tmp_path / 'seg' / f'{ids[u]}.npz')
        assert sorted(new.files) == ['end', 'log_evidence', 'post', 'start', 'unit', 'units']
        start, end, unit, post = (new[k] for k in ('start', 'end', 'unit', 'post'))
        assert start.dtype == end.dtype == unit.dtype == np.int32 and post.dtype == np.float64
        assert new['log_evidence'].dtype == np.float64 and new['log_evidence'].shape == ()
        assert list(new['units']) == [str(v) for v in model.start_pdf]
        for got, want in zip((start, end, unit, post), segs[u]):
            assert np.array_equal(got, npy(want))
        assert float(new['log_evidence']) == float(evidence[u])
        assert abs(float(evidence[u]) - float(scores[u])) <= 10 * tol * (1. + abs(float(scores[u])))
        assert (post >= .01).all() and (post <= 1. + tol).all()
        assert (end >= start).all() and (end - start < 30).all() and end.max() <= T - 1
        assert unit.max() < n_units
        key = (start.astype(np.int64) * n_units + unit) * (T + 1) + end
        assert (np.diff(key) > 0).all()
        assert out[u].split() == [ids[u], '%.6f' % float(evidence[u]), str(len(start)), str(T)]
        total += len(start)
    assert total > 0
    hist = np.load(hist_file)
    want = npy(beer.unit_durations_batch(model, utts, 30))
    assert hist.dtype == np.float64 and hist.shape == (n_units, 30)
    assert np.abs(hist - want).max() <= tol * sum((35, 50, 41))
    # the expected number of units that last at most 30 frames cannot pass the number of frames
    assert 0 < hist.sum() <= 35 + 50 + 41
