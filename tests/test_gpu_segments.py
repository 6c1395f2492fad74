"""The unit segment lattices (csrc/hmm_segments.hip) against the float64 truth of
tests/segments_truth.py, on the smallest shapes at which each form of the two kernels can go wrong.

Tolerance, derived as in tests/test_gpu_lattice.py: every output of utterance u is a float64 sum of
at most 2 T_u + 2 terms whose partial sums are bounded by B_u, compared with a truth that sums the
same terms:  |out - truth| <= 4 (T_u + 1) 2^-52 B_u + r |truth|,  r = 0 for float64 outputs and
2^-23 for the float32-stored rows; -inf must match -inf exactly.  On integer inputs every output is
exactly the truth.

 * One table of cases: each names the form `beer_hmm_segments_route` must report (team size, arcs
   in LDS, bins in LDS); together they reach team sizes 4, 8, 64, 128 and 256 with strided lanes,
   S > 256 (where e waits in the scratch), arcs read from global memory, bins in the output rows,
   graphs of different sizes in one launch, alignment chains with a repeated unit, a dead
   utterance.
 * `starts` and `best` bit for bit `hk.max_marginals`'; the row maximum of `seg` the start margin;
   two calls the same bits; a smaller max_dur the same bits in what is left; guards around every
   buffer the two kernels write.
 * Lengths 1, 2, 3, 7, 33, 65 with max_dur 1, 2, T, T + 5; -inf inputs; no frames; no utterance;
   beam 0 against the segmentation of `hk.viterbi`'s path.
 * The model level: `unit_segments`, `unit_segments_batch`, bound alignment graphs,
   `beer hmm lattice --segments`."""

import ctypes
import functools
import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import lattice_truth as lt
import segments_truth as st
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
R = {torch.float64: 0., torch.float32: 2. ** -23}       # rounding of the stored rows
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
K, L, BL = st.BLOCK, st.ARCS_LDS, st.BINS_LDS
INF = float('inf')
GUARD, SENTINEL = 5, -12345.678

# graphs: (builder, arguments) of every distinct graph; gids, lens: the utterances; route: what
# beer_hmm_segments_route must report in both precisions
Case = namedtuple('Case', 'name graphs gids lens n_cat route')
LOOP = dict(open_end=True)
CASES = [
    Case('loop3x3', [('loop', ([3, 3, 3],), LOOP)], [0] * 6, [1, 2, 3, 7, 33, 65], 3, K | L | BL | 2),
    Case('five', [('loop', ([5] * 4,), LOOP)], [0] * 3, [7, 33, 12], 4, K | L | BL | 3),
    Case('forty', [('loop', ([40, 40, 40],), dict(skips=(1, 6), open_end=True))], [0] * 2, [33, 9], 3,
         K | L | BL | 6),
    # (the units end in their last state alone: 9 frames cannot cross one of 70 states by 9s)
    Case('seventy', [('loop', ([70, 70, 3],), dict(skips=(1, 9)))], [0] * 3, [33, 20, 5], 3,
         K | L | BL | 7),
    Case('big', [('loop', ([300, 3],), dict(skips=(1, 7, 50), open_end=True))], [0] * 3, [33, 9, 2], 2,
         K | L | BL | 8),
    Case('arcs', [('loop', ([3] * 72,), LOOP)], [0] * 2, [9, 4], 72, K | BL | 2),
    Case('bins', [('loop', ([3, 3, 3],), dict(open_end=True, labels=[0, 1000, 2048]))], [0] * 2,
         [7, 33], 2049, K | L | 2),
    Case('chain', [('chain', ([1, 0, 1, 2, 1], 2), {})], [0] * 3, [12, 25, 10], 3, K | L | BL | 3),
    # (7 frames cannot cross the chain's 15 states: a dead utterance between live ones)
    Case('mixed', [('loop', ([3, 3, 3],), LOOP), ('chain', ([1, 0, 1, 2, 1], 3), {}),
                   ('loop', ([5] * 3,), LOOP)], [0, 1, 2, 1, 0, 2, 1], [33, 40, 12, 20, 2, 7, 7], 3,
         K | L | BL | 4),
]
IDS = [c.name for c in CASES]


def test_the_cases_reach_every_form():
    assert {_hip.segments_team(c.route) for c in CASES} >= {4, 8, 16, 64, 128, 256}
    assert {c.route & 0xF00 for c in CASES} >= {L | BL, BL, L}
    assert {1, 2, 3, 7, 33, 65} <= {T for c in CASES for T in c.lens}


def packed(llhs, dtype):
    if not llhs:
        return torch.zeros(0, dtype=dtype, device='cuda')
    return torch.cat([tt(np.asarray(l, dtype=NP[dtype])).reshape(-1) for l in llhs])


def compiled(g):
    return beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                    [int(i) for i in range(g['S'])])


@functools.lru_cache(maxsize=None)
def case_data(name, np_dtype, integer):
    '''(arrays, cats, llhs, truths) of a case, computed once and never changed; truths per
    utterance: (best, frame [T, n_cat], seg [T, n_cat, T + 5], B_u).'''
    case = CASES[IDS.index(name)]
    built = [(st.loop_graph if kind == 'loop' else st.chain_graph)(*args, seed=3 + k, real=not integer,
                                                                  **kw)
             for k, (kind, args, kw) in enumerate(case.graphs)]
    arrays, cats = [b[0] for b in built], [b[1:] for b in built]
    rng = np.random.RandomState(len(name) + 17 * integer)
    llhs = []
    for u, (T, gid) in enumerate(zip(case.lens, case.gids)):
        S = arrays[gid]['S']
        llh = rng.randint(-4, 1, size=(T, S)).astype(np_dtype) if integer else \
            (rng.randn(T, S) * 3).astype(np_dtype)
        if u % 3 == 1 and T > 3:
            llh[rng.rand(T, S) < .1] = -np.inf               # (an utterance with holes)
        llhs.append(llh)
    truths = []
    for llh, gid in zip(llhs, case.gids):
        g, (arc_cat, init_cat) = arrays[gid], cats[gid]
        best, _, frame, _ = lt.max_marginals(g, llh, arc_cat, init_cat, case.n_cat)
        seg = st.segments(g, llh, arc_cat, init_cat, case.n_cat, len(llh) + 5)
        truths.append((best, frame, seg, lt.bound(g, llh)))
    return arrays, cats, llhs, truths


def run(case, arrays, cats, llhs, dtype, beam, max_dur, lens=None, gids=None):
    lens, gids = case.lens if lens is None else lens, case.gids if gids is None else gids
    batch = hk.HmmBatch([compiled(g) for g in arrays], gids, lens, dtype)
    flat = packed(llhs, dtype)
    out = hk.segment_margins(batch, flat, [c[0] for c in cats], [c[1] for c in cats], case.n_cat,
                             beam, max_dur)
    return batch, flat, out


def within(values, beam):
    return (values >= -beam) & np.isfinite(values)


def share(got, want, B, T, r, what, exact):
    'As test_gpu_lattice.share: the largest share of the bound used; `exact`: equality.'
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f'{what}: shape {got.shape}, not {want.shape}'
    assert not np.isnan(got).any(), f'{what}: NaN'
    if exact:
        assert np.array_equal(got, want), f'{what} is not exactly the truth'
        return 0.
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), f'{what}: -inf in other places than the truth'
    assert (got[~fin] == -np.inf).all(), f'{what}: +inf'
    tol = np.broadcast_to(lt.tolerance(B, T, want, r), want.shape)
    d = np.abs(got[fin] - want[fin])
    worst = float((d / tol[fin]).max(initial=0.))
    assert worst <= 1., f'{what}: off by {d.max():.3e}, {worst:.3f} of the bound'
    return worst


def hold(out, truths, lens, n_cat, beam, max_dur, dtype, what, exact=False):
    '''Every output of every utterance against the truth; the entries are the cells of the
    returned `starts` within the beam, row-major.  Returns the largest share of the bound.'''
    best, starts, entry_frame, entry_cat, seg = out
    assert best.dtype == torch.float64 and best.shape == (len(lens),)
    assert starts.dtype == dtype and starts.shape == (sum(lens), n_cat)
    assert entry_frame.dtype == torch.int64 and entry_cat.dtype == torch.int32
    assert seg.dtype == dtype and seg.shape == (len(entry_frame), max_dur)
    best, starts, entry_frame, entry_cat, seg = (npy(o) for o in out)
    at = np.argwhere(within(starts.astype(np.float64), beam))
    assert np.array_equal(entry_frame, at[:, 0]) and np.array_equal(entry_cat, at[:, 1]), \
        f'{what}: the entries are not the cells of starts within the beam'
    worst, f0 = 0., 0
    for u, (tb, tframe, tseg, B) in enumerate(truths):
        T = lens[u]
        tag = f'{what} utterance {u}'
        worst = max(worst, share(best[u], tb, B, T, 0., tag + ': best', exact))
        worst = max(worst, share(starts[f0:f0 + T], tframe, B, T, R[dtype], tag + ': starts', exact))
        mine = (entry_frame >= f0) & (entry_frame < f0 + T)
        if exact:
            assert mine.sum() == within(tframe, beam).sum()
        cut = tseg[:, :, :max_dur] if max_dur <= tseg.shape[2] else \
            np.concatenate([tseg, np.full(tseg.shape[:2] + (max_dur - tseg.shape[2],), -np.inf)], 2)
        want = cut[entry_frame[mine] - f0, entry_cat[mine]]
        worst = max(worst, share(seg[mine], want, B, T, R[dtype], tag + ': seg', exact))
        if not np.isfinite(tb):
            assert best[u] == -np.inf and not mine.any(), f'{tag}: dead, yet it has entries'
        f0 += T
    if not exact:
        print(f'{what}: within {worst:.3f} of the bound')
    return worst


def same_bits(a, b, what):
    for name, x, y in zip(('best', 'starts', 'entry_frame', 'entry_cat', 'seg'), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and \
            torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), \
            f'{what}: {name} differs in its bits'


@DTYPES
@pytest.mark.parametrize('name', IDS)
def test_segment_margins_are_the_truth(name, dtype):
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name, NP[dtype], False)
    T = max(case.lens)
    batch, flat, out = run(case, arrays, cats, llhs, dtype, INF, T)
    smap = hk.segment_map(batch.source_graphs, [c[0] for c in cats], [c[1] for c in cats], case.n_cat)
    route = hk.segments_route(batch, case.n_cat, smap.max_closure)
    assert route == case.route, f'route {route:#x}, the table says {case.route:#x}'
    assert route == st.route_formula(batch.struct.max_states, batch.struct.max_arcs,
                                     flat.element_size(), case.n_cat, smap.max_closure)
    before = flat.clone()
    hold(out, truths, case.lens, case.n_cat, INF, T, dtype, name)
    assert torch.equal(flat, before), 'pc_llhs was written'
    # the project's own kernel: the same best and the same start margins, bit for bit
    mm = hk.max_marginals(batch, flat, [c[0] for c in cats], [c[1] for c in cats], case.n_cat,
                          states=False, per_frame=True)
    assert torch.equal(out[0].view(torch.int64), mm[0].view(torch.int64)), 'best differs'
    assert torch.equal(out[1].view(torch.uint8), mm[2].view(torch.uint8)), 'starts differ'
    # folding by maximum has no order: the same bits again, also with a map built beforehand
    same_bits(out, hk.segment_margins(batch, flat, [c[0] for c in cats], [c[1] for c in cats],
                                      case.n_cat, INF, T, seg_map=smap), 'a second call')
    # a beam: fewer entries, the same rows; a smaller max_dur: the same cells
    small = hk.segment_margins(batch, flat, [c[0] for c in cats], [c[1] for c in cats], case.n_cat,
                               2.5, 3)
    hold(small, truths, case.lens, case.n_cat, 2.5, 3, dtype, name + ' beam 2.5')
    keep = within(npy(out[1]).astype(np.float64), 2.5)[npy(out[2]), npy(out[3])]
    assert torch.equal(small[4], out[4][torch.from_numpy(keep).cuda()][:, :3])


@DTYPES
@pytest.mark.parametrize('name', IDS)
def test_integer_inputs_are_exact(name, dtype):
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name, np.float64, True)
    T = max(case.lens)
    batch, flat, out = run(case, arrays, cats, llhs, dtype, INF, T + 5)
    hold(out, truths, case.lens, case.n_cat, INF, T + 5, dtype, name, exact=True)
    best, starts, entry_frame, entry_cat, seg = (npy(o) for o in out)
    assert (seg <= 0).all() and (starts <= 0).all()
    # the best segment of an entry is the entry's start margin
    assert np.array_equal(seg.max(1), starts[entry_frame, entry_cat])
    assert all(np.isfinite(b) == np.isfinite(t[0]) for b, t in zip(best, truths))


@DTYPES
@pytest.mark.parametrize('max_dur', [1, 2, 65, 70])
def test_every_length_with_every_max_dur(max_dur, dtype):
    case = CASES[0]
    assert case.lens == [1, 2, 3, 7, 33, 65]
    for integer in (True, False):
        arrays, cats, llhs, truths = case_data(case.name, np.float64 if integer else NP[dtype], integer)
        for beam in (INF, 4.):
            _, _, out = run(case, arrays, cats, llhs, dtype, beam, max_dur)
            hold(out, truths, case.lens, 3, beam, max_dur, dtype, f'max_dur {max_dur}', exact=integer)


def unique_best(seed):
    'A loop of 3 units x 3 states and integer inputs on which one path alone is the best.'
    g, arc_cat, init_cat = st.loop_graph([3, 3, 3], seed=seed, open_end=True)
    rng = np.random.RandomState(seed)
    llhs = [rng.randint(-4, 1, size=(T, 9)).astype(np.float64) for T in (33, 7, 1)]
    for llh in llhs:
        best, mm, _, _ = lt.max_marginals(g, llh)
        if not np.isfinite(best) or ((mm == 0).sum(1) != 1).any():
            return None
    return g, arc_cat, init_cat, llhs


@DTYPES
def test_beam_zero_keeps_the_viterbi_segmentation_alone(dtype):
    found = next(filter(None, map(unique_best, range(400))))
    g, arc_cat, init_cat, llhs = found
    lens = [len(l) for l in llhs]
    batch = hk.HmmBatch([compiled(g)], [0] * 3, lens, dtype)
    flat = packed(llhs, dtype)
    best, starts, entry_frame, entry_cat, seg = hk.segment_margins(batch, flat, [arc_cat], [init_cat],
                                                                   3, 0., max(lens))
    start, end, unit, margin = (npy(v) for v in hk.segments_within(entry_frame, entry_cat, seg, 0.))
    assert not margin.any() and margin.dtype == np.float64 and unit.dtype == np.int32
    path = npy(hk.viterbi(batch, flat))
    labels, f0 = st._labels(g, arc_cat), 0
    for T in lens:
        want = sorted((s + f0, c, e + f0) for c, s, e in st.viterbi_segments(path[f0:f0 + T], labels,
                                                                             init_cat))
        mine = (start >= f0) & (start < f0 + T)
        assert list(zip(start[mine].tolist(), unit[mine].tolist(), end[mine].tolist())) == want
        # the segments tile the utterance
        assert want[0][0] == f0 and want[-1][2] == f0 + T - 1
        assert all(a[2] + 1 == b[0] for a, b in zip(want, want[1:]))
        f0 += T


# --- edges -----------------------------------------------------------------------------------------

@DTYPES
def test_dead_utterances_no_frames_and_no_utterance(dtype):
    g, arc_cat, init_cat = st.loop_graph([3, 3, 3], seed=5, open_end=True, real=True)
    case = Case('edges', None, [0] * 5, [6, 0, 9, 4, 5], 3, None)
    rng = np.random.RandomState(6)
    llhs = [(rng.randn(T, 9) * 3).astype(NP[dtype]) for T in case.lens]
    llhs[0][:, 1] = -np.inf                                  # a state that is never there
    llhs[2][4] = -np.inf                                     # a frame without a state: dead
    llhs[3][1, ::2] = -np.inf
    truths = []
    for llh in llhs:
        if len(llh):
            best, _, frame, _ = lt.max_marginals(g, llh, arc_cat, init_cat, 3)
            truths.append((best, frame, st.segments(g, llh, arc_cat, init_cat, 3, 9),
                           lt.bound(g, llh)))
        else:
            truths.append((-np.inf, np.zeros((0, 3)), np.zeros((0, 3, 9)), 1.))
    _, _, out = run(case, [g], [(arc_cat, init_cat)], llhs, dtype, INF, 9)
    hold(out, truths, case.lens, 3, INF, 9, dtype, 'edges')
    assert float(out[0][1]) == -np.inf and float(out[0][2]) == -np.inf
    assert (out[1][6:15] == -np.inf).all()
    # no state may end: everything -inf, no entry, no NaN
    dead = dict(g, final=np.full(9, -np.inf))
    _, _, out = run(case, [dead], [(arc_cat, init_cat)], llhs, dtype, INF, 9)
    assert (out[0] == -np.inf).all() and (out[1] == -np.inf).all()
    assert len(out[2]) == 0 and len(out[3]) == 0 and out[4].shape == (0, 9)
    # no utterance
    _, _, out = run(case, [g], [(arc_cat, init_cat)], [], dtype, 10., 4, lens=[], gids=[])
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0,), (0, 4)]
    assert out[1].dtype == dtype and out[4].dtype == dtype and out[2].dtype == torch.int64


def test_no_category_anywhere_and_the_refusals():
    g, arc_cat, init_cat = st.loop_graph([3, 3], seed=1, open_end=True)
    none = (np.full(len(arc_cat), -1, np.int32), np.full(6, -1, np.int32))
    case = Case('none', None, [0], [5], 2, None)
    llhs = [np.zeros((5, 6))]
    batch, flat, out = run(case, [g], [none], llhs, torch.float64, INF, 5)
    assert np.isfinite(float(out[0][0])) and (out[1] == -np.inf).all() and out[4].shape == (0, 5)
    for kw in (dict(beam=-1., max_dur=5), dict(beam=float('nan'), max_dur=5), dict(beam=1., max_dur=0)):
        with pytest.raises(ValueError):
            hk.segment_margins(batch, flat, [arc_cat], [init_cat], 2, **kw)
    with pytest.raises(ValueError):
        hk.segment_margins(batch, flat, [arc_cat + 2], [init_cat], 2, 1., 5)
    with pytest.raises(ValueError, match='segment map'):
        hk.segment_margins(batch, flat, [arc_cat], [init_cat], 2, 1., 5,
                           seg_map=hk.segment_map(batch.source_graphs, [arc_cat], [init_cat], 3))
    with pytest.raises(_hip.HipInvalid):
        hk.segments_route(batch, 0)
    with pytest.raises(_hip.HipInvalid):
        hk.segments_route(batch, 2, 7)                       # more than the graph's states


@DTYPES
@pytest.mark.parametrize('name', ['loop3x3', 'big', 'bins', 'mixed'])
def test_nothing_is_written_beside_the_outputs(name, dtype):
    'The two entry points on sentinel-guarded buffers; entries out of range get -inf rows.'
    case = CASES[IDS.index(name)]
    arrays, cats, llhs, truths = case_data(name, np.float64, True)
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
    n_ws = _hip.lib().beer_hmm_segments_scratch_doubles(dcode, batch.ref())
    assert n_ws == (n * batch.struct.max_states if batch.struct.max_states > 256 else 0)

    def guarded(size, dt):
        buf = torch.full((size + 2 * GUARD,), SENTINEL, dtype=dt, device=dev)
        return buf, buf[GUARD:GUARD + size]
    bufs = {k: guarded(size, dt) for k, size, dt in (
        ('d', m, torch.float64), ('x', m, torch.float64), ('ws', n_ws, torch.float64),
        ('starts', f * n_cat, dtype), ('best', n, torch.float64))}
    _hip.call('beer_hmm_segment_trellis', dcode, batch.ref(), _hip.ptr(flat), ctypes.byref(amap),
              n_cat, *[_hip.ptr(bufs[k][1]) for k in ('d', 'x', 'ws', 'starts', 'best')])
    torch.cuda.synchronize()
    want = hk.segment_margins(batch, flat, arc_cats, init_cats, n_cat, INF, 7)
    starts = bufs['starts'][1].view(f, n_cat)
    assert torch.equal(starts, want[1]) and torch.equal(bufs['best'][1], want[0])
    # the entries of the library's own call, and two that the last utterance cannot have: a
    # category out of range, and a frame of the first utterance
    assert n > 1 and case.lens[-1] > 0
    entry_frame = torch.cat([want[2], torch.tensor([f - 1, 0], dtype=torch.int64, device=dev)])
    entry_cat = torch.cat([want[3], torch.tensor([n_cat, 0], dtype=torch.int32, device=dev)])
    entry_off = torch.searchsorted(want[2], batch.bufs['frame_off'])
    entry_off[-1] += 2
    ne = len(entry_frame)
    bufs['seg'] = guarded(ne * 7, dtype)
    _hip.call('beer_hmm_segment_margins', dcode, batch.ref(), _hip.ptr(flat),
              ctypes.byref(smap.struct(torch.device('cuda', torch.cuda.current_device()))), n_cat,
              _hip.ptr(bufs['d'][1]), _hip.ptr(bufs['x'][1]), _hip.ptr(bufs['best'][1]),
              _hip.ptr(entry_frame), _hip.ptr(entry_cat), _hip.ptr(entry_off), ne, 7,
              _hip.ptr(bufs['seg'][1]))
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + view.numel():] == SENTINEL).all(), \
            f'a guard element of {k} was written'
    seg = bufs['seg'][1].view(ne, 7)
    assert torch.equal(seg[:-2], want[4]) and (seg[-2:] == -np.inf).all()


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
    src, dst = lt.out_arcs(arrays)
    arc_cat = np.asarray([firsts.index(ids[j]) if i != j and ids[j] in firsts else -1
                          for i, j in zip(src, dst)], dtype=np.int32)
    init_cat = -np.ones(len(ids), dtype=np.int32)
    for k, u in enumerate(start_pdf):
        for j, p in enumerate(ids):
            if int(start_pdf[u]) <= p <= int(end_pdf[u]):
                init_cat[j] = k
    return arc_cat, init_cat


def hold_segments(got, arrays, llh, hand, n_units, beam, max_dur, what):
    '''(best, start, end, unit, margin) of `unit_segments` against the truth: every segment the
    truth has clearly within the beam is there, none that is clearly outside, every margin within
    the bound; the order and the types.'''
    best, start, end, unit, margin = got
    assert best.dtype == torch.float64 and margin.dtype == torch.float64
    assert start.dtype == end.dtype == unit.dtype == torch.int32 and start.is_cuda
    best, start, end, unit, margin = float(best), npy(start), npy(end), npy(unit), npy(margin)
    T = len(llh)
    truth = st.segments(arrays, llh, hand[0], hand[1], n_units, max_dur)
    tb = lt.max_marginals(arrays, llh)[0]
    tol = float(lt.tolerance(lt.bound(arrays, llh), T, 0.))
    assert abs(best - tb) <= tol
    assert (margin >= -beam).all() and (end >= start).all() and (end - start < max_dur).all()
    key = (start.astype(np.int64) * n_units + unit) * (T + 1) + end
    assert (np.diff(key) > 0).all(), f'{what}: not sorted by (start, unit, end)'
    want = truth[start, unit, end - start]
    assert np.isfinite(want).all() and np.abs(margin - want).max(initial=0.) <= tol
    sure = np.argwhere((truth >= -beam + tol) & np.isfinite(truth))
    have = set(zip(start.tolist(), unit.tolist(), (end - start).tolist()))
    assert all((s, c, k) in have for s, c, k in sure.tolist()), f'{what}: a segment is missing'
    assert len(have) <= ((truth >= -beam - tol) & np.isfinite(truth)).sum()
    return len(have)


@pytest.mark.parametrize('kind', ['phoneloop', 'bigram'])
def test_unit_segments_and_the_batch_function(kind):
    model = make_model(kind)
    arrays, ids = dense_arrays(model.graph), model.graph.pdf_id_mapping
    n_units = len(model.start_pdf)
    hand = unit_categories_by_hand(arrays, ids, model.start_pdf, model.end_pdf)
    lens = [23, 40, 9, 31, 3]
    utts = utterances(lens, 3)
    for X, (beam, max_dur) in zip(utts, ((6., None), (3., 12), (INF, None), (0.5, 40), (6., None))):
        got = model.unit_segments(X, beam=beam, max_dur=max_dur, scale=.9)
        n = hold_segments(got, arrays, model_llh(model, X, ids, .9), hand, n_units, beam,
                          max_dur or len(X), kind)
        assert n >= 1 or len(X) < 4              # (3 frames cannot cross a unit: no path at all)
    one_by_one = [model.unit_segments(X, beam=4., scale=.9) for X in utts]
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        best, segs = beer.unit_segments_batch(model, utts, beam=4., scale=.9, max_frames=max_frames)
        assert best.shape == (len(lens),) and best.dtype == torch.float64 and len(segs) == len(lens)
        for u, want in enumerate(one_by_one):
            # (the same kernels on the same inputs: the same bits)
            assert float(best[u]) == float(want[0]) or (np.isinf(float(best[u])) and np.isinf(float(want[0])))
            assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(segs[u], want[1:])), u
    again = beer.unit_segments_batch(model, (torch.cat(utts), lens), beam=4., scale=.9, max_dur=50)
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
    stale = [float(model.unit_segments(X, inference_graph=bound[i])[0]) for i, X in enumerate(utts)]
    gen = torch.Generator().manual_seed(1)
    for p in model.transitions.parameters_of_groups():
        conc = p.posterior.params.concentrations
        conc.add_(torch.rand(conc.shape, generator=gen, dtype=torch.float64).to(conc) * 3)
    model._on_transitions_update()
    tmap, log_a = CategoryMap(model), expected_log_probs(model.transitions)
    n_units = len(model.start_pdf)
    singles = []
    for i, X in enumerate(utts):
        dense = gset[i].to_dense()
        src, dst, cats, last = tmap.arcs(seqs[i], dense)
        trans = np.full((len(last), len(last)), -np.inf)
        trans[src, dst] = log_a[cats]
        arrays = dict(S=len(last), init=dense.init_log_probs.double().numpy(),
                      final=dense.final_log_probs.double().numpy(), trans=trans)
        hand = unit_categories_by_hand(arrays, dense.pdf_id_mapping, model.start_pdf, model.end_pdf)
        llh = model_llh(model, X, dense.pdf_id_mapping, .8)
        got = model.unit_segments(X, beam=5., inference_graph=bound[i], scale=.8)
        hold_segments(got, arrays, llh, hand, n_units, 5., lens[i], f'bound graph {i}')
        assert float(model.unit_segments(X, inference_graph=bound[i])[0]) != stale[i]
        # a chain: every path begins with the first unit of the transcription
        first = list(model.start_pdf).index(seqs[i][0])
        assert (npy(got[3])[npy(got[1]) == 0] == first).all()
        singles.append(got)
    best, segs = beer.unit_segments_batch(model, utts, beam=5., inference_graphs=list(bound),
                                          scale=.8, max_frames=50)
    for i, want in enumerate(singles):
        assert float(best[i]) == float(want[0])
        assert all(torch.equal(a, b) for a, b in zip(segs[i], want[1:])), i


def cli(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_lattice_segments(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    cli(['dataset', 'create', str(tmp_path), feats, ds])
    plain = cli(['hmm', 'lattice', '--beam', '4', mdl, ds, str(tmp_path / 'plain')]).strip().split('\n')
    out = cli(['hmm', 'lattice', '--beam', '4', '--segments', '--max-dur', '30', mdl, ds,
               str(tmp_path / 'seg')]).strip().split('\n')
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    n_units = len(model.start_pdf)
    best, segs = beer.unit_segments_batch(model, utts, beam=4., max_dur=30)
    assert sorted(os.listdir(tmp_path / 'seg')) == [f'{u}.npz' for u in ids]
    total = 0
    for u, T in zip(range(3), (35, 50, 41)):
        old, new = np.load(tmp_path / 'plain' / f'{ids[u]}.npz'), np.load(tmp_path / 'seg' / f'{ids[u]}.npz')
        assert sorted(old.files) == ['frame', 'margin', 'score', 'unit', 'units']
        assert sorted(new.files) == sorted(old.files + ['seg_start', 'seg_end', 'seg_unit', 'seg_margin'])
        for k in old.files:                                 # without the flag: as it was
            assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
        start, end, unit, margin = (new[k] for k in ('seg_start', 'seg_end', 'seg_unit', 'seg_margin'))
        assert start.dtype == end.dtype == unit.dtype == np.int32 and margin.dtype == np.float64
        for got, want in zip((start, end, unit, margin), segs[u]):
            assert np.array_equal(got, npy(want))
        assert (margin >= -4.).all() and (end >= start).all() and (end - start < 30).all()
        assert end.max() <= T - 1 and unit.max() < n_units
        key = (start.astype(np.int64) * n_units + unit) * (T + 1) + end
        assert (np.diff(key) > 0).all()
        # every segment begins at an entry of the start lattice
        entries = set(zip(new['frame'].tolist(), new['unit'].tolist()))
        assert set(zip(start.tolist(), unit.tolist())) <= entries
        assert plain[u].split() == [ids[u], '%.6f' % float(best[u]), str(len(old['frame'])), str(T)]
        assert out[u].split() == plain[u].split() + [str(len(start))]
        total += len(start)
    assert total > 0
