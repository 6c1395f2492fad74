"""beer_hsmm_arc_posteriors (csrc/hsmm.hip) and its Python face `hk.duration_arc_posteriors`
against the truth of tests/hsmm_arcs_truth.py.

Tolerances are those of tests/test_gpu_durations.py: `tol` = 1e-10 (float64) / 1e-5 (float32) on
the rows (helpers.rel_err), its flat 1e-5 on accumulated totals.  The outputs of one launch agree
with one another far more closely: utt_out and total_out are sums of the same fp64 terms in
another order (1e-13 relative), and so is the sum of the rows of a float64 frame_out; float32
rows are those terms rounded once, 2^-24 relative each.

 * One static table: each case names the route `beer_hsmm_arcs_route` must report, and the table
   as a whole reaches every team size, both places of the ring and every combination of the two
   bin bits, with n_cat on either side of every threshold the header documents.
 * Random categories with a share of -1, self-loops given real categories, hub arcs categorised
   one by one.
 * Three graphs in one launch, an utterance of no frames, a dead utterance between live ones,
   -inf edges, the ring wrapping, a per-frame shift of +-3e4 over 4096 frames.
 * total_out accumulates, guards around every output, the shared outputs against
   beer_hsmm_forward_backward (bit for bit where that takes the full CSR too).
 * The unit-start categories on a duration PhoneLoop's own graph, alignment graphs and tables."""

from collections import namedtuple
import ctypes

import numpy as np
import pytest
import torch

import fb_truth as ft
import hsmm_arcs_truth as hat
import hsmm_truth as ht
from helpers import rel_err

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.models.sequence import unit_start_categories          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402
from test_gpu_durations import (FLAT, NP, TOL, _data, _graph_arrays, _ids, _model,    # noqa: E402
                                compiled, guarded, guards_hold, packed, raw_fb, tables)

DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
B, R, LD, F, U = ht.BLOCK, ht.RING_LDS, ht.LOWDEG, hat.FRAME_LDS, hat.UTT_LDS
SAME = 1e-13                        # sums of the same fp64 terms in another order
ROUNDED = 2. ** -23                 # ... of those terms rounded once to float32

Case = namedtuple('Case', 'S nO hub D lens n_cat route min_dur seed')
CASES = []


def add(S, nO, D, n_cat, route, hub=0, lens=None, min_dur=1):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, D, lens or ft.lengths((1, 5, 9)[i % 3], 700 + i), n_cat, route,
                      min_dur, 700 + i))


add(1, 2, 1, 3, B | R | F | U | 0, lens=[1])              # S = 1 and T = 1
add(3, 2, 2, 4, B | R | F | U | 1, lens=[5])
add(3, 3, 9, 4, B | R | F | U | 4, lens=[4, 2, 1])        # D > T
add(8, 3, 1, 5, B | R | F | U | 0)                        # D = 1: the HMM without self-loops
for D_, lg_ in ((1, 0), (2, 1), (3, 2), (5, 3), (9, 4), (17, 5), (33, 6), (64, 6)):
    add(4, 3, D_, 6, B | R | F | U | lg_)                 # every team size
add(130, 3, 3, 6, B | R | F | U | 0)                      # one state above the last team of two
add(300, 3, 5, 9, B | R | F | U | 0, lens=[9, 1, 4])      # states stride beyond 256 threads
add(96, 3, 128, 7, B | F | U | 1, lens=[40, 9])           # 192 KiB of ring: in `ws`
add(8, 3, 3, 1024, B | R | F | U | 2, lens=[5, 9])        # the last n_cat of a frame's LDS bins
add(8, 3, 3, 1025, B | R | U | 2, lens=[5, 9])            # ... and the first beyond
add(8, 3, 3, 4096, B | R | U | 2, lens=[5, 9])            # the last n_cat of the utterance's
add(8, 3, 3, 4097, B | R | 2, lens=[5, 9])                # ... and the first beyond
add(150, 3, 64, 24, B | R | F | U | 0, lens=[9, 3])       # 384 bytes beside the ring: both fit,
add(150, 3, 64, 48, B | R | F | 0, lens=[9, 3])           # the frame's alone,
add(150, 3, 64, 49, B | R | 0, lens=[9, 3])               # neither
add(12, 3, 4, 5, B | R | F | U | 2, hub=8)                # hub sources and destinations overlap
add(120, 3, 33, 40, B | R | F | U | 1, hub=40, lens=[9, 33])     # the phone loop of config 3
add(8, 4, 5, 6, B | R | F | U | 3, lens=[9, 1, 6, 8, 1, 2], min_dur=2)   # dead among live


def case_id(c):
    return f'{c.seed}-S{c.S}-hub{c.hub}-D{c.D}-cat{c.n_cat}-n{len(c.lens)}'


def test_the_cases_reach_every_value_of_the_route():
    routes = {c.route for c in CASES}
    assert {r & 0xF for r in routes} == set(range(7))
    assert {r & (R | F | U) for r in routes} == {R | F | U, F | U, R | U, R | F, R}
    assert not any(r & LD for r in routes)
    assert {1, 3, 4, 130, 300} <= {c.S for c in CASES}
    assert {1, 2, 3, 5, 9, 17, 33, 64, 128} <= {c.D for c in CASES}
    assert {1024, 1025, 4096, 4097, 24, 48, 49} <= {c.n_cat for c in CASES}
    assert any(c.hub for c in CASES) and any(0 < min(c.lens) == 1 and c.S == 1 for c in CASES)


def arc_map(arc_cats, init_cats):
    'The beer_arc_map of per-graph category arrays, and the device tensors it points into.'
    keep = [tt(np.concatenate(arc_cats).astype(np.int32)), tt(np.concatenate(init_cats).astype(np.int32)),
            tt(np.concatenate([[0], np.cumsum([len(a) for a in arc_cats])[:-1]]).astype(np.int64)),
            tt(np.concatenate([[0], np.cumsum([len(a) for a in init_cats])[:-1]]).astype(np.int64))]
    return _hip.ArcMap(*[k.data_ptr() for k in keep]), keep


def raw_arcs(batch, flat, log_dur, leave_w, S_total, arc_cats, init_cats, n_cat, frames=True,
             utts=True, total=True, prefill=None, shared=True):
    '''beer_hsmm_arc_posteriors into the middle of sentinel-filled buffers: dict(gamma, ev, cnt,
    ent, g0, frame, utt, total) after the guards were checked.'''
    D = log_dur.shape[1]
    S = max(batch.n_states)
    code = _hip.dtype_code(batch.dtype)
    extra = _hip.lib().beer_hsmm_arcs_scratch_doubles(code, batch.ref(), D)
    ws = torch.empty(2 * batch.n_elems + 2 * batch.n_frames + extra + 1, dtype=torch.float64,
                     device='cuda')
    gb, gamma = guarded((batch.n_elems,), batch.dtype)
    eb, ev = guarded((batch.nutt,), torch.float64)
    cb, cnt = guarded((S_total * D,), torch.float64)
    nb, ent = guarded((S,), torch.float64)
    zb, g0 = guarded((S,), torch.float64)
    fb, frame = guarded((batch.n_frames * n_cat,), batch.dtype)
    ub, utt = guarded((batch.nutt * n_cat,), torch.float64)
    tb, tot = guarded((n_cat,), torch.float64)
    for v in (cnt, ent, g0, tot):
        v.zero_()
    if prefill is not None:
        tot.copy_(tt(prefill))
    amap, keep = arc_map(arc_cats, init_cats)
    _hip.call('beer_hsmm_arc_posteriors', code, batch.ref(), _hip.ptr(flat), _hip.ptr(log_dur),
              _hip.ptr(leave_w), D, S_total, ctypes.byref(amap), n_cat, _hip.ptr(ws),
              _hip.ptr(gamma), _hip.ptr(ev), _hip.ptr(cnt), _hip.ptr(ent) if shared else None,
              _hip.ptr(g0) if shared else None, _hip.ptr(frame) if frames else None,
              _hip.ptr(utt) if utts else None, _hip.ptr(tot) if total else None)
    torch.cuda.synchronize()
    for buf, what in ((gb, 'gamma'), (eb, 'evidence'), (cb, 'dur_counts'), (nb, 'entry_sum'),
                      (zb, 'gamma0_sum'), (fb, 'frame_out'), (ub, 'utt_out'), (tb, 'total_out')):
        guards_hold(buf, what)
    for given, v, what in ((frames, frame, 'frame_out'), (utts, utt, 'utt_out')):
        assert given or bool((v == -12345.678).all()), f'a NULL {what} was written'
    assert total or not tot.any(), 'a NULL total_out was written'
    return dict(gamma=gamma.clone(), ev=ev.clone(), cnt=cnt.clone().view(S_total, D),
                ent=ent.clone(), g0=g0.clone(), frame=frame.clone().view(batch.n_frames, n_cat),
                utt=utt.clone().view(batch.nutt, n_cat), total=tot.clone())


def hold(truths, lens, out, dtype, what, prefill=None):
    '''frame_out, utt_out and total_out of a batch against the truths of its utterances [(frame,
    utt)], and against one another.'''
    tol = TOL[dtype]
    frame, utt, total = npy(out['frame']).astype(np.float64), npy(out['utt']), npy(out['total'])
    assert not np.isnan(frame).any() and not np.isnan(utt).any() and not np.isnan(total).any()
    want = np.concatenate([t[0] for t in truths]) if sum(lens) else np.zeros_like(frame)
    err = rel_err(frame, want)
    print(f'{what}: rows rel_err {err:.3e} (bound {tol:.0e})')
    assert err <= tol, f'{what}: rows rel_err {err:.3e} > {tol:.1e}'
    want_utt = np.stack([t[1] for t in truths])
    err_u = rel_err(utt, want_utt)
    base = np.zeros_like(total) if prefill is None else np.asarray(prefill)
    err_t = rel_err(total - base, want_utt.sum(0))
    print(f'{what}: utt_out rel_err {err_u:.3e}, total_out {err_t:.3e} (bound {FLAT:.0e})')
    assert err_u <= FLAT and err_t <= FLAT
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, t in enumerate(truths):
        rows = frame[off[u]:off[u + 1]]
        if not t[0].any():
            assert not rows.any() and not utt[u].any(), f'{what} utterance {u}: not zeros'
        same = SAME if dtype == torch.float64 else ROUNDED
        assert rel_err(rows.sum(0), utt[u]) <= same * max(len(rows), 1), f'{what} utterance {u}'
        assert (rows >= 0).all() and (rows.sum(1) <= 1 + 10 * tol).all()
    scale = max(np.abs(utt.sum(0)).max(), np.abs(base).max(), 1e-300)
    assert np.abs(total - base - utt.sum(0)).max() <= SAME * len(lens) * scale, \
        f'{what}: total_out is not the sum of utt_out'


def make_case(case, dtype):
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype])
    flavour = ft.FLAVOURS[case.seed % 3]
    S_total = case.S if flavour == 'perm' else case.S + 3
    ids = ft.pdf_ids(case.S, flavour, S_total, case.seed)
    lens = list(case.lens)
    _, llhs = ft.inputs(g, lens, ids, S_total, 1., case.seed, NP[dtype])
    ld, lw = tables(S_total, case.D, case.seed, case.min_dur)
    batch = hk.HmmBatch([compiled(g, ids)], [0] * len(lens), lens, dtype)
    return g, ids, S_total, lens, llhs, ld, lw, batch


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_arc_posteriors_are_the_truth(case, dtype):
    g, ids, S_total, lens, llhs, ld, lw, batch = make_case(case, dtype)
    size = tt(llhs[0]).element_size()
    route = hk.duration_arcs_route(batch, case.D, case.n_cat, True)
    assert route == case.route, f'route {route:#x}, the table says {case.route:#x}'
    assert route == hat.route_formula(case.S, case.D, size, case.n_cat, 1)
    old = hk.duration_route(batch, case.D)
    if case.hub:
        assert old & LD, 'beer_hsmm_forward_backward walks the hub here: the new call must not'
    arc_cat, init_cat = hat.random_categories(g, case.n_cat, case.seed, drop=.3)
    src, dst = hat.out_arcs(g)
    if case.S > 1:
        assert ((src == dst) & (arc_cat >= 0)).any(), 'a self-loop carries a category'
    if case.hub:
        E, _, B_, _ = g['hub']
        on_hub = np.isin(src, E) & np.isin(dst, B_) & (src != dst)
        assert len(set(arc_cat[on_hub])) > 2, 'hub arcs in different categories'
    flat = packed(llhs)
    before = flat.clone()
    pre = np.random.RandomState(case.seed).uniform(1., 2., size=case.n_cat)
    out = raw_arcs(batch, flat, tt(ld), tt(lw), S_total, [arc_cat], [init_cat], case.n_cat,
                   prefill=pre)
    assert torch.equal(flat, before), 'pc_llhs was written'
    truths = [hat.arc_posteriors(g, ld, lw, l, arc_cat, init_cat, case.n_cat, ids) for l in llhs]
    hold(truths, lens, out, dtype, case_id(case), prefill=pre)
    if case.min_dur > 1:
        dead = [not t[0].any() for t in truths]
        assert dead == [False, True, False, False, True, False]
        assert [float(e) == -np.inf for e in out['ev']] == dead
    # the outputs shared with beer_hsmm_forward_backward: the same bits on the full CSR, within
    # the tolerance where that call walks the low-degree image
    gamma, ev, cnt, ent, g0 = raw_fb(batch, flat, tt(ld), tt(lw), S_total)
    if old & LD:
        assert rel_err(npy(out['gamma']), npy(gamma)) <= 2 * TOL[dtype]
        fin = np.isfinite(npy(ev))
        assert (np.isfinite(npy(out['ev'])) == fin).all()
        assert np.abs(npy(out['ev'])[fin] - npy(ev)[fin]).max(initial=0.) <= \
            2 * TOL[dtype] * (np.abs(npy(ev)[fin]).max(initial=0.) + 1)
        same = 2 * TOL[dtype]
    else:
        assert torch.equal(out['gamma'], gamma) and torch.equal(out['ev'], ev)
        same = SAME
    for name, other in (('cnt', cnt), ('ent', ent), ('g0', g0)):
        assert rel_err(npy(out[name]), npy(other)) <= same, name
    # gamma and the evidence: the same bits on a second run, whatever outputs are asked for
    again = raw_arcs(batch, flat, tt(ld), tt(lw), S_total, [arc_cat], [init_cat], case.n_cat,
                     frames=False, utts=False, shared=False)
    assert torch.equal(again['gamma'], out['gamma']) and torch.equal(again['ev'], out['ev'])
    assert rel_err(npy(again['total']), npy(out['total']) - pre) <= SAME * len(lens)
    only = raw_arcs(batch, flat, tt(ld), tt(lw), S_total, [arc_cat], [init_cat], case.n_cat,
                    frames=False, total=False)
    assert rel_err(npy(only['utt']), npy(out['utt'])) <= SAME
    # the Python face
    res = hk.duration_arc_posteriors(batch, flat, tt(ld), tt(lw), [arc_cat], [init_cat],
                                     case.n_cat, per_frame=True, per_utt=True, total=True)
    assert torch.equal(res[0], out['gamma']) and torch.equal(res[1], out['ev'])
    assert rel_err(npy(res[5]), npy(out['frame'])) <= (SAME if dtype == torch.float64 else ROUNDED)
    assert rel_err(npy(res[6]), npy(out['utt'])) <= SAME
    assert rel_err(npy(res[7]), npy(out['total']) - pre) <= SAME * len(lens)
    res = hk.duration_arc_posteriors(batch, flat, tt(ld), tt(lw), [arc_cat], [init_cat],
                                     case.n_cat, per_frame=False, total=True, want_counts=False)
    assert res[2] is None and res[5] is None and res[6] is None and res[7].shape == (case.n_cat,)


MIXED_LENS, MIXED_GIDS = [33, 9, 0, 32, 2, 40, 1], [0, 1, 2, 2, 0, 2, 1]


@DTYPES
def test_graphs_of_different_sizes_and_an_utterance_of_no_frames(dtype):
    sizes, D, n_cat = (7, 65, 129), 5, 11
    arrays = [ft.make_graph(S, ft.offsets(3, S), 2100 + k, 0, NP[dtype]) for k, S in enumerate(sizes)]
    S_total = 140
    idl = [ft.pdf_ids(S, 'partial', S_total, 2200 + k) for k, S in enumerate(sizes)]
    graphs = [compiled(g, ids) for g, ids in zip(arrays, idl)]
    rng = np.random.RandomState(5)
    llhs = [(rng.randn(T, sizes[k]) * 3).astype(NP[dtype]) for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    ld, lw = tables(S_total, D, 6)
    cats = [hat.random_categories(g, n_cat, 2300 + k, drop=.3) for k, g in enumerate(arrays)]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert hk.duration_arcs_route(batch, D, n_cat) == B | R | F | U | 0
    out = raw_arcs(batch, packed(llhs), tt(ld), tt(lw), S_total, [c[0] for c in cats],
                   [c[1] for c in cats], n_cat, shared=False)
    truths = [hat.arc_posteriors(arrays[k], ld, lw, l, cats[k][0], cats[k][1], n_cat, idl[k])
              for l, k in zip(llhs, MIXED_GIDS)]
    hold(truths, MIXED_LENS, out, dtype, 'three graphs')
    assert float(out['ev'][2]) == 0. and not npy(out['utt'])[2].any()
    # an empty batch does nothing
    empty = hk.HmmBatch(graphs[:1], [], [], dtype)
    res = hk.duration_arc_posteriors(empty, packed(llhs)[:0], tt(ld), tt(lw), cats[0][:1],
                                     [cats[0][1]], n_cat, per_frame=True, per_utt=True, total=True)
    assert res[5].shape == (0, n_cat) and res[6].shape == (0, n_cat) and not res[7].any()


@DTYPES
def test_the_ring_wraps(dtype):
    S, D, T, n_cat = 8, 33, 300, 7
    g = ft.make_graph(S, ft.offsets(3, S), 67, 0, NP[dtype])
    _, llhs = ft.inputs(g, [T, 70], np.arange(S), S, 1., 68, NP[dtype])
    ld, lw = tables(S, D, 69, min_dur=2)
    arc_cat, init_cat = hat.random_categories(g, n_cat, 70, drop=.2)
    batch = hk.HmmBatch([compiled(g)], [0, 0], [T, 70], dtype)
    out = raw_arcs(batch, packed(llhs), tt(ld), tt(lw), S, [arc_cat], [init_cat], n_cat)
    truths = [hat.arc_posteriors(g, ld, lw, l, arc_cat, init_cat, n_cat) for l in llhs]
    hold(truths, [T, 70], out, dtype, 'T=300 D=33')


@DTYPES
def test_a_per_frame_shift_moves_nothing_in_the_rows(dtype):
    '''T = 4096, S = 8, D = 8, k_t in +-3e4 added to every entry of row t (exactly: everything is
    a multiple of 1/64): the rows are those of the unshifted inputs.'''
    S, D, T, n_cat = 8, 8, 4096, 5
    g = ft.make_graph(S, ft.offsets(3, S), 71, 0, NP[dtype])
    rng = np.random.RandomState(72)
    base = (rng.randint(-512, 513, size=(T, S)) / 64.).astype(NP[dtype])
    k = rng.randint(-30000 * 64, 30000 * 64 + 1, size=T) / 64.
    shifted = (base.astype(np.float64) + k[:, None]).astype(NP[dtype])
    assert (shifted.astype(np.float64) - k[:, None] == base.astype(np.float64)).all()
    ld, lw = tables(S, D, 73)
    arc_cat, init_cat = hat.random_categories(g, n_cat, 74, drop=.2)
    batch = hk.HmmBatch([compiled(g)], [0], [T], dtype)
    out = raw_arcs(batch, packed([shifted]), tt(ld), tt(lw), S, [arc_cat], [init_cat], n_cat)
    truth = hat.arc_posteriors(g, ld, lw, base.astype(np.float64), arc_cat, init_cat, n_cat)
    hold([truth], [T], out, dtype, 'shifted')
    plain = raw_arcs(batch, packed([base]), tt(ld), tt(lw), S, [arc_cat], [init_cat], n_cat)
    assert rel_err(npy(out['frame']), npy(plain['frame'])) <= TOL[dtype]


@DTYPES
def test_minus_infinity_edges(dtype):
    'Minimum duration 2 on every state and -inf emission entries: no NaN, the truth.'
    S, D, n_cat = 8, 5, 6
    g = ft.make_graph(S, ft.offsets(4, S), 74, 0, NP[dtype])
    lens = [9, 6, 8, 2]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 75, NP[dtype])
    rng = np.random.RandomState(76)
    for l in llhs:
        if len(l) > 2:
            l[rng.randint(0, len(l), size=6), rng.randint(0, S, size=6)] = -np.inf
    ld, lw = tables(S, D, 77, min_dur=2)
    assert np.isinf(ld[:, 0]).all()
    arc_cat, init_cat = hat.random_categories(g, n_cat, 78, drop=.3)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    out = raw_arcs(batch, packed(llhs), tt(ld), tt(lw), S, [arc_cat], [init_cat], n_cat)
    truths = [hat.arc_posteriors(g, ld, lw, l, arc_cat, init_cat, n_cat) for l in llhs]
    assert all(t[0].any() for t in truths)
    hold(truths, lens, out, dtype, '-inf edges')


def test_the_python_face_checks_and_names_the_limit():
    g = ft.make_graph(8, ft.offsets(3, 8), 80, 0)
    batch = hk.HmmBatch([compiled(g)], [0], [4], torch.float64)
    flat = packed([np.zeros((4, 8))])
    A = len(hat.out_arcs(g)[0])
    ok = (np.zeros(A, np.int32), np.zeros(8, np.int32))
    with pytest.raises(_hip.HipError, match='BEER_HSMM_MAX_DUR'):
        hk.duration_arcs_route(batch, _hip.HSMM_MAX_DUR + 1, 3)
    with pytest.raises(_hip.HipError, match='at least one category'):
        hk.duration_arcs_route(batch, 4, 0)
    with pytest.raises(ValueError, match='outside'):
        hk.duration_arc_posteriors(batch, flat, tt(np.zeros((8, 3))), None, [ok[0] + 3], [ok[1]], 3)
    with pytest.raises(ValueError, match='duration_arc_posteriors: none of per_frame, per_utt'):
        hk.duration_arc_posteriors(batch, flat, tt(np.zeros((8, 3))), None, [ok[0]], [ok[1]], 3,
                                   per_frame=False)
    with pytest.raises(ValueError, match='BEER_HSMM_MAX_DUR'):
        hk.duration_arc_posteriors(batch, flat, tt(np.zeros((8, 200))), None, [ok[0]], [ok[1]], 3)


# --- on a model's own graphs and tables ------------------------------------------------------------

MODELS = pytest.mark.parametrize('kind', ['normalset', 'mixtureset'])


@DTYPES
@MODELS
def test_unit_start_categories_on_a_duration_phone_loop(kind, dtype):
    '''The kernel layer on a duration PhoneLoop's graph, duration tables and emissions, under
    `unit_start_categories`: the rows are the truth, a row sums to the boundary posterior (1 at
    the first frame, never more), and the sum over the frames is the phone count of the model's
    own E-step, `gamma0_sum[starts] + entry_sum[starts]` -- on the model's graph and on an
    alignment graph, where a unit repeated in the transcription is one category.'''
    model, units = _model(kind, dtype)
    tol = TOL[dtype]
    log_dur, leave_w = model._duration_tables()
    ld, lw = npy(log_dur), npy(leave_w)
    lens = [23, 9, 3]
    X = _data(model, lens, 51, dtype)
    off = np.concatenate([[0], np.cumsum(lens)])
    P = len(model.start_pdf)
    starts = [int(model.start_pdf[u]) for u in model.start_pdf]
    seqs = [['s0', 's1', 's0'], ['s2', 's3'], ['s1']]
    aligned = list(beer.graph.compile_alignments(seqs, units))
    stats = model.sufficient_statistics(X)
    pc_all = model._emissions().expected_log_likelihood(stats)
    for u, T in enumerate(lens):
        x, pc = X[off[u]:off[u + 1]], pc_all[off[u]:off[u + 1]]
        for graph in (model.graph, aligned[u]):
            g, ids = _graph_arrays(graph), _ids(graph)
            cats = unit_start_categories(graph, model.start_pdf, model.end_pdf)
            batch = hk.HmmBatch([graph], [0], [T], dtype)
            flat = hk.gather(batch, pc, 1.)
            l = npy(pc)[:, ids]
            want, want_utt = hat.arc_posteriors(g, ld, lw, l, cats[0], cats[1], P, ids)
            res = hk.duration_arc_posteriors(batch, flat, log_dur, leave_w, [cats[0]], [cats[1]],
                                             P, per_frame=True, per_utt=True, total=True)
            frame, utt, total = npy(res[5]), npy(res[6]), npy(res[7])
            assert frame.shape == (T, P) and res[5].dtype == dtype
            assert rel_err(frame, want) <= tol
            assert rel_err(utt[0], want_utt) <= FLAT and rel_err(total, want_utt) <= FLAT
            assert (frame.sum(1) <= 1 + 10 * tol).all() and abs(frame[0].sum() - 1) <= 10 * tol
            p = ht.posteriors(g, ld, lw, l, ids)
            first = np.isin(ids, starts)
            by_unit = np.zeros(P)
            np.add.at(by_unit, [starts.index(i) for i in ids[first]],
                      (p['gamma0_sum'] + p['entry_sum'])[first])
            assert rel_err(utt[0], by_unit) <= FLAT
            if graph is model.graph:
                # ... and the counts the existing E-step keeps for the phone weights
                model.expected_log_likelihood(model.sufficient_statistics(x))
                g0, entry = model.cache['dur_entries']
                assert rel_err(utt[0], npy(g0[starts] + entry[starts])) <= FLAT
                model.clear_cache()
