"""The explicit-duration (hidden semi-Markov) kernels of csrc/hsmm.hip against the float64 truth of
tests/hsmm_truth.py, on graphs that sit on the boundaries of their forms.

Tolerances, `tol` = 1e-10 (float64) / 1e-5 (float32), the project's:
 * helpers.rel_err(...) <= tol for gamma, dur_counts, entry_sum and gamma0_sum;
 * evidence and Viterbi scores within evidence_truth.total_bound, sized with the per-frame
   magnitudes sum_j gamma_t(j) l_t(j) of the truth.

 * One static table: each case names the route `beer_hsmm_route` must report, and the table as a
   whole reaches every team size and both values of either flag.
 * D = 1 with lam = 0 (the HMM without self-loops), the geometric equivalence against the truth
   and against `hk.forward_backward` on the GPU.
 * The ring wraps (T = 300, D = 33); T = 4096 with a per-frame shift of +-3e4.
 * -inf edges: minimum durations, -inf emissions, an infeasible utterance among feasible ones.
 * Guards around every output, `pc_llhs` unchanged, NULL outputs, the same bits on two runs.
 * Viterbi: the score, the returned path's own score, and the exact path on integer inputs.
 * The model level: a PhoneLoop over NormalSet and over MixtureSet emissions -- the E-step's
   statistics, phone counts and duration counts against the truth on the model's own tables, one
   update, batch = sum of utterances, decode / log_evidence and their batched forms, alignment
   graphs, durations learned from data whose states last 3 or 4 frames -- and the command line."""

from collections import namedtuple

import numpy as np
import pytest
import torch

import evidence_truth as et
import fb_truth as ft
import hsmm_truth as ht
from helpers import rel_err

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
B, R, LD = ht.BLOCK, ht.RING_LDS, ht.LOWDEG
GUARD, SENTINEL = 5, -12345.678
DMAX = _hip.HSMM_MAX_DUR

# S, offsets of the circulant graph, hub members, D, utterances, pdf-id flavour, the route
Case = namedtuple('Case', 'S nO hub D nutt flavour route seed')
CASES = []


def add(S, nO, D, route, hub=0, nutt=None):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, D, nutt or (1, 5, 9)[i % 3], ft.FLAVOURS[i % 3], route, 900 + i))


add(1, 2, 1, B | R | LD | 0)
add(1, 2, 3, B | R | LD | 2, nutt=9)           # S = 1, D = 3: T >= 4 has no segmentation
add(1, 2, DMAX, B | R | LD | 6)
add(3, 2, 2, B | R | LD | 1)
add(3, 3, 33, B | R | LD | 6)
add(8, 3, 3, B | R | LD | 2)
add(8, 2, 8, B | R | LD | 3, nutt=9)
add(8, 8, 33, B | R | LD | 5)                  # every arc present
add(16, 3, 16, B | R | LD | 4)
add(12, 12, 8, B | R | 3)                      # 12 arcs a state: no low-degree image
add(64, 3, 8, B | R | LD | 2)
add(64, 3, DMAX, B | R | LD | 2, hub=8)        # 64 (8 + 256) doubles = 132 KiB of LDS
add(65, 3, 3, B | R | LD | 1)
add(65, 12, 2, B | R | 1)
add(120, 3, 33, B | R | LD | 1, hub=40)        # the phone loop of config 3
add(120, 3, DMAX, B | LD | 1, hub=40, nutt=5)  # its ring no longer fits LDS
add(257, 3, 2, B | R | LD | 0)
add(257, 3, DMAX, B | LD | 0, nutt=5)
add(1024, 2, 1, B | R | LD | 0, nutt=1)
add(1024, 2, DMAX, B | LD | 0, nutt=1)
add(300, 12, 33, B | 0, nutt=5)
add(12, 3, 4, B | R | LD | 2, hub=8)           # hub sources 0..7 and destinations 4..11 overlap


def case_id(c):
    return f'{c.seed}-S{c.S}-O{c.nO}-hub{c.hub}-D{c.D}-n{c.nutt}-{c.flavour}'


def test_the_cases_reach_every_value_of_the_route():
    routes = {c.route for c in CASES}
    assert {r & 0xF for r in routes} == set(range(7))
    assert {r & (R | LD) for r in routes} == {0, R, LD, R | LD}
    assert {1, 3, 8, 64, 65, 120, 257, 1024} <= {c.S for c in CASES}
    assert {1, 2, 3, 8, 33, DMAX} <= {c.D for c in CASES}
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


def tables(S_total, D, seed, min_dur=1):
    '(log_dur [S_total, D], leave_w [S_total]) float64: rows on a grid of 1/64, some entries -inf.'
    rng = np.random.RandomState(seed + 41)
    ld = np.round(rng.uniform(-3., 0., size=(S_total, D)) * 64) / 64
    ld[:, :min(min_dur - 1, D - 1)] = -np.inf
    if D > 2:
        ld[rng.randint(0, S_total, size=max(S_total // 4, 1)), rng.randint(1, D)] = -np.inf
    return ld, np.round(rng.uniform(0., 1., size=S_total) * 64) / 64


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n]


def guards_hold(buf, what):
    assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), \
        f'a guard element of {what} was written'


def raw_fb(batch, flat, log_dur, leave_w, S_total, counts=True, shared=True):
    '''beer_hsmm_forward_backward into the middle of sentinel-filled buffers: (gamma, evidence,
    dur_counts, entry_sum, gamma0_sum) after the guards were checked.'''
    D = log_dur.shape[1]
    S = max(batch.n_states)
    extra = _hip.lib().beer_hsmm_scratch_doubles(_hip.dtype_code(batch.dtype), batch.ref(), D)
    ws = torch.empty(2 * batch.n_elems + 2 * batch.n_frames + extra + 1, dtype=torch.float64,
                     device='cuda')
    gb, gamma = guarded((batch.n_elems,), batch.dtype)
    eb, ev = guarded((batch.nutt,), torch.float64)
    cb, cnt = guarded((S_total * D,), torch.float64)
    nb, ent = guarded((S,), torch.float64)
    zb, g0 = guarded((S,), torch.float64)
    for v in (cnt, ent, g0):
        v.zero_()
    _hip.call('beer_hsmm_forward_backward', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(flat), _hip.ptr(log_dur), _hip.ptr(leave_w), D, S_total, _hip.ptr(ws),
              _hip.ptr(gamma), _hip.ptr(ev), _hip.ptr(cnt) if counts else None,
              _hip.ptr(ent) if counts and shared else None,
              _hip.ptr(g0) if counts and shared else None)
    torch.cuda.synchronize()
    for buf, what in ((gb, 'gamma'), (eb, 'evidence'), (cb, 'dur_counts'), (nb, 'entry_sum'),
                      (zb, 'gamma0_sum')):
        guards_hold(buf, what)
    if not counts:
        assert not cnt.any() and not ent.any() and not g0.any(), 'a NULL output was written'
    return gamma.clone(), ev.clone(), cnt.clone().view(S_total, D), ent.clone(), g0.clone()


def hold(truths, llhs, gamma, ev, tol, what, cnt=None, ent=None, g0=None):
    'Everything of a batch against the truth of its utterances.'
    gamma, ev = npy(gamma), npy(ev)
    assert not np.isnan(gamma).any() and not np.isnan(ev).any(), f'{what}: NaN'
    g_true = np.concatenate([t['gamma'].reshape(-1) for t in truths])
    err = rel_err(gamma, g_true)
    print(f'{what}: gamma rel_err {err:.3e} (bound {tol:.0e})')
    assert err <= tol, f'{what}: gamma rel_err {err:.3e} > {tol:.1e}'
    off, worst = 0, 0.
    for u, (t, l) in enumerate(zip(truths, llhs)):
        n = t['gamma'].size
        rows = gamma[off:off + n].reshape(t['gamma'].shape).sum(1)
        off += n
        if not np.isfinite(t['Z']):
            assert ev[u] == t['Z'] and not rows.any(), f'{what} utterance {u}: infeasible'
            continue
        assert np.abs(rows - 1.).max() <= 10 * tol, f'{what} utterance {u}: rows sum to {rows}'
        bound = et.total_bound(ht.frame_terms(t, l), t['Z'], tol)
        d = abs(ev[u] - t['Z'])
        worst = max(worst, d / bound)
        assert d <= bound, f'{what} utterance {u}: evidence off by {d:.3e} > {bound:.3e}'
    print(f'{what}: evidence within {worst:.3e} of its bounds')
    for name, got in (('dur_counts', cnt), ('entry_sum', ent), ('gamma0_sum', g0)):
        if got is not None:
            want = sum(t[name] for t in truths)
            err = rel_err(npy(got), want)
            print(f'{what}: {name} rel_err {err:.3e}')
            assert err <= tol, f'{what}: {name} rel_err {err:.3e} > {tol:.1e}'


def path_bound(l, path, want, tol):
    'evidence_truth.total_bound with the best path\'s own per-frame terms l_t(path_t).'
    c = np.asarray(l, dtype=np.float64)[np.arange(len(l)), path]
    return et.total_bound(c, want, tol)


def make_case(case, dtype, min_dur=1):
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype])
    S_total = case.S if case.flavour == 'perm' else case.S + 3
    ids = ft.pdf_ids(case.S, case.flavour, S_total, case.seed)
    lens = ft.lengths(case.nutt, case.seed)
    _, llhs = ft.inputs(g, lens, ids, S_total, 1., case.seed, NP[dtype])
    ld, lw = tables(S_total, case.D, case.seed, min_dur)
    batch = hk.HmmBatch([compiled(g, ids)], [0] * len(lens), lens, dtype)
    return g, ids, S_total, lens, llhs, ld, lw, batch


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_forward_backward_is_the_truth(case, dtype):
    g, ids, S_total, lens, llhs, ld, lw, batch = make_case(case, dtype)
    route = hk.duration_route(batch, case.D)
    assert route == case.route, f'route {route:#x}, the table says {case.route:#x}'
    s = batch.struct
    assert route == ht.route_formula(case.S, case.D, tt(llhs[0]).element_size(), s.all_lowdeg,
                                     s.max_degree, s.max_hubs)
    flat = packed(llhs)
    before = flat.clone()
    gamma, ev, cnt, ent, g0 = raw_fb(batch, flat, tt(ld), tt(lw), S_total)
    truths = [ht.posteriors(g, ld, lw, l, ids) for l in llhs]
    hold(truths, llhs, gamma, ev, TOL[dtype], case_id(case), cnt, ent, g0)
    assert torch.equal(flat, before), 'pc_llhs was written'
    # the nullable outputs left out, a second run, the Python face: the same bits
    g2, e2, _, _, _ = raw_fb(batch, flat, tt(ld), tt(lw), S_total, counts=False)
    assert torch.equal(g2, gamma) and torch.equal(e2, ev)
    g3, e3, c3, n3, z3 = hk.duration_forward_backward(batch, flat, tt(ld), tt(lw))
    assert torch.equal(g3, gamma) and torch.equal(e3, ev)
    assert c3.shape == (S_total, case.D) and rel_err(npy(c3), npy(cnt)) <= 1e-13
    assert rel_err(npy(n3), npy(ent)) <= 1e-13 and rel_err(npy(z3), npy(g0)) <= 1e-13
    g4, e4, c4, n4, z4 = hk.duration_forward_backward(batch, flat, tt(ld), tt(lw),
                                                      want_counts=False)
    assert torch.equal(g4, gamma) and c4 is None and n4 is None and z4 is None
    # without leave_w: NULL means 0
    g5, e5, _, _, _ = hk.duration_forward_backward(batch, flat, tt(ld), None)
    g6, e6, _, _, _ = hk.duration_forward_backward(batch, flat, tt(ld), tt(np.zeros_like(lw)))
    assert torch.equal(g5, g6) and torch.equal(e5, e6)


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_viterbi_score_is_the_truth_and_the_path_has_it(case, dtype):
    g, ids, S_total, lens, llhs, ld, lw, batch = make_case(case, dtype)
    flat = packed(llhs)
    path, score = hk.duration_viterbi(batch, flat, tt(ld), tt(lw))
    p2, s2 = hk.duration_viterbi(batch, flat, tt(ld), tt(lw))
    assert torch.equal(path, p2) and torch.equal(score, s2)
    mapped, _ = hk.duration_viterbi(batch, flat, tt(ld), tt(lw), map_pdf=True)
    path, score, mapped = npy(path), npy(score), npy(mapped)
    assert path.dtype == np.int64 and score.dtype == np.float64
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, l in enumerate(llhs):
        want_path, want = ht.best_path(g, ld, lw, l, ids)
        got = path[off[u]:off[u + 1]]
        if not np.isfinite(want):
            assert score[u] == want and (got == -1).all()
            continue
        bound = path_bound(l, want_path, want, TOL[dtype])
        assert abs(score[u] - want) <= bound, f'utterance {u}: {score[u]} for {want}'
        own = ht.path_score(g, ld, lw, l, got, ids)
        assert abs(own - want) <= bound, f'utterance {u}: the path scores {own}, the best {want}'
        assert (mapped[off[u]:off[u + 1]] == np.asarray(ids)[got]).all()


@DTYPES
@pytest.mark.parametrize('S,nO,hub,D', [(3, 3, 0, 4), (8, 3, 0, 3), (64, 8, 0, 8), (12, 12, 0, 5),
                                        (120, 3, 40, 33), (257, 3, 0, 2)])
def test_viterbi_path_is_exact_on_integer_inputs(S, nO, hub, D, dtype):
    'Integer weights, log-likelihoods and duration laws: every sum is exact, ties included.'
    g = ft.make_graph(S, ft.offsets(nO, S), 77, hub, NP[dtype], integer=True)
    lens = [1, 2, 31, 33, 9]
    llhs = ft.viterbi_inputs(S, lens, 78, NP[dtype])
    rng = np.random.RandomState(79)
    ld = rng.randint(-2, 1, size=(S, D)).astype(np.float64)
    lw = rng.randint(0, 2, size=S).astype(np.float64)
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    path, score = hk.duration_viterbi(batch, packed(llhs), tt(ld), tt(lw))
    path, score = npy(path), npy(score)
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, l in enumerate(llhs):
        want_path, want = ht.best_path(g, ld, lw, l)
        assert score[u] == want
        assert (path[off[u]:off[u + 1]] == want_path).all(), f'utterance {u}'


MIXED_LENS, MIXED_GIDS = [33, 9, 32, 2, 40, 1], [0, 1, 2, 0, 2, 1]


@DTYPES
def test_graphs_of_different_sizes_in_one_launch(dtype):
    'Alignment-graph style: the form follows the largest graph, every utterance its own.'
    sizes, D = (7, 65, 129), 5
    arrays = [ft.make_graph(S, ft.offsets(3, S), 2100 + k, 0, NP[dtype]) for k, S in enumerate(sizes)]
    S_total = 140
    idl = [ft.pdf_ids(S, 'partial', S_total, 2200 + k) for k, S in enumerate(sizes)]
    graphs = [compiled(g, ids) for g, ids in zip(arrays, idl)]
    rng = np.random.RandomState(5)
    llhs = [(rng.randn(T, sizes[k]) * 3).astype(NP[dtype]) for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    ld, lw = tables(S_total, D, 6)
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert hk.duration_route(batch, D) == B | R | LD | 0
    gamma, ev, cnt, _, _ = raw_fb(batch, packed(llhs), tt(ld), tt(lw), S_total, shared=False)
    truths = [ht.posteriors(arrays[k], ld, lw, l, idl[k]) for l, k in zip(llhs, MIXED_GIDS)]
    hold(truths, llhs, gamma, ev, TOL[dtype], 'three graphs', cnt)
    _, _, c2, n2, z2 = hk.duration_forward_backward(batch, packed(llhs), tt(ld), tt(lw))
    assert n2 is None and z2 is None and rel_err(npy(c2), npy(cnt)) <= 1e-13
    path, score = hk.duration_viterbi(batch, packed(llhs), tt(ld), tt(lw))
    off = np.concatenate([[0], np.cumsum(MIXED_LENS)])
    for u, (l, k) in enumerate(zip(llhs, MIXED_GIDS)):
        _, want = ht.best_path(arrays[k], ld, lw, l, idl[k])
        bound = et.total_bound(ht.frame_terms(truths[u], l), want, TOL[dtype])
        assert abs(float(score[u]) - want) <= bound
        own = ht.path_score(arrays[k], ld, lw, l, npy(path)[off[u]:off[u + 1]], idl[k])
        assert abs(own - want) <= bound


@DTYPES
def test_one_frame_stays_with_no_law_are_the_hmm_without_self_loops(dtype):
    'D = 1, lam = 0: the HMM whose self-loops were cut, by the HMM oracle.'
    S = 8
    g = ft.make_graph(S, ft.offsets(3, S), 61, 0, NP[dtype])
    cut = dict(g, trans=g['trans'].copy())
    np.fill_diagonal(cut['trans'], -np.inf)
    lens = ft.lengths(9, 62)
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 63, NP[dtype])
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    gamma, ev, _, ent, g0 = hk.duration_forward_backward(batch, packed(llhs),
                                                         tt(np.zeros((S, 1))), None)
    t = ft.truth(cut, llhs)
    assert rel_err(npy(gamma), np.concatenate([x.reshape(-1) for x in t['gamma']])) <= TOL[dtype]
    assert rel_err(npy(g0), t['gamma0']) <= TOL[dtype]
    assert rel_err(npy(ent), t['xi_dense'].sum(0)) <= TOL[dtype]
    for u, l in enumerate(llhs):
        c, total = et.evidence(cut, l)
        assert abs(float(ev[u]) - total) <= et.total_bound(c, total, TOL[dtype])


@DTYPES
@pytest.mark.parametrize('S,hub', [(8, 0), (12, 4), (120, 40)])
def test_geometric_duration_laws_are_the_hmm(S, hub, dtype):
    '''log_dur[j][d-1] = (d - 1) trans_jj, D >= T, no leave_w: gamma and Z of the untouched graph,
    by the oracle and by the HMM kernels on the GPU; entry_sum = the off-diagonal column sums of
    xi_sum.'''
    tol = TOL[dtype]
    g = ft.make_graph(S, ft.offsets(3, S), 64, hub, NP[dtype])
    lens = ft.lengths(9, 65)
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 66, NP[dtype])
    ld = ht.geometric_log_dur(g, max(lens))
    graph = compiled(g)
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    flat = packed(llhs)
    gamma, ev, _, ent, g0 = hk.duration_forward_backward(batch, flat, tt(ld), None)
    t = ft.truth(g, llhs, factored_hub=False)
    xi = t['xi_dense'].copy()
    np.fill_diagonal(xi, 0.)
    assert rel_err(npy(gamma), np.concatenate([x.reshape(-1) for x in t['gamma']])) <= tol
    assert rel_err(npy(ent), xi.sum(0)) <= tol and rel_err(npy(g0), t['gamma0']) <= tol
    for u, l in enumerate(llhs):
        c, total = et.evidence(g, l)
        assert abs(float(ev[u]) - total) <= et.total_bound(c, total, tol)
    hmm_gamma = hk.forward_backward(batch, flat)[0]
    hmm_ev, _ = hk.log_evidence(batch, flat)
    assert rel_err(npy(gamma), npy(hmm_gamma)) <= 2 * tol
    assert np.abs(npy(ev) - npy(hmm_ev)).max() <= 2 * tol * (np.abs(npy(hmm_ev)).max() + 1)


@DTYPES
def test_the_ring_wraps(dtype):
    S, D, T = 8, 33, 300
    g = ft.make_graph(S, ft.offsets(3, S), 67, 0, NP[dtype])
    _, llhs = ft.inputs(g, [T, 70], np.arange(S), S, 1., 68, NP[dtype])
    ld, lw = tables(S, D, 69, min_dur=2)
    batch = hk.HmmBatch([compiled(g)], [0, 0], [T, 70], dtype)
    gamma, ev, cnt, ent, g0 = raw_fb(batch, packed(llhs), tt(ld), tt(lw), S)
    truths = [ht.posteriors(g, ld, lw, l) for l in llhs]
    hold(truths, llhs, gamma, ev, TOL[dtype], 'T=300 D=33', cnt, ent, g0)


@DTYPES
def test_a_per_frame_shift_moves_nothing_but_the_evidence(dtype):
    '''T = 4096, S = 8, D = 8, k_t in +-3e4 added to every entry of row t.  The truth is taken on
    the kernel's own inputs with the shift subtracted again in float64, which is exact (the
    log-likelihoods and the shifts are multiples of 1/64); its evidence is that result plus the
    sum of the shifts.'''
    S, D, T = 8, 8, 4096
    tol = TOL[dtype]
    g = ft.make_graph(S, ft.offsets(3, S), 71, 0, NP[dtype])
    rng = np.random.RandomState(72)
    base = (rng.randint(-512, 513, size=(T, S)) / 64.).astype(NP[dtype])
    k = rng.randint(-30000 * 64, 30000 * 64 + 1, size=T) / 64.
    shifted = (base.astype(np.float64) + k[:, None]).astype(NP[dtype])
    back = shifted.astype(np.float64) - k[:, None]
    assert (back == base.astype(np.float64)).all()
    ld, lw = tables(S, D, 73)
    batch = hk.HmmBatch([compiled(g)], [0], [T], dtype)
    gamma, ev, cnt, ent, g0 = raw_fb(batch, packed([shifted]), tt(ld), tt(lw), S)
    t = ht.posteriors(g, ld, lw, back)
    moved = dict(t, Z=t['Z'] + k.sum())
    hold([moved], [shifted], gamma, ev, tol, 'shifted', cnt, ent, g0)
    path, score = hk.duration_viterbi(batch, packed([shifted]), tt(ld), tt(lw))
    _, want = ht.best_path(g, ld, lw, back)
    bound = et.total_bound(ht.frame_terms(moved, shifted), want + k.sum(), tol)
    assert abs(float(score[0]) - (want + k.sum())) <= bound
    assert abs(ht.path_score(g, ld, lw, back, npy(path)) - want) <= bound


@DTYPES
def test_minus_infinity_edges(dtype):
    '''Minimum duration 2 on every state, -inf emission entries, and an utterance with no
    segmentation (T = 1 under a minimum duration of 2) between feasible ones.'''
    S, D = 8, 5
    g = ft.make_graph(S, ft.offsets(4, S), 74, 0, NP[dtype])
    lens = [9, 1, 6, 8, 1, 2]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 75, NP[dtype])
    rng = np.random.RandomState(76)
    for l in llhs:
        if len(l) > 2:
            l[rng.randint(0, len(l), size=6), rng.randint(0, S, size=6)] = -np.inf
    ld, lw = tables(S, D, 77, min_dur=2)
    assert np.isinf(ld[:, 0]).all()
    batch = hk.HmmBatch([compiled(g)], [0] * len(lens), lens, dtype)
    gamma, ev, cnt, ent, g0 = raw_fb(batch, packed(llhs), tt(ld), tt(lw), S)
    truths = [ht.posteriors(g, ld, lw, l) for l in llhs]
    assert [np.isfinite(t['Z']) for t in truths] == [True, False, True, True, False, True]
    hold(truths, llhs, gamma, ev, TOL[dtype], '-inf edges', cnt, ent, g0)
    path, score = hk.duration_viterbi(batch, packed(llhs), tt(ld), tt(lw))
    path, score = npy(path), npy(score)
    off = np.concatenate([[0], np.cumsum(lens)])
    for u, l in enumerate(llhs):
        _, want = ht.best_path(g, ld, lw, l)
        got = path[off[u]:off[u + 1]]
        if not np.isfinite(want):
            assert score[u] == -np.inf and (got == -1).all()
        else:
            bound = et.total_bound(ht.frame_terms(truths[u], l), want, TOL[dtype])
            assert abs(score[u] - want) <= bound
            assert abs(ht.path_score(g, ld, lw, l, got) - want) <= bound


def test_the_python_face_names_the_limit():
    g = ft.make_graph(8, ft.offsets(3, 8), 80, 0)
    batch = hk.HmmBatch([compiled(g)], [0], [4], torch.float64)
    flat = packed([np.zeros((4, 8))])
    with pytest.raises(ValueError, match='BEER_HSMM_MAX_DUR'):
        hk.duration_forward_backward(batch, flat, tt(np.zeros((8, DMAX + 1))))
    with pytest.raises(_hip.HipError, match='BEER_HSMM_MAX_DUR'):
        hk.duration_route(batch, DMAX + 1)
    with pytest.raises(ValueError, match='pdf id'):
        hk.duration_viterbi(batch, flat, tt(np.zeros((7, 3))))
    big = ft.make_graph(_hip.HSMM_MAX_STATES + 1, (0, 1), 81, 0)
    bbig = hk.HmmBatch([compiled(big)], [0], [2], torch.float64)
    with pytest.raises(_hip.HipError, match='BEER_HSMM_MAX_STATES'):
        hk.duration_route(bbig, 2)


# --- the model level -----------------------------------------------------------------------------

import io                                                            # noqa: E402
import os                                                            # noqa: E402
import pickle                                                        # noqa: E402
import sys                                                           # noqa: E402

from aligned_truth import loop_and_units                             # noqa: E402
from helpers import GOLDEN, assert_stats_close                       # noqa: E402
from transitions_truth import loop_topology                          # noqa: E402
from beer_amd.cli import main as cli_main                            # noqa: E402

DEV = torch.device('cuda')
FLAT = 1e-5                         # the repository's flat tolerance on accumulated statistics
MODELS = pytest.mark.parametrize('kind', ['normalset', 'mixtureset'])


def _model(kind, dtype=torch.float64, D=6, strength=1., seed=3, loop=.6):
    '''(model on the device, units): a PhoneLoop of 4 units x 3 states over diagonal NormalSet
    emissions, or over a MixtureSet of two Gaussians a state on 2-d data.'''
    dim, ncomp = (3, 1) if kind == 'normalset' else (2, 2)
    units, graph, start, end, ems = loop_and_units(4, 0, dim, 'diagonal', ncomp,
                                                   loop_topology(loop), seed)
    if kind == 'normalset':
        ems = beer.NormalSet.create(torch.zeros(dim), torch.ones(dim), size=12, prior_strength=1.,
                                    noise_std=1., cov_type='diagonal')
    model = beer.PhoneLoop.create(graph.compile(), start, end, ems, max_duration=D,
                                  durations_prior_strength=strength)
    model = model.double() if dtype == torch.float64 else model.float()
    return model.to(DEV), units


def _data(model, lens, seed, dtype=torch.float64):
    ndim = 3 if isinstance(model._emissions(), beer.NormalSet) else 2
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.randn(sum(lens), ndim) * 1.5).to(DEV, dtype)


def _graph_arrays(graph):
    'The fb_truth-style dict of a compiled graph (dense or of a compiled set), float64.'
    g = graph.to_dense() if hasattr(graph, 'to_dense') else graph
    return dict(S=g.n_states, init=npy(g.init_log_probs.double()), hub=None,
                final=npy(g.final_log_probs.double()), trans=npy(g.trans_log_probs.double()))


def _ids(graph):
    m = graph.pdf_id_mapping
    return np.arange(graph.n_states) if m is None else np.asarray([int(i) for i in m])


def _truth_stats(model, X, lens, scale=1., graphs=None):
    '''What the E-step must accumulate, from the truth on the model's own tables: (dict
    {parameter: statistics}, per-utterance truths, per-utterance llhs).'''
    stats = model.sufficient_statistics(X)
    ems = model._emissions()
    pc_all = npy(ems.expected_log_likelihood(stats).double())
    ld, lw = npy(model.durations.log_dur()), npy(model.durations.leave_w())
    off = np.concatenate([[0], np.cumsum(lens)])
    sr = np.zeros_like(pc_all)
    counts = np.zeros_like(ld)
    phones = np.zeros(len(model.start_pdf))
    starts = [int(model.start_pdf[u]) for u in model.start_pdf]
    truths, llhs = [], []
    for u in range(len(lens)):
        graph = model.graph if graphs is None else graphs[u]
        ids = _ids(graph)
        # (the gather rounds scale * pc once, in the model's precision)
        l = (X.new_tensor(scale) * ems.expected_log_likelihood(stats)[off[u]:off[u + 1]])
        l = npy(l)[:, ids]
        t = ht.posteriors(_graph_arrays(graph), ld, lw, l, ids)
        np.add.at(sr[off[u]:off[u + 1]].T, ids, t['gamma'].T)
        counts += t['dur_counts']
        if graphs is None:
            phones += t['gamma0_sum'][starts] + t['entry_sum'][starts]
        truths.append(t)
        llhs.append(l)
    want = dict(ems.accumulate(stats, tt(scale * sr).to(X.dtype)))
    want.update(model.durations.accumulate_counts(tt(counts)))
    cat = model.categorical
    ref = cat.mean_field_factorization()[0][0].stats
    want.update(cat.accumulate(cat.sufficient_statistics(tt(phones).to(ref.dtype).view(1, -1))))
    return want, truths, llhs, counts


def _hold_stats(got, want, ndim, what):
    assert set(got) == set(want), f'{what}: the parameters with statistics differ'
    for p in want:
        g, w = npy(got[p].double()), npy(want[p].double())
        assert g.shape == w.shape, f'{what}: {g.shape} for {w.shape}'
        if w.ndim == 2 and w.shape[1] == 2 * ndim + 2:
            assert_stats_close(g, w, ndim, FLAT, what)
        else:
            err = rel_err(g, w)
            assert err <= FLAT, f'{what}: statistics of shape {w.shape}: rel_err {err:.3e}'


@DTYPES
@MODELS
def test_the_e_step_accumulates_what_the_truth_does(kind, dtype):
    model, _ = _model(kind, dtype)
    lens = [9, 3, 33, 4, 14]
    X = _data(model, lens, 31, dtype)
    ndim = X.shape[1]
    scale = .75
    want, truths, llhs, counts = _truth_stats(model, X, lens, scale)
    # the model's own E-step on the ragged batch
    stats = model.sufficient_statistics(X)
    exp_llh = model.expected_log_likelihood(stats, scale=scale, utt_lengths=lens)
    per_frame = np.concatenate([(t['gamma'] * l).sum(1) for t, l in zip(truths, llhs)])
    assert rel_err(npy(exp_llh), per_frame) <= TOL[dtype]
    _hold_stats(model.accumulate(stats), want, ndim, 'expected_log_likelihood + accumulate')
    model.clear_cache()
    # the batched E-step, in sub-batches too
    for max_frames in (1 << 24, 20):
        elbo = beer.accumulate_elbo(model, (X, lens), datasize=1000, scale=scale,
                                    max_frames=max_frames)
        _hold_stats(elbo._acc_stats, want, ndim, f'accumulate_elbo (max_frames={max_frames})')
    # ... equals the sum over single utterances, in value and in statistics
    off = np.concatenate([[0], np.cumsum(lens)])
    total = None
    for u in range(len(lens)):
        one = beer.evidence_lower_bound(model, X[off[u]:off[u + 1]], datasize=1000, scale=scale)
        total = one if total is None else total + one
    assert abs(float(total) - float(elbo)) <= TOL[dtype] * 10 * abs(float(elbo))
    _hold_stats(total._acc_stats, want, ndim, 'sum of evidence_lower_bound')
    # one update of the durations' group at learning rate 1: posterior = prior + the truth's counts
    assert model.mean_field_factorization()[-1] == [model.durations.weights]
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization()[-1:], lrate=1.)
    optim.init_step()
    elbo = beer.accumulate_elbo(model, (X, lens), datasize=sum(lens), scale=scale)
    elbo.backward()
    optim.step()
    w = model.durations.weights
    got = npy(w.posterior.params.concentrations.double())
    assert rel_err(got, npy(w.prior.params.concentrations.double()) + counts) <= FLAT
    assert np.abs(counts.sum() - sum(t['gamma0_sum'].sum() + t['entry_sum'].sum()
                                     for t in truths)) <= 1e-9 * counts.sum()


@DTYPES
@MODELS
def test_decode_score_and_posteriors_are_the_truth(kind, dtype):
    model, _ = _model(kind, dtype)
    lens = [9, 2, 33, 3, 14]             # (two frames cannot cross a unit of three states)
    X = _data(model, lens, 32, dtype)
    _, truths, llhs, _ = _truth_stats(model, X, lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    utts = [X[off[u]:off[u + 1]] for u in range(len(lens))]
    ld, lw = npy(model.durations.log_dur()), npy(model.durations.leave_w())
    g, ids = _graph_arrays(model.graph), _ids(model.graph)
    paths = beer.decode_batch(model, utts)
    scores = beer.log_evidence_batch(model, utts)
    pred = beer.log_evidence_batch(model, utts, predictive=True)
    assert scores.dtype == torch.float64 and pred.shape == scores.shape
    for u, x in enumerate(utts):
        one = model.decode(x)
        assert torch.equal(one, paths[u].cpu()), f'utterance {u}: decode_batch != decode'
        _, want = ht.best_path(g, ld, lw, llhs[u], ids)
        if not np.isfinite(want):
            assert u == 1 and (one == -1).all() and float(scores[u]) == -np.inf
            assert float(model.log_evidence(x)) == -np.inf and not npy(model.posteriors(x)).any()
            continue
        state = np.searchsorted(ids, npy(one)) if (np.diff(ids) > 0).all() else None
        assert state is not None
        own = ht.path_score(g, ld, lw, llhs[u], state, ids)
        bound = path_bound(llhs[u], state, want, TOL[dtype])
        assert abs(own - want) <= bound, f'utterance {u}: the decoded path scores {own}, not {want}'
        ev = model.log_evidence(x)
        assert float(ev) == float(scores[u]), f'utterance {u}: log_evidence_batch != log_evidence'
        t = truths[u]
        assert abs(float(ev) - t['Z']) <= et.total_bound(ht.frame_terms(t, llhs[u]), t['Z'], TOL[dtype])
        assert float(model.log_evidence(x, predictive=True)) == float(pred[u])
        assert rel_err(npy(model.posteriors(x)), t['gamma']) <= TOL[dtype]
    assert not torch.equal(pred, scores)


@DTYPES
def test_alignment_graphs_share_the_duration_laws(dtype):
    model, units = _model('mixtureset', dtype)
    seqs = [['s0', 's1', 's0'], ['s2'], ['s1', 's3', 's1', 's2'], ['s3', 's0']]
    lens = [40, 7, 33, 12]
    graphs = list(beer.graph.compile_alignments(seqs, units))
    assert len(set(graphs[0].pdf_id_mapping)) < len(graphs[0].pdf_id_mapping)
    X = _data(model, lens, 33, dtype)
    want, truths, llhs, counts = _truth_stats(model, X, lens, 1., graphs)
    assert all(np.isfinite(t['Z']) for t in truths)
    elbo = beer.accumulate_elbo(model, (X, lens), datasize=500, inference_graphs=graphs)
    _hold_stats(elbo._acc_stats, want, X.shape[1], 'accumulate_elbo on alignment graphs')
    off = np.concatenate([[0], np.cumsum(lens)])
    utts = [X[off[u]:off[u + 1]] for u in range(len(lens))]
    total = None
    for u, x in enumerate(utts):
        one = beer.evidence_lower_bound(model, x, datasize=500, inference_graph=graphs[u])
        total = one if total is None else total + one
    assert abs(float(total) - float(elbo)) <= TOL[dtype] * 10 * abs(float(elbo))
    _hold_stats(total._acc_stats, want, X.shape[1], 'evidence_lower_bound on alignment graphs')
    paths = beer.decode_batch(model, utts, inference_graphs=graphs)
    scores = beer.log_evidence_batch(model, utts, inference_graphs=graphs)
    for u, x in enumerate(utts):
        assert torch.equal(model.decode(x, inference_graph=graphs[u]), paths[u].cpu())
        ev = model.log_evidence(x, inference_graph=graphs[u])
        assert float(ev) == float(scores[u])
        t = truths[u]
        assert abs(float(ev) - t['Z']) <= et.total_bound(ht.frame_terms(t, llhs[u]), t['Z'], TOL[dtype])
        # a forced alignment spells its transcription
        first = {int(model.start_pdf[n]): n for n in model.start_pdf}
        p = npy(paths[u])
        spelled = [first[int(p[0]) // 3 * 3]] + [first[int(b)] for a, b in zip(p[:-1], p[1:])
                                                 if a != b and int(b) in first]
        assert spelled == seqs[u]


def test_durations_are_learned():
    '''Data drawn from an HSMM whose states last exactly 3 or 4 frames: after ten VB iterations
    every state's E[p(3)] + E[p(4)] exceeds the same mass under its initial geometric row.'''
    dim, n_units, D = 8, 4, 6
    units, graph, start, end, _ = loop_and_units(n_units, 0, dim, 'diagonal', 1, loop_topology(.6), 5)
    rng = np.random.RandomState(41)
    means = rng.randn(3 * n_units, dim) * 3.
    # the emissions start near the states' own means (the test is about the durations): prior
    # N(0, 1)-ish on every state, posterior means = the true means + noise
    K = 3 * n_units
    f64 = lambda a: torch.as_tensor(a, dtype=torch.float64)          # noqa: E731
    rest = (torch.ones(K, 1, dtype=torch.float64), torch.ones(K, 1, dtype=torch.float64),
            torch.ones(K, dim, dtype=torch.float64))
    NG = beer.dists.NormalGamma
    ems = beer.NormalSet(beer.ConjugateBayesianParameter(
        NG.from_std_parameters(torch.zeros(K, dim, dtype=torch.float64), *[r.clone() for r in rest]),
        NG.from_std_parameters(f64(means + .5 * rng.randn(K, dim)), *[r.clone() for r in rest])))
    model = beer.PhoneLoop.create(graph.compile(), start, end, ems, max_duration=D).double().to(DEV)
    utts = []
    for _ in range(40):
        frames = []
        for unit in rng.randint(0, n_units, size=6):
            for k in range(3):
                d = rng.randint(3, 5)
                frames.append(means[3 * unit + k] + .3 * rng.randn(d, dim))
        utts.append(torch.from_numpy(np.concatenate(frames)).to(DEV))
    p0, _ = model.durations.expected_durations()
    before = (p0[:, 2] + p0[:, 3]).numpy()
    np.testing.assert_allclose(before, (.6 ** 2 + .6 ** 3) * .4 / (.4 * sum(.6 ** k for k in range(D))),
                               rtol=1e-6)
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
    n = sum(len(u) for u in utts)
    for _ in range(10):
        optim.init_step()
        elbo = beer.accumulate_elbo(model, utts, datasize=n)
        elbo.backward()
        optim.step()
    p1, mean = model.durations.expected_durations()
    after = (p1[:, 2] + p1[:, 3]).numpy()
    print('E[p(3)] + E[p(4)] per state:', np.round(after, 3), 'from', before[0])
    assert (after > before).all()


# --- the command line ----------------------------------------------------------------------------

HMM_CONF = """
- group_name: sil
  n_normal_per_state: 2
  prior_strength: 1.
  noise_std: 0.5
  cov_type: diagonal
  shared_cov: no
  topology:
  - {start_id: 0, end_id: 1, trans_prob: 1.0}
  - {start_id: 1, end_id: 1, trans_prob: 0.5}
  - {start_id: 1, end_id: 2, trans_prob: 0.5}
  - {start_id: 2, end_id: 2, trans_prob: 0.5}
  - {start_id: 2, end_id: 3, trans_prob: 0.5}
- group_name: speech
  n_normal_per_state: 2
  prior_strength: 1.
  noise_std: 0.5
  cov_type: diagonal
  shared_cov: no
  topology:
  - {start_id: 0, end_id: 1, trans_prob: 1.0}
  - {start_id: 1, end_id: 1, trans_prob: 0.75}
  - {start_id: 1, end_id: 2, trans_prob: 0.25}
  - {start_id: 2, end_id: 2, trans_prob: 0.75}
  - {start_id: 2, end_id: 3, trans_prob: 0.25}
  - {start_id: 3, end_id: 3, trans_prob: 0.75}
  - {start_id: 3, end_id: 4, trans_prob: 0.25}
"""


def _run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_explicit_durations_on_the_reference_corpus(tmp_path):
    t = str(tmp_path)
    (tmp_path / 'hmm.yml').write_text(HMM_CONF)
    (tmp_path / 'units').write_text('sil sil\na speech\nb speech\nc speech\n')
    _run(['dataset', 'create', t, os.path.join(GOLDEN, 'ref_feats.npz'), f'{t}/ds.pkl'])
    _run(['-s', '1', 'hmm', 'mkphones', '-d', f'{t}/ds.pkl', f'{t}/hmm.yml', f'{t}/units',
          f'{t}/hmms.mdl'])
    _run(['hmm', 'mkphoneloopgraph', '--start-end-group', 'sil', f'{t}/units', f'{t}/g.pkl'])
    _run(['hmm', 'mkdecodegraph', f'{t}/g.pkl', f'{t}/hmms.mdl', f'{t}/dg.pkl'])
    _run(['hmm', 'mkphoneloop', '--max-duration', '12', '--durations-prior-strength', '2',
          '--weights-prior', 'dirichlet', f'{t}/dg.pkl', f'{t}/hmms.mdl', f'{t}/0.mdl'])
    m0 = pickle.load(open(f'{t}/0.mdl', 'rb'))
    assert m0.durations.max_duration == 12 and len(m0.durations) == 11
    # accumulate + update, then train
    _run(['hmm', 'accumulate', f'{t}/0.mdl', f'{t}/ds.pkl', f'{t}/e.pkl'], stdin='utt0\nutt1\nutt2\n')
    for _ in range(len(m0.mean_field_factorization())):
        _run(['hmm', 'update', '-o', f'{t}/optim.pth', f'{t}/0.mdl', f'{t}/1.mdl'],
             stdin=f'{t}/e.pkl\n')
    _run(['hmm', 'train', '-e', '2', f'{t}/0.mdl', f'{t}/ds.pkl', f'{t}/2.mdl'])
    m2 = pickle.load(open(f'{t}/2.mdl', 'rb'))
    a, b = m0.durations.weights, m2.durations.weights
    np.testing.assert_array_equal(a.prior.params.concentrations.numpy(),
                                  b.prior.params.concentrations.numpy())
    moved = (b.posterior.params.concentrations - a.posterior.params.concentrations).sum()
    assert float(moved) > 1.
    out = _run(['hmm', 'decode', f'{t}/2.mdl', f'{t}/ds.pkl'])
    assert sorted(l.split()[0] for l in out.strip().split('\n')) == ['utt0', 'utt1', 'utt2']
    out = _run(['hmm', 'score', f'{t}/2.mdl', f'{t}/ds.pkl'])
    rows = [l.split() for l in out.strip().split('\n')]
    assert sorted(r[0] for r in rows) == ['utt0', 'utt1', 'utt2']
    assert all(np.isfinite(float(r[1])) for r in rows)
    os.makedirs(f'{t}/post')
    _run(['hmm', 'posteriors', '-S', f'{t}/2.mdl', f'{t}/ds.pkl', f'{t}/post'])
    post = np.load(f'{t}/post/utt0.npy')
    assert post.shape[1] == 11 and np.abs(post.sum(1) - 1).max() < 1e-4
    lines = _run(['hmm', 'durations', f'{t}/2.mdl']).strip().split('\n')
    assert len(lines) == 11
    unit, state, mean, mode, *probs = lines[3].split()
    assert (unit, state) == ('a', '1') and len(probs) == 12 and 1 <= int(mode) <= 12
    assert abs(sum(float(p) for p in probs) - 1) < 1e-4
    assert abs(float(mean) - sum((k + 1) * float(p) for k, p in enumerate(probs))) < 1e-2
    # the subcommands of the refused combinations exit with the model's message
    for argv, what in ((['hmm', 'decode', '--nbest', '2', f'{t}/2.mdl', f'{t}/ds.pkl'],
                        'decode_nbest'),
                       (['hmm', 'decode', '--nsamples', '2', f'{t}/2.mdl', f'{t}/ds.pkl'],
                        'sample_paths'),
                       (['hmm', 'boundaries', f'{t}/2.mdl', f'{t}/ds.pkl', f'{t}/b'], 'unit_starts'),
                       (['hmm', 'mkphoneloopbigram', '--weights-prior', 'dirichlet2', f'{t}/2.mdl',
                         f'{t}/x.mdl'], 'BigramPhoneLoop')):
        with pytest.raises(SystemExit) as err:
            _run(argv)
        assert 'explicit durations' in str(err.value) and what in str(err.value)
