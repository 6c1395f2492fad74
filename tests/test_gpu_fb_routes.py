"""Every kernel route of the forward-backward / Viterbi dispatch of csrc/hmm.hip against the
oracle, on graphs that sit on the dispatch boundaries (tests/fb_truth.py).

One static table: each case names the family `beer_hmm_forward_backward` must launch for it
(`beer_hmm_fb_route`), and each test first holds the C layer's choice, what Python made
of it (`hk.fused_ok`, `batch.last_alpha_is_log`) and the table against each other -- if the two
layers disagree, `trans_posteriors_dense` reads scaled probabilities as logarithms.  Then every
output of every entry point that runs on that route is compared with the float64 oracle:
float64 to 1e-9 (1e-11 for the mean log-normaliser), float32 to 1e-5 or the error of the
oracle's own float32 run.  Batches are ragged, 1 to 9 frames (the one-wave kernels load 4 frames
ahead and rescale every 2), of 1, 5 and 9 utterances (never a multiple of the 4 waves of a
workgroup)."""

from collections import namedtuple

import numpy as np
import pytest
import torch

import fb_truth as ft
from helpers import assert_close, assert_within_f32_band

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

WAVE, LOWDEG, GENERAL, BIG = _hip.FB_WAVE, _hip.FB_LOWDEG, _hip.FB_GENERAL, _hip.FB_GENERAL_BIG


def wave(spl, deg):
    return WAVE | (spl << 4) | deg


Case = namedtuple('Case', 'S nO hub nutt flavour scale S_total route seed')
# how the fused launch hands the posteriors back to pdf ids (hk.posteriors_fused): plain stores
# (a permutation; ids left out of more than 512 columns), atomic adds (repeats, more than 512
# columns), whole rows through LDS (repeats / ids left out, at most 512 columns)
VARIANTS = [('perm', 1., None), ('repeat', .7, 512), ('partial', 1., 513), ('perm', .7, None),
            ('repeat', 1., 513), ('partial', .7, 512)]
CASES = []


def add(S, nO, route, hub=0, nutt=None):
    i = len(CASES)
    flavour, scale, S_total = VARIANTS[i % len(VARIANTS)]
    if _hip.fb_family(route) != WAVE:                   # (no fused launch beyond the one-wave kernels)
        flavour, S_total = 'perm', None
    CASES.append(Case(S, nO, hub, nutt or (1, 5, 9)[(i // 6 + i) % 3], flavour, scale,
                      S_total or S, route, i))


SPL_OF = [(1, 1), (2, 1), (63, 1), (64, 1), (65, 2), (127, 2), (128, 2), (129, 4), (255, 4), (256, 4)]
DEG_OF = [(1, 2), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)]
# 1. the one-wave kernels: every state boundary against every degree boundary (a graph of one
#    or two states has degree 1 or 2 whatever the offsets)
for S_, spl_ in SPL_OF:
    for nO_, deg_ in DEG_OF:
        add(S_, nO_, wave(spl_, deg_ if S_ > 2 else 2))
# 2. nine arcs a state: no low-degree image, the general kernel
for S_ in (63, 64, 65, 128, 129, 256, 257):
    add(S_, 9, GENERAL)
# 3. beyond 256 states: one thread per state up to 512 states, then the general kernel (with few
#    enough arcs for its lists to fit LDS in either precision, with the transition posteriors)
for S_ in (257, 511, 512):
    for nO_ in (1, 2, 3, 5, 8):
        add(S_, nO_, LOWDEG | 512)
for nO_ in (1, 2, 3, 5):
    add(513, nO_, GENERAL)
# 4. a hub of 1, 2 and 64 members a side stays on the one-wave kernels (64 members of 64 states:
#    every arc is a hub arc, the image's degree is 1)
for m_ in (1, 2, 64):
    for S_, spl_ in [(64, 1), (65, 2), (128, 2), (129, 4), (256, 4)]:
        for nO_, deg_ in [(2, 2), (5, 8)]:
            add(S_, nO_, wave(spl_, 2 if (S_, m_) == (64, 64) else deg_), hub=m_)
# 5. a hub of 65 members: one thread per state, 128 / 256 / 512 threads
for S_, thr_ in [(66, 128), (127, 128), (128, 128), (129, 256), (255, 256), (256, 256), (257, 512),
                 (512, 512)]:
    for nO_ in (2, 5):
        add(S_, nO_, LOWDEG | thr_, hub=65)
add(130, 3, wave(4, 4), hub=64)
add(130, 3, LOWDEG | 256, hub=65)
# beyond 512 states a declared hub changes nothing: the general kernel, hub arcs in the matrix
add(513, 3, GENERAL, hub=2)
# 6. a dense graph whose arc lists do not fit a CU's LDS
add(100, 100, BIG, nutt=5)
# 7. every batch size on both sides of every state boundary
for S_, route_ in [(64, wave(1, 4)), (65, wave(2, 4)), (128, wave(2, 4)), (129, wave(4, 4)),
                   (256, wave(4, 4)), (257, LOWDEG | 512), (512, LOWDEG | 512), (513, GENERAL)]:
    for nutt_ in (1, 5, 9):
        add(S_, 4, route_, nutt=nutt_)


def case_offsets(case):
    return ft.offsets(case.nO, case.S)


def out_mode(case):
    'The `atomic_out` argument hk.posteriors_fused picks for the case (include/beer_hip.h).'
    if case.flavour == 'perm':
        return 0
    if case.flavour == 'repeat' and case.S == 1:        # (one state repeats nothing: an id left out)
        return 2 if case.S_total <= hk.FUSED_ROW_MAX else 0
    return 2 if case.S_total <= hk.FUSED_ROW_MAX else (1 if case.flavour == 'repeat' else 0)


def case_id(case):
    fam = {WAVE: 'wave', LOWDEG: 'lowdeg', GENERAL: 'general', BIG: 'big'}[_hip.fb_family(case.route)]
    return f'{case.seed}-S{case.S}-O{case.nO}-hub{case.hub}-n{case.nutt}-{case.flavour}-{fam}'


NP = {torch.float64: np.float64, torch.float32: np.float32}


class Checker:
    'float64: 1e-9 (`tight` for the log-normaliser); float32: 1e-5 or the oracle\'s own float32 error.'

    def __init__(self, dtype, t64, t32):
        self.f32, self.t64, self.t32 = dtype == torch.float32, t64, t32

    def __call__(self, got, key, what, tight=1e-9, pick=lambda a: a):
        got = np.asarray(npy(got) if torch.is_tensor(got) else got, dtype=np.float64)
        want = np.asarray(pick(self.t64[key]), dtype=np.float64)
        got = got.reshape(want.shape)
        if self.f32:
            err, band = assert_within_f32_band(got, want, np.asarray(pick(self.t32[key]), np.float64),
                                               f'{what} {key}', tol=1e-5)
        else:
            assert_close(got, want, tight, f'{what} {key}')


def build(case, dtype):
    'graph arrays, CompiledGraph (hub declared, pdf ids attached) of a case'
    g = ft.make_graph(case.S, case_offsets(case), case.seed, case.hub, NP[dtype])
    ids = ft.pdf_ids(case.S, case.flavour, case.S_total, case.seed)
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in ids])
    if g['hub'] is not None:
        E, a, B, c = g['hub']
        graph.set_hub(E, tt(a), B, tt(c))
    return g, ids, graph


def route_of(batch, dtype, want_xi):
    return _hip.lib().beer_hmm_fb_route(_hip.dtype_code(dtype), batch.ref(), int(want_xi),
                                        int(want_xi))


def packed(llhs):
    return torch.cat([tt(l).reshape(-1) for l in llhs])


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_every_entry_point_on_its_route(case, dtype):
    S, nutt, scale = case.S, case.nutt, case.scale
    fam = _hip.fb_family(case.route)
    is_wave = fam == WAVE
    g, ids, graph = build(case, dtype)
    lens = ft.lengths(nutt, case.seed)
    pc_all, llhs = ft.inputs(g, lens, ids, case.S_total, scale, case.seed, NP[dtype])
    batch = hk.HmmBatch([graph], [0] * nutt, lens, dtype)
    # --- the route: the C layer, Python's restatement, the table
    for want_xi in (0, 1):
        assert route_of(batch, dtype, want_xi) == case.route
    assert hk.fused_ok(batch) == is_wave
    scratch = [_hip.lib().beer_hmm_fb_scratch_doubles(_hip.dtype_code(dtype), batch.ref(), x)
               for x in (0, 1)]
    # (the scratch the general kernel would need: also what `dense_xi=True` below is given)
    assert fam not in (GENERAL, BIG) or all((n > 0) == (fam == BIG) for n in scratch)
    factored = fam in (WAVE, LOWDEG)
    kw = dict(ids=ids, S_total=case.S_total, scale=scale, factored_hub=factored)
    t64 = ft.truth(g, llhs, dtype=np.float64, **kw)
    t32 = ft.truth(g, llhs, dtype=np.float32, **kw) if dtype == torch.float32 else None
    check = Checker(dtype, t64, t32)
    flat = packed(llhs)
    cat = np.concatenate

    def check_fb(res, what, xi):
        gam, x, g0, ln, flow = res
        check(gam, 'gamma', what, pick=lambda a: cat([v.reshape(-1) for v in a]))
        check(ln, 'lognorm', what, tight=1e-11)
        if xi:
            check(x, 'xi_sum', what)
            check(flow, 'hub_flow', what)
            check(g0, 'gamma0', what)

    # --- forward_backward without and with the transition posteriors
    check_fb(hk.forward_backward(batch, flat, want_lognorm=True), 'fb', False)
    assert batch.last_alpha_is_log == (not is_wave)
    check_fb(hk.forward_backward(batch, flat, want_xi=True, want_lognorm=True), 'fb+xi', True)
    assert batch.last_alpha_is_log == (not is_wave)

    # --- the general kernel forced, then the per-frame transition posteriors of one utterance
    u = int(np.argmax(lens))
    one = hk.HmmBatch([graph], [0], [lens[u]], dtype)
    gam1, x1, _, _, flow1 = hk.forward_backward(one, tt(llhs[u]).reshape(-1), want_xi=True,
                                                dense_xi=True)
    assert one.last_alpha_is_log and one.struct.all_lowdeg == batch.struct.all_lowdeg
    xi64 = ft.xi_frames(g, llhs[u])
    one_check = Checker(dtype, dict(xi=xi64, xi_sum=xi64.sum(0), gamma=t64['gamma'][u], zero=np.zeros(S)),
                        dict(xi=ft.xi_frames(g, llhs[u], np.float32),
                             gamma=t32['gamma'][u], zero=np.zeros(S)) if t32 else None)
    if t32:
        one_check.t32['xi_sum'] = one_check.t32['xi'].astype(np.float64).sum(0)
    one_check(gam1, 'gamma', 'dense')
    one_check(x1, 'xi_sum', 'dense')
    one_check(flow1, 'zero', 'dense')
    xi = hk.trans_posteriors_dense(one, tt(llhs[u]).reshape(-1), gam1, graph.trans_log_probs)
    assert tuple(xi.shape) == xi64.shape
    one_check(xi, 'xi', 'per-frame')

    # --- the transition counts: arcs of the low-degree image on the one-wave kernels, the dense
    #     matrix and the last frames' posteriors beyond them
    def check_counts(counts, what):
        kind, a, b = counts
        if is_wave:
            assert kind == 'arcs'
            check(a[:len(t64['arc_counts'])], 'arc_counts', what)     # (at least one element long)
            check(b, 'src_flow', what)
        else:
            assert kind == 'dense'
            check(a, 'xi_dense', what)
            check(b, 'last', what)

    def run_counts(what):
        gam, g0, flow, x, counts = hk.forward_backward_counts(batch, flat)
        check(gam, 'gamma', what, pick=lambda a: cat([v.reshape(-1) for v in a]))
        check(g0, 'gamma0', what)
        if is_wave:
            check(flow, 'hub_flow', what)
        check_counts(counts, what)

    run_counts('counts')

    # --- gather + forward-backward + scatter in one launch
    def run_fused(what, transitions):
        utt = torch.zeros(nutt, dtype=torch.float64, device=batch.device)
        frame = torch.full((batch.n_frames,), 7., dtype=dtype, device=batch.device)
        res = hk.posteriors_fused(batch, tt(pc_all), scale, want_counts=True, utt_llh=utt,
                                  frame_llh=frame, want_transitions=transitions)
        check(res[0], 'state_resps', what)
        check(res[1], 'gamma0', what)
        check(res[2], 'hub_flow', what)
        check(utt, 'utt_llh', what)
        check(frame, 'frame_llh', what)
        if transitions:
            check_counts(res[3], what)

    if is_wave:
        repeats, covers = batch.pdf_ids_profile(case.S_total)
        mode = 2 if (repeats or not covers) and case.S_total <= hk.FUSED_ROW_MAX else int(repeats)
        assert mode == out_mode(case)
        run_fused('fused', False)
        run_fused('fused+counts', True)
        # --- the log-space twin takes every utterance of every launch, with the same results
        old = _hip.set_option('fb_log', 1)
        try:
            with hk.counting_log_space() as c:
                check_fb(hk.forward_backward(batch, flat, want_lognorm=True), 'log fb', False)
                check_fb(hk.forward_backward(batch, flat, want_xi=True, want_lognorm=True),
                         'log fb+xi', True)
                run_counts('log counts')
                run_fused('log fused', False)
                run_fused('log fused+counts', True)
            assert batch.last_alpha_is_log is False
            assert c.launches == 5 and int(c.count) == c.launches * nutt
        finally:
            _hip.set_option('fb_log', old)
    else:
        with pytest.raises(_hip.HipInvalid):
            hk.posteriors_fused(batch, tt(pc_all), scale)


# --- graphs of different sizes in one launch ---------------------------------------------------

MIXED = [('wave', (7, 65, 128), wave(2, 4)), ('lowdeg', (40, 300, 512), LOWDEG | 512),
         ('general', (40, 300, 513), GENERAL)]
MIXED_LENS, MIXED_GIDS = [9, 1, 4, 2, 6], [0, 1, 2, 1, 0]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('name,sizes,route', MIXED, ids=[m[0] for m in MIXED])
def test_graphs_of_different_sizes_in_one_launch(name, sizes, route, dtype):
    '''Three graphs of different sizes, the largest on a boundary, in one launch of each family.
    The template arguments and the workgroup are chosen by the batch's maxima, so an utterance's
    "own" call is a one-utterance batch over the same three graphs: the same kernel, and the
    result must be the same bit for bit -- a wave or a workgroup must not see its neighbours.'''
    graphs, arrays = [], []
    for k, S in enumerate(sizes):
        g = ft.make_graph(S, ft.offsets(3, S), 1000 + k, 0, NP[dtype])
        arrays.append(g)
        graphs.append(beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                               list(range(S))))
    rng = np.random.RandomState(len(name))
    llhs = [(rng.randn(T, sizes[k]) * 3).astype(NP[dtype]) for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    assert route_of(batch, dtype, 0) == route
    assert hk.fused_ok(batch) == (_hip.fb_family(route) == WAVE)
    gam, _, _, ln, _ = hk.forward_backward(batch, packed(llhs), want_lognorm=True)
    assert batch.last_alpha_is_log == (_hip.fb_family(route) != WAVE)
    gam, ln = npy(gam), npy(ln)
    off = 0
    for u, (T, k) in enumerate(zip(MIXED_LENS, MIXED_GIDS)):
        mine = gam[off:off + T * sizes[k]]
        off += T * sizes[k]
        own = hk.HmmBatch(graphs, [k], [T], dtype)
        assert route_of(own, dtype, 0) == route
        g1, _, _, ln1, _ = hk.forward_backward(own, tt(llhs[u]).reshape(-1), want_lognorm=True)
        np.testing.assert_array_equal(mine, npy(g1), err_msg=f'utterance {u}')
        np.testing.assert_array_equal(ln[u], npy(ln1)[0], err_msg=f'utterance {u}')
        t64 = ft.truth(arrays[k], [llhs[u]])
        t32 = ft.truth(arrays[k], [llhs[u]], dtype=np.float32) if dtype == torch.float32 else None
        check = Checker(dtype, t64, t32)
        check(mine, 'gamma', f'utterance {u}', pick=lambda a: a[0])
        check(ln[u:u + 1], 'lognorm', f'utterance {u}', tight=1e-11)


# --- Viterbi -----------------------------------------------------------------------------------
# Integer-valued inputs: every sum is exact in float32, the float32 and float64 oracle paths are
# the same (tests/test_fb_routes_host.py), and ties between sources are frequent -- the path must
# be the oracle's exactly.  S: four lanes a state (4 S <= 512), one state per thread, the strided
# loop; more than 4 arcs a state spread one state's sources over all four lanes of its quad; the
# lengths sit around the back-pointer chunk of 32 frames.

VCase = namedtuple('VCase', 'S nO seed')
VCASES = [VCase(S_, nO_, 100 * k_ + nO_)
          for k_, (S_, nOs_) in enumerate([(1, (2,)), (2, (2,)), (7, (2, 3, 5, 8, 12)), (64, (2, 5, 12)),
                                           (128, (2, 3, 5, 8, 12)), (129, (2, 3, 5, 8, 12)),
                                           (256, (3, 8, 12)), (257, (2, 5, 12)), (300, (2, 3, 5, 8, 12))])
          for nO_ in nOs_]
# every arc present: the arc lists of the larger one do not fit beside the trellis in LDS
# (arcs_in_lds = 0), on the quad scheme and on one state per thread
VCASES += [VCase(100, 100, 901), VCase(130, 130, 902)]


def vcase_offsets(vc):
    return ft.offsets(vc.nO, vc.S)


def vcase_graph(vc, dtype=np.float64):
    return ft.make_graph(vc.S, vcase_offsets(vc), vc.seed, 0, dtype, integer=True)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('vc', VCASES, ids=lambda vc: f'S{vc.S}-O{vc.nO}')
def test_viterbi_path_is_the_oracles(vc, dtype):
    S = vc.S
    g = vcase_graph(vc, NP[dtype])
    ids = ft.pdf_ids(S, 'repeat', S + 3, vc.seed)
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in ids])
    lens = list(ft.VITERBI_LENGTHS)
    llhs = ft.viterbi_inputs(S, lens, vc.seed, NP[dtype])
    want = np.concatenate([ft.best_path(g, l) for l in llhs])
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    flat = packed(llhs)
    np.testing.assert_array_equal(npy(hk.viterbi(batch, flat)), want)
    np.testing.assert_array_equal(npy(hk.viterbi(batch, flat, map_pdf=True)), ids[want])


VMIXED_SIZES, VMIXED_LENS, VMIXED_GIDS = (7, 129, 300), [33, 65, 32, 2, 64, 1], [0, 1, 2, 0, 2, 1]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_viterbi_on_graphs_of_different_sizes_in_one_launch(dtype):
    'The workgroup is sized by the largest graph: the small one then runs four lanes a state.'
    graphs, arrays = [], []
    for k, S in enumerate(VMIXED_SIZES):
        g = ft.make_graph(S, ft.offsets(5, S), 2000 + k, 0, NP[dtype], integer=True)
        arrays.append(g)
        graphs.append(beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                               list(range(S))))
    llhs = [ft.viterbi_inputs(VMIXED_SIZES[k], [T], 2100 + u, NP[dtype])[0]
            for u, (T, k) in enumerate(zip(VMIXED_LENS, VMIXED_GIDS))]
    want = np.concatenate([ft.best_path(arrays[k], l) for l, k in zip(llhs, VMIXED_GIDS)])
    batch = hk.HmmBatch(graphs, VMIXED_GIDS, VMIXED_LENS, dtype)
    np.testing.assert_array_equal(npy(hk.viterbi(batch, packed(llhs))), want)
