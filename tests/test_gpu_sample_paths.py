"""The posterior path sampler (csrc/hmm_sample.hip) against the float64 truth of
tests/sample_truth.py, on graphs that sit on the boundaries of its forms.

 * Stepwise exactness: every path is walked from its last frame back; at each frame the
   kernel's choice, given the kernel's own next state, must be the term whose interval of the
   truth's CDF holds the uniform -- the interval widened by `tol` (1e-5 float32, 1e-10 float64) on
   at most 1 % of the steps of a case, never a term of weight 0.
 * The trellis: exp(alpha_ws) within `tol` of the truth's normalised forward values.
 * One static table: each case names the forms `beer_hmm_sample_route` must report for it in
   either precision, and the table as a whole reaches every value the route can take.
 * Edges (uniforms 0 and 1 - 2^-53, an utterance the graph cannot end, T = 1), the statistics of
   4096 draws of one launch, and the model level: evidence_lower_bound / accumulate_elbo with
   `sample=`, `sample_paths_batch`, `beer hmm decode --nsamples`."""

import io
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import fb_truth as ft
import sample_truth as st
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
A, Q = st.ARCS_LDS, st.QUAD

# lengths: around the back-trace chunks of 32, 8 and 2 frames
LONG = tuple(ft.VITERBI_LENGTHS) + (7, 8, 9, 3)

# S, offsets, hub members, utterances (a number: fb_truth.lengths; 'long': LONG), pdf-id flavour,
# the forms of the route in float64 and in float32 (chunk | arcs in LDS | four lanes a state)
Case = namedtuple('Case', 'S nO hub nutt flavour f64 f32 seed')
CASES = []


def add(S, nO, f64, f32=None, hub=0, nutt=None):
    i = len(CASES)
    CASES.append(Case(S, nO, hub, nutt or (1, 5, 9)[i % 3], ft.FLAVOURS[i % 3], f64,
                      f64 if f32 is None else f32, 300 + i))


# small graphs, degrees 2 / 3 / 4 / 8: one lane scans a row (S <= 8: the last frame too)
add(1, 2, 32 | A | Q)
add(3, 2, 32 | A | Q)
add(3, 3, 32 | A | Q)
add(8, 2, 32 | A | Q, nutt='long')
add(8, 3, 32 | A | Q)
add(8, 4, 32 | A | Q)
add(8, 8, 32 | A | Q)
# the last frame by the wave: 64 states one block of lanes, 65 two
add(64, 2, 32 | A | Q)
add(64, 8, 32 | A | Q)
add(65, 3, 32 | A | Q)
add(65, 4, 32 | A | Q)
add(65, 8, 32 | A | Q)
# rows of 9 and 12 arcs: the wave scan between the frames
add(64, 9, 32 | A | Q)
add(124, 12, 32 | A | Q)
# hubs: a phone start has an arc from every phone end -- rows of 40 / 64 / 100 (+ degree) arcs
add(120, 3, 32 | A | Q, hub=40)
add(256, 3, 8, 8 | A, hub=64)
add(300, 3, 8, hub=100)
# every arc present: the lists do not fit LDS beside the chunk; rows of 100 / 128 arcs
add(100, 100, 32 | Q, nutt=5)
add(128, 128, 8 | Q, nutt=5)
# 125 .. 128 states: a chunk of 8 frames, still four lanes a state; beyond, one thread a state
add(125, 3, 8 | A | Q)
add(128, 3, 8 | A | Q, nutt='long')
add(129, 3, 8 | A)
add(200, 4, 8 | A, nutt='long')
add(508, 2, 8 | A)
# beyond 508 states: a chunk of 2 frames; 12 arcs a state no longer fit
add(509, 3, 2 | A, nutt='long')
add(600, 12, 2)


def case_id(c):
    return f'{c.seed}-S{c.S}-O{c.nO}-hub{c.hub}-n{c.nutt}-{c.flavour}'


def test_the_cases_reach_every_value_of_the_route():
    'Static: forms of the table x samples per workgroup = everything the route can return.'
    forms = {c.f64 for c in CASES} | {c.f32 for c in CASES}
    assert forms == {32 | A | Q, 32 | Q, 8 | A | Q, 8 | Q, 8 | A, 8, 2 | A, 2}
    assert {1 if n == 1 else 4 for n in NSAMPLES} == {1, 4}


NSAMPLES = (1, 3)


def packed(llhs):
    return torch.cat([tt(l).reshape(-1) for l in llhs])


def build(case, dtype):
    g = ft.make_graph(case.S, ft.offsets(case.nO, case.S), case.seed, case.hub, NP[dtype])
    S_total = case.S if case.flavour == 'perm' else case.S + 3
    ids = ft.pdf_ids(case.S, case.flavour, S_total, case.seed)
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in ids])
    if g['hub'] is not None:
        E, a, B, c = g['hub']
        graph.set_hub(E, tt(a), B, tt(c))
    return g, ids, graph


def hold(g_of, llhs, lens, U, path, alpha, tol, what):
    '''Trellis and paths of a batch against the truth: (steps, widened, largest deviation of
    exp(alpha)).  `g_of[u]`: the graph arrays of utterance u.'''
    path, alpha = npy(path), npy(alpha)
    steps = widened = 0
    dev = 0.
    f0 = e0 = 0
    for u, T in enumerate(lens):
        g, S = g_of[u], g_of[u]['S']
        la = st.forward(g, llhs[u])
        got = alpha[e0:e0 + T * S].reshape(T, S)
        assert not np.isnan(got).any(), f'{what} utterance {u}: NaN in the trellis'
        d = np.abs(np.exp(got) - np.exp(la)).max()
        assert d <= tol, f'{what} utterance {u}: exp(alpha) off by {d:.3e} > {tol:.1e}'
        dev = max(dev, d)
        mine = path[:, f0:f0 + T]
        n, w = st.check_paths(g, llhs[u], U[:, f0:f0 + T], mine, tol, la=la)
        steps, widened = steps + n, widened + w
        assert all(st.valid_path(g, p) for p in mine), f'{what} utterance {u}: invalid path'
        f0, e0 = f0 + T, e0 + T * S
    return steps, widened, dev


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_paths_follow_the_rule_step_by_step(case, dtype):
    g, ids, graph = build(case, dtype)
    lens = list(LONG) if case.nutt == 'long' else ft.lengths(case.nutt, case.seed)
    _, llhs = ft.inputs(g, lens, np.arange(case.S), case.S, 1., case.seed, NP[dtype])
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    flat = packed(llhs)
    rng = np.random.RandomState(case.seed)
    steps = widened = 0
    for n in NSAMPLES:
        want = (case.f64 if dtype == torch.float64 else case.f32) | (1 if n == 1 else 4) << 12
        route = hk.sample_route(batch, n)
        assert route == want, f'route {route:#x}, the table says {want:#x}'
        assert route == st.route_formula(case.S, batch.struct.max_arcs, flat.element_size(), n)
        U = rng.random_sample((n, sum(lens)))
        path, alpha = hk.sample_paths(batch, flat, tt(U), return_trellis=True)
        assert path.shape == (n, sum(lens)) and path.dtype == torch.int64
        s, w, dev = hold([g] * len(lens), llhs, lens, U, path, alpha, TOL[dtype], f'n={n}')
        steps, widened = steps + s, widened + w
        print(f'{case_id(case)} n={n}: {s} steps, {w} widened, exp(alpha) off by {dev:.2e}')
        # the same draws as pdf ids
        mapped = hk.sample_paths(batch, flat, tt(U), map_pdf=True)
        np.testing.assert_array_equal(npy(mapped), ids[npy(path)])
    assert widened <= 0.01 * steps, f'{widened} of {steps} steps needed the widened interval'


MIXED_SIZES, MIXED_LENS, MIXED_GIDS = (7, 65, 129), [33, 65, 32, 2, 64, 1], [0, 1, 2, 0, 2, 1]


@DTYPES
def test_graphs_of_different_sizes_in_one_launch(dtype):
    'Alignment-graph style: the forms follow the largest graph, every utterance its own.'
    graphs, arrays = [], []
    for k, S in enumerate(MIXED_SIZES):
        g = ft.make_graph(S, ft.offsets(3 + 3 * k, S), 2000 + k, 0, NP[dtype])
        arrays.append(g)
        graphs.append(beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                               list(range(S))))
    rng = np.random.RandomState(5)
    llhs = [(rng.randn(T, MIXED_SIZES[k]) * 3).astype(NP[dtype])
            for T, k in zip(MIXED_LENS, MIXED_GIDS)]
    batch = hk.HmmBatch(graphs, MIXED_GIDS, MIXED_LENS, dtype)
    for n in NSAMPLES:
        assert hk.sample_route(batch, n) == (8 | A) | (1 if n == 1 else 4) << 12
        U = rng.random_sample((n, sum(MIXED_LENS)))
        path, alpha = hk.sample_paths(batch, packed(llhs), tt(U), return_trellis=True)
        steps, widened, _ = hold([arrays[k] for k in MIXED_GIDS], llhs, MIXED_LENS, U, path,
                                 alpha, TOL[dtype], f'n={n}')
        assert widened <= 0.01 * steps


# --- validity and edges ------------------------------------------------------------------------

@DTYPES
def test_extreme_uniforms_give_valid_paths(dtype):
    'u = 0 and u = 1 - 2^-53 on every frame: the first and the last term of non-zero weight.'
    for S, nO, hub in [(8, 3, 0), (120, 3, 40)]:
        g = ft.make_graph(S, ft.offsets(nO, S), 77, hub, NP[dtype])
        graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                         list(range(S)))
        lens = [1, 2, 9, 33]
        _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 78, NP[dtype])
        batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
        U = np.stack([np.zeros(sum(lens)), np.full(sum(lens), 1 - 2. ** -53)])
        path, alpha = hk.sample_paths(batch, packed(llhs), tt(U), return_trellis=True)
        hold([g] * len(lens), llhs, lens, U, path, alpha, TOL[dtype], f'S={S}')
        f0 = 0
        for l, T in zip(llhs, lens):                    # and they are the truth's own paths
            np.testing.assert_array_equal(npy(path)[:, f0:f0 + T], st.sample(g, l, U[:, f0:f0 + T]))
            f0 += T


@DTYPES
def test_an_utterance_the_graph_cannot_end_gives_the_documented_fallback(dtype):
    '''final is finite on the last state only, which no utterance of 1 or 2 frames reaches: the
    total of the last frame is 0 -> state 0; a frame whose likelihoods are all -inf leaves every
    total 0 -> the first arc of every row.  Defined behaviour: finite indices, no NaN.'''
    S = 8
    g = ft.make_graph(S, (0, 1), 5, 0, NP[dtype])
    g['final'][:] = -np.inf
    g['final'][S - 1] = 0.
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), list(range(S)))
    lens = [1, 2, 12, 5]
    _, llhs = ft.inputs(g, lens, np.arange(S), S, 1., 6, NP[dtype])
    llhs[3][2] = -np.inf                                # nothing explains frame 2 of utterance 3
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    U = np.random.RandomState(7).random_sample((3, sum(lens)))
    path, alpha = hk.sample_paths(batch, packed(llhs), tt(U), return_trellis=True)
    path, alpha = npy(path), npy(alpha)
    assert not np.isnan(alpha).any()
    assert ((path >= 0) & (path < S)).all()
    assert (path[:, 0] == 0).all() and (path[:, 2] == 0).all()          # T = 1, T = 2: state 0
    f0 = 0
    for l, T in zip(llhs, lens):
        np.testing.assert_array_equal(path[:, f0:f0 + T], st.sample(g, l, U[:, f0:f0 + T]))
        st.check_paths(g, l, U[:, f0:f0 + T], path[:, f0:f0 + T], TOL[dtype])
        f0 += T
    # utterance 2 (12 frames) does reach the last state: an ordinary draw
    assert (path[:, 3 + 11] == S - 1).all()
    # utterance 3: from frame 2 on nothing is reachable
    assert np.isinf(alpha[-3 * S:]).all()


@DTYPES
def test_one_frame(dtype):
    S = 65
    g = ft.make_graph(S, ft.offsets(3, S), 9, 0, NP[dtype])
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), list(range(S)))
    _, llhs = ft.inputs(g, [1], np.arange(S), S, 1., 9, NP[dtype])
    batch = hk.HmmBatch([graph], [0], [1], dtype)
    U = np.random.RandomState(9).random_sample((3, 1))
    path, alpha = hk.sample_paths(batch, packed(llhs), tt(U), return_trellis=True)
    hold([g], llhs, [1], U, path, alpha, TOL[dtype], 'T=1')
    assert set(npy(path).reshape(-1)) <= {0, 1, 2}      # init is finite on the first three states


def test_arguments_are_checked():
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), [0, 1, 2])
    batch = hk.HmmBatch([graph], [0], [4], torch.float64)
    flat = torch.zeros(12, dtype=torch.float64, device='cuda')
    for bad in (torch.rand(1, 5, dtype=torch.float64), torch.rand(1, 4), torch.rand(4, dtype=torch.float64)):
        with pytest.raises(ValueError):
            hk.sample_paths(batch, flat, bad)
    with pytest.raises(ValueError):
        hk.sample_paths(batch, flat, nsamples=0)
    rc = _hip.lib().beer_hmm_sample_paths(_hip.F64, batch.ref(), _hip.ptr(flat), None, 1, None,
                                          None, 0, None)
    assert rc == _hip.EINVAL
    gen = torch.Generator(device='cuda')
    gen.manual_seed(3)
    a = hk.sample_paths(batch, flat, nsamples=5, generator=gen)
    gen.manual_seed(3)
    b = hk.sample_paths(batch, flat, nsamples=5, generator=gen)
    assert a.shape == (5, 4) and torch.equal(a, b)


# --- statistics on the device --------------------------------------------------------------------

@DTYPES
def test_frequencies_of_4096_draws_of_one_launch(dtype):
    g, llh, U = st.stat_case()
    g = {k: (v.astype(NP[dtype]) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    llh = llh.astype(NP[dtype])
    S = st.STAT_S
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']), list(range(S)))
    batch = hk.HmmBatch([graph], [0], [st.STAT_T], dtype)
    path = npy(hk.sample_paths(batch, tt(llh).reshape(-1), tt(U)))
    gam, xi = st.posteriors(g, llh)
    fg, fx = st.path_frequencies(path, S)
    dev_g, dev_x = np.abs(fg - gam).max(), np.abs(fx - xi).max()
    print(f'largest deviation: states {dev_g:.4f}, pairs {dev_x:.4f} (bound {st.STAT_BOUND:.4f})')
    assert dev_g <= st.STAT_BOUND and dev_x <= st.STAT_BOUND
    # every draw is the truth's own
    steps, widened = st.check_paths(g, llh, U[:256], path[:256], TOL[dtype])
    assert widened <= 0.01 * steps


# --- model level ---------------------------------------------------------------------------------

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
        model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet',
                                    train_transitions=kind == 'learned')
        assert type(model) is beer.PhoneLoop and (model.transitions is not None) == (kind == 'learned')
    return model.double().to('cuda')


KINDS = ('hmm', 'phoneloop', 'bigram', 'learned')


def utterances(lens, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randn(T, D) * 1.5).to('cuda') for T in lens]


def same_elbo(a, b, exact=True, what=''):
    if exact:
        assert float(a) == float(b), f'{what}: {float(a)!r} != {float(b)!r}'
    else:
        np.testing.assert_allclose(float(a), float(b), rtol=1e-10, err_msg=what)
    assert set(a._acc_stats) == set(b._acc_stats)
    for p, sa in a._acc_stats.items():
        if exact:
            assert torch.equal(sa, b._acc_stats[p]), f'{what}: statistics differ'
        else:
            np.testing.assert_allclose(npy(sa), npy(b._acc_stats[p]), rtol=1e-10, atol=1e-12,
                                       err_msg=what)


def own_path(model, X, u):
    'hk.sample_paths on the per-state log-likelihoods the model computes for X.'
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    batch = hk.HmmBatch([model.graph], [0], [len(X)], pc_all.dtype)
    return hk.sample_paths(batch, hk.gather(batch, pc_all, 1.), u.reshape(1, -1))[0]


@pytest.mark.parametrize('kind', KINDS)
def test_elbo_with_a_drawn_path_is_the_elbo_of_that_path(kind):
    model = make_model(kind)
    if kind == 'phoneloop':
        dg = model.graph.device_graph(torch.float64)
        assert getattr(getattr(dg, 'lowdeg', None), 'n_hubs', 0) >= 1
    (X,) = utterances([57], 1)
    u = torch.rand(len(X), dtype=torch.float64, device='cuda',
                   generator=torch.Generator(device='cuda').manual_seed(4))
    path = own_path(model, X, u)
    drawn = beer.evidence_lower_bound(model, X, datasize=1000, sample=u)
    given = beer.evidence_lower_bound(model, X, datasize=1000, state_path=path)
    same_elbo(drawn, given, what=kind)
    viterbi = beer.evidence_lower_bound(model, X, datasize=1000, viterbi=True)
    assert float(viterbi) != float(drawn)               # (a drawn path is not the best one)
    # sample=True draws from the default generator: two calls differ, a reseeded one repeats
    torch.manual_seed(11)
    a = beer.evidence_lower_bound(model, X, sample=True)
    b = beer.evidence_lower_bound(model, X, sample=True)
    torch.manual_seed(11)
    c = beer.evidence_lower_bound(model, X, sample=True)
    assert float(a) == float(c) and float(a) != float(b)


@pytest.mark.parametrize('kind', KINDS)
def test_accumulate_elbo_with_drawn_paths_is_the_sum_over_the_utterances(kind):
    model = make_model(kind)
    lens = [23, 40, 9, 31]
    utts = utterances(lens, 2)
    total = sum(lens)
    u = torch.rand(total, dtype=torch.float64, device='cuda',
                   generator=torch.Generator(device='cuda').manual_seed(5))
    batched = beer.accumulate_elbo(model, utts, datasize=total, sample=u)
    one_by_one = beer.evidence_lower_bound(datasize=total)
    f0 = 0
    for X in utts:
        one_by_one = one_by_one + beer.evidence_lower_bound(model, X, datasize=total,
                                                            sample=u[f0:f0 + len(X)])
        f0 += len(X)
    np.testing.assert_allclose(float(batched), float(one_by_one) + 0., rtol=1e-10)
    for p, s in one_by_one._acc_stats.items():
        np.testing.assert_allclose(npy(batched._acc_stats[p]), npy(s), rtol=1e-10, atol=1e-12)
    # in sub-batches (a small max_frames): the same uniforms reach the same frames
    split = beer.accumulate_elbo(model, utts, datasize=total, sample=u, max_frames=45)
    same_elbo(split, batched, exact=False, what='sub-batches')


def test_sample_paths_batch_is_sample_paths_per_utterance():
    model = make_model('phoneloop')
    lens = [23, 40, 9]
    utts = utterances(lens, 3)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(6)
    got = beer.sample_paths_batch(model, utts, nsamples=2, generator=gen)
    gen.manual_seed(6)
    U = torch.rand(2, sum(lens), dtype=torch.float64, device='cuda', generator=gen)
    assert [tuple(p.shape) for p in got] == [(2, T) for T in lens]
    f0 = 0
    for X, p in zip(utts, got):
        pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
        batch = hk.HmmBatch([model.graph], [0], [len(X)], pc_all.dtype)
        want = hk.sample_paths(batch, hk.gather(batch, pc_all, 1.), U[:, f0:f0 + len(X)],
                               map_pdf=True)
        assert torch.equal(p, want)
        f0 += len(X)
    gen.manual_seed(6)
    single = model.sample_path(utts[0], nsamples=2, generator=gen)
    assert single.shape == (2, lens[0]) and not single.is_cuda


def run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_decode_nsamples(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    run(['dataset', 'create', str(tmp_path), feats, ds])
    out = run(['hmm', 'decode', '--nsamples', '2', '--seed', '1', mdl, ds])
    lines = out.strip().split('\n')
    assert [l.split(' ', 1)[0] for l in lines] == \
        [f'utt{i}-{k}' for i in range(3) for k in (1, 2)]
    assert all(len(l.split()) >= 2 for l in lines)
    assert run(['hmm', 'decode', '--nsamples', '2', '--seed', '1', mdl, ds]) == out
    assert run(['hmm', 'decode', '--nsamples', '2', '--seed', '2', mdl, ds]) != out
    per_frame = run(['hmm', 'decode', '--per-frame', '--nsamples', '1', '--seed', '1', mdl, ds])
    assert [len(l.split()) - 1 for l in per_frame.strip().split('\n')] == [35, 50, 41]
    # without --nsamples the command is what it was
    plain = run(['hmm', 'decode', mdl, ds]).strip().split('\n')
    assert [l.split(' ', 1)[0] for l in plain] == ['utt0', 'utt1', 'utt2']
