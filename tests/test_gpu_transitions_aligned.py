'''Learned transition probabilities trained against alignment graphs, on the GPU: the counts by
category of every forward-backward path against the float64 numpy truth of
tests/aligned_truth.py, conservation, the outputs that must not move, the refresh of the bound
image, Viterbi / state paths, one VB step, recovery of known self-loops, the captured
iteration and the command line.

Tolerances (tests/test_gpu_transitions.py): counts within 1e-10 (float64) / 1e-5 (float32) of
the truth relative to the largest count; hard counts exactly equal.'''

import ctypes
import functools
import io
import os
import pickle
import sys
import zipfile

import numpy as np
import pytest
import torch

from aligned_truth import (CategoryMap, alignment_set, expected_log_probs, loop_model,
                           utterance_counts)

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import main as cli_main
from beer_amd.inference.batch import accumulate_elbo

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DTYPES = [torch.float64, torch.float32]
SCALE = .8


def _tol(dtype):
    return 1e-10 if dtype == torch.float64 else 1e-5


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _transcription(n_speech, n_nonspeech, rng):
    seq = [f's{rng.randint(3)}' for _ in range(n_speech)] + ['n0'] * n_nonspeech
    rng.shuffle(seq)
    return seq


class Case:
    '''The shared case of a dtype: a loop of 3 + 1 units, transcriptions of 3, 14 (twice, ONE
    graph object), 75, 150 and 270 states, every utterance with at least twice as many frames
    as its graph has states (distinct lengths), and the truth of every utterance.  Units s1 / s2
    may occur, unit names beyond the loop do not exist: the categories no transcription names
    are those of the units a draw leaves out -- `unused` lists them per subset.'''

    def __init__(self, dtype):
        rng = np.random.RandomState(5)
        self.dtype = dtype
        model, self.units = loop_model(dtype, seed=3)
        self.model = model.to(DEV)
        # (posteriors away from the prior: E[ln a] differs from category to category)
        g = torch.Generator().manual_seed(1)
        for p in model.transitions.parameters_of_groups():
            conc = p.posterior.params.concentrations
            conc.add_(torch.rand(conc.shape, generator=g, dtype=torch.float64).to(conc) * 3)
        model._on_transitions_update()
        self.tmap = CategoryMap(model)
        self.seqs = [['s0'], ['s0', 'n0', 's0', 's0'], _transcription(20, 3, rng),
                     _transcription(45, 3, rng), _transcription(85, 3, rng)]
        self.gset = alignment_set(self.units, self.seqs)
        self.bound = model.bind_alignment_graphs(self.gset)
        assert [g.n_states for g in self.bound] == [3, 14, 75, 150, 270]
        # utterance -> graph: the two 14-state utterances share one graph object
        self.graph_of = [0, 1, 1, 2, 3, 4]
        self.lens = [7, 40, 33, 160, 310, 545]
        self.X = torch.from_numpy(rng.randn(sum(self.lens), 4) * 1.5).to(DEV, dtype)
        self.off = np.concatenate([[0], np.cumsum(self.lens)])
        self.pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(self.X))
        self.log_a = expected_log_probs(model.transitions)
        pc = self.pc_all.double().cpu().numpy() * SCALE
        self.counts, self.gammas = [], []
        for u, gi in enumerate(self.graph_of):
            dense = self.gset[gi].to_dense()
            llh = pc[self.off[u]:self.off[u + 1]][:, np.asarray(dense.pdf_id_mapping)]
            c, gamma = utterance_counts(self.tmap, self.log_a, self.seqs[gi], dense, llh)
            self.counts.append(c)
            self.gammas.append(gamma)

    def subset(self, utts):
        '(graphs per utterance, lengths, frames, pc_all rows, truth, unused categories) of `utts`.'
        rows = np.concatenate([np.arange(self.off[u], self.off[u + 1]) for u in utts])
        rows = torch.from_numpy(rows).to(DEV)
        graphs = [self.bound[self.graph_of[u]] for u in utts]
        used = set()
        for u in utts:
            for name in self.seqs[self.graph_of[u]]:
                used.update(c for (n, _, _), c in self.tmap.intra.items() if n == name)
                used.add(self.tmap.exit[name])
        unused = sorted(set(range(self.tmap.n_categories)) - used)
        return (graphs, [self.lens[u] for u in utts], self.X[rows], self.pc_all[rows].contiguous(),
                sum(self.counts[u] for u in utts), unused)

    def batch(self, graphs, lens, lowdeg=True):
        uniq, ids, seen = [], [], {}
        for g in graphs:
            if id(g) not in seen:
                seen[id(g)] = len(uniq)
                uniq.append(g)
            ids.append(seen[id(g)])
        self.bound.refresh(self.dtype)
        return hk.HmmBatch(uniq, ids, lens, self.dtype, lowdeg=lowdeg)


@functools.lru_cache(maxsize=None)
def case(dtype):
    return Case(dtype)


WAVE = [0, 1, 2, 3, 4]                       # the mixed batch of the one-wave kernels
SUBSETS = {'mixed': WAVE, '3': [0], '14': [1], '75': [3], '150': [4]}


def _check(got, want, unused, dtype, what):
    got = got.cpu().numpy()
    print(f'{what}: relative error {_rel(got, want):.3e}')
    assert _rel(got, want) < _tol(dtype), (what, _rel(got, want))
    assert not got[unused].any(), (what, 'a category no transcription names got counts')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('which', list(SUBSETS))
def test_counts_of_the_one_wave_kernels(dtype, which):
    'Fused call, packed call and the log-space twin alone, mixed batch and every size alone.'
    c = case(dtype)
    graphs, lens, _, pc_all, want, unused = c.subset(SUBSETS[which])
    batch = c.batch(graphs, lens)
    assert hk.fused_ok(batch) and batch.bound_set is c.bound
    assert batch.struct.n_graphs == len(set(map(id, graphs)))
    tc = hk.posteriors_fused(batch, pc_all, SCALE, want_transitions=True)[3]
    assert tc[0] == 'cat'
    _check(tc[1], want, unused, dtype, 'fused')
    pc = hk.gather(batch, pc_all, SCALE)
    tc = hk.forward_backward_counts(batch, pc)[4]
    _check(tc[1], want, unused, dtype, 'packed')
    old = _hip.set_option('fb_log', 1)
    try:
        with hk.counting_log_space() as n:
            tf = hk.posteriors_fused(batch, pc_all, SCALE, want_transitions=True)[3]
            tp = hk.forward_backward_counts(batch, pc)[4]
        assert int(n.count) == 2 * len(lens)
    finally:
        _hip.set_option('fb_log', old)
    _check(tf[1], want, unused, dtype, 'fused, log space')
    _check(tp[1], want, unused, dtype, 'packed, log space')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('utts, lowdeg', [([5], True), ([0, 1, 2, 3, 4, 5], True), (WAVE, False)],
                         ids=['270', 'mixed', 'general'])
def test_counts_beyond_the_one_wave_kernels(dtype, utts, lowdeg):
    '''A 270-state transcription alone and in the mixed batch: one thread per state
    (fb_lowdeg_kernel); the mixed batch without its low-degree images: the general kernel
    (fb_utterance), which graphs of more than 512 states take.'''
    c = case(dtype)
    graphs, lens, _, pc_all, want, unused = c.subset(utts)
    batch = c.batch(graphs, lens, lowdeg=lowdeg)
    assert not hk.fused_ok(batch)
    tc = hk.forward_backward_counts(batch, hk.gather(batch, pc_all, SCALE))[4]
    assert tc[0] == 'cat'
    _check(tc[1], want, unused, dtype, 'beyond the one-wave kernels')


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_source_state_keeps_its_posterior_mass(dtype):
    '''Conservation at acoustic scale 0.8: the counts of a state's categories add up to the
    posteriors of its pdf id summed over all frames (state_resps / scale).'''
    c = case(dtype)
    graphs, lens, _, pc_all, _, _ = c.subset(WAVE)
    batch = c.batch(graphs, lens)
    sr, _, _, tc = hk.posteriors_fused(batch, pc_all, SCALE, want_transitions=True)
    counts = tc[1].cpu().numpy()
    mass = sr.double().sum(dim=0).cpu().numpy() / SCALE
    tr, ids = c.model.transitions, np.asarray(c.model.graph.pdf_id_mapping)
    by_state = np.zeros(c.model.graph.n_states)
    np.add.at(by_state, np.asarray(tr.cat_src), counts)
    owners = sorted(set(tr.cat_src))
    err = np.abs(by_state[owners] - mass[ids[owners]]).max() / counts.max()
    print(f'conservation: {err:.3e}')
    assert err < _tol(dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_nothing_else_moves(dtype):
    '''The mapped call and the plain call on the same refreshed image: bit-identical
    state_resps, utt_llh, frame_llh and gamma0_sum, and the packed calls' gamma.  (gamma0_sum
    is a sum of fp64 atomics over the utterances: a chain starts in ONE state, whose first-frame
    posterior is 1 to the last bit or two, and the utterances' lengths differ by far, so the
    few terms meet in the same order in both launches.)'''
    c = case(dtype)
    graphs, lens, _, pc_all, _, _ = c.subset(WAVE)
    batch = c.batch(graphs, lens)
    out = []
    for mapped in (False, True):
        llh = torch.zeros(len(lens), dtype=torch.float64, device=DEV)
        frame = torch.empty(sum(lens), dtype=dtype, device=DEV)
        g0 = torch.zeros(max(batch.n_states), dtype=torch.float64, device=DEV)
        res = hk.posteriors_fused(batch, pc_all, SCALE, utt_llh=llh, frame_llh=frame,
                                  want_transitions=mapped, gamma0_sum=g0)
        out.append((res[0], llh, frame, g0))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[0][3].sum()) == pytest.approx(len(lens), rel=1e-6)
    pc = hk.gather(batch, pc_all, SCALE)
    assert torch.equal(hk.forward_backward(batch, pc)[0], hk.forward_backward_counts(batch, pc)[0])
    old = _hip.set_option('fb_log', 1)
    try:
        assert torch.equal(hk.forward_backward(batch, pc)[0],
                           hk.forward_backward_counts(batch, pc)[0])
    finally:
        _hip.set_option('fb_log', old)


def _image_weights(blob_h, struct, base, dtype):
    '''{array name: (sources, destinations, weights)} of one graph of an arena image read back
    to the host: both CSR orders of the graph and of its low-degree image.'''
    np_dt = np.float64 if dtype == torch.float64 else np.float32

    def arr(ptr, n, dt):
        return np.frombuffer(blob_h, dtype=dt, count=n, offset=ptr - base)
    S, A = struct.n_states, struct.n_arcs
    ld = _hip.GraphLowDeg.from_buffer_copy(
        blob_h[struct.lowdeg - base:struct.lowdeg - base + ctypes.sizeof(_hip.GraphLowDeg)])
    rows = lambda ptr: np.repeat(np.arange(S), np.diff(arr(ptr, S + 1, np.int32)))   # noqa: E731
    return {
        'in_w': (arr(struct.in_src, A, np.int32), arr(struct.in_dst, A, np.int32),
                 arr(struct.in_w, A, np_dt)),
        'out_w': (arr(struct.out_src, A, np.int32), arr(struct.out_dst, A, np.int32),
                  arr(struct.out_w, A, np_dt)),
        'lowdeg in_w': (arr(ld.in_src, A, np.int32), rows(ld.in_ptr), arr(ld.in_w, A, np_dt)),
        'lowdeg out_w': (rows(ld.out_ptr), arr(ld.out_dst, A, np.int32), arr(ld.out_w, A, np_dt)),
    }


@pytest.mark.parametrize('dtype', DTYPES)
def test_refresh_writes_the_new_expected_log_probabilities(dtype):
    '''After one update of the transitions' group every weight of the bound image is E[ln a] of
    its arc's category, exactly, in both CSR orders and in the low-degree image; the GraphSet's
    own image is what it was.'''
    model, units = loop_model(dtype, seed=3)
    model = model.to(DEV)
    seqs = [['s0'], ['s0', 'n0', 's0', 's0'], ['n0', 's1', 's2', 'n0', 's1']]
    gset = alignment_set(units, seqs)
    bound = model.bind_alignment_graphs(gset)
    own_before = gset.device_image(dtype)[0].clone()
    lens = [9, 35, 50]
    X = torch.from_numpy(np.random.RandomState(2).randn(sum(lens), 4)).to(DEV, dtype)
    tr = model.transitions
    optim = beer.VBConjugateOptimizer([tr.parameters_of_groups()], lrate=1.)
    optim.init_step()
    elbo = accumulate_elbo(model, (X, lens), inference_graphs=bound)
    before = bound.device_image(dtype)[0].clone()
    elbo.backward()
    optim.step()
    bound.refresh(dtype)
    torch.cuda.synchronize()
    blob, structs = bound.device_image(dtype)
    assert not torch.equal(blob, before)
    blob_h = blob.cpu().numpy().tobytes()
    log_a = tr.log_probs().to(dtype).cpu().numpy()
    for u in range(len(seqs)):
        st = structs[u]
        src, dst = bound[u].arcs
        cat_of = {(int(a), int(b)): int(k) for a, b, k in zip(src, dst, bound[u].arc_categories)}
        for name, (s, d, w) in _image_weights(blob_h, st, blob.data_ptr(), dtype).items():
            want = log_a[[cat_of[(int(a), int(b))] for a, b in zip(s, d)]]
            np.testing.assert_array_equal(w, want, err_msg=f'graph {u}, {name}')
    assert torch.equal(gset.device_image(dtype)[0], own_before)
    assert bound.device_image(dtype)[0].data_ptr() != gset.device_image(dtype)[0].data_ptr()


def _hard_counts(c, utts, paths):
    'A Python count over the state paths of `utts` with the test\'s own category map.'
    hard = np.zeros(c.tmap.n_categories)
    for u, p in zip(utts, paths):
        seq = c.seqs[c.graph_of[u]]
        states = c.tmap.chain(seq)
        for a, b in zip(p[:-1], p[1:]):
            hard[c.tmap.arc(seq, int(a), int(b))] += 1
        _, name, l = states[int(p[-1])]
        if l == c.tmap.sizes[name] - 1 and int(p[-1]) == len(states) - 1:
            hard[c.tmap.exit[name]] += 1
    return hard


def _as_stats(tr, counts):
    'Dirichlet statistics of the counts: the last column of every row replaced by the row sum.'
    out, first = np.array(counts, dtype=np.float64), 0
    for n, states in zip(tr.arities, tr.group_states):
        block = out[first:first + n * len(states)].reshape(len(states), n)
        block[:, -1] = block.sum(axis=1)
        first += n * len(states)
    return out


def _stats_of(model, elbo):
    return torch.cat([elbo._acc_stats[p].reshape(-1).double().cpu()
                      for p in model.transitions.parameters_of_groups()]).numpy()


@pytest.mark.parametrize('dtype', DTYPES)
def test_viterbi_and_state_paths_count_the_path(dtype):
    c = case(dtype)
    utts = [0, 1, 2, 3, 4, 5]
    graphs, lens, X, pc_all, _, _ = c.subset(utts)
    batch = c.batch(graphs, lens)
    path = hk.viterbi(batch, hk.gather(batch, pc_all, SCALE))
    paths = [p.cpu().numpy() for p in torch.split(path, lens)]
    hard = _hard_counts(c, utts, paths)
    assert hard.sum() == sum(lens)
    tc = hk.path_counts(batch, path, None)
    np.testing.assert_array_equal(tc[1].cpu().numpy(), hard)
    # the batched E-step, decoding itself and given the paths
    want = _as_stats(c.model.transitions, hard)
    elbo = accumulate_elbo(c.model, (X, lens), inference_graphs=graphs, scale=SCALE, viterbi=True)
    np.testing.assert_array_equal(_stats_of(c.model, elbo), want)
    elbo = accumulate_elbo(c.model, (X, lens), inference_graphs=graphs, scale=SCALE,
                           state_paths=[torch.from_numpy(p) for p in paths])
    np.testing.assert_array_equal(_stats_of(c.model, elbo), want)
    # one utterance through the model's own entry
    u = 3
    f0 = int(np.sum(lens[:u]))
    elbo = beer.evidence_lower_bound(c.model, X[f0:f0 + lens[u]], inference_graph=graphs[u],
                                     scale=SCALE, state_path=torch.from_numpy(paths[u]).to(DEV))
    np.testing.assert_array_equal(_stats_of(c.model, elbo),
                                  _as_stats(c.model.transitions, _hard_counts(c, [u], [paths[u]])))


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_vb_step_against_numpy(dtype):
    c = case(dtype)
    utts = [0, 1, 2, 3, 4, 5]
    graphs, lens, X, _, want, _ = c.subset(utts)
    model = c.model
    want_stats = _as_stats(model.transitions, want)
    # (the truth was computed at the acoustic scale of the other tests)
    elbo = accumulate_elbo(model, (X, lens), inference_graphs=graphs, scale=SCALE)
    stats = _stats_of(model, elbo)
    print(f'batched statistics: {_rel(stats, want_stats):.3e}')
    assert _rel(stats, want_stats) < _tol(dtype)
    # a bound set as it is, without the list
    few = accumulate_elbo(model, (X[:sum(lens[:2])], lens[:2]), scale=SCALE,
                          inference_graphs=model.bind_alignment_graphs(c.gset)[:2])
    assert _rel(_stats_of(model, few), _as_stats(model.transitions, c.counts[0] + c.counts[1])) \
        < _tol(dtype)
    # the phone weights get no counts from alignment graphs
    wparam = model.categorical.mean_field_factorization()[0][0]
    assert not elbo._acc_stats[wparam].any()
    # per utterance
    total, first = 0., 0
    for u, T in enumerate(lens):
        one = beer.evidence_lower_bound(model, X[first:first + T], datasize=sum(lens),
                                        inference_graph=graphs[u], scale=SCALE)
        total = total + _stats_of(model, one)
        assert not one._acc_stats[wparam].any()
        first += T
    # (rtol as for the free loop, tests/test_gpu_transitions.py; the floor is for counts of
    # paths so unlikely that the scaled and the log-space recursion round them differently)
    if dtype == torch.float64:
        np.testing.assert_allclose(total, stats, rtol=1e-10, atol=1e-12)
    else:
        np.testing.assert_allclose(total, stats, rtol=1e-5, atol=1e-5 * np.abs(stats).max())
    assert _rel(total, want_stats) < _tol(dtype)


def _sampled_corpus(model, units, true_loop, rng, n_utts=200):
    '''State paths sampled through known transcriptions (4-8 phones): every state of unit `name`
    stays with probability true_loop[name]; well-separated emissions.  Returns (X, lengths,
    transcriptions, state means).'''
    D = 6
    means = rng.randn(model.graph.n_states, D) * 4
    names = list(units)
    seqs, lens, frames = [], [], []
    for _ in range(n_utts):
        seq = [names[rng.randint(len(names))] for _ in range(rng.randint(4, 9))]
        states = []
        for name in seq:
            for l in range(3):
                states += [model.start_pdf[name] + l] * rng.geometric(1 - true_loop[name])
        seqs.append(seq)
        lens.append(len(states))
        frames.append(means[np.asarray(states)] + rng.randn(len(states), D))
    return np.concatenate(frames), lens, seqs, means


@pytest.mark.parametrize('learned', [True, False])
def test_recovery_of_known_self_loops(learned):
    rng = np.random.RandomState(17)
    model, units = loop_model(torch.float64, learned=learned, n_speech=4, n_nonspeech=0, D=6,
                              ncomp=1, seed=0)
    model = model.to(DEV)
    true_loop = {'s0': .5, 's1': .5, 's2': .9, 's3': .9}
    Xn, lens, seqs, means = _sampled_corpus(model, units, true_loop, rng)
    X = torch.from_numpy(Xn).to(DEV)
    # emissions started at the truth (state s emits pdf ids[s])
    ids = np.asarray(model.graph.pdf_id_mapping)
    mean = model._emissions().modelsets[0].normalset.means_precisions.posterior.params.mean
    pdf_means = np.zeros_like(means)
    pdf_means[ids] = means
    mean.copy_(torch.from_numpy(pdf_means).to(mean))
    graphs = alignment_set(units, seqs)
    graphs = model.bind_alignment_graphs(graphs) if learned else list(graphs)
    before = model.graph.trans_log_probs.clone()
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
    for _ in range(10):
        optim.init_step()
        elbo = accumulate_elbo(model, (X, lens), inference_graphs=graphs)
        elbo.backward()
        optim.step()
    if not learned:
        # fixed transitions: the units' self-loops are the 0.75 they were made with
        loops = torch.diagonal(model.graph.trans_log_probs).exp().cpu().numpy()
        np.testing.assert_allclose(loops, .75, rtol=1e-6)
        assert torch.equal(torch.diagonal(model.graph.trans_log_probs), torch.diagonal(before))
        return
    probs, _ = model.expected_transition_probs()
    loop = torch.diagonal(probs).numpy()
    assert {n for s in seqs for n in s} == set(true_loop)
    for name, p in true_loop.items():
        got = loop[model.start_pdf[name]:model.end_pdf[name] + 1]
        print(name, p, got)
        assert (np.abs(got - p) < abs(.75 - p)).all(), (name, got)


def _posteriors(model):
    return [t.detach().double().cpu().numpy() for p in model.bayesian_parameters()
            for t in p.posterior._tensors()]


@pytest.mark.parametrize('dtype', DTYPES)
def test_captured_iteration_replays_the_eager_one(dtype):
    from beer_amd.inference.captured import CapturedIteration
    rng = np.random.RandomState(23)
    seqs = [['s0', 'n0', 's0', 's0'], _transcription(20, 3, rng), ['s1', 'n0', 's2', 's2']]
    lens = [45, 170, 30]
    X = torch.from_numpy(rng.randn(sum(lens), 4) * 1.5).to(DEV, dtype)
    results = []
    for captured in (False, True):
        model, units = loop_model(dtype, seed=13)
        model = model.to(DEV)
        bound = model.bind_alignment_graphs(alignment_set(units, seqs))
        assert [g.n_states for g in bound] == [14, 75, 14]
        optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
        if captured:
            it = CapturedIteration(model, optim, (X, lens), inference_graphs=bound)
            modes = []
            for _ in range(9):
                it()
                modes.append(it.mode)
            assert modes[-1] == 'replayed' and 'captured' in modes, modes
        else:
            for _ in range(9):
                optim.init_step()
                elbo = accumulate_elbo(model, (X, lens), inference_graphs=bound)
                elbo.backward()
                optim.step()
        results.append(_posteriors(model))
    # (the statistics are atomic sums in the order the waves arrive, and nine iterations feed
    # on each other: 1e-12 per iteration as in tests/test_gpu_transitions.py, fp32's 1e-5)
    tol = 1e-11 if dtype == torch.float64 else 1e-4
    moved = 0.
    for a, b in zip(*results):
        assert np.abs(a - b).max() <= tol * max(np.abs(a).max(), 1.)
    model0, _ = loop_model(dtype, seed=13)
    for p0, p in zip(model0.transitions.parameters_of_groups(),
                     model.transitions.parameters_of_groups()):
        moved += float((p.posterior.params.concentrations.cpu() -
                        p0.posterior.params.concentrations).abs().sum())
    assert moved > 1.


# (the configuration of tests/test_gpu_transitions.py without the arc from the end state of `sil`
# back to its start state: in a phone loop that arc is part of the unit's exit -- it shares the
# entry end -> start with leaving and entering `sil` again --, so an alignment chain, where it
# is an arc of its own beside the one to the next phone, has two arcs of one category and is
# refused; see test_transitions_aligned_host.py)
HMM_CONF = """
- group_name: sil
  n_normal_per_state: 3
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
  n_normal_per_state: 4
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


def test_cli_accumulates_learned_transitions_from_an_alignment_archive(tmp_path):
    t = str(tmp_path)
    (tmp_path / 'hmm.yml').write_text(HMM_CONF)
    (tmp_path / 'units').write_text('sil sil\na speech\nb speech\nc speech\nd speech\n')
    _run(['dataset', 'create', t, os.path.join(GOLDEN, 'ref_feats.npz'), f'{t}/ds.pkl'])
    _run(['-s', '1', 'hmm', 'mkphones', '-d', f'{t}/ds.pkl', f'{t}/hmm.yml', f'{t}/units',
          f'{t}/hmms.mdl'])
    _run(['hmm', 'mkphoneloopgraph', '--start-end-group', 'sil', f'{t}/units', f'{t}/g.pkl'])
    _run(['hmm', 'mkdecodegraph', f'{t}/g.pkl', f'{t}/hmms.mdl', f'{t}/dg.pkl'])
    _run(['hmm', 'mkphoneloop', '--train-transitions', '--transitions-prior-strength', '2',
          '--weights-prior', 'dirichlet', f'{t}/dg.pkl', f'{t}/hmms.mdl', f'{t}/0.mdl'])
    _run(['hmm', 'mkphoneloop', '--weights-prior', 'dirichlet', f'{t}/dg.pkl', f'{t}/hmms.mdl',
          f'{t}/fixed.mdl'])
    os.makedirs(f'{t}/ali')
    _run(['hmm', 'mkaligraph', f'{t}/hmms.mdl', f'{t}/ali'],
         stdin='utt0 sil a b sil\nutt1 sil c a a sil\n')          # (utt2: the free loop)
    with zipfile.ZipFile(f'{t}/alis.npz', 'w') as z:
        for f in sorted(os.listdir(f'{t}/ali')):
            z.write(os.path.join(f'{t}/ali', f), f)
    utts = 'utt0\nutt1\nutt2\n'
    _run(['hmm', 'accumulate', '-a', f'{t}/alis.npz', f'{t}/0.mdl', f'{t}/ds.pkl', f'{t}/e.pkl'],
         stdin=utts)
    _run(['hmm', 'update', '-o', f'{t}/optim.pth', f'{t}/0.mdl', f'{t}/1.mdl'], stdin=f'{t}/e.pkl\n')
    _run(['hmm', 'accumulate', '-a', f'{t}/alis.npz', f'{t}/1.mdl', f'{t}/ds.pkl', f'{t}/e1.pkl'],
         stdin=utts)
    _run(['hmm', 'update', '-o', f'{t}/optim.pth', f'{t}/1.mdl', f'{t}/2.mdl'], stdin=f'{t}/e1.pkl\n')
    m0 = pickle.load(open(f'{t}/0.mdl', 'rb'))
    m2 = pickle.load(open(f'{t}/2.mdl', 'rb'))
    moved = 0.
    for a, b in zip(m0.transitions.parameters_of_groups(), m2.transitions.parameters_of_groups()):
        np.testing.assert_array_equal(a.prior.params.concentrations.numpy(),
                                      b.prior.params.concentrations.numpy())
        moved += float((b.posterior.params.concentrations - a.posterior.params.concentrations)
                       .abs().sum())
    assert moved > 1.
    # a model with fixed transitions: the ELBO file of the same command is what the two
    # batches gave before (aligned utterances on their graphs, the others on the free loop)
    _run(['hmm', 'accumulate', '-a', f'{t}/alis.npz', f'{t}/fixed.mdl', f'{t}/ds.pkl',
          f'{t}/ef.pkl'], stdin=utts)
    got, count = pickle.load(open(f'{t}/ef.pkl', 'rb'))
    assert count == 3
    fixed = pickle.load(open(f'{t}/fixed.mdl', 'rb')).to(DEV)
    ds = pickle.load(open(f'{t}/ds.pkl', 'rb'))
    alis = np.load(f'{t}/alis.npz', allow_pickle=True)
    want = accumulate_elbo(fixed, [ds[u].features for u in ('utt0', 'utt1')], datasize=ds.size,
                           inference_graphs=[alis[u][0] for u in ('utt0', 'utt1')]) + \
        accumulate_elbo(fixed, [ds['utt2'].features], datasize=ds.size)
    assert float(got) == pytest.approx(float(want), rel=1e-6)
    by_uuid = {p.uuid: v for p, v in got._acc_stats.items()}
    assert len(by_uuid) == len(want._acc_stats)
    for p, v in want._acc_stats.items():
        a, b = by_uuid[p.uuid].double().cpu().numpy(), v.double().cpu().numpy()
        assert np.abs(a - b).max() <= 1e-5 * max(np.abs(b).max(), 1.)
