'''Bigram phone loop on the GPU: the reference goldens, the fused kernel against the general
path at the recipe's shape, the batched accumulation against the per-utterance loop.'''

import io
import os
import warnings

import numpy as np
import pytest
import torch

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import compat, hmm as hmm_cmds
from helpers import assert_close, orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRIORS = ('dirichlet2', 'hierarchical_dirichlet_process')


class _Spy:
    'Records the names of the entry points called through _hip.call.'

    def __init__(self, monkeypatch):
        self.names = []
        real = _hip.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(_hip, 'call', call)


def _golden(prior, suffix=''):
    g = np.load(os.path.join(GOLDEN, f'g20_bigram_{prior}{suffix}.npz'))
    model = compat.load(io.BytesIO(np.asarray(g['model']).tobytes()))
    return g, model.to(torch.device('cuda'))


def _npy(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('suffix', ['', '_p24'])
@pytest.mark.parametrize('prior', PRIORS)
def test_bigram_goldens(prior, suffix, monkeypatch):
    'P = 5 and P = 24 phones, 3 VB iterations, against the reference.'
    g, model = _golden(prior, suffix)
    spy = _Spy(monkeypatch)
    X = torch.from_numpy(g['X']).cuda()
    stats = model.sufficient_statistics(X)
    exp_llh = model.expected_log_likelihood(stats)
    assert 'beer_hmm_posteriors_bigram' in spy.names
    assert_close(_npy(exp_llh), g['exp_llh'], 1e-9, 'exp_llh')
    sr = model.cache['scaled_pdf_resps']
    mapping = list(model.graph.pdf_id_mapping)
    assert_close(_npy(sr)[:, mapping], g['gamma'], 1e-7, 'gamma')
    assert_close(_npy(model.cache['bigram_counts']), g['xi_block'], 1e-8, 'xi block')
    model.clear_cache()
    params = [p for group in model.mean_field_factorization() for p in group]
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
    elbos = []
    for it in range(3):
        optim.init_step()
        elbo = beer.evidence_lower_bound(model, X, datasize=len(X))
        for k, p in enumerate(params):
            assert_close(_npy(elbo._acc_stats[p]), g[f'acc{it}.{k}'], 1e-8, f'acc{it}.{k}')
        elbo.backward()
        optim.step()
        elbos.append(float(elbo))
        for k, p in enumerate(params):
            assert_close(_npy(p.posterior.natural_parameters()), g[f'it{it}.post{k}'], 1e-7,
                         f'it{it}.post{k}')
        trans, want = _npy(model.graph.trans_log_probs), g[f'it{it}.trans']
        assert np.array_equal(np.isfinite(trans), np.isfinite(want))
        fin = np.isfinite(want)
        assert_close(trans[fin], want[fin], 1e-7, f'it{it}.trans')
    assert_close(np.asarray(elbos), g['elbos'], 1e-9, 'elbos')
    np.testing.assert_array_equal(_npy(model.decode(X)), g['decode'])


# --- the recipe's shape: 100 units x 3 states x 4 diagonal Gaussians, D = 39 ----------------

_TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
         {'start_id': 1, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 2, 'trans_prob': .5},
         {'start_id': 2, 'end_id': 3, 'trans_prob': .5}, {'start_id': 3, 'end_id': 3, 'trans_prob': .5},
         {'start_id': 3, 'end_id': 4, 'trans_prob': .5}]
_TOPO1 = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
          {'start_id': 1, 'end_id': 2, 'trans_prob': .5}]


def build_loop(P, D, prior, dtype, seed=0, topology=_TOPO, ncomp=4):
    torch.manual_seed(seed)
    conf = {'g': {'topology': topology, 'n_normal_per_state': ncomp, 'prior_strength': 1.,
                  'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(P)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(D), torch.ones(D))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    model = hmm_cmds.phone_loop(graph, start, end, ems, prior)
    model = model.double() if dtype == torch.float64 else model.float()
    return model.to(torch.device('cuda'))


def _utterances(n, D, seed, dtype, lo=30, hi=400):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi, size=n).tolist()
    X = torch.from_numpy(rng.randn(sum(lens), D) * 1.5).to('cuda', dtype)
    return X, lens


def _posteriors(model, X, lens, fused):
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    batch = hk.HmmBatch([model.graph], [0] * len(lens), lens, pc_all.dtype)
    llh = torch.zeros(len(lens), dtype=torch.float64, device='cuda')
    if fused:
        assert hk.bigram_ok(batch)
        sr, counts = hk.posteriors_bigram(batch, pc_all, .8, utt_llh=llh)
        return sr, counts, llh
    pc = hk.gather(batch, pc_all, .8)
    gamma, xi, _, _, _ = hk.forward_backward(batch, pc, want_xi=True, dense_xi=True)
    sr, _ = hk.scatter(batch, pc, gamma, pc_all.shape[1], .8, want_exp_llh=False, utt_llh=llh)
    return sr, model.bigram_counts(xi), llh


@pytest.fixture(scope='module')
def recipe():
    out = {}
    for dtype in (torch.float64, torch.float32):
        model = build_loop(100, 39, 'dirichlet2', dtype)
        X, lens = _utterances(200, 39, 1, dtype)
        out[dtype] = (model, X, lens)
    return out


def test_recipe_shape_fused_equals_general_path(recipe, monkeypatch):
    model, X, lens = recipe[torch.float64]
    assert len(model.start_pdf) == 100 and model.graph.n_states == 300
    spy = _Spy(monkeypatch)
    sr, counts, llh = _posteriors(model, X, lens, fused=True)
    assert spy.names.count('beer_hmm_posteriors_bigram') == 1
    sr_g, counts_g, llh_g = _posteriors(model, X, lens, fused=False)
    assert_close(_npy(sr), _npy(sr_g), 1e-10, 'posteriors')
    assert_close(_npy(counts), _npy(counts_g), 1e-10, 'bigram counts')
    assert_close(_npy(llh), _npy(llh_g), 1e-10, 'utterance llh')
    assert float(counts.sum()) > len(lens)          # phones do change


def test_recipe_shape_float32_against_float64(recipe):
    '''The float32 kernel against the float64 one on the same log-likelihoods (rounded to
    float32: what the float32 path is given), at a flat 1e-5.'''
    m64, X64, lens = recipe[torch.float64]
    m32, _, _ = recipe[torch.float32]
    sr64, c64, l64 = _posteriors(m64, X64, lens, fused=True)
    pc = m64._emissions().expected_log_likelihood(m64.sufficient_statistics(X64)).float()
    batch = hk.HmmBatch([m32.graph], [0] * len(lens), lens, torch.float32)
    assert hk.bigram_ok(batch)
    l32 = torch.zeros(len(lens), dtype=torch.float64, device='cuda')
    sr32, c32 = hk.posteriors_bigram(batch, pc, .8, utt_llh=l32)
    assert sr32.dtype == torch.float32
    np.testing.assert_allclose(_npy(sr32), _npy(sr64), rtol=0, atol=1e-5)
    assert_close(_npy(c32), _npy(c64), 1e-5, 'bigram counts')
    assert_close(_npy(l32), _npy(l64), 1e-5, 'utterance llh')


def test_recipe_shape_counts_per_utterance_against_the_oracle(recipe):
    '''The counts of the shortest utterances against the numpy restatement of the reference
    (`orc.posteriors`, per-frame xi [T-1, S, S]): 100 phones, so the block's second half
    (phones 64 .. 99) is covered too.'''
    model, X, lens = recipe[torch.float64]
    off = np.concatenate([[0], np.cumsum(lens)])
    pc_all = _npy(model._emissions().expected_log_likelihood(model.sufficient_statistics(X)))
    g = model.graph
    init, final, trans = (_npy(t).astype(np.float64) for t in
                          (g.init_log_probs, g.final_log_probs, g.trans_log_probs))
    ends, starts = list(model.end_pdf.values()), list(model.start_pdf.values())
    for u in np.argsort(lens, kind='stable')[:3]:
        llhs = pc_all[off[u]:off[u + 1]][:, list(g.pdf_id_mapping)] * .8
        _, xi, _ = orc.posteriors(llhs, init, final, trans, trans_posteriors=True)
        want = xi.sum(axis=0)[np.ix_(ends, starts)]
        _, counts, _ = _posteriors(model, X[off[u]:off[u + 1]], [lens[u]], fused=True)
        assert_close(_npy(counts), want, 1e-8, f'utterance {u}')


@pytest.mark.parametrize('P', [100, 120])
def test_float32_dirichlet2_from_mkphoneloopbigram_against_the_general_path(P):
    '''mkphoneloopbigram's dirichlet2 gives every concentration 1 / P: the block entries are
    about -P, below float32's range from P ~ 104.  The float32 kernel must keep them.'''
    uni = build_loop(P, 39, 'dirichlet_process', torch.float32, ncomp=1)
    model = hmm_cmds.bigram_loop(uni, 'dirichlet2').to(torch.device('cuda'))
    block = model.bigram_counts(model.graph.trans_log_probs[None].double())
    assert float(block.max()) < -P + 1
    # segments of 20 frames around a random point each: the evidence for changing phone
    # (tens of nats a frame) outweighs the ~P nats a transition costs
    rng = np.random.RandomState(8)
    lens = rng.randint(3, 10, size=60) * 20
    X = np.concatenate([np.repeat(rng.randn(n // 20, 39) * 3, 20, axis=0) +
                        rng.randn(n, 39) * .3 for n in lens])
    X, lens = torch.from_numpy(X).to('cuda', torch.float32), lens.tolist()
    sr, counts, llh = _posteriors(model, X, lens, fused=True)
    sr_g, counts_g, llh_g = _posteriors(model, X, lens, fused=False)
    np.testing.assert_allclose(_npy(sr), _npy(sr_g), rtol=0, atol=1e-5)
    assert_close(_npy(counts), _npy(counts_g), 1e-5, 'bigram counts')
    assert_close(_npy(llh), _npy(llh_g), 1e-5, 'utterance llh')
    # the phones do change (with the block lost -- exp(-P) is 0 in float32 from P ~ 104 -- every
    # utterance would stay in one phone)
    assert float(counts_g.sum()) > len(lens) and float(counts.sum()) > len(lens)


@pytest.mark.parametrize('prior', PRIORS)
def test_bigram_batch_equals_per_utterance_loop(prior):
    g, model = _golden(prior)
    rng = np.random.RandomState(3)
    lens = [37, 90, 52, 41]
    utts = [torch.from_numpy(rng.randn(T, g['X'].shape[1]) * 1.5).cuda() for T in lens]
    N = 5000
    loop = beer.evidence_lower_bound(datasize=N)
    for x in utts:
        loop += beer.evidence_lower_bound(model, x, datasize=N, scale=.7)
    batched = beer.accumulate_elbo(model, utts, datasize=N, scale=.7)
    assert_close(float(batched), float(loop), 1e-11)
    for group in model.mean_field_factorization():
        for p in group:
            assert_close(_npy(batched._acc_stats[p]), _npy(loop._acc_stats[p]), 1e-10)


@pytest.mark.parametrize('prior', PRIORS)
def test_alignment_graphs_give_zero_bigram_counts(prior):
    g, model = _golden(prior)
    rng = np.random.RandomState(4)
    utts = [torch.from_numpy(rng.randn(T, g['X'].shape[1])).cuda() for T in (40, 25)]
    elbo = beer.accumulate_elbo(model, utts, datasize=100,
                                inference_graphs=[model.graph, model.graph])
    wparam = model.categoricalset.mean_field_factorization()[0][0]
    assert float(elbo._acc_stats[wparam].abs().sum()) == 0.
    assert np.isfinite(float(elbo))


def test_more_phones_than_the_kernel_takes_use_the_general_path(monkeypatch):
    model = build_loop(130, 3, 'dirichlet2', torch.float64, topology=_TOPO1, ncomp=1)
    X, lens = _utterances(6, 3, 2, torch.float64, 20, 60)
    spy = _Spy(monkeypatch)
    utts = list(torch.split(X, lens))
    batched = beer.accumulate_elbo(model, utts, datasize=1000)
    assert 'beer_hmm_posteriors_bigram' not in spy.names
    loop = beer.evidence_lower_bound(datasize=1000)
    for x in utts:
        loop += beer.evidence_lower_bound(model, x, datasize=1000)
    assert_close(float(batched), float(loop), 1e-11)
    wparam = model.categoricalset.mean_field_factorization()[0][0]
    assert_close(_npy(batched._acc_stats[wparam]), _npy(loop._acc_stats[wparam]), 1e-10)


@pytest.mark.parametrize('prior', PRIORS)
def test_bigram_training_from_a_unigram(prior, monkeypatch):
    '''mkphoneloop -> mkphoneloopbigram -> accumulate -> update -> decode, in process.'''
    uni = build_loop(12, 5, 'dirichlet_process', torch.float64)
    bi = hmm_cmds.bigram_loop(uni, prior)
    X, lens = _utterances(20, 5, 5, torch.float64, 20, 80)
    utts = list(torch.split(X, lens))
    spy = _Spy(monkeypatch)
    optim = beer.VBConjugateOptimizer(bi.conjugate_bayesian_parameters(keepgroups=True), 1.)
    values = []
    for _ in range(3):
        optim.init_step()
        elbo = beer.accumulate_elbo(bi, utts, datasize=len(X))
        elbo.backward()
        optim.step()
        values.append(float(elbo))
    assert 'beer_hmm_posteriors_bigram' in spy.names
    assert values[-1] > values[0]
    paths = beer.decode_batch(bi, utts)
    for u in (0, 9):
        np.testing.assert_array_equal(_npy(paths[u]), _npy(bi.decode(utts[u])))


def test_captured_iteration_of_a_bigram_loop_stays_eager():
    g, model = _golden('dirichlet2')
    rng = np.random.RandomState(6)
    lens = [30, 44, 27]
    X = torch.from_numpy(rng.randn(sum(lens), g['X'].shape[1])).cuda()
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
    it = beer.CapturedIteration(model, optim, (X, lens), datasize=len(X))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for _ in range(3):
            it()
    assert it.mode == 'eager'
