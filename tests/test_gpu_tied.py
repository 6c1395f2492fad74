'''Tied-mixture emissions on the GPU (`beer_tied_lognorm`, `beer_tied_accumulate`,
`beer.TiedMixtureSet`) against the float64 truth of tests/tied_truth.py.  Tolerances are the
project's: float64 1e-10 relative, float32 a flat 1e-5 with the accumulated statistics held
per block.'''

import numpy as np
import pytest
import torch

import beer_amd as beer
from beer_amd import hmm_kernels as hk, kernels
from beer_amd.stats import FrameStats
from helpers import assert_close, assert_stats_close, rel_err

import tied_truth as tt

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
COVS = ('full', 'diagonal', 'isotropic')
DTYPES = {'float64': torch.float64, 'float32': torch.float32}
TOL = {'float64': 1e-10, 'float32': 1e-5}


def _npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, DTYPES[dtype])


def _run(case, dtype, cov_type=None):
    '''Both kernels on a case of tied_truth: dict(pc, m, r, C[, acc], count).'''
    l, g = (_dev(case[n], dtype) for n in ('l', 'g'))
    lw = _dev(case['lw'], 'float64')
    count = torch.zeros((), dtype=torch.int64, device=DEV)
    pc, m = kernels.tied_lognorm(l, lw, count)
    r, C = kernels.tied_accumulate(l, m, pc, lw, g)
    out = {'pc': _npy(pc), 'm': _npy(m), 'r': _npy(r), 'C': _npy(C), 'count': int(count)}
    if cov_type is not None:
        stats = FrameStats(_dev(case['X'], dtype), cov_type)
        out['acc'] = _npy(kernels.normal_accumulate(stats, r, None, l.shape[1], 1, cov_type))
    return out


def _truth(case, cov_type=None):
    pc, m = tt.lognorm(case['l'], case['lw'])
    stats = None if cov_type is None else tt.suffstats(case['X'], cov_type)
    C, r, acc = tt.statistics(case['l'], case['lw'], pc, case['g'], stats)
    return {'pc': pc, 'm': m, 'r': r, 'C': C, 'acc': acc}


def _check(got, truth, tol, D=None, what=''):
    for name in ('pc', 'm', 'r', 'C'):
        print(f'{what} {name}: rel err {rel_err(got[name], truth[name]):.3e}')
    for name in ('pc', 'm', 'r', 'C'):
        assert_close(got[name], truth[name], tol, f'{what} {name}')
    if truth.get('acc') is not None:
        assert_stats_close(got['acc'], truth['acc'], D, tol, f'{what} acc')


# ---- 1. kernel level ---------------------------------------------------------------------

@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('cov_type', COVS)
@pytest.mark.parametrize('shape', tt.KERNEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernels_against_truth(shape, cov_type, dtype):
    S, K, D, T = shape
    case = tt.kernel_case(11, S, K, D, T, cov_type, dtype)
    got, truth = _run(case, dtype, cov_type), _truth(case, cov_type)
    _check(got, truth, TOL[dtype], D, f'{shape} {cov_type} {dtype}')


# ---- 2. conservation ---------------------------------------------------------------------

@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', tt.KERNEL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conservation(shape, dtype):
    S, K, D, T = shape
    case = tt.kernel_case(12, S, K, D, T, 'diagonal', dtype)
    got, g, tol = _run(case, dtype), case['g'], TOL[dtype]
    assert_close(got['r'].sum(axis=1), g.sum(axis=1), tol, 'sum_k r = sum_s g')
    assert_close(got['C'].sum(axis=1), g.sum(axis=0), tol, 'sum_k C = sum_t g')
    assert_close(got['C'].sum(axis=0), got['r'].sum(axis=0), tol, 'sum_s C = sum_t r')


# ---- 3. range ----------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('shape', tt.RANGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ordinary_data_stays_linear(shape, dtype):
    '(a) frames from the pool, concentrations in [1, 4]: within tolerance, counter exactly 0.'
    S, K, D, T = shape
    case = tt.kernel_case(13, S, K, D, T, 'full', dtype)
    got, truth = _run(case, dtype, 'full'), _truth(case, 'full')
    _check(got, truth, TOL[dtype], D, f'{shape} {dtype}')
    assert got['count'] == 0


def test_underflowing_states_take_the_log_space_way():
    '(b) float32: every pc finite and within tolerance, the counter is what the truth says.'
    case = tt.extreme_case(14)
    got, truth = _run(case, 'float32', 'diagonal'), _truth(case, 'diagonal')
    assert np.isfinite(got['pc']).all()
    _check(got, truth, 1e-5, case['X'].shape[1], 'extreme')
    p = tt.linear_sum(case['l'], case['lw'])
    tau = tt.THRESHOLD['float32']
    lo, hi = int((p < tau / 2).sum()), int((p < 2 * tau).sum())
    print(f'log-space entries: {got["count"]}, truth below tau/2: {lo}, below 2 tau: {hi}')
    assert got['count'] > 0
    assert lo <= got['count'] <= hi


# ---- model level -------------------------------------------------------------------------

from beer_amd.cli import hmm as hmm_cmds                                       # noqa: E402
from beer_amd.inference.batch import accumulate_elbo                          # noqa: E402
from transitions_truth import NON_SPEECH, SPEECH                               # noqa: E402
from helpers import orc                                                        # noqa: E402

UNIGRAM_PRIORS = ('dirichlet', 'dirichlet_process', 'gamma_dirichlet_process')


def _build(kind='hmm', prior='gamma_dirichlet_process', pool=12, cov='diagonal', n_speech=3,
           joint=False, learned=False, D=4, seed=0, dtype=torch.float64, warm=True):
    '''(model, units): a loop of `n_speech` 3-state units whose states share a pool of `pool`
    Gaussians (built by the command line's `build_units` from `shared_normal_pool`), with
    `joint` beside an untied non-speech unit; one VB step on noise so that no posterior is
    its prior.'''
    torch.manual_seed(seed)
    common = {'prior_strength': 1., 'noise_std': 1., 'cov_type': cov, 'shared_cov': False}
    conf = {'speech': {'topology': SPEECH, 'shared_normal_pool': pool, **common}}
    grouped = {'speech': [f's{i}' for i in range(n_speech)]}
    if joint:
        conf['nonspeech'] = {'topology': NON_SPEECH, 'n_normal_per_state': 2, **common}
        grouped['nonspeech'] = ['n0']
    units, ems = hmm_cmds.build_units(conf, grouped, torch.zeros(D), torch.ones(D))
    names = [n for g in grouped.values() for n in g]
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    if kind == 'hmm':
        model = beer.HMM.create(graph.compile(), ems, train_transitions=learned)
    else:
        model = hmm_cmds.phone_loop(graph, start, end, ems, prior, train_transitions=learned)
    model = (model.double() if dtype == torch.float64 else model.float()).to(DEV)
    if warm:
        X, lens = _utterances(4, D, seed + 100, dtype)
        optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
        for _ in range(len(model.mean_field_factorization())):
            optim.init_step()
            accumulate_elbo(model, (X, lens)).backward()
            optim.step()
    return model, units


def _utterances(n, D, seed, dtype, lo=20, hi=120):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi, size=n).tolist()
    X = torch.from_numpy(rng.randn(sum(lens), D) * 1.5).to(DEV, dtype)
    return X, lens


def _std(dist):
    return tuple(_npy(getattr(dist.params, n)) for n in dist._std_params_def)


def _groups_of(model):
    'The emission groups of `model` as tied_truth / the oracle take them, with their parameters.'
    from beer_amd.inference.batch import _groups
    out, params = [], []
    for grp, S, G in _groups(model._emissions()):
        ns = grp.normalset
        mp, w = ns.means_precisions, grp.categoricalset.weights
        d = {'cov_type': ns.cov_type, 'post': _std(mp.posterior), 'prior': _std(mp.prior),
             'w_post': _std(w.posterior)[0], 'w_prior': _std(w.prior)[0], 'S': S, 'G': G}
        d['tied'] = isinstance(grp, beer.TiedMixtureSet)
        out.append(d)
        params.append((mp, w))
    return out, params


def _graph_dict(graph):
    return {'init': _npy(graph.init_log_probs), 'final': _npy(graph.final_log_probs),
            'trans': _npy(graph.trans_log_probs), 'order': [int(i) for i in graph.pdf_id_mapping]}


def _split(X, lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    return [X[off[u]:off[u + 1]] for u in range(len(lens))]


def _check_model(model, X, lens, graphs=None, tol=1e-10, **kwargs):
    '''`accumulate_elbo` against the per-utterance loop (value and every statistic) and against
    the truth (value -- with the model's own KL term, which this feature does not touch --
    and the statistics of every emission group).'''
    N = sum(lens)
    batched = accumulate_elbo(model, (X, lens), datasize=N, inference_graphs=graphs, **kwargs)
    loop = beer.evidence_lower_bound(datasize=N)
    for u, Xu in enumerate(_split(X, lens)):
        extra = {} if graphs is None else {'inference_graph': graphs[u]}
        loop = loop + beer.evidence_lower_bound(model, Xu, datasize=N, **extra, **kwargs)
    assert_close(float(batched.value), float(loop.value), tol, 'batched vs loop: value')
    for p in model.bayesian_parameters():
        assert_close(_npy(batched._acc_stats[p]), _npy(loop._acc_stats[p]).reshape(
            batched._acc_stats[p].shape), tol, 'batched vs loop: statistics')
    groups, params = _groups_of(model)
    gd = _graph_dict(model.graph) if graphs is None else [_graph_dict(g.to_dense()) for g in graphs]
    truth = tt.hmm_step([_npy(x) for x in _split(X, lens)], groups, gd, datasize=N,
                        scale=kwargs.get('scale', 1.), viterbi=kwargs.get('viterbi', False))
    kl = float(torch.as_tensor(model.kl_div_posterior_prior()).sum())
    value = truth['value'] + len(lens) * (truth['kl'] - kl)
    assert_close(float(batched.value), value, tol, 'value vs truth')
    for (mp, w), (acc, wstats) in zip(params, truth['acc']):
        assert_close(_npy(batched._acc_stats[mp]), acc, tol, 'Gaussian statistics vs truth')
        assert_close(_npy(batched._acc_stats[w]), wstats, tol, 'weight statistics vs truth')
    return batched, truth


def test_hmm_against_truth_with_the_oracle_kl():
    'A plain HMM has emission parameters only: here the KL term is the oracle\'s too.'
    model, _ = _build('hmm')
    X, lens = _utterances(5, 4, 1, torch.float64)
    _, truth = _check_model(model, X, lens)
    kl = float(torch.as_tensor(model.kl_div_posterior_prior()).sum())
    assert_close(kl, truth['kl'], 1e-10, 'KL')


@pytest.mark.parametrize('cov', COVS)
def test_hmm_every_covariance(cov):
    model, _ = _build('hmm', cov=cov, pool=20, seed=2)
    X, lens = _utterances(4, 4, 3, torch.float64)
    _check_model(model, X, lens)


@pytest.mark.parametrize('prior', UNIGRAM_PRIORS)
def test_phone_loop(prior):
    model, _ = _build('ploop', prior, seed=4)
    X, lens = _utterances(6, 4, 5, torch.float64)
    _check_model(model, X, lens)


def test_bigram_phone_loop():
    model, _ = _build('ploop', 'dirichlet2', seed=6)
    assert isinstance(model, beer.BigramPhoneLoop)
    X, lens = _utterances(6, 4, 7, torch.float64)
    _check_model(model, X, lens)


@pytest.mark.parametrize('kwargs', [{}, {'viterbi': True}, {'scale': .5}],
                         ids=['plain', 'viterbi', 'scale'])
def test_free_loop_variants(kwargs):
    model, _ = _build('ploop', 'dirichlet', seed=8)
    X, lens = _utterances(5, 4, 9, torch.float64)
    _check_model(model, X, lens, **kwargs)


@pytest.mark.parametrize('kwargs', [{}, {'viterbi': True}, {'scale': .5}],
                         ids=['plain', 'viterbi', 'scale'])
def test_alignment_graphs_with_repeated_pdf_ids(kwargs):
    model, units = _build('ploop', 'gamma_dirichlet_process', seed=10)
    X, lens = _utterances(4, 4, 11, torch.float64, lo=30)
    seqs = [['s0', 's1', 's0'], ['s2', 's2'], ['s1', 's0', 's1', 's2'], ['s0']]
    graphs = list(beer.graph.compile_alignments(seqs, units))
    assert len(set(graphs[0].pdf_id_mapping)) < len(graphs[0].pdf_id_mapping)
    _check_model(model, X, lens, graphs=graphs, **kwargs)


def test_joint_tied_and_untied_groups():
    model, _ = _build('ploop', 'gamma_dirichlet_process', joint=True, seed=12)
    from beer_amd.inference.batch import _groups
    kinds = [type(g).__name__ for g, _, _ in _groups(model._emissions())]
    assert kinds == ['TiedMixtureSet', 'MixtureSet']
    X, lens = _utterances(5, 4, 13, torch.float64)
    _check_model(model, X, lens)
    _check_model(model, X, lens, scale=.5)


@pytest.mark.parametrize('kind', ['hmm', 'ploop'])
def test_learned_transitions_on_top(kind):
    model, _ = _build(kind, 'dirichlet', learned=True, seed=14)
    assert model.transitions is not None
    X, lens = _utterances(5, 4, 15, torch.float64)
    _check_model(model, X, lens)


def test_decode_batch_matches_decode():
    model, _ = _build('ploop', seed=16)
    X, lens = _utterances(4, 4, 17, torch.float64)
    paths = beer.decode_batch(model, (X, lens))
    for Xu, path in zip(_split(X, lens), paths):
        assert np.array_equal(_npy(model.decode(Xu)), _npy(path))


# ---- 5. five VB iterations -----------------------------------------------------------------

def _sample(model, n_utts, T, seed):
    'Frames of a random walk through the model\'s graph, each from its state\'s tied mixture.'
    rng = np.random.default_rng(seed)
    g = _graph_dict(model.graph)
    groups, _ = _groups_of(model)
    mean = groups[0]['post'][0]
    w = groups[0]['w_post'] / groups[0]['w_post'].sum(axis=1, keepdims=True)
    trans = np.exp(g['trans'])
    trans /= trans.sum(axis=1, keepdims=True)
    init = np.exp(g['init']) / np.exp(g['init']).sum()
    utts = []
    for _ in range(n_utts):
        s, rows = rng.choice(len(init), p=init), []
        for _ in range(T):
            k = rng.choice(w.shape[1], p=w[g['order'][s]])
            rows.append(mean[k] + .3 * rng.standard_normal(mean.shape[1]))
            s = rng.choice(len(init), p=trans[s])
        utts.append(np.asarray(rows))
    return utts


@pytest.mark.parametrize('cov', ['full', 'diagonal'])
def test_five_vb_iterations(cov):
    '''lrate 1, float64: the ELBO of every iteration (1e-9 relative) and the posterior after
    every step -- weight concentrations and the pool's standard parameters -- against the
    truth's E-step and M-step.'''
    model, _ = _build('hmm', cov=cov, pool=9, seed=18, warm=False)
    utts = _sample(model, 6, 60, 19)
    lens = [len(u) for u in utts]
    X = torch.from_numpy(np.concatenate(utts)).to(DEV)
    groups, params = _groups_of(model)
    gd = _graph_dict(model.graph)
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
    assert len(model.mean_field_factorization()) == 1
    for it in range(5):
        optim.init_step()
        elbo = accumulate_elbo(model, (X, lens))
        truth = tt.hmm_step(utts, groups, gd)
        assert_close(float(elbo.value), truth['value'], 1e-9, f'ELBO, iteration {it}')
        elbo.backward()
        optim.step()
        groups = tt.mstep(groups, truth['acc'])
        (mp, w), = params
        assert_close(_std(w.posterior)[0], groups[0]['w_post'], 1e-9, f'concentrations {it}')
        for name, got, want in zip(mp.posterior._std_params_def, _std(mp.posterior),
                                   groups[0]['post']):
            assert_close(got.reshape(np.shape(want)), want, 1e-8, f'pool {name}, iteration {it}')


# ---- 6. / 7. what exists -------------------------------------------------------------------

def test_one_tied_mixture_is_a_mixture():
    'S = 1: the statistics of `Mixture` over the same NormalSet (1e-12, float64).'
    torch.manual_seed(20)
    D, K = 5, 10
    ns = beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=K, noise_std=1.,
                               cov_type='full').double().to(DEV)
    tied = beer.TiedMixtureSet.create(1, ns, prior_strength=2.).double().to(DEV)
    mix = beer.Mixture(tied.categoricalset[0], ns)
    X = torch.from_numpy(np.random.RandomState(21).randn(200, D) * 1.5).to(DEV)
    stats = tied.sufficient_statistics(X)
    pc = tied.expected_log_likelihood(stats)
    acc = tied.accumulate(stats, torch.ones(len(X), 1, dtype=X.dtype, device=DEV))
    value = mix.expected_log_likelihood(stats)
    ref = mix.accumulate(stats)
    assert_close(_npy(pc)[:, 0], _npy(value), 1e-12, 'log-normaliser')
    assert_close(_npy(acc[ns.means_precisions]), _npy(ref[ns.means_precisions]), 1e-12, 'pool')
    assert_close(_npy(acc[tied.categoricalset.weights])[0], _npy(ref[mix.categorical.weights]),
                 1e-12, 'weights')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_untied_paths_are_untouched(dtype):
    '''An untied HMM: `accumulate_elbo` gives the statistics, bit for bit, that the entry points
    this change does not touch give for the same posteriors.'''
    torch.manual_seed(22)
    D, S, G = 4, 6, 4
    ns = beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=S * G, noise_std=1.,
                               cov_type='diagonal')
    ems = beer.MixtureSet.create(S, ns)
    graph = beer.graph.Graph()
    states = [graph.add_state(pdf_id=s) for s in range(S)]
    graph.start_state, graph.end_state = graph.add_state(), graph.add_state()
    for s in states:
        graph.add_arc(graph.start_state, s)
        graph.add_arc(s, graph.end_state)
        for d in states:
            graph.add_arc(s, d)
    graph.normalize()
    model = beer.HMM.create(graph.compile(), ems)
    model = (model.double() if dtype == torch.float64 else model.float()).to(DEV)
    X, lens = _utterances(3, D, 23, dtype)
    captured = {}

    def spying(real):
        def call(*args, **kwargs):
            out = real(*args, **kwargs)
            captured['sr'] = out[0].clone()           # (both return the state posteriors first)
            return out
        return call
    from beer_amd.inference import batch as batch_mod
    import unittest.mock as mock
    with mock.patch.object(batch_mod.hk, 'scatter', spying(hk.scatter)), \
            mock.patch.object(batch_mod.hk, 'posteriors_fused', spying(hk.posteriors_fused)):
        elbo = accumulate_elbo(model, (X, lens))
    stats = FrameStats(X, 'diagonal')
    _, resps = kernels.mixtureset_estep(stats, ns.means_precisions.natural_form(),
                                        ems.leaf_log_weights(), S, G, 'diagonal')
    acc = kernels.normal_accumulate(stats, resps, captured['sr'], S, G, 'diagonal')
    got = elbo._acc_stats[ns.means_precisions]
    assert torch.equal(got, acc.to(got.dtype))


# ---- 3c. an alignment graph that forces a state far from the frames ------------------------

def _sparse_model(dtype, unused, apart, K=128, D=6, own=8, seed=24):
    '''(model, units): three 3-state units over a pool of K unit-variance Gaussians in four
    clusters `apart` standard deviations apart -- the 24 Gaussians the states of s0 use around
    the origin, those of s1 and s2 around apart e_0 and apart e_1, the rest around -apart e_0.  State s uses
    the `own` Gaussians s * own .. and has concentration `unused` on every other one.'''
    torch.manual_seed(seed)
    common = {'prior_strength': 1., 'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}
    conf = {'speech': {'topology': SPEECH, 'shared_normal_pool': K, **common}}
    names = ['s0', 's1', 's2']
    units, _ = hmm_cmds.build_units(conf, {'speech': names}, torch.zeros(D), torch.ones(D))
    graph, _, _ = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    ns = beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=K, noise_std=.5,
                               cov_type='diagonal')
    centre = torch.zeros(K, D)
    centre[3 * own:6 * own, 0] = apart
    centre[6 * own:9 * own, 1] = apart
    centre[9 * own:, 0] = -apart
    ns.means_precisions.posterior.params.mean.add_(centre)          # (nothing memoised yet)
    alpha = tt.sparse_rows(np.random.default_rng(seed), 9, K, own)
    alpha[alpha < 1.] = unused
    tied = beer.TiedMixtureSet(beer.CategoricalSet.create(torch.from_numpy(alpha).float(), 1.), ns)
    model = beer.HMM.create(graph.compile(), tied)
    return (model.double() if dtype == torch.float64 else model.float()).to(DEV), units


@pytest.mark.parametrize('dtype,unused,apart', [(torch.float32, 1. / 128, 14.),
                                                (torch.float64, 1e-3, 40.)],
                         ids=['float32', 'float64'])
def test_forced_state_whose_linear_sum_underflows(dtype, unused, apart):
    '''Every frame lies next to a Gaussian of unit s0, the transcription says s1 (s1 s2): the
    only states allowed have p = 0 in the linear domain.  The forward-backward completes and
    the statistics are the truth's.

    The geometry, from the number formats: a state underflows when its own Gaussians have
    e < 2^-94 (float32), i.e. lie more than sqrt(2 * 94 ln 2) = 11.4 standard deviations from
    the frame -- 14 here -- and the Gaussians next to the frame carry w = exp(psi(1/128) -
    psi(.)) = e^-130 (float64: e < 2^-970 beyond sqrt(2 * 970 ln 2) = 36.7 standard deviations
    -- 40 here -- and concentration 1e-3, w = e^-1003).  The frames sit at the
    ORIGIN: float32 evaluates l = -x'Px/2 + m'Px - ... with an absolute error of about
    2^-24 |x|^2 (the Gaussian kernels, not what is tested here), which 30 standard deviations
    from the origin is 1e-3 -- enough to move the state posteriors by more than the 1e-5 the
    statistics are held to -- and a few 1e-7 at |x|^2 ~ D.'''
    model, units = _sparse_model(dtype, unused, apart)
    groups, params = _groups_of(model)
    rng = np.random.default_rng(25)
    lens = [40, 55]
    mean = groups[0]['post'][0]
    X = torch.from_numpy(mean[rng.integers(0, 24, sum(lens))] +
                         rng.standard_normal((sum(lens), mean.shape[1]))).to(DEV, dtype)
    graphs = list(beer.graph.compile_alignments([['s1'], ['s1', 's2']], units))
    before = kernels.tied_log_entries()
    elbo = accumulate_elbo(model, (X, lens), inference_graphs=graphs)
    taken = kernels.tied_log_entries() - before
    print('entries in log space:', taken, 'of', sum(lens) * 9)
    assert taken >= 3 * lens[0]                 # (at least the three states the first may be in)
    assert np.isfinite(float(elbo.value))
    truth = tt.hmm_step([_npy(x) for x in _split(X, lens)], groups,
                        [_graph_dict(g.to_dense()) for g in graphs])
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    kl = float(torch.as_tensor(model.kl_div_posterior_prior()).sum())
    assert_close(float(elbo.value), truth['value'] + len(lens) * (truth['kl'] - kl), tol, 'value')
    (mp, w), (acc, wstats) = params[0], truth['acc'][0]
    got = _npy(elbo._acc_stats[mp])
    assert np.isfinite(got).all()
    errs = assert_stats_close(got, acc, mean.shape[1], tol, 'Gaussian statistics')
    print('Gaussian statistics:', errs, 'weights:', rel_err(_npy(elbo._acc_stats[w]), wstats))
    assert_close(_npy(elbo._acc_stats[w]), wstats, tol, 'weight statistics')


# ---- CapturedIteration ---------------------------------------------------------------------

def test_captured_iteration_records_a_tied_model():
    'The shard form: eager, captured, replayed -- the values and posteriors of the eager loop.'
    def run(captured):
        model, _ = _build('ploop', 'dirichlet', seed=26, warm=False)
        X, lens = _utterances(5, 4, 27, torch.float64)
        optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
        it = beer.CapturedIteration(model, optim, (X, lens))
        values, modes = [], []
        for _ in range(6):
            values.append(float(it() if captured else it._eager()))
            modes.append(it.mode)
        return values, modes, [_npy(p.posterior.natural_parameters())
                               for g in model.mean_field_factorization() for p in g]
    eager, _, post_e = run(False)
    replay, modes, post_r = run(True)
    assert 'replayed' in modes, modes
    assert_close(np.asarray(replay), np.asarray(eager), 1e-12, 'elbos')
    for a, b in zip(post_r, post_e):
        assert_close(a, b, 1e-12, 'posteriors')


# ---- 8. command line -----------------------------------------------------------------------

def run(argv, stdin=''):
    import io
    import sys
    from beer_amd.cli import main as cli_main
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_command_line_workflow_with_a_shared_pool(tmp_path):
    '''mkphones with `shared_normal_pool` on the workflow corpus -> mkphoneloop -> two
    accumulate / update epochs -> decode.'''
    import os
    import pickle
    import sys
    from helpers import GOLDEN, load_golden
    sys.path.insert(0, GOLDEN)
    from workflow_conf import HMM_CONF, SEED, shards, write_inputs
    corpus = load_golden('g17_corpus')
    tmp = str(tmp_path)
    paths = write_inputs(corpus, tmp)
    K = 24
    conf = HMM_CONF.replace('- group_name: speech-unit\n  n_normal_per_state: 2',
                            f'- group_name: speech-unit\n  shared_normal_pool: {K}')
    assert conf != HMM_CONF
    open(paths['hmmconf'], 'w').write(conf)
    run(['features', 'extract', paths['feaconf'], paths['wavscp'], paths['feadir']])
    run(['features', 'archive', paths['feadir'], paths['feats']])
    run(['dataset', 'create', tmp, paths['feats'], paths['dataset']])
    run(['-s', str(SEED), 'hmm', 'mkphones', '-d', paths['dataset'], paths['hmmconf'],
         paths['units'], paths['hmms']])
    run(['hmm', 'mkphoneloopgraph', '--start-end-group', 'non-speech-unit', paths['units'],
         paths['ploop_graph']])
    run(['hmm', 'mkdecodegraph', paths['ploop_graph'], paths['hmms'], paths['decode_graph']])
    mdl = os.path.join(tmp, '0.mdl')
    run(['hmm', 'mkphoneloop', paths['decode_graph'], paths['hmms'], mdl])
    model = pickle.load(open(mdl, 'rb'))
    tied = [m for m in model._emissions().modelsets if isinstance(m, beer.TiedMixtureSet)]
    assert len(tied) == 1 and len(tied[0].modelset) == K
    uttids = sorted(corpus['uttids'].tolist())
    logged = []
    for epoch in (1, 2):
        pkls = []
        for j, shard in enumerate(shards(uttids)):
            pkl = os.path.join(tmp, f'elbo_{epoch}_{j}.pkl')
            run(['hmm', 'accumulate', mdl, paths['dataset'], pkl], stdin='\n'.join(shard) + '\n')
            pkls.append(pkl)
        new = os.path.join(tmp, f'{epoch}.mdl')
        run(['hmm', 'update', '-o', os.path.join(tmp, 'optim.pth'), mdl, new],
            stdin='\n'.join(pkls) + '\n')
        total, count = None, 0
        for pkl in pkls:
            e, c = pickle.load(open(pkl, 'rb'))
            total, count = (e if total is None else total + e), count + c
        logged.append(float(total) / (count * total._datasize))
        mdl = new
    print('ELBO per frame:', logged)
    assert np.isfinite(logged).all() and logged[1] > logged[0]
    final = pickle.loads(pickle.dumps(pickle.load(open(mdl, 'rb'))))
    tied = [m for m in final._emissions().modelsets if isinstance(m, beer.TiedMixtureSet)]
    assert len(tied[0].modelset) == K and len(tied[0]) == len(tied[0].categoricalset)
    dec = run(['hmm', 'decode', mdl, paths['dataset']])
    assert len([line for line in dec.strip().split('\n') if line]) == len(uttids)
