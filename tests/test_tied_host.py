'''Tied mixtures without a GPU: the model's construction and protocol, how the batched E-step
and the command line see it, and the truth of the GPU tests (tests/tied_truth.py) held against
the oracle's `Mixture` and `MixtureSet`.'''

import pickle
import uuid
import warnings

import numpy as np
import pytest
import torch

import beer_amd as beer
from beer_amd.cli import hmm as hmm_cmds
from beer_amd.inference.batch import _groups, _n_gaussians, _normalset
from helpers import assert_close, orc
from transitions_truth import NON_SPEECH, SPEECH

import tied_truth as tt

COVS = ('full', 'diagonal', 'isotropic')


def _pool(K=8, D=4, cov='diagonal'):
    return beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=K, cov_type=cov)


# ---- the model ----------------------------------------------------------------------------

@pytest.mark.parametrize('cov', COVS)
def test_create_shapes_and_members(cov):
    ns = _pool(8, 4, cov)
    tied = beer.TiedMixtureSet.create(3, ns, prior_strength=2.)
    assert len(tied) == 3 and tied.normalset is ns and len(tied.modelset) == 8
    conc = tied.categoricalset.weights.posterior.params.concentrations
    assert tuple(conc.shape) == (3, 8)
    assert torch.allclose(conc, torch.full((3, 8), 2. / 8))       # uniform rows x strength
    member = tied[1]
    assert isinstance(member, beer.Mixture) and member.modelset is ns
    assert tuple(member.categorical.weights.posterior.params.concentrations.shape) == (8,)
    part = tied[1:]
    assert isinstance(part, beer.TiedMixtureSet) and len(part) == 2 and part.modelset is ns
    with pytest.raises(IndexError):
        tied['a']


def test_create_refuses_what_is_not_a_pool_of_gaussians():
    ns = _pool(8)
    with pytest.raises(NotImplementedError):
        beer.TiedMixtureSet.create(2, beer.MixtureSet.create(4, ns))
    with pytest.raises(ValueError):
        beer.TiedMixtureSet(beer.CategoricalSet.create(torch.ones(2, 5) / 5), ns)


def test_mean_field_groups_are_merged_into_one():
    tied = beer.TiedMixtureSet.create(3, _pool())
    groups = tied.mean_field_factorization()
    assert len(groups) == 1
    assert set(map(id, groups[0])) == {id(tied.modelset.means_precisions),
                                       id(tied.categoricalset.weights)}
    # ... and a joint set of a tied and an untied group stays one group
    joint = beer.JointModelSet([tied, beer.MixtureSet.create(2, _pool(6))])
    assert len(joint.mean_field_factorization()) == 1
    assert len(joint) == 5 and isinstance(joint[4], beer.Mixture)


def test_pickle_and_dtype_round_trip():
    tied = beer.TiedMixtureSet.create(3, _pool(), prior_strength=1.5)
    again = pickle.loads(pickle.dumps(tied))
    assert len(again) == 3 and len(again.modelset) == 8
    a = tied.categoricalset.weights.posterior.params.concentrations
    b = again.categoricalset.weights.posterior.params.concentrations
    assert torch.equal(a, b)
    assert again.double().categoricalset.weights.posterior.params.concentrations.dtype == \
        torch.float64
    assert again.float().modelset.means_precisions.posterior.params.mean.dtype == torch.float32


def test_dense_statistics_are_refused():
    tied = beer.TiedMixtureSet.create(3, _pool())
    with pytest.raises(NotImplementedError, match='dense'):
        tied.expected_log_likelihood(torch.zeros(5, 10))
    with pytest.raises(NotImplementedError, match='dense'):
        tied.accumulate(torch.zeros(5, 10), torch.zeros(5, 3))


def test_groups_of_mixed_emissions():
    tied = beer.TiedMixtureSet.create(3, _pool(8))
    untied = beer.MixtureSet.create(2, _pool(6))
    plain = _pool(4)
    groups = _groups(beer.JointModelSet([tied, untied, plain]))
    assert [(type(g).__name__, S, G) for g, S, G in groups] == \
        [('TiedMixtureSet', 3, 8), ('MixtureSet', 2, 3), ('NormalSet', 4, 1)]
    # columns S, statistics rows K (not S x G) for the tied group
    assert [_n_gaussians(*g) for g in groups] == [8, 6, 4]
    assert _normalset(groups[0][0]) is tied.modelset
    with pytest.raises(NotImplementedError):
        _groups(beer.Mixture.create(_pool()))


# ---- the command line -----------------------------------------------------------------------

def _conf(pool=None, ncomp=2):
    common = {'prior_strength': 1., 'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}
    speech = {'topology': SPEECH, **common}
    if ncomp is not None:
        speech['n_normal_per_state'] = ncomp
    if pool is not None:
        speech['shared_normal_pool'] = pool
    return {'speech': speech, 'nonspeech': {'topology': NON_SPEECH, 'n_normal_per_state': 3,
                                             **common}}


GROUPED = {'speech': ['a', 'b', 'c', 'd'], 'nonspeech': ['sil']}


def test_yaml_key_builds_a_tied_group_and_warns_about_the_ignored_key():
    with pytest.warns(UserWarning, match='n_normal_per_state is ignored'):
        units, ems = hmm_cmds.build_units(_conf(pool=16), GROUPED, torch.zeros(5), torch.ones(5))
    speech, nonspeech = ems.modelsets
    assert isinstance(speech, beer.TiedMixtureSet) and isinstance(nonspeech, beer.MixtureSet)
    assert len(speech) == 12 and len(speech.modelset) == 16 and len(nonspeech) == 5
    assert len(ems) == 17 and len(units) == 5
    with warnings.catch_warnings():
        warnings.simplefilter('error')                        # no key to ignore: no warning
        hmm_cmds.build_units(_conf(pool=16, ncomp=None), GROUPED, torch.zeros(5), torch.ones(5))
    # the decoding graph and the alignment graphs are built from the units as before
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(list(units)), units)
    assert sorted(start) == sorted(units) and len(graph.compile().pdf_id_mapping) == 17
    again = pickle.loads(pickle.dumps(ems))
    assert isinstance(again.modelsets[0], beer.TiedMixtureSet)


def _parent_build_units(groups_conf, grouped_names, mean, var):
    'The loop of `build_units` as it was before `shared_normal_pool` existed.'
    units, sets, next_pdf = {}, [], 0
    for group, names in grouped_names.items():
        conf = groups_conf[group]
        topo = hmm_cmds.UnitTopology(conf['topology'])
        for name in names:
            units[name] = topo.graph(next_pdf)
            next_pdf += topo.n_emitting
        n_states = topo.n_emitting * len(names)
        normals = beer.NormalSet.create(
            mean=mean, cov=var, size=n_states * conf['n_normal_per_state'],
            prior_strength=conf['prior_strength'], noise_std=conf['noise_std'],
            cov_type=conf['cov_type'], shared_cov=conf['shared_cov'])
        sets.append(beer.MixtureSet.create(n_states, normals,
                                           prior_strength=conf['prior_strength']))
    return units, beer.JointModelSet(sets)


class _Canonical(pickle.Pickler):
    """Tensors by value (torch's own reduction names their storage by its address)."""

    def reducer_override(self, obj):
        if isinstance(obj, torch.Tensor):
            return tuple, ((str(obj.dtype), tuple(obj.shape), obj.detach().numpy().tobytes()),)
        return NotImplemented


def test_without_the_key_mkphones_writes_what_it_wrote(monkeypatch):
    '''Same seed, no `shared_normal_pool`: byte for byte the pickle of the loop above -- with
    what no seed governs made equal for both: the parameters' uuids numbered in creation
    order, tensors pickled by value instead of by storage address.'''
    def dump(build):
        import io
        counter = iter(range(1, 1000))
        monkeypatch.setattr(uuid, 'uuid4', lambda: uuid.UUID(int=next(counter)))
        torch.manual_seed(3)
        out = io.BytesIO()
        _Canonical(out).dump(build(_conf(), GROUPED, torch.zeros(5), torch.ones(5)))
        return out.getvalue()
    new, old = dump(hmm_cmds.build_units), dump(_parent_build_units)
    assert len(new) > 10000 and new == old


# ---- the truth against the oracle ---------------------------------------------------------

@pytest.mark.parametrize('cov', COVS)
def test_truth_with_one_state_is_the_oracle_mixture(cov):
    case = tt.kernel_case(31, 1, 9, 5, 80, cov)
    stats = tt.suffstats(case['X'], cov)
    lw = orc.log_weights(case['alpha'][0])
    assert_close(orc.log_weights_set(case['alpha'])[0], lw, 1e-14, 'log weights')
    per_frame, resps = orc.mixture_estep(stats, case['exp_T'], 5, lw)
    acc_w, acc_n = orc.mixture_accumulate(stats, resps)
    l = tt.pool_llh(case['X'], cov, case['exp_T'])
    pc, _ = tt.lognorm(l, lw[None, :])
    C, r, acc = tt.statistics(l, lw[None, :], pc, np.ones((80, 1)), stats)
    assert_close(pc[:, 0], per_frame, 1e-12, 'log-normaliser')
    assert_close(r, resps, 1e-12, 'responsibilities')
    assert_close(acc, acc_n, 1e-12, 'Gaussian statistics')
    assert_close(tt.weight_stats(C)[0], acc_w, 1e-12, 'weight statistics')


@pytest.mark.parametrize('cov', COVS)
def test_truth_with_disjoint_blocks_is_the_oracle_mixtureset(cov):
    'Log-weight rows that are -inf outside disjoint blocks: the oracle\'s MixtureSet.'
    S, G, D, T = 4, 3, 5, 70
    case = tt.kernel_case(32, S, S * G, D, T, cov)
    stats = tt.suffstats(case['X'], cov)
    lw_set = orc.log_weights_set(case['alpha'][:, :G])
    log_norm, comp = orc.mixtureset_estep(stats, case['exp_T'], D, lw_set)
    g = case['g']
    wstats, nstats = orc.mixtureset_accumulate(stats, comp, g)
    lw = np.full((S, S * G), -np.inf)
    for s in range(S):
        lw[s, s * G:(s + 1) * G] = lw_set[s]
    l = tt.pool_llh(case['X'], cov, case['exp_T'])
    pc, _ = tt.lognorm(l, lw)
    C, r, acc = tt.statistics(l, lw, pc, g, stats)
    assert_close(pc, log_norm, 1e-12, 'log-normalisers')
    assert_close(acc, nstats, 1e-12, 'Gaussian statistics')
    blocks = np.stack([C[s, s * G:(s + 1) * G] for s in range(S)])
    assert_close(orc.cat_suffstats(blocks), wstats, 1e-12, 'weight statistics')
    assert np.all(C[lw == -np.inf] == 0)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('shape', tt.RANGE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ordinary_inputs_are_far_above_the_threshold(shape, dtype):
    '''The inputs of the GPU test `test_ordinary_data_stays_linear`: concentrations in [1, 4]
    give lw >= psi(1) - psi(4 K) > -7.5 and the frame's best Gaussian has e = 1, so
    p[t,s] >= e^-8, dozens of orders of magnitude above the threshold of either dtype.'''
    S, K, D, T = shape
    case = tt.kernel_case(13, S, K, D, T, 'full', dtype)
    assert case['lw'].min() > -7.5
    p = tt.linear_sum(case['l'], case['lw'])
    assert p.min() >= np.exp(-8.)
    assert p.min() > 1e20 * tt.THRESHOLD[dtype]


def test_extreme_inputs_are_below_it_and_far_from_it():
    'The inputs of the GPU range test (b): finite log-normalisers, entries below 2^-94, none near.'
    case = tt.extreme_case(14)
    pc, _ = tt.lognorm(case['l'], case['lw'])
    assert np.isfinite(pc).all()
    p, tau = tt.linear_sum(case['l'], case['lw']), tt.THRESHOLD['float32']
    assert (p < tau / 2).sum() > 0
    assert (p < tau / 2).sum() == (p < 2 * tau).sum()


def test_conservation_of_the_truth():
    case = tt.kernel_case(33, 7, 20, 4, 90, 'diagonal')
    pc, _ = tt.lognorm(case['l'], case['lw'])
    C, r, _ = tt.statistics(case['l'], case['lw'], pc, case['g'])
    assert_close(r.sum(axis=1), case['g'].sum(axis=1), 1e-12, 'sum_k r = sum_s g')
    assert_close(C.sum(axis=1), case['g'].sum(axis=0), 1e-12, 'sum_k C = sum_t g')
    assert_close(C.sum(axis=0), r.sum(axis=0), 1e-12, 'sum_s C = sum_t r')
