'''Nested mixtures on the host: construction, the mean-field grouping against the
reference's, the reference's pickles, the flattening of nested emission groups.'''

import io
import os

import numpy as np
import pytest
import torch

import beer_amd as beer
from beer_amd.cli import compat
from beer_amd.inference import batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
COVS = ('full', 'diagonal', 'isotropic')


def _golden(name):
    return np.load(os.path.join(GOLDEN, f'g21_nested_{name}.npz'))


def _load(arr):
    return compat.load(io.BytesIO(np.asarray(arr).tobytes()))


def _normalset(size, cov_type='diagonal', D=2):
    torch.manual_seed(0)
    return beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=size, prior_strength=1.,
                                 noise_std=1., cov_type=cov_type)


@pytest.mark.parametrize('cov_type', COVS)
def test_notebook_model_builds(cov_type):
    ns = _normalset(12, cov_type)
    mset = beer.MixtureSet.create(4, ns)
    model = beer.Mixture.create(mset)
    assert model.nested and mset.nested is False
    assert model.normalset is ns and mset.normalset is ns
    assert len(mset) == 4 and mset.n_comp_per_mixture == 3 and mset.n_leaves_per_mixture == 3
    assert tuple(model.categorical.weights.posterior._tensors()[0].shape) == (4,)


def test_deeper_nesting_counts_the_leaves():
    ns = _normalset(2 * 3 * 4)
    inner = beer.MixtureSet.create(6, ns)
    outer = beer.MixtureSet.create(2, inner)
    assert outer.nested and outer.normalset is ns
    assert outer.n_comp_per_mixture == 3 and outer.n_leaves_per_mixture == 12
    assert beer.Mixture.create(outer).normalset is ns


def test_flat_models_are_not_nested():
    ns = _normalset(4)
    assert not beer.Mixture.create(ns).nested
    assert beer.MixtureSet.create(2, ns).normalset is ns


def test_sb_categoricalset_as_inner_weights():
    ns = _normalset(12)
    root = beer.SBCategorical.create(3, prior_strength=1.)
    cset = beer.SBCategoricalSet.create(4, root, prior_strength=1.)
    mset = beer.MixtureSet(cset, ns)
    assert len(mset) == 4 and mset.n_leaves_per_mixture == 3
    groups = beer.Mixture.create(mset).mean_field_factorization()
    assert len(groups) == 1 and cset.stickbreaking in groups[0]


@pytest.mark.parametrize('name', list(COVS) + ['hmm'])
def test_mean_field_grouping_matches_the_reference(name):
    'One group: the Gaussians, the inner Dirichlets, the outer Dirichlet, in that order.'
    g = _golden(name)
    model = _load(g['model'])
    groups = model.mean_field_factorization()
    assert [len(grp) for grp in groups] == list(g['group_sizes'])
    params = [p for grp in groups for p in grp]
    for p, shape in zip(params, g['param_shapes']):
        # (rows of the natural parameters; a Dirichlet's row: its categories)
        rows = tuple(p.posterior._tensors()[0].shape)
        want = tuple(int(n) for n in shape if n)
        assert rows[0] == want[0]
        if type(p.posterior).__name__ == 'Dirichlet':
            assert rows == want
    ems = model.modelset if name != 'hmm' else model._emissions()
    assert params[0] is ems.normalset.means_precisions


def test_reference_pickles_load():
    g = _golden('pickles')
    deep = _load(g['depth3'])
    assert type(deep) is beer.Mixture
    assert type(deep.modelset) is beer.MixtureSet and type(deep.modelset.modelset) is beer.MixtureSet
    assert len(deep.modelset) == 2 and deep.modelset.n_leaves_per_mixture == 6
    assert len(deep.normalset) == 12
    assert [len(grp) for grp in deep.mean_field_factorization()] == [4]
    sets = _load(g['mixtureset2'])
    assert type(sets) is beer.MixtureSet and sets.nested
    assert sets.normalset.cov_type == 'full' and sets.n_leaves_per_mixture == 4


def test_nested_emission_groups_flatten():
    'HMM emissions: a nested MixtureSet is one group of S mixtures of its leaves.'
    model = _load(_golden('hmm')['model'])
    groups = batch._groups(model._emissions())
    assert [(S, G) for _, S, G in groups] == [(3, 6)]
    assert batch._normalset(groups[0][0]) is model._emissions().normalset
    flat = beer.MixtureSet.create(2, _normalset(6))
    joint = beer.JointModelSet([flat, model._emissions()])
    assert [(S, G) for _, S, G in batch._groups(joint)] == [(2, 3), (3, 6)]
