'''Bigram phone loop on the host: the command line and the reference's pickles.'''

import argparse
import io
import os

import numpy as np
import pytest

import beer_amd as beer
from beer_amd.cli import compat, hmm as hmm_cmds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _parser(cmd):
    parser = argparse.ArgumentParser()
    cmd.setup(parser)
    return parser


def test_cli_accepts_the_bigram_command_and_priors():
    assert hmm_cmds.mkphoneloopbigram in hmm_cmds.COMMANDS
    for prior in ('dirichlet2', 'hierarchical_dirichlet_process'):
        args = _parser(hmm_cmds.mkphoneloopbigram).parse_args(
            ['--weights-prior', prior, 'uni.mdl', 'bi.mdl'])
        assert (args.weights_prior, args.phoneloop, args.out) == (prior, 'uni.mdl', 'bi.mdl')
        args = _parser(hmm_cmds.mkphoneloop).parse_args(
            ['--weights-prior', prior, 'graph', 'hmms', 'out'])
        assert args.weights_prior == prior
    with pytest.raises(SystemExit):
        _parser(hmm_cmds.mkphoneloopbigram).parse_args(
            ['--weights-prior', 'dirichlet', 'uni.mdl', 'bi.mdl'])


def _load_pickle(arr):
    return compat.load(io.BytesIO(np.asarray(arr).tobytes()))


@pytest.mark.parametrize('key', ['mkphoneloop.dirichlet2', 'mkphoneloopbigram.dirichlet2',
                                 'mkphoneloop.hierarchical_dirichlet_process',
                                 'mkphoneloopbigram.hierarchical_dirichlet_process'])
def test_reference_bigram_pickles_load(key):
    g = np.load(os.path.join(GOLDEN, 'g20_bigram_pickles.npz'))
    model = _load_pickle(g[key])
    assert type(model) is beer.BigramPhoneLoop
    for name in ('graph', 'modelset', 'start_pdf', 'end_pdf', 'categoricalset'):
        assert name in model.__dict__ or name in model._modules, name
    cset = model.categoricalset
    P = len(model.start_pdf)
    if key.endswith('hierarchical_dirichlet_process'):
        assert type(cset) is beer.SBCategoricalSet
        assert cset.n_components == P
        assert type(cset.root_sb_categorical) is beer.SBCategorical
        conc = cset.stickbreaking.posterior.params.concentrations
        assert tuple(conc.shape) == (P * P, 2)
        # the posterior starts as the root's sticks, repeated for every row
        root = cset.root_sb_categorical.stickbreaking.posterior.params.concentrations
        np.testing.assert_array_equal(conc.numpy(), root.repeat(P, 1).numpy())
    else:
        assert type(cset) is beer.CategoricalSet
        conc = cset.weights.prior.params.concentrations.numpy()
        # mkphoneloopbigram ignores the unigram: every concentration 1 / P; mkphoneloop: P/2 / P
        want = 1. / P if key.startswith('mkphoneloopbigram') else .5
        np.testing.assert_allclose(conc, want, rtol=1e-12)


def test_hdp_from_a_dirichlet_unigram_is_a_clear_error():
    import torch
    cat = beer.Categorical.create(torch.ones(4) / 4, prior_strength=2.)
    with pytest.raises(ValueError, match='stick-breaking root'):
        beer.SBCategoricalSet.create(4, cat, prior_strength=2.)
