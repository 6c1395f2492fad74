'''Learned HMM transition probabilities on the host: categories, prior, pickles, CLI.'''

import argparse
import os
import pickle

import numpy as np
import pytest
import torch

from transitions_truth import NON_SPEECH, decode_graph

import beer_amd as beer
from beer_amd.cli import compat, hmm as hmm_cmds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _transitions(strength=1., **kw):
    graph, start, end, _ = decode_graph(**kw)
    cg = graph.compile()
    tr = beer.HMMTransitions.create(cg.trans_log_probs, list(end.values()),
                                    list(start.values()), strength)
    return tr, start, end, cg.trans_log_probs


def test_categories_and_prior_of_the_recipe_topologies():
    tr, start, end, trans0 = _transitions(strength=2.5, n_speech=3, n_nonspeech=2)
    # speech units: every state loop + next (2), the end state loop + exit (2); non-speech:
    # the first four states 4 arcs each, the end state loop + exit (2)
    assert tr.arities == [2, 4]
    ends, starts = set(end.values()), set(start.values())
    assert len(tr.group_states[0]) == 3 * 3 + 2 * 1
    assert len(tr.group_states[1]) == 2 * 4
    assert sorted(tr.exits()) == sorted(ends)
    assert len(tr.cat_src) == 2 * (3 * 3 + 2) + 4 * 8
    # no category crosses from a unit's end to a start state (the phone weights' block)
    for i, j in zip(tr.cat_src, tr.cat_dst):
        assert not (i in ends and j in starts)
    # prior concentrations: strength x the compiled graph's probabilities (exit: the residual)
    p = trans0.exp().double()
    first = 0
    pairs = list(zip(tr.cat_src, tr.cat_dst))
    for cs, n, states in zip(tr.categoricalsets, tr.arities, tr.group_states):
        conc = cs.weights.prior.params.concentrations.double()
        assert tuple(conc.shape) == (len(states), n)
        for r, j in enumerate(states):
            cats = pairs[first + r * n:first + (r + 1) * n]
            assert all(i == j for i, _ in cats)
            inside = sum(float(p[j, d]) for _, d in cats if d >= 0)
            want = [float(p[j, d]) if d >= 0 else 1 - inside for _, d in cats]
            np.testing.assert_allclose(conc[r].numpy(), 2.5 * np.array(want), rtol=1e-6)
        first += n * len(states)
    # a speech unit's end: loop .75, exit .25; a non-speech first state: four arcs of .25
    e = sorted(ends)[0]
    row = tr.group_states[0].index(e)
    np.testing.assert_allclose(sorted(tr.categoricalsets[0].weights.prior.params.concentrations[row]
                                      .tolist()), [2.5 * .25, 2.5 * .75], rtol=1e-6)
    # one mean-field group of their own
    assert tr.mean_field_factorization() == [tr.parameters_of_groups()]


def test_a_multi_exit_topology_is_refused():
    two_exits = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
                 {'start_id': 1, 'end_id': 2, 'trans_prob': .25}, {'start_id': 1, 'end_id': 3, 'trans_prob': .25},
                 {'start_id': 2, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 3, 'trans_prob': .5}]
    # (the decode graph builder itself refuses such a unit: only one state may precede its exit)
    with pytest.raises(ValueError):
        decode_graph(speech=two_exits, n_nonspeech=0)
    # a graph whose unit leaves from two states, with the ends named: refused
    cg = hmm_cmds.UnitTopology(two_exits).graph(0).compile()
    trans = torch.full((4, 4), -float('inf'))
    trans[:2, :2] = cg.trans_log_probs
    trans[2:, 2:] = cg.trans_log_probs
    trans[1, 2] = trans[0, 2] = np.log(.25)           # both states of unit 0 reach unit 1
    with pytest.raises(ValueError):
        beer.HMMTransitions.create(trans, [1, 3], [0, 2])
    with pytest.raises(ValueError):
        beer.HMMTransitions.create(trans, [1, 1], [0, 2])


def test_bigram_loops_refuse_learned_transitions():
    graph, start, end, ems = decode_graph()
    with pytest.raises(ValueError):
        hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet2', train_transitions=True)
    with pytest.raises(ValueError):
        beer.BigramPhoneLoop.create(graph.compile(), start, end, ems, train_transitions=True)


def test_pickle_round_trip():
    tr, *_ = _transitions(strength=3.)
    tr.categoricalsets[1].weights.posterior.params.concentrations[0, 0] += 7.
    back = pickle.loads(pickle.dumps(tr))
    assert isinstance(back, beer.HMMTransitions)
    assert (back.cat_src, back.cat_dst, back.arities, back.group_states) == \
        (tr.cat_src, tr.cat_dst, tr.arities, tr.group_states)
    for a, b in zip(back.parameters_of_groups(), tr.parameters_of_groups()):
        np.testing.assert_array_equal(a.posterior.params.concentrations.numpy(),
                                      b.posterior.params.concentrations.numpy())
        np.testing.assert_array_equal(a.prior.params.concentrations.numpy(),
                                      b.prior.params.concentrations.numpy())
        assert a.uuid == b.uuid
    np.testing.assert_allclose(back.expected_probs().numpy(), tr.expected_probs().numpy())


def test_reference_pickle_has_no_learned_transitions():
    ploop = compat.load(open(os.path.join(GOLDEN, 'ref_phoneloop.pkl'), 'rb'))
    assert type(ploop) is beer.PhoneLoop
    assert ploop.transitions is None
    assert len(ploop.mean_field_factorization()) == 1
    with pytest.raises(ValueError):
        ploop.expected_transition_probs()
    # (a missing attribute is still an AttributeError)
    with pytest.raises(AttributeError):
        ploop.no_such_attribute


def test_cli_flag_parses_and_builds():
    parser = argparse.ArgumentParser()
    hmm_cmds.mkphoneloop.setup(parser)
    args = parser.parse_args(['--train-transitions', '--transitions-prior-strength', '4',
                              'graph', 'hmms', 'out'])
    assert args.train_transitions and args.transitions_prior_strength == 4.
    args = parser.parse_args(['graph', 'hmms', 'out'])
    assert not args.train_transitions and args.transitions_prior_strength == 1.


def test_plain_hmm_topology():
    topo = hmm_cmds.UnitTopology(NON_SPEECH)
    cg = topo.graph(0).compile()
    tr = beer.HMMTransitions.create(cg.trans_log_probs)
    # one exit (the last state: its row does not sum to one), every other state's arcs
    # stay inside the unit
    assert list(tr.exits()) == [topo.n_emitting - 1]
    assert tr.arities == [2, 4]
