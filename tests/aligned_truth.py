'''Helpers of the tests of learned transitions trained against alignment graphs
(tests/test_transitions_aligned_host.py, tests/test_gpu_transitions_aligned.py): a phone loop
over the recipe's unit topologies together with its units, alignment graphs of transcriptions,
a category map built from (unit name, local source state, local destination state) -- never
from pdf ids, which is how the code under test finds it -- and the float64 numpy truth of the
counts of every category.'''

import numpy as np
import torch

from transitions_truth import NON_SPEECH, SPEECH, forward_backward

import beer_amd as beer
from beer_amd.cli import hmm as hmm_cmds
from beer_amd.graph import compile_alignments


def loop_and_units(n_speech=3, n_nonspeech=1, D=4, cov='diagonal', ncomp=2, speech=SPEECH, seed=0):
    '(units {name: Graph}, graph, start_pdf, end_pdf, emissions) of a phone loop over mixed units.'
    torch.manual_seed(seed)
    common = {'n_normal_per_state': ncomp, 'prior_strength': 1., 'noise_std': 1.,
              'cov_type': cov, 'shared_cov': False}
    conf = {'speech': {'topology': speech, **common},
            'nonspeech': {'topology': NON_SPEECH, **common}}
    grouped = {'speech': [f's{i}' for i in range(n_speech)],
               'nonspeech': [f'n{i}' for i in range(n_nonspeech)]}
    if not n_nonspeech:
        del conf['nonspeech'], grouped['nonspeech']
    units, ems = hmm_cmds.build_units(conf, grouped, torch.zeros(D), torch.ones(D))
    names = [n for g in grouped.values() for n in g]
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return units, graph, start, end, ems


def loop_model(dtype=torch.float64, learned=True, on_host=False, **kwargs):
    '''(model on the host, units): a phone loop of 3 + 1 units unless told otherwise.
    `on_host`: for machines without a GPU -- the callbacks that write E[ln w] / E[ln a] into the
    loop's graph (Dirichlet kernels) are left out while the model is made, so its graph keeps
    the weights it was compiled with; categories, pdf ids and the refusals do not depend on them.'''
    units, graph, start, end, ems = loop_and_units(**kwargs)
    if on_host:
        from unittest import mock
        with mock.patch.object(beer.PhoneLoop, '_on_weights_update', lambda self: None), \
                mock.patch.object(beer.PhoneLoop, '_on_transitions_update', lambda self: None):
            model = beer.PhoneLoop.create(graph.compile(), start, end, ems,
                                          train_transitions=learned)
    else:
        model = beer.PhoneLoop.create(graph.compile(), start, end, ems, train_transitions=learned)
    return (model.double() if dtype == torch.float64 else model.float()), units


def unit_sizes(model):
    '{unit name: number of emitting states}: the units own consecutive states of the loop.'
    return {name: model.end_pdf[name] - model.start_pdf[name] + 1 for name in model.start_pdf}


class CategoryMap:
    '''The categories of the model's transitions by (unit name, local source state, local
    destination state) and (unit name) -> exit, from the states the loop gives each unit
    (`start_pdf` / `end_pdf` hold STATES of the loop's graph, whatever their name says).'''

    def __init__(self, model):
        tr = model.transitions
        self.sizes = unit_sizes(model)
        where = {}
        for name, first in model.start_pdf.items():
            for l in range(self.sizes[name]):
                where[first + l] = (name, l)
        self.intra, self.exit = {}, {}
        for c, (i, j) in enumerate(zip(tr.cat_src, tr.cat_dst)):
            name, l = where[i]
            if j >= 0:
                assert where[j][0] == name
                self.intra[(name, l, where[j][1])] = c
            else:
                assert l == self.sizes[name] - 1
                self.exit[name] = c
        self.n_categories = len(tr.cat_src)

    def chain(self, seq):
        '[(position in the transcription, unit name, local state)] of an alignment chain\'s states.'
        return [(k, name, l) for k, name in enumerate(seq) for l in range(self.sizes[name])]

    def arc(self, seq, a, b):
        'Category of the arc a -> b of the chain of `seq`; KeyError when it has none.'
        states = self.chain(seq)
        (ka, name, la), (kb, _, lb) = states[a], states[b]
        if ka == kb:
            return self.intra[(name, la, lb)]
        if la != self.sizes[name] - 1:
            raise KeyError((seq, a, b))
        return self.exit[name]

    def arcs(self, seq, dense):
        '''Categories of the arcs of the dense graph of `seq`, sorted by (source, destination),
        and per state the category of its last-frame posterior (-1: none).'''
        trans = dense.trans_log_probs.double().numpy()
        src, dst = np.nonzero(np.isfinite(trans))
        cats = np.asarray([self.arc(seq, a, b) for a, b in zip(src, dst)], dtype=np.int32)
        states = self.chain(seq)
        fin = dense.final_log_probs.double().numpy()
        last = np.asarray([self.exit[name] if np.isfinite(f) and l == self.sizes[name] - 1 else -1
                           for (_, name, l), f in zip(states, fin)], dtype=np.int32)
        return src, dst, cats, last


def expected_log_probs(transitions):
    'E[ln a] of every category from the posterior concentrations, float64 on the host.'
    parts = []
    for p in transitions.parameters_of_groups():
        conc = p.posterior.params.concentrations.detach().to('cpu', torch.float64)
        parts.append((torch.digamma(conc) - torch.digamma(conc.sum(-1, keepdim=True))).reshape(-1))
    return torch.cat(parts).numpy()


def utterance_counts(tmap, log_a, seq, dense, llh):
    '''Counts of every category from one utterance: the float64 numpy forward-backward on the
    dense matrix of its graph with E[ln a] on the arcs; `llh` [T, S] per-state log-likelihoods.
    Returns (counts [n_categories], gamma [T, S]).'''
    src, dst, cats, last = tmap.arcs(seq, dense)
    S = len(last)
    trans = np.full((S, S), -np.inf)
    trans[src, dst] = log_a[cats]
    gamma, xi = forward_backward(dense.init_log_probs.double().numpy(),
                                 dense.final_log_probs.double().numpy(), trans, llh)
    counts = np.zeros(tmap.n_categories)
    np.add.at(counts, cats, xi[src, dst])
    keep = last >= 0
    np.add.at(counts, last[keep], gamma[-1][keep])
    return counts, gamma


def alignment_set(units, sequences):
    return compile_alignments(sequences, units)
