"""Explicit state durations (hidden semi-Markov model, Ferguson 1980): every emitting state owns
a categorical law over how long one stay lasts, 1 .. D frames, under a Dirichlet prior, learned
in the VB loop.  Not in the reference, whose states stay a geometric number of frames (the
self-loop of conf/hmm.yml).  The laws are tied by pdf id, so alignment graphs share them with
the free loop; the recursions are `beer_hsmm_forward_backward` / `beer_hsmm_viterbi`
(include/beer_hip.h has the definitions)."""

import numpy as np
import torch

from .. import _hip
from .basemodel import Model
from .weights import CategoricalSet

__all__ = ['StateDurations']


def _pdf_ids(graph):
    ids = graph.pdf_id_mapping
    return np.arange(graph.n_states, dtype=np.int64) if ids is None else \
        np.asarray([int(i) for i in ids], dtype=np.int64)


class StateDurations(Model):
    '''One `CategoricalSet` of [S_total, D] Dirichlet rows, row = pdf id: E[ln p], the KL and the
    update are the existing Dirichlet kernels.  Its own mean-field group, as `HMMTransitions`.
    `self_loops` [S_total] float64 keeps the self-loop probability the rows were made from: the
    other arcs of a state are renormalised by 1 / (1 - a_self) once its stay is the law's.'''

    @classmethod
    def create(cls, graph, max_duration, prior_strength=1.):
        '''Row id(j): prior and initial posterior concentrations `prior_strength` x the geometric
        law of state j's self-loop, a^(d-1) (1 - a), truncated at D = `max_duration` and
        renormalised (a state without a self-loop, and a pdf id no state has: the uniform law).
        ValueError: D outside 1 .. BEER_HSMM_MAX_DUR, states that share a pdf id with different
        self-loops, a self-loop of probability 1.'''
        D = int(max_duration)
        if not 1 <= D <= _hip.HSMM_MAX_DUR:
            raise ValueError(f'explicit durations: max_duration = {max_duration} is outside '
                             f'1 .. {_hip.HSMM_MAX_DUR} (BEER_HSMM_MAX_DUR)')
        trans = graph.trans_log_probs.detach().to('cpu', torch.float64)
        ids = _pdf_ids(graph)
        S_total = int(ids.max()) + 1
        a_state = torch.diagonal(trans).exp().numpy()
        a = np.full(S_total, -1.)
        for j, i in enumerate(ids):
            if a[i] >= 0 and abs(a[i] - a_state[j]) > 1e-6:
                raise ValueError(f'explicit durations: the states that share pdf id {i} have '
                                 f'different self-loops ({a[i]:.6g} and {a_state[j]:.6g}); one '
                                 'duration law cannot start from both')
            a[i] = a_state[j]
        if (a >= 1 - 1e-12).any():
            raise ValueError('explicit durations: a state whose self-loop has probability 1 is '
                             'never left')
        rows = np.full((S_total, D), 1. / D)
        d = np.arange(D)
        for i in np.nonzero(a > 0)[0]:
            law = a[i] ** d * (1 - a[i])
            rows[i] = law / law.sum()
        dtype = graph.trans_log_probs.dtype
        cset = CategoricalSet.create(torch.as_tensor(rows, dtype=dtype), prior_strength)
        return cls(cset, torch.as_tensor(np.maximum(a, 0.), dtype=torch.float64))

    def __init__(self, categoricalset, self_loops):
        super().__init__()
        self.categoricalset = categoricalset
        self.register_buffer('self_loops', self_loops)

    def __getstate__(self):
        state = super().__getstate__()
        state.pop('_memo', None)
        state.pop('_leave', None)
        return state

    @property
    def max_duration(self):
        return self.weights.posterior.params.concentrations.shape[1]

    @property
    def weights(self):
        return self.categoricalset.weights

    def __len__(self):
        return self.weights.posterior.params.concentrations.shape[0]

    def mean_field_factorization(self):
        'One group of their own: the Dirichlet rows.'
        return [[self.weights]]

    def log_dur(self):
        '''E[ln p] as the device table [S_total, D] float64 of the kernels, made once per
        parameter version (the Dirichlet's own memo says when it changed).'''
        src = self.categoricalset.log_weights()
        memo = self.__dict__.get('_memo')
        if memo is None or memo[0] is not src:
            memo = (src, _hip.on_device(src.detach(), torch.float64))
            self.__dict__['_memo'] = memo
        return memo[1]

    def leave_w(self):
        '-ln(1 - a_self) per pdf id, [S_total] float64 on the device.'
        memo = self.__dict__.get('_leave')
        if memo is None or memo.device.type != 'cuda':
            memo = _hip.on_device(-torch.log1p(-self.self_loops.detach().to(torch.float64)))
            self.__dict__['_leave'] = memo
        return memo

    def expected_durations(self):
        '(E[p] [S_total, D] float64, its means in frames [S_total] float64), on the host.'
        conc = self.weights.posterior.params.concentrations.detach().to('cpu', torch.float64)
        p = conc / conc.sum(dim=1, keepdim=True)
        return p, (p * torch.arange(1, p.shape[1] + 1, dtype=torch.float64)).sum(dim=1)

    def accumulate_counts(self, counts):
        'Statistics of the Dirichlet rows from the duration counts [S_total, D] (any device).'
        ref = self.weights.posterior.params.concentrations
        counts = counts.to(dtype=ref.dtype, device=ref.device)
        cstats = self.categoricalset.sufficient_statistics(counts)
        return self.categoricalset.accumulate_from_jointresps(cstats[None])

    # -- Model protocol (the statistics come from the HMM's E-step)
    def sufficient_statistics(self, data):
        return data

    def expected_log_likelihood(self, stats):
        raise NotImplementedError('the durations are scored inside the HMM\'s E-step')

    def accumulate(self, stats, parent_msg=None):
        return self.accumulate_counts(stats)
