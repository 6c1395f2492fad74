"""Weights of discrete choices: mixing weights of a mixture, of the mixtures of
HMM states (`CategoricalSet`), and phone weights of a phone loop with a
Dirichlet or a truncated stick-breaking (Dirichlet-process) prior, the latter
optionally under a Gamma hyper-prior on its concentration.

Interface of beer/models/categorical.py:39-209 and categoricalset.py:15-64:
class names, `create(...)` arguments, the parameter attributes pickled models
carry (`weights`, `stickbreaking`, `concentration`, `ordering`) and the callback
protocol of the stick-breaking models (statistics are re-shaped BEFORE the
update, the hyper-prior moves AFTER it: SURVEY.md appendix B, quirk Q10).

Numerics: E[ln pi] of the Dirichlet models is one kernel call
(`beer_dirichlet_log_weights`, memoised per parameter version); the stick
bookkeeping -- ordering the sticks by count, the tail sums, the running sum of
E[ln(1 - v)] -- is `beer_sb_transform_stats` / `beer_sb_log_weights`
(csrc/expfam.hip), not a chain of sort / flip / cumsum launches.
"""

import torch

from .. import _hip
from ..dists import Dirichlet, Gamma
from .basemodel import Model
from .modelset import ModelSet
from .parameters import ConjugateBayesianParameter

__all__ = ['Categorical', 'SBCategorical', 'SBCategoricalHyperPrior', 'CategoricalSet',
           'SBCategoricalSet']


def _twin(dist_cls, *std_params):
    'Parameter whose prior and posterior start from the same standard parameters.'
    make = lambda: dist_cls.from_std_parameters(*[p.clone() for p in std_params])   # noqa: E731
    return ConjugateBayesianParameter(make(), make())


# ---- Dirichlet-distributed weights ---------------------------------------------------------

class _DirichletWeights:
    '''What `Categorical` and `CategoricalSet` share: one parameter `weights`
    holding the Dirichlet(s), statistics by the Dirichlet's likelihood function.'''

    @classmethod
    def create(cls, weights, prior_strength=1.):
        return cls(_twin(Dirichlet, weights.detach() * prior_strength))

    @property
    def mean(self):
        return self.weights.value()

    def mean_field_factorization(self):
        return [[self.weights]]

    def sufficient_statistics(self, data):
        return self.weights.likelihood_fn.sufficient_statistics(data)

    def expected_log_likelihood(self, stats):
        return self.weights.likelihood_fn(self.weights.natural_form(), stats)

    def log_weights(self):
        'E[ln pi] of every category (of every row for a set): one kernel call, memoised.'
        return self.weights.posterior.log_weights()


class Categorical(_DirichletWeights, Model):
    'One categorical distribution under a Dirichlet prior.'

    def __init__(self, weights):
        super().__init__()
        self.weights = weights

    def accumulate(self, stats):
        return {self.weights: stats.sum(dim=0)}


class CategoricalSet(_DirichletWeights, ModelSet):
    'S categorical distributions (the mixture weights of S states), one Dirichlet row each.'

    def __init__(self, weights):
        super().__init__()
        self.weights = weights

    def accumulate(self, stats, resps):
        return {self.weights: resps.t() @ stats}

    def accumulate_from_jointresps(self, jointresps_stats):
        return {self.weights: jointresps_stats.sum(dim=0)}

    def __len__(self):
        return len(self.weights)

    def __getitem__(self, key):
        rows = self.weights[key]
        return type(self)(rows) if isinstance(key, slice) else Categorical(rows)


# ---- stick-breaking weights ------------------------------------------------------------------

class SBCategorical(Model):
    '''Categorical whose weights are built from sticks, pi_i = v_i prod_{j before i}
    (1 - v_j), v_i ~ Beta stored as a two-column Dirichlet; the sticks are kept in
    order of decreasing count (`ordering[r]` = category of stick r).'''

    @classmethod
    def _sticks(cls, truncation, prior_strength):
        ab = torch.ones(truncation, 2)
        ab[:, 1] = prior_strength
        return _twin(Dirichlet, ab)

    @classmethod
    def create(cls, truncation, prior_strength=1.):
        return cls(cls._sticks(truncation, prior_strength))

    def __init__(self, stickbreaking):
        super().__init__()
        self.stickbreaking = stickbreaking
        conc = stickbreaking.posterior.params.concentrations
        # (any truncation, like the reference: up to 1024 sticks the kernels rank them in
        # LDS, beyond that on the global arrays -- csrc/expfam.hip)
        self.ordering = torch.arange(conc.shape[0], device=conc.device)
        stickbreaking.register_callback(self._transform_stats, notify_before_update=True)

    # -- kernels
    def _conc(self):
        return _hip.on_device(self.stickbreaking.posterior.params.concentrations)

    def _transform_stats(self):
        '''Before the update: re-order the sticks by the counts that just arrived and
        turn the counts [P] into the sticks' statistics [P, 2].'''
        counts = _hip.on_device(self.stickbreaking.stats)
        ordering = torch.empty(counts.shape[0], dtype=torch.int64, device=counts.device)
        pairs = torch.empty(counts.shape[0], 2, dtype=counts.dtype, device=counts.device)
        _hip.call('beer_sb_transform_stats', _hip.dtype_code(counts.dtype), counts.shape[0],
                  _hip.ptr(counts), _hip.ptr(ordering), _hip.ptr(pairs))
        home = self.stickbreaking.stats.device                 # where the model lives
        self.ordering = ordering.to(home)
        self.stickbreaking.stats = pairs.to(home)

    def _log_weights_and_tail(self):
        '(E[ln pi] [P] in the categories order, sum_i E[ln(1 - v_i)] as a 0-dim tensor).'
        conc = self._conc()
        order = _hip.on_device(self.ordering)
        log_w = torch.empty(conc.shape[0], dtype=conc.dtype, device=conc.device)
        tail = torch.empty((), dtype=conc.dtype, device=conc.device)
        _hip.call('beer_sb_log_weights', _hip.dtype_code(conc.dtype), conc.shape[0],
                  _hip.ptr(conc), _hip.ptr(order), _hip.ptr(log_w), _hip.ptr(tail))
        return log_w, tail

    # -- model protocol
    @property
    def reverse_ordering(self):
        'Stick of every category: the inverse permutation of `ordering`.'
        inverse = torch.empty_like(self.ordering)
        inverse[self.ordering] = torch.arange(len(self.ordering), device=self.ordering.device)
        return inverse

    @property
    def mean(self):
        'E[pi] under independent sticks: E[v_i] prod_{j before i} E[1 - v_j].'
        conc = self.stickbreaking.posterior.params.concentrations
        ab = conc[self.ordering.to(conc.device)]
        total = ab.sum(dim=-1) + torch.finfo(ab.dtype).eps
        stick, rest = ab[:, 0] / total, (ab[:, 1] / total).cumprod(dim=0)
        stick[1:] = stick[1:] * rest[:-1]
        return stick[self.reverse_ordering.to(stick.device)]

    def sufficient_statistics(self, data):
        return data

    def mean_field_factorization(self):
        return [[self.stickbreaking]]

    def log_weights(self):
        return self._log_weights_and_tail()[0]

    def expected_log_likelihood(self, stats):
        return stats @ self.log_weights().to(dtype=stats.dtype, device=stats.device)

    def accumulate(self, stats):
        return {self.stickbreaking: stats.sum(dim=0)}


class SBCategoricalHyperPrior(SBCategorical):
    '''Stick-breaking categorical whose concentration (the second Beta parameter of
    every stick's prior) has a Gamma prior: after every update of the sticks the
    Gamma posterior takes one full natural-gradient step on (sum_i E[ln(1 - v_i)], P)
    and writes its mean back into the sticks' prior.'''

    @classmethod
    def create(cls, truncation, prior_strength=1., hyper_prior_strength=1.):
        mean = torch.ones(1) * prior_strength
        shape = torch.ones_like(mean) * hyper_prior_strength
        concentration = _twin(Gamma, shape, hyper_prior_strength / mean)
        return cls(cls._sticks(truncation, prior_strength), concentration)

    def __init__(self, stickbreaking, concentration):
        super().__init__(stickbreaking)
        self.concentration = concentration
        stickbreaking.register_callback(self._on_stickbreaking_update)
        concentration.register_callback(self._on_concentration_update)
        self._on_concentration_update()

    def _on_concentration_update(self):
        self.stickbreaking.prior.params.concentrations[:, 1] = self.concentration.value()

    def _on_stickbreaking_update(self):
        _, tail = self._log_weights_and_tail()
        n_sticks = torch.full_like(tail, float(len(self.ordering)))
        self.concentration.stats = torch.stack([tail, n_sticks]).to(self.concentration.stats.device)
        self.concentration.natural_grad_update(lrate=1.)


# ---- a set of stick-breaking categoricals under one root (hierarchical DP) ---------------

class SBCategoricalSet(Model):
    '''n_components stick-breaking categoricals (the rows of a bigram model) whose prior
    is centred on a root `SBCategorical`: the hierarchical Dirichlet process of
    beer/models/categoricalset.py:167-307.  Every row's sticks follow the ROOT's ordering
    and are never re-sorted; the root itself is not re-estimated (the reference leaves its
    update unregistered) and is not part of the mean-field groups.'''

    @classmethod
    def create(cls, n_components, root_sb_categorical, prior_strength=1.,
               optim_cls=torch.optim.Adam, optim_args=None, epochs=15_000):
        if optim_args is None:
            optim_args = {'lr': 1e-3}
        if not isinstance(root_sb_categorical, SBCategorical):
            raise ValueError('the hierarchical Dirichlet process needs a stick-breaking root '
                             f'(SBCategorical), got {type(root_sb_categorical).__name__}: a '
                             'unigram trained with the "dirichlet" prior has no sticks')
        mean = root_sb_categorical.mean
        K = len(mean)
        params = torch.ones(n_components, K, 2, dtype=mean.dtype, device=mean.device)
        # the prior from the root's mean and 1 - its running sum, in CATEGORY order
        # (categoricalset.py:141-154)
        params[:, :, 0] = prior_strength * mean
        params[:, :, 1] = prior_strength * (1 - mean.cumsum(dim=0))
        prior = Dirichlet.from_std_parameters(params.reshape(-1, 2))
        post = root_sb_categorical.stickbreaking.posterior.params.concentrations
        posterior = Dirichlet.from_std_parameters(post.repeat(n_components, 1).clone())
        param = ConjugateBayesianParameter(prior, posterior)
        return cls(n_components, param, root_sb_categorical, prior_strength, optim_cls,
                   optim_args, epochs)

    def __init__(self, n_components, stickbreaking, root_sb_categorical, concentration,
                 optim_cls, optim_args, epochs):
        super().__init__()
        self.n_components = n_components
        self.stickbreaking = stickbreaking
        self.root_sb_categorical = root_sb_categorical
        self.concentration = concentration
        self.optim_cls = optim_cls
        self.optim_args = optim_args
        self.epochs = epochs
        stickbreaking.register_callback(self._transform_stats, notify_before_update=True)

    @property
    def ordering(self):
        return self.root_sb_categorical.ordering

    @property
    def reverse_ordering(self):
        return self.root_sb_categorical.reverse_ordering

    def _conc(self):
        return _hip.on_device(self.stickbreaking.posterior.params.concentrations)

    def _transform_stats(self):
        '''Before the update: the counts [n, K] of every row, in the root's stick order,
        as the sticks' statistics [n K, 2]: (count of the stick, counts of it and of the
        sticks after it) (categoricalset.py:215-224); `beer_sb_set_transform_stats`.'''
        home = self.stickbreaking.stats.device
        counts = _hip.on_device(self.stickbreaking.stats)
        order = _hip.on_device(self.ordering)
        K = order.shape[0]
        pairs = torch.empty(self.n_components * K, 2, dtype=counts.dtype, device=counts.device)
        _hip.call('beer_sb_set_transform_stats', _hip.dtype_code(counts.dtype),
                  self.n_components, K, _hip.ptr(counts), _hip.ptr(order), _hip.ptr(pairs))
        self.stickbreaking.stats = pairs.to(home)

    def _log_prob_rows(self):
        '''E[ln pi] of every row [n, K] in category order, every row's sticks in the root's
        order: one `beer_sb_set_log_weights` launch.'''
        conc = self._conc()
        order = _hip.on_device(self.ordering)
        K = order.shape[0]
        out = torch.empty(self.n_components, K, dtype=conc.dtype, device=conc.device)
        _hip.call('beer_sb_set_log_weights', _hip.dtype_code(conc.dtype), self.n_components, K,
                  _hip.ptr(conc), _hip.ptr(order), _hip.ptr(out))
        return out

    @property
    def mean(self):
        c = self.stickbreaking.posterior.params.concentrations
        c = c.reshape(self.n_components, -1, 2)[:, self.ordering.to(c.device), :]
        norm = c.sum(dim=-1) + torch.finfo(c.dtype).eps
        weights = c[:, :, 0] / norm
        residual = (c[:, :, 1] / norm).cumprod(dim=1)
        weights[:, 1:] = weights[:, 1:] * residual[:, :-1]
        return weights[:, self.reverse_ordering.to(c.device)]

    def sufficient_statistics(self, data):
        return data

    def mean_field_factorization(self):
        return [[self.stickbreaking]]

    def log_weights(self):
        'E[ln pi] of every row [n, K], categories in their own order.'
        return self._log_prob_rows()

    def expected_log_likelihood(self, stats):
        log_prob = self._log_prob_rows()
        return stats @ log_prob.to(dtype=stats.dtype, device=stats.device)

    def accumulate(self, stats):
        raise NotImplementedError('SBCategoricalSet is trained from joint responsibilities '
                                  '(accumulate_from_jointresps)')

    def accumulate_from_jointresps(self, stats):
        return {self.stickbreaking: stats.sum(dim=0)}
