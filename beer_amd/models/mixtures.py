"""Mixture and MixtureSet: the E-step of a GMM (config C1/C2) and of the GMM
emissions of HMM states (config C3).

API mirror of beer/models/mixture.py:14-115 and beer/models/mixtureset.py:
22-133.  `expected_log_likelihood` runs `beer_mixtureset_estep` (per-component
llh + logsumexp + responsibilities straight from the frames) and `accumulate`
runs `beer_normal_accumulate` (responsibility-weighted N_k, sum r x,
sum r xx^T in fp64): two kernel calls replace the reference's
cat / mul / mm / logsumexp / exp / mm sequence and its [T, Q] tensor.

Nested mixtures (components that are themselves a `MixtureSet`, at any depth) run
as the flat mixture over their leaves: a leaf's log-weight is the sum of its
ancestors' E[ln pi], the softmax over all leaves gives the value and the joint
responsibilities, and every level's weight statistics are sums of the leaf counts
over its subtrees ("Nested mixtures").  The same kernels run.

`TiedMixtureSet` (no reference counterpart): S mixtures that share ONE pool of K Gaussians
and differ in their weights only -- the pool is evaluated once per frame, and what is
state-specific are three [T, K] x [K, S]-shaped products (`beer_tied_lognorm`,
`beer_tied_accumulate`; DESIGN.md, "Tied mixtures").
"""

import torch

from .. import kernels
from .basemodel import DiscreteLatentModel
from .gaussians import NormalSet
from .modelset import ModelSet
from .weights import Categorical, CategoricalSet, SBCategorical, SBCategoricalSet

__all__ = ['Mixture', 'MixtureSet', 'TiedMixtureSet']


def _merge_groups(l1, l2):
    'Zip two mean-field factorizations, padding the shorter one.'
    l1, l2 = list(l1), list(l2)
    n = max(len(l1), len(l2))
    l1 += [[] for _ in range(n - len(l1))]
    l2 += [[] for _ in range(n - len(l2))]
    return [u + v for u, v in zip(l1, l2)]


def _fused(modelset):
    'True when the component set is a plain NormalSet the kernels can take.'
    return isinstance(modelset, NormalSet)


def _like(param, t):
    ref = param.stats
    return t.to(dtype=ref.dtype, device=ref.device)


def _leaves(modelset):
    'The NormalSet under a (possibly nested) set of mixtures.'
    while isinstance(modelset, MixtureSet):
        modelset = modelset.modelset
    if not isinstance(modelset, NormalSet):
        raise NotImplementedError('Mixture components must be a NormalSet or a MixtureSet '
                                  f'of NormalSets, got {type(modelset).__name__}')
    return modelset


def _leaf_counts(acc):
    'N_k of every leaf [K] (fp64) from accumulated Gaussian statistics [K, Q].'
    return -2. * acc[:, -2]


def _weight_stats(weights, counts):
    '''{parameter: statistics} of the weights `weights` (one categorical or a set of them)
    from the counts of their categories ([n] or [rows, n], fp64): the raw counts for
    stick-breaking weights, the Dirichlet's statistics (last column: the row total) else.'''
    param = weights.mean_field_factorization()[0][0]
    if isinstance(weights, (SBCategorical, SBCategoricalSet)):
        return {param: _like(param, counts)}
    stats = counts.clone()
    stats[..., -1] = counts.sum(dim=-1)
    return {param: _like(param, stats)}


class Mixture(DiscreteLatentModel):
    'Bayesian mixture model.'

    @classmethod
    def create(cls, modelset, categorical=None, prior_strength=1.):
        tensor = modelset.mean_field_factorization()[0][0].prior._tensors()[0]
        if categorical is None:
            weights = torch.ones(len(modelset), dtype=tensor.dtype, device=tensor.device)
            weights /= len(modelset)
            categorical = Categorical.create(weights, prior_strength)
        return cls(categorical, modelset)

    def __init__(self, categorical, modelset):
        super().__init__(modelset)
        self.categorical = categorical

    @property
    def nested(self):
        'True when the components are themselves mixtures (a MixtureSet).'
        return isinstance(self.modelset, MixtureSet)

    @property
    def normalset(self):
        'The Gaussians at the leaves: the components, or those of the nested sets.'
        return _leaves(self.modelset)

    def _log_weights(self, tensorconf=None):
        'E[ln pi] of every component; of every LEAF when nested (the sum over its ancestors).'
        lw = self.categorical.log_weights()
        if not self.nested:
            return lw
        inner = self.modelset.leaf_log_weights()
        return (lw.to(inner.dtype)[:, None] + inner).reshape(-1)

    def mean_field_factorization(self):
        return _merge_groups(self.modelset.mean_field_factorization(),
                             self.categorical.mean_field_factorization())

    def sufficient_statistics(self, data):
        return self.modelset.sufficient_statistics(data)

    def expected_log_likelihood(self, stats, labels=None, **kwargs):
        '''Per-frame ELBO term sum_k r ln N_k - sum_k r (ln r - E ln pi_k),
        i.e. logsumexp_k(l_tk + E ln pi_k); with `labels` the log-likelihood
        of the labelled component (mixture.py:70-93).'''
        if not _fused(self.modelset):
            return self._nested_expected_log_likelihood(stats, labels)
        ns = self.modelset
        K = len(ns)
        if kernels.is_dense(stats):
            return self._dense_expected_log_likelihood(stats, labels)
        wide = kernels.wide_mixture_split(stats, K, ns.cov_type) if labels is None else None
        if wide:
            # more than 256 components: blocks on the matrix cores, two-level softmax;
            # the cache holds the factored responsibilities (`.dense()` -> [T, K])
            log_norm, resps = kernels.wide_mixture_estep(
                stats, ns.means_precisions.natural_form(), self._log_weights().view(1, K), K,
                ns.cov_type, wide)
        else:
            log_norm, resps = kernels.mixtureset_estep(
                stats, ns.means_precisions.natural_form(), self._log_weights().view(1, K),
                1, K, ns.cov_type, labels=labels)
        self.cache['resps'] = resps
        value = log_norm.view(-1)
        if kernels.has_source(stats):
            # differentiable frames (one sample per frame of a VAE): the gradient flows
            # through sum_k r_k l_k only, as in the statistics-in variant below
            value = kernels.attach_frame_grad(
                stats, value, resps.dense() if wide else resps,
                ns.means_precisions.natural_form())
        return value

    def _log_mean_weights(self):
        '''ln E[pi] of every component (float64); of every LEAF when nested: the sum of the
        ln E[pi] down to it -- the predictive twin of `_log_weights`.'''
        lw = self.categorical.mean.double().log()
        if not self.nested:
            return lw
        inner = self.modelset.leaf_log_mean_weights()
        return (lw.to(inner.device)[:, None] + inner).reshape(-1)

    def predictive_log_likelihood(self, data_or_stats):
        '''ln p(x_t | posterior) [T]: the posterior-predictive density of the mixture,
        ln sum_k E[pi_k] St_k(x_t) -- the mean weights and the Student-t predictive densities of
        the Gaussians, not E[ln pi] and the expected log-likelihoods.  Frames [T, D] or their
        lazy statistics; dense or differentiable statistics raise `NotImplementedError`.'''
        ns = self.normalset
        K = len(ns)
        stats = kernels.predictive_frames(data_or_stats, ns.means_precisions.likelihood_fn.dim,
                                          ns.cov_type)
        return kernels.mixtureset_predictive(
            stats, ns.means_precisions.posterior.predictive_table(),
            self._log_mean_weights().view(1, K), 1, K, ns.cov_type).view(-1)

    def _dense_expected_log_likelihood(self, stats, labels):
        '''Statistics-in variant (prior of a VAE): same value, and the gradient
        w.r.t. the statistics flows through sum_k r_k l_k only (mixture.py:92).'''
        ns = self.modelset
        K = len(ns)
        fn = ns.means_precisions.likelihood_fn
        nparams = ns.means_precisions.natural_form()
        pc = kernels.dense_llh(stats, nparams, fn.dim)
        if labels is None:
            log_norm, resps = kernels.dense_softmax(pc, self._log_weights().view(1, K), 1, K)
            value = log_norm.view(-1)
        else:
            lab = torch.as_tensor(labels).to(device=pc.device, dtype=torch.int64).view(-1, 1)
            resps = torch.zeros_like(pc).scatter_(1, lab, 1.)
            value = kernels.rowdot(pc, resps)
        self.cache['resps'] = resps
        return kernels.attach_stats_grad(stats, value, resps, nparams)

    def _nested_expected_log_likelihood(self, stats, labels):
        '''Components that are mixtures: the flat mixture over the K leaves.  Without labels
        the value is logsumexp over the leaves of l_tk + (sum of the ancestors' E ln pi),
        with labels the labelled component's log-normaliser (its own leaves only, the outer
        weight left out); the cache holds the joint responsibilities over the leaves.  No
        gradient: the reference's MixtureSet detaches its log-normaliser (mixtureset.py:93).'''
        ns = self.normalset
        K, M = len(ns), len(self.modelset)
        nparams = ns.means_precisions.natural_form()
        dense = kernels.is_dense(stats)
        if dense:
            pc = kernels.dense_llh(stats, nparams, ns.means_precisions.likelihood_fn.dim)
        if labels is None:
            lw = self._log_weights().view(1, K)
            if dense:
                log_norm, resps = kernels.dense_softmax(pc, lw, 1, K)
            else:
                wide = kernels.wide_mixture_split(stats, K, ns.cov_type)
                if wide:
                    log_norm, resps = kernels.wide_mixture_estep(stats, nparams, lw, K,
                                                                 ns.cov_type, wide)
                else:
                    log_norm, resps = kernels.mixtureset_estep(stats, nparams, lw, 1, K,
                                                               ns.cov_type)
            self.cache['resps'], self.cache['state_resps'] = resps, None
            return log_norm.view(-1).detach()
        # the M outer components as M mixtures of their leaves
        lw = self.modelset.leaf_log_weights()
        if dense:
            log_norm, resps = kernels.dense_softmax(pc, lw, M, K // M)
        else:
            log_norm, resps = kernels.mixtureset_estep(stats, nparams, lw, M, K // M,
                                                       ns.cov_type)
        lab = torch.as_tensor(labels).to(device=log_norm.device, dtype=torch.int64).view(-1, 1)
        onehot = torch.zeros_like(log_norm).scatter_(1, lab, 1.)
        self.cache['resps'], self.cache['state_resps'] = resps, onehot
        return kernels.rowdot(log_norm, onehot)

    def _weights_accumulate(self, acc):
        '{weights parameter: statistics} of every level from the Gaussian statistics [K, Q].'
        K = acc.shape[0]
        if not self.nested:
            wparam = self.categorical.mean_field_factorization()[0][0]
            if isinstance(self.categorical, SBCategorical):
                # stick-breaking weights take the raw counts N_k (categorical.py:149-151)
                wacc = -2. * acc[:, -2]
            else:
                wacc = kernels.weights_from_acc(acc, 1, K).view(-1)
            return {wparam: _like(wparam, wacc)}
        counts = _leaf_counts(acc).view(len(self.modelset), -1)
        return {**_weight_stats(self.categorical, counts.sum(dim=-1)),
                **self.modelset.leaf_weights_accumulate(counts)}

    def accumulate(self, stats):
        ns = self.normalset
        K = len(ns)
        sr = self.cache.get('state_resps')
        S, G = (K, 1) if sr is None else (sr.shape[1], K // sr.shape[1])
        if kernels.is_dense(stats):
            acc = kernels.dense_accumulate(stats, self.cache['resps'], sr, S, G)
        else:
            acc = kernels.normal_accumulate(stats, self.cache['resps'], sr, S, G, ns.cov_type)
        return {**self._weights_accumulate(acc),
                ns.means_precisions: _like(ns.means_precisions, acc)}

    def posteriors(self, data):
        'Responsibilities of the components [T, K]; nested: the leaves\' summed per component.'
        stats = self.sufficient_statistics(data)
        ns = self.normalset
        K = len(ns)
        _, resps = kernels.mixtureset_estep(
            stats, ns.means_precisions.natural_form(), self._log_weights().view(1, K),
            1, K, ns.cov_type)
        if self.nested:
            resps = resps.view(len(resps), len(self.modelset), -1).sum(dim=-1)
        return resps


class MixtureSet(ModelSet):
    'Set of S mixtures with G components each (component k belongs to k // G).'

    @classmethod
    def create(cls, size, modelset, prior_strength=1.):
        n_comp = len(modelset) // size
        weights = torch.ones(size, n_comp) / n_comp
        return cls(CategoricalSet.create(weights, prior_strength), modelset)

    def __init__(self, categoricalset, modelset):
        super().__init__()
        self.categoricalset = categoricalset
        self.modelset = modelset

    @property
    def n_comp_per_mixture(self):
        return len(self.modelset) // len(self)

    @property
    def nested(self):
        'True when the components are themselves mixtures (a MixtureSet).'
        return isinstance(self.modelset, MixtureSet)

    @property
    def normalset(self):
        'The Gaussians at the leaves: the components, or those of the nested sets.'
        return _leaves(self.modelset)

    @property
    def n_leaves_per_mixture(self):
        'Gaussians under every mixture of the set (`n_comp_per_mixture` when not nested).'
        return len(self.normalset) // len(self)

    def _log_weights(self, tensorconf=None):
        return self.categoricalset.log_weights()

    def leaf_log_weights(self):
        '''E[ln pi] of every leaf Gaussian of every mixture [S, L]: the sum of the E[ln pi]
        of the leaf and of its ancestors inside this set.'''
        lw = self._log_weights()
        if not self.nested:
            return lw
        inner = self.modelset.leaf_log_weights()
        S, M = lw.shape
        return (lw.to(inner.dtype)[:, :, None] + inner.view(S, M, -1)).reshape(S, -1)

    def leaf_weights_accumulate(self, counts):
        '''{weights parameter: statistics} of this set and of the sets under it from the
        counts of the leaves [S, L] (fp64): a level's counts are the leaf counts summed
        over the subtrees of its categories.'''
        per = counts.reshape(len(self), self.n_comp_per_mixture, -1)
        out = _weight_stats(self.categoricalset, per.sum(dim=-1))
        if self.nested:
            out.update(self.modelset.leaf_weights_accumulate(per.reshape(-1, per.shape[-1])))
        return out

    def weights_accumulate(self, acc):
        '''{weights parameter: statistics} of every level from the leaves' Gaussian
        statistics [S * L, Q].'''
        if not self.nested and isinstance(self.categoricalset, CategoricalSet):
            wparam = self.categoricalset.weights
            S, G = len(self), self.n_comp_per_mixture
            return {wparam: _like(wparam, kernels.weights_from_acc(acc, S, G))}
        return self.leaf_weights_accumulate(_leaf_counts(acc).view(len(self), -1))

    def mean_field_factorization(self):
        return _merge_groups(self.modelset.mean_field_factorization(),
                             self.categoricalset.mean_field_factorization())

    def sufficient_statistics(self, data):
        return self.modelset.sufficient_statistics(data)

    def expected_log_likelihood(self, stats):
        '''Per-state mixture log-normaliser [T, S]; caches the component resps (the
        joint responsibilities of the leaves when nested).'''
        ns = self.normalset
        S, G = len(self), self.n_leaves_per_mixture
        if kernels.is_dense(stats):
            # statistics-in: no gradient, the log-normaliser is detached
            # (mixtureset.py:93)
            fn = ns.means_precisions.likelihood_fn
            pc = kernels.dense_llh(stats, ns.means_precisions.natural_form(), fn.dim)
            log_norm, resps = kernels.dense_softmax(pc, self.leaf_log_weights(), S, G)
        else:
            log_norm, resps = kernels.mixtureset_estep(
                stats, ns.means_precisions.natural_form(), self.leaf_log_weights(), S, G,
                ns.cov_type)
        self.cache['resps'] = resps.view(-1, S, G)
        return log_norm

    def leaf_log_mean_weights(self):
        '''ln E[pi] of every leaf Gaussian of every mixture [S, L] (float64): the sum of the
        ln E[pi] of the leaf and of its ancestors inside this set (`leaf_log_weights` with
        the logarithm of the mean in place of the mean of the logarithm).'''
        lw = self.categoricalset.mean.double().log()
        if not self.nested:
            return lw
        inner = self.modelset.leaf_log_mean_weights()
        S, M = lw.shape
        return (lw.to(inner.device)[:, :, None] + inner.view(S, M, -1)).reshape(S, -1)

    def predictive_log_likelihood(self, data_or_stats):
        '''Per-state posterior-predictive log-density [T, S]: ln sum_g E[pi_sg] St_sg(x_t), one
        kernel (`kernels.mixtureset_predictive`), nothing cached.  Frames [T, D] or their lazy
        statistics; dense or differentiable statistics raise `NotImplementedError`.'''
        ns = self.normalset
        S, G = len(self), self.n_leaves_per_mixture
        stats = kernels.predictive_frames(data_or_stats, ns.means_precisions.likelihood_fn.dim,
                                          ns.cov_type)
        return kernels.mixtureset_predictive(
            stats, ns.means_precisions.posterior.predictive_table(),
            self.leaf_log_mean_weights(), S, G, ns.cov_type)

    def accumulate(self, stats, resps):
        'Joint (state x component) responsibilities -> weights + Gaussian stats.'
        ns = self.normalset
        S, G = len(self), self.n_leaves_per_mixture
        comp = self.cache['resps'].reshape(-1, S * G)
        if kernels.is_dense(stats):
            acc = kernels.dense_accumulate(stats, comp, resps, S, G)
        else:
            acc = kernels.normal_accumulate(stats, comp, resps, S, G, ns.cov_type)
        return {**self.weights_accumulate(acc),
                ns.means_precisions: _like(ns.means_precisions, acc)}

    def __len__(self):
        cset = self.categoricalset
        return cset.n_components if isinstance(cset, SBCategoricalSet) else len(cset)

    def __getitem__(self, key):
        ncpm = self.n_comp_per_mixture
        if isinstance(key, int):
            return Mixture(self.categoricalset[key],
                           self.modelset[slice(key * ncpm, (key + 1) * ncpm)])
        if isinstance(key, slice):
            start = 0 if key.start is None else key.start * ncpm
            stop = len(self) if key.stop is None else key.stop * ncpm
            step = 1 if key.step is None else key.step * ncpm
            return self.__class__(self.categoricalset[key],
                                  self.modelset[slice(start, stop, step)])
        raise IndexError(f'Unsupported index: {key}')


class TiedMixtureSet(ModelSet):
    '''Set of S mixtures over the SAME K Gaussians (a tied-mixture / semi-continuous
    emission model): `modelset` is one `NormalSet`, the pool, and `categoricalset` holds a
    Dirichlet row of K weights per mixture.'''

    @classmethod
    def create(cls, size, modelset, prior_strength=1.):
        if not isinstance(modelset, NormalSet):
            raise NotImplementedError('the pool of a TiedMixtureSet must be a NormalSet, got '
                                      f'{type(modelset).__name__}')
        tensor = modelset.mean_field_factorization()[0][0].prior._tensors()[0]
        K = len(modelset)
        weights = torch.full((size, K), 1. / K, dtype=tensor.dtype, device=tensor.device)
        return cls(CategoricalSet.create(weights, prior_strength), modelset)

    def __init__(self, categoricalset, modelset):
        super().__init__()
        if categoricalset.weights.posterior.params.concentrations.shape[-1] != len(modelset):
            raise ValueError('a TiedMixtureSet needs one weight per Gaussian of the pool')
        self.categoricalset = categoricalset
        self.modelset = modelset

    @property
    def normalset(self):
        'The shared pool.'
        return self.modelset

    def _log_weights(self, tensorconf=None):
        'E[ln pi] [S, K] in float64 whatever the model\'s dtype (`Dirichlet.log_weights64`).'
        return self.categoricalset.weights.posterior.log_weights64()

    def mean_field_factorization(self):
        return _merge_groups(self.modelset.mean_field_factorization(),
                             self.categoricalset.mean_field_factorization())

    def sufficient_statistics(self, data):
        return self.modelset.sufficient_statistics(data)

    def estep(self, stats):
        '''(l [T, K], m [T], pc [T, S], lw [S, K]): the pool's expected log-likelihoods, their
        row maxima, the mixtures' log-normalisers and the E[ln pi] they were computed with --
        what `kernels.tied_accumulate` takes.'''
        if kernels.is_dense(stats):
            raise NotImplementedError('TiedMixtureSet takes frames, not dense statistics (the '
                                      'prior of a VAE): not supported')
        ns = self.modelset
        pool = kernels.normal_llh(stats, ns.means_precisions.natural_form(), ns.cov_type)
        lw = self._log_weights()
        pc, m = kernels.tied_lognorm(pool, lw, kernels.tied_log_counter(pool.device))
        return pool, m, pc, lw

    def expected_log_likelihood(self, stats):
        'Per-state mixture log-normaliser [T, S]; caches what `accumulate` needs.'
        tied = self.estep(stats)
        self.cache['tied'] = tied
        return tied[2]

    def predictive_log_likelihood(self, data_or_stats):
        raise NotImplementedError('TiedMixtureSet has no posterior-predictive density yet: the '
                                  'predictive kernels take mixtures that own their Gaussians')

    def weights_accumulate(self, counts):
        '{weights parameter: statistics} from the counts C [S, K] (last column <- row sum).'
        return _weight_stats(self.categoricalset, counts)

    def accumulate(self, stats, resps):
        'State posteriors [T, S] -> statistics of the weights and of the pool.'
        if kernels.is_dense(stats):
            raise NotImplementedError('TiedMixtureSet takes frames, not dense statistics')
        ns = self.modelset
        r, counts = kernels.tied_accumulate(*self.cache['tied'], resps)
        acc = kernels.normal_accumulate(stats, r, None, len(ns), 1, ns.cov_type)
        return {**self.weights_accumulate(counts),
                ns.means_precisions: _like(ns.means_precisions, acc)}

    def __len__(self):
        return len(self.categoricalset)

    def __getitem__(self, key):
        if isinstance(key, int):
            return Mixture(self.categoricalset[key], self.modelset)
        if isinstance(key, slice):
            return self.__class__(self.categoricalset[key], self.modelset)
        raise IndexError(f'Unsupported index: {key}')
