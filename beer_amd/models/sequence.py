"""HMM and PhoneLoop.

API mirror of beer/models/hmm.py:13-121 and beer/models/phoneloop.py:13-101.
The per-utterance methods below drive the same ragged-batch kernels as the
batched accumulator (beer_amd/inference/batch.py) with a batch of one.
"""

import numpy as np
import torch

from .. import _hip, hmm_kernels as hk, kernels
from ..stats import reference_layout_enabled
from .basemodel import DiscreteLatentModel, Model
from .gaussians import NormalSet
from .modelset import DynamicallyOrderedModelSet
from .durations import StateDurations
from .weights import Categorical, CategoricalSet, SBCategorical, SBCategoricalSet

__all__ = ['HMM', 'PhoneLoop', 'BigramPhoneLoop', 'HMMTransitions', 'StateDurations']


class HMMTransitions(Model):
    '''Learned transition probabilities of the units of an HMM (not in the reference, whose
    transition probabilities are the constants of conf/hmm.yml).  Every emitting state that
    owns categories has one per outgoing arc inside its unit, and the unit's end state one
    more, `exit` (the probability of leaving the unit: the residual of a phone loop's end
    state).  States are grouped by their number of categories into one `CategoricalSet`
    (Dirichlet rows) per arity, so that E[ln a], the KL and the update are the existing
    Dirichlet kernels.  Category c of the flat order (groups in `arities` order, rows, slots)
    is the arc `cat_src[c]` -> `cat_dst[c]`, or the exit of `cat_src[c]` when `cat_dst[c]`
    is -1.'''

    @classmethod
    def create(cls, trans_log_probs, end_states=(), start_states=(), prior_strength=1.):
        '''From a compiled graph's transition log-probabilities: `end_states` / `start_states`
        name the units' end / start states (a phone loop's end_pdf / start_pdf values: the
        block end -> start is not learned); without them every state with an incomplete row
        owns an exit.  Units are the connected parts of the graph once that block is removed;
        a unit whose exit is reached from more than one state is refused (ValueError).  Prior
        concentrations: prior_strength x the graph's transition probabilities.'''
        trans = trans_log_probs.detach().to('cpu', torch.float64)
        S = trans.shape[0]
        ends, starts = [int(i) for i in end_states], [int(i) for i in start_states]
        if len(set(ends)) != len(ends) or len(set(starts)) != len(starts):
            raise ValueError('learned transitions need distinct end / start states per unit')
        if set(ends) & set(starts):
            raise ValueError('learned transitions need units of at least two emitting states '
                             '(a unit whose start state is its end state)')
        intra = torch.isfinite(trans) & (trans.exp() > 0)
        if ends:
            intra[torch.as_tensor(ends)[:, None], torch.as_tensor(starts)[None, :]] = False
        probs = torch.where(intra, trans.exp(), torch.zeros_like(trans))
        mass = probs.sum(dim=1)
        exits = set(ends) if ends else {j for j in range(S) if mass[j] < 1 - 1e-6}
        # units: connected parts of the intra-unit arcs
        parent = list(range(S))

        def root(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i
        for i, j in torch.nonzero(intra).tolist():
            parent[root(i)] = root(j)
        per_unit = {}
        for e in exits:
            per_unit.setdefault(root(e), []).append(e)
        for r, members in per_unit.items():
            if len(members) > 1:
                raise ValueError('learned transitions: a unit whose exit is reached from more '
                                 f'than one state (states {sorted(members)})')
        if ends:
            # every other state of a unit must keep all of its mass inside the unit
            leak = [j for j in range(S) if j not in exits and mass[j] < 1 - 1e-6 and
                    bool(torch.isfinite(trans[j]).any())]
            if leak:
                raise ValueError('learned transitions: a unit whose exit is reached from more '
                                 f'than one state (states {leak[:8]} leave their unit)')
        rows = {}
        for j in range(S):
            dsts = torch.nonzero(intra[j]).view(-1).tolist()
            cats = [(d, float(probs[j, d])) for d in dsts]
            if j in exits:
                cats.append((-1, max(float(1 - mass[j]), 0.)))
            if cats:
                rows[j] = cats
        if not rows:
            raise ValueError('learned transitions: the graph has no arcs to learn')
        arities = sorted({len(c) for c in rows.values()})
        sets, src, dst, group_states = [], [], [], []
        for n in arities:
            states = [j for j in sorted(rows) if len(rows[j]) == n]
            w = torch.tensor([[p for _, p in rows[j]] for j in states],
                             dtype=trans_log_probs.dtype)
            sets.append(CategoricalSet.create(w, prior_strength))
            group_states.append(states)
            for j in states:
                src += [j] * n
                dst += [d for d, _ in rows[j]]
        return cls(sets, arities, group_states, src, dst)

    def __init__(self, categoricalsets, arities, group_states, cat_src, cat_dst):
        super().__init__()
        self.categoricalsets = torch.nn.ModuleList(categoricalsets)
        self.arities = list(arities)
        self.group_states = [list(g) for g in group_states]
        self.cat_src, self.cat_dst = list(cat_src), list(cat_dst)

    def __getstate__(self):
        state = super().__getstate__()
        state.pop('_index_memo', None)
        return state

    # -- categories
    def parameters_of_groups(self):
        return [cs.mean_field_factorization()[0][0] for cs in self.categoricalsets]

    def mean_field_factorization(self):
        'One group of their own: every arity\'s Dirichlet rows.'
        return [self.parameters_of_groups()]

    def intra(self):
        '(categories, sources, destinations) of the arcs inside the units.'
        cats = [c for c, d in enumerate(self.cat_dst) if d >= 0]
        return cats, [self.cat_src[c] for c in cats], [self.cat_dst[c] for c in cats]

    def exits(self):
        '{state: category} of the units\' exits.'
        return {self.cat_src[c]: c for c, d in enumerate(self.cat_dst) if d < 0}

    def index_tensors(self, device, end_states=()):
        '''int64 tensors on `device`, made once per (device, end states): (intra categories,
        their sources, their destinations, exit categories, their states, the exit categories
        of `end_states` in that order).'''
        key = (str(device), tuple(end_states))
        memo = self.__dict__.setdefault('_index_memo', {})
        if key not in memo:
            cats, src, dst = self.intra()
            ex = self.exits()
            missing = [e for e in end_states if e not in ex]
            if missing:
                raise ValueError(f'learned transitions: end states {missing} own no exit')
            t = lambda v: torch.as_tensor(v, dtype=torch.int64, device=device)   # noqa: E731
            memo[key] = (t(cats), t(src), t(dst), t(list(ex.values())), t(list(ex.keys())),
                         t([ex[e] for e in end_states]))
        return memo[key]

    def log_probs(self):
        'E[ln a] of every category, flat [n_categories] (one Dirichlet kernel per arity).'
        parts = [cs.log_weights().reshape(-1) for cs in self.categoricalsets]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def expected_probs(self):
        'E[a] of every category, flat [n_categories].'
        parts = []
        for p in self.parameters_of_groups():
            conc = p.posterior.params.concentrations
            parts.append((conc / conc.sum(dim=-1, keepdim=True)).reshape(-1))
        return torch.cat(parts)

    def accumulate_counts(self, counts):
        '''Statistics of every arity's Dirichlet rows from the counts of every category,
        flat [n_categories] (any device / dtype).'''
        out, first = {}, 0
        for cs, n, states in zip(self.categoricalsets, self.arities, self.group_states):
            ref = cs.mean_field_factorization()[0][0].posterior.params.concentrations
            block = counts[first:first + n * len(states)].to(dtype=ref.dtype, device=ref.device)
            first += n * len(states)
            cstats = cs.sufficient_statistics(block.view(len(states), n))
            out.update(cs.accumulate_from_jointresps(cstats[None]))
        return out

    def counts_from_kernel(self, arc_pos, arc_counts, src_flow):
        '''Category counts [n_categories] fp64 from the one-wave count kernels' outputs: the
        intra-unit arcs at their positions `arc_pos` in the low-degree image's arc order, the
        exits from the source flows.'''
        cats, _, _, ex_cat, ex_src, _ = self.index_tensors(arc_counts.device)
        counts = torch.zeros(len(self.cat_src), dtype=torch.float64, device=arc_counts.device)
        counts[cats] = arc_counts[arc_pos]
        counts[ex_cat] = src_flow[ex_src]
        return counts

    def counts_from_dense(self, xi, last):
        '''Category counts [n_categories] fp64 from a dense xi_sum [S, S] that holds every arc
        (the general kernel's, or a state path's) and the last frames' posteriors [S]: the
        arcs inside the units, and an exit = the rest of its state's row + its last frames.'''
        cats, src, dst, ex_cat, ex_src, _ = self.index_tensors(xi.device)
        xi = xi.to(torch.float64)
        inside = xi[src, dst]
        counts = torch.zeros(len(self.cat_src), dtype=torch.float64, device=xi.device)
        counts[cats] = inside
        kept = torch.zeros(xi.shape[0], dtype=torch.float64, device=xi.device).index_add_(
            0, src, inside)
        counts[ex_cat] = (xi.sum(dim=1) - kept + last.to(torch.float64))[ex_src]
        return counts

    # -- Model protocol (the statistics come from the HMM's E-step)
    def sufficient_statistics(self, data):
        return data

    def expected_log_likelihood(self, stats):
        raise NotImplementedError('the transitions are scored inside the HMM\'s E-step')

    def accumulate(self, stats, parent_msg=None):
        return self.accumulate_counts(stats)


def _transitions_of(model):
    return getattr(model, 'transitions', None)


class HMM(DiscreteLatentModel):
    '''Hidden Markov Model; its transition probabilities are fixed unless it was created
    with `train_transitions=True` (`transitions`: `HMMTransitions`, None = fixed).'''

    @classmethod
    def create(cls, graph, modelset, train_transitions=False, transitions_prior_strength=1.,
               max_duration=0, durations_prior_strength=1.):
        '''`max_duration` D > 0 (not in the reference): explicit state durations of 1 .. D frames
        (`StateDurations`, learned under Dirichlet priors of strength
        `durations_prior_strength`); 0: the geometric stay of the self-loops.'''
        cls._check_durations_with(max_duration, train_transitions)
        transitions = HMMTransitions.create(graph.trans_log_probs,
                                            prior_strength=transitions_prior_strength) \
            if train_transitions else None
        durations = StateDurations.create(graph, max_duration, durations_prior_strength) \
            if max_duration else None
        return cls(graph, modelset, transitions, durations)

    def __init__(self, graph, modelset, transitions=None, durations=None):
        super().__init__(DynamicallyOrderedModelSet(modelset))
        self.graph = graph
        self.transitions = transitions
        self.durations = durations
        if transitions is not None:
            self._attach_transitions()

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            # (models pickled before transitions / durations could be learned, the reference's
            #  included)
            if name in ('transitions', 'durations'):
                return None
            raise

    # -- explicit durations ---------------------------------------------------------
    @staticmethod
    def _check_durations_with(max_duration, train_transitions):
        if max_duration and train_transitions:
            raise NotImplementedError(
                'explicit durations (max_duration > 0) with learned transitions '
                '(train_transitions=True) are not supported: a stay is the duration law\'s, and '
                'the transition counts of the kernels include the self-loops')

    def _refuse_durations(self, what):
        'NotImplementedError naming the combination, for what explicit durations do not cover.'
        if self.durations is not None:
            raise NotImplementedError(
                f'explicit durations (max_duration > 0) with {what} are not supported: the '
                'explicit-duration kernels cover forward-backward, Viterbi and the evidence only')

    def _duration_tables(self):
        return self.durations.log_dur(), self.durations.leave_w()

    # -- learned transitions --------------------------------------------------------
    def _attach_transitions(self):
        for param in self.transitions.parameters_of_groups():
            param.register_callback(self._on_transitions_update)
        self._on_transitions_update()

    def _exit_states(self):
        return ()

    def _write_transitions(self):
        'trans[i, j] = E[ln a_ij] of every arc inside a unit; returns E[ln a] of every category.'
        trans = self.graph.trans_log_probs
        logp = self.transitions.log_probs().to(dtype=trans.dtype, device=trans.device)
        cats, src, dst = self.transitions.index_tensors(trans.device, self._exit_states())[:3]
        trans[src, dst] = logp[cats]
        return logp

    def _on_transitions_update(self):
        '''The graph's intra-unit transition log-probabilities rewritten with E[ln a] after an
        update of the transitions; the device image is refreshed in place.'''
        self._write_transitions()
        self.graph.weights_rewritten()

    # index arithmetic on device tensors when the graph and the transitions live on the GPU:
    # the update of the transitions' group may be captured as a HIP graph
    def _transitions_update_capturable(self):
        trans = self.graph.trans_log_probs
        if not trans.is_cuda:
            return False
        if not all(p.posterior.params.concentrations.is_cuda
                   for p in self.transitions.parameters_of_groups()):
            return False
        # (what the callbacks index with, and what they share, is made NOW: a host -> device
        # copy or an allocation inside a recording cannot be kept)
        self.transitions.index_tensors(trans.device, self._exit_states())
        self._shared_logs()
        return True

    def _shared_logs(self):
        'What the callbacks of two mean-field groups share (PhoneLoop); nothing here.'
        return None

    def __getstate__(self):
        state = super().__getstate__()
        state.pop('_shared_memo', None)
        return state

    _on_transitions_update.device_only = _transitions_update_capturable

    def expected_transition_probs(self):
        '''The learned transition probabilities E[a] (posterior means): ([S, S] fp64 with
        E[a_ij] on the arcs inside the units, 0 elsewhere; [S] fp64 with every end state's
        E[a_exit], 0 elsewhere).  ValueError when the transitions are not learned.'''
        if self.transitions is None:
            raise ValueError('the transition probabilities of this model are not learned '
                             '(create it with train_transitions=True)')
        S = self.graph.n_states
        probs = self.transitions.expected_probs().detach().to('cpu', torch.float64)
        cats, src, dst = self.transitions.intra()
        mat = torch.zeros(S, S, dtype=torch.float64)
        mat[torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64)] = \
            probs[torch.as_tensor(cats, dtype=torch.int64)]
        ex = torch.zeros(S, dtype=torch.float64)
        for state, c in self.transitions.exits().items():
            ex[state] = probs[c]
        return mat, ex

    def transition_counts(self, dgraph, counts):
        '''Counts of every category of the learned transitions [n_categories] fp64 from what a
        forward-backward call gave (hmm_kernels: `posteriors_fused(want_transitions=True)`,
        `forward_backward_counts`, `path_counts`): ('arcs', arc_counts, src_flow) on the
        device image `dgraph` of the model's graph, or ('dense', xi_sum, last).'''
        kind, a, b = counts
        if kind == 'cat':                   # (bound alignment graphs: by category already)
            return a
        if kind == 'dense':
            return self.transitions.counts_from_dense(a, b)
        _, src, dst = self.transitions.intra()
        pos = dgraph.arc_positions(src, dst)
        return self.transitions.counts_from_kernel(pos, a, b)

    @staticmethod
    def _refuse_transitions(what):
        raise ValueError(f'learned transitions (train_transitions=True) with {what} are not '
                         'supported: per-utterance graphs would need a category map per '
                         'compiled arc -- bind them to the model first '
                         '(bound = model.bind_alignment_graphs(graphs), then pass bound / bound[u])')

    def bind_alignment_graphs(self, graphs):
        '''Alignment graphs bound to this model's learned transitions: a `BoundGraphSet`, a
        sequence whose items stand wherever an inference graph is taken (`inference_graph=`,
        `inference_graphs=`).  `graphs`: a `GraphSet`, a list of `SparseGraph` or a list of
        dense `CompiledGraph`.  With s(p) the state of `self.graph` whose pdf id is p, an arc
        with the pdf ids (p, q) counts for the category of the arc s(p) -> s(q) inside a unit,
        else for the exit of s(p); a state with a final probability counts its last-frame
        posterior for the exit of s(p) when it owns one.  ValueError: fixed transitions, a
        pdf id that two states of the model share, an arc without a category, two arcs of one
        state with the same category (an exit that branches: its compile-time branch
        probabilities would be lost).  The set owns its device image; it is not pickled with
        the model.'''
        from ..graph import BoundGraphSet, _csr_tables
        if self.transitions is None:
            raise ValueError('bind_alignment_graphs: the transition probabilities of this model '
                             'are not learned (create it with train_transitions=True)')
        tables = _csr_tables(graphs)
        arc_cat, last_cat = self._alignment_categories(*tables)
        return BoundGraphSet(tables, arc_cat, last_cat, self.transitions)

    def _alignment_categories(self, state_off, arc_off, init, fin, pdf, src, dst, prob):
        'Host arrays: the category of every arc, and of every state\'s last-frame posterior.'
        import numpy as np
        own = self.graph.pdf_id_mapping
        own = np.arange(self.graph.n_states) if own is None else \
            np.asarray([int(i) for i in own], dtype=np.int64)
        if len(np.unique(own)) != len(own):
            raise ValueError('bind_alignment_graphs: the pdf_id_mapping of the model\'s graph '
                             'repeats a pdf id; the states of an alignment graph cannot be told apart')
        S = self.graph.n_states
        state_of = np.full(max(int(own.max()), int(pdf.max()) if len(pdf) else 0) + 2, -1, np.int64)
        state_of[own] = np.arange(S)
        tr = self.transitions
        intra = np.full((S, S), -1, dtype=np.int32)
        exits = np.full(S + 1, -1, dtype=np.int32)          # (slot S: a pdf id the model lacks)
        for c, (i, j) in enumerate(zip(tr.cat_src, tr.cat_dst)):
            if j >= 0:
                intra[i, j] = c
            else:
                exits[i] = c
        n = len(state_off) - 1
        gidx = np.repeat(np.arange(n, dtype=np.int64), np.diff(arc_off))
        gsrc, gdst = state_off[gidx] + src, state_off[gidx] + dst
        sp, sq = state_of[pdf[gsrc]], state_of[pdf[gdst]]
        cat = np.where((sp >= 0) & (sq >= 0), intra[sp, sq], -1)
        cat = np.where(cat < 0, exits[np.where(sp >= 0, sp, S)], cat).astype(np.int32)
        bad = np.nonzero(cat < 0)[0]
        if len(bad):
            a = int(bad[0])
            raise ValueError(f'bind_alignment_graphs: graph {int(gidx[a])}, arc {int(src[a])} -> '
                             f'{int(dst[a])} (pdf ids {int(pdf[gsrc[a]])} -> {int(pdf[gdst[a]])}) '
                             'is neither an arc inside a unit of the model nor leaves a unit\'s '
                             'end state')
        # (arcs are sorted by source: two arcs of one state with one category sort together)
        order = np.lexsort((cat, gsrc))
        same = (gsrc[order][1:] == gsrc[order][:-1]) & (cat[order][1:] == cat[order][:-1])
        if same.any():
            a = int(order[1:][same][0])
            raise ValueError(f'bind_alignment_graphs: graph {int(gidx[a])}, state {int(src[a])} '
                             f'(pdf id {int(pdf[gsrc[a]])}) has two arcs of one category (an exit '
                             'that branches to two successors): the branch probabilities the '
                             'graph was compiled with would be lost')
        sl = state_of[pdf]
        last = np.where(fin > 0, exits[np.where(sl >= 0, sl, S)], -1).astype(np.int32)
        return cat, last

    def _bound_set(self, graphs):
        '''The `BoundGraphSet` every graph of `graphs` (one graph, a list, the set itself)
        belongs to; ValueError unless they are bound to this model's transitions.'''
        items = [graphs] if hasattr(graphs, 'n_states') else graphs
        owner = graphs if getattr(graphs, 'is_bound', False) else \
            (getattr(items[0], '_set', None) if len(items) else None)
        if not getattr(owner, 'is_bound', False) or owner.transitions is not self.transitions:
            self._refuse_transitions('alignment graphs (inference_graph) that are not bound to '
                                     'this model')
        if owner is not graphs and any(getattr(g, '_set', None) is not owner for g in items):
            raise ValueError('learned transitions: the alignment graphs of one call must come '
                             'from one bound set')
        return owner

    # -- helpers ---------------------------------------------------------------
    def _emissions(self):
        return self.modelset.original_modelset

    def _pc_llhs(self, stats, inference_graph):
        order = inference_graph.pdf_id_mapping
        return self.modelset.expected_log_likelihood(stats, order)

    def _batch_of_one(self, graph, n_frames, dtype):
        return hk.HmmBatch([graph], [0], [n_frames], dtype)

    def _inference(self, pc_llhs, inference_graph, viterbi=False, state_path=None,
                   trans_posteriors=False):
        '''State posteriors (+ summed transition posteriors) from per-state
        log-likelihoods [T, S]; hmm.py:40-62.'''
        pc = _hip.on_device(pc_llhs)
        batch = self._batch_of_one(inference_graph, len(pc), pc.dtype)
        flat = pc.reshape(-1)
        if viterbi or state_path is not None:
            path = hk.viterbi(batch, flat) if state_path is None else state_path
            gamma, xi, g0 = hk.path_posteriors(batch, path, want_xi=trans_posteriors)
        else:
            gamma, xi, g0, _, _ = hk.forward_backward(batch, flat, want_xi=trans_posteriors,
                                                      dense_xi=True)
        gamma = gamma.view(len(pc), -1)
        return ((gamma, xi) if trans_posteriors else gamma), None

    # -- Model interface ---------------------------------------------------------
    def mean_field_factorization(self):
        mff = self.modelset.mean_field_factorization()
        if self.transitions is not None:
            mff = list(mff) + self.transitions.mean_field_factorization()
        if self.durations is not None:
            mff = list(mff) + self.durations.mean_field_factorization()
        return mff

    def sufficient_statistics(self, data):
        return self.modelset.sufficient_statistics(data)

    def expected_log_likelihood(self, stats, inference_graph=None, viterbi=False,
                                state_path=None, scale=1., utt_lengths=None, sample=False):
        '''sum_s gamma_ts * scale * l_ts per frame (hmm.py:73-92).  Without an
        inference graph the model's own graph is used and the transition
        posteriors are kept (PhoneLoop needs them).  `utt_lengths` (not in
        the reference) treats the frames as that many consecutive utterances,
        each decoded with the same graph, in one ragged batch.  `sample` (not in the
        reference): True, or a float64 tensor of one uniform per frame -- a state path is
        drawn from the posterior (`hk.sample_paths`) and trained on as `state_path=` is.'''
        sample = hk.check_sample(sample, len(stats), viterbi, state_path)
        if self.durations is not None:
            if viterbi or state_path is not None or sample is not None:
                self._refuse_durations('viterbi=, state_path= or sample= training')
            return self._duration_expected_log_likelihood(stats, inference_graph, scale,
                                                          utt_lengths)
        trans_posts = inference_graph is None
        learned = self.transitions is not None
        # (alignment graphs of a learned model: bound ones only -- checked before any device work)
        bound = self._bound_set(inference_graph) if learned and inference_graph is not None \
            else None
        self.cache.pop('trans_counts', None)
        graph = self.graph if inference_graph is None else inference_graph
        dense = kernels.is_dense(stats)
        emissions = self._emissions()
        # (no gradient through the posteriors: detached statistics, hmm.py:81-87)
        pc_all = emissions.expected_log_likelihood(stats.detach())
        self.modelset.cache['order'] = graph.pdf_id_mapping
        T, S_total = pc_all.shape
        if bound is not None:
            # (E[ln a] on every arc of the image before the recursion)
            bound.refresh(pc_all.dtype)
        if utt_lengths is None:
            batch = self._batch_of_one(graph, T, pc_all.dtype)
        else:
            lengths = [int(n) for n in utt_lengths]
            if sum(lengths) != T:
                raise ValueError('utt_lengths do not add up to the number of frames')
            batch = hk.HmmBatch([graph], [0] * len(lengths), lengths, pc_all.dtype)
        flow = g0 = None
        # a ragged batch (`utt_lengths`, not in the reference) on graphs the one-wave kernel
        # takes: gather + forward-backward + scatter in ONE launch, as `accumulate_elbo` runs
        # an HMM shard (the per-state posteriors [T, n_states] are not kept then -- a phone
        # loop counts from the first-frame posteriors and hub flows the kernel sums)
        fused = utt_lengths is not None and not viterbi and state_path is None and \
            sample is None and hk.fused_ok(batch)
        need_counts = trans_posts and hasattr(self, 'start_pdf')
        if fused and need_counts:
            fused = getattr(getattr(batch.dgraphs[0], 'lowdeg', None), 'n_hubs', 0) >= 1
        if fused:
            # (the per-frame value sum_s gamma l comes out of the same launch)
            exp_llh = torch.empty(T, dtype=pc_all.dtype, device=pc_all.device)
            if learned:
                state_resps, g0, flow, tc = hk.posteriors_fused(
                    batch, pc_all, scale, want_counts=need_counts, frame_llh=exp_llh,
                    want_transitions=True)
                self.cache['trans_counts'] = self.transition_counts(batch.dgraphs[0], tc)
            else:
                state_resps, g0, flow = hk.posteriors_fused(batch, pc_all, scale,
                                                            want_counts=need_counts,
                                                            frame_llh=exp_llh)
            self.cache.pop('resps', None)
            if trans_posts:
                self.cache['trans_resps'] = None
                self.cache['hub_flow'] = flow
                self.cache['first_resps'] = g0
            self.cache['scaled_pdf_resps'] = state_resps
            self.cache['scale'] = scale
            return self._with_gradient(stats, exp_llh, state_resps, emissions, dense)
        pc_llhs = hk.gather(batch, pc_all, scale)
        if sample is not None:
            state_path = hk.sample_paths(batch, pc_llhs, hk.sample_uniforms(sample))[0]
        if viterbi or state_path is not None:
            path = hk.viterbi(batch, pc_llhs) if state_path is None else state_path
            gamma, xi, g0 = hk.path_posteriors(batch, path, want_xi=trans_posts)
            if learned:
                self.cache['trans_counts'] = self.transition_counts(
                    batch.dgraphs[0], hk.path_counts(batch, path, xi))
        elif learned:
            # forward-backward with the transition counts (one-wave kernels: no dense xi, the
            # phone counts come from the first-frame posteriors and the hub flows)
            gamma, g0, flow, xi, tc = hk.forward_backward_counts(batch, pc_llhs)
            self.cache['trans_counts'] = self.transition_counts(batch.dgraphs[0], tc)
        else:
            per_frame = trans_posts and reference_layout_enabled() and utt_lengths is None
            # (per frame: the general kernel -- log-space forward values, hub arcs in the matrix)
            gamma, xi, g0, _, flow = hk.forward_backward(batch, pc_llhs,
                                                         want_xi=trans_posts and not per_frame,
                                                         dense_xi=per_frame)
            if per_frame:
                # the reference's [T-1, S, S] tensor, hub arcs included: no separate flows
                xi = hk.trans_posteriors_dense(batch, pc_llhs, gamma, graph.trans_log_probs)
                flow = None
        state_resps, exp_llh = hk.scatter(batch, pc_llhs, gamma, S_total, scale)
        self.cache['resps'] = gamma.view(T, -1)
        if trans_posts:
            # summed over time: [S, S]; transitions through a declared hub (phone
            # loop) are summed over their sources in 'hub_flow' [S] instead
            self.cache['trans_resps'] = xi
            self.cache['hub_flow'] = flow
            # posteriors of the FIRST frame, summed over the utterances of a ragged batch
            # (`utt_lengths`): what a phone loop counts besides the flows (phoneloop.py:88-95,
            # once per utterance in the reference's loop)
            self.cache['first_resps'] = g0
        self.cache['scaled_pdf_resps'] = state_resps
        self.cache['scale'] = scale
        return self._with_gradient(stats, exp_llh, state_resps, emissions, dense)

    def _duration_expected_log_likelihood(self, stats, inference_graph, scale, utt_lengths):
        '''The E-step under explicit durations: gather, `hk.duration_forward_backward`, scatter.
        The cache gets the duration counts and -- on the model's own graph -- the segment
        entries per state a phone loop counts its phones from.'''
        graph = self.graph if inference_graph is None else inference_graph
        if kernels.is_dense(stats) or kernels.has_source(stats):
            self._refuse_durations('a VAE prior (differentiable statistics)')
        emissions = self._emissions()
        pc_all = emissions.expected_log_likelihood(stats.detach())
        self.modelset.cache['order'] = graph.pdf_id_mapping
        T, S_total = pc_all.shape
        if utt_lengths is None:
            batch = self._batch_of_one(graph, T, pc_all.dtype)
        else:
            lengths = [int(n) for n in utt_lengths]
            if sum(lengths) != T:
                raise ValueError('utt_lengths do not add up to the number of frames')
            batch = hk.HmmBatch([graph], [0] * len(lengths), lengths, pc_all.dtype)
        pc_llhs = hk.gather(batch, pc_all, scale)
        log_dur, leave_w = self._duration_tables()
        gamma, _, counts, entry, g0 = hk.duration_forward_backward(batch, pc_llhs, log_dur, leave_w)
        state_resps, exp_llh = hk.scatter(batch, pc_llhs, gamma, S_total, scale)
        self.cache['resps'] = gamma.view(T, -1)
        self.cache['dur_counts'] = counts
        self.cache['dur_entries'] = (g0, entry) if inference_graph is None else None
        self.cache['scaled_pdf_resps'] = state_resps
        self.cache['scale'] = scale
        return exp_llh

    @staticmethod
    def _with_gradient(stats, exp_llh, state_resps, emissions, dense):
        'The value with its gradient w.r.t. differentiable statistics / frames (a VAE\'s prior).'
        if dense and isinstance(emissions, NormalSet):
            # statistics-in (prior of a VAE): d exp_llh / d stats through
            # sum_s gamma_ts * scale * l_ts with detached posteriors (hmm.py:81-87)
            exp_llh = kernels.attach_stats_grad(
                stats, exp_llh, state_resps, emissions.means_precisions.natural_form())
        elif isinstance(emissions, NormalSet) and kernels.has_source(stats):
            # the same for statistics that are phi(z_t) of differentiable frames (a VAE with
            # one sample per frame): the frame kernels above, the gradient w.r.t. the frames
            exp_llh = kernels.attach_frame_grad(
                stats, exp_llh, state_resps, emissions.means_precisions.natural_form())
        return exp_llh

    def accumulate(self, stats, parent_msg=None):
        # scale * resps scattered back to pdf ids was produced with the E-step.
        retval = {**self._emissions().accumulate(stats, self.cache['scaled_pdf_resps'])}
        if self.transitions is not None:
            retval.update(self.transitions.accumulate_counts(self.cache['trans_counts']))
        if self.durations is not None:
            retval.update(self.durations.accumulate_counts(self.cache['dur_counts']))
        return retval

    # -- DiscreteLatentModel interface ------------------------------------------------
    def _emission_llhs(self, stats, predictive):
        '''The per-pdf matrix [T, S_total] a search runs on: the expected log-likelihoods, or
        with `predictive` the posterior-predictive (Student-t, mean-weight) log-densities.'''
        if predictive:
            return self._emissions().predictive_log_likelihood(stats)
        return self._emissions().expected_log_likelihood(stats)

    def _search_batch(self, data, inference_graph, predictive=False):
        '''(batch, pc_all, n_frames) of a search over one utterance: the `HmmBatch` of `data` on
        the inference graph (None: the model's own), the emission log-likelihoods by pdf id
        [n_frames, S_total] and its length.  A graph bound to the model's learned transitions
        gets E[ln a] on its arcs first.  Host-side argument checks come before this call.'''
        graph = self.graph if inference_graph is None else inference_graph
        stats = self.sufficient_statistics(data)
        pc_all = self._emission_llhs(stats, predictive)
        if getattr(getattr(graph, '_set', None), 'is_bound', False):
            self._bound_set(graph).refresh(pc_all.dtype)
        return self._batch_of_one(graph, len(stats), pc_all.dtype), pc_all, len(stats)

    def _search_input(self, data, inference_graph, scale, predictive=False):
        '''(batch, pc_llhs, n_frames): `_search_batch` with the log-likelihoods gathered by state
        and multiplied by `scale`, packed as the HMM kernels read them.'''
        batch, pc_all, n_frames = self._search_batch(data, inference_graph, predictive)
        return batch, hk.gather(batch, pc_all, scale), n_frames

    def _checked_categories(self, inference_graph, arc_cat, init_cat, n_cat, per_frame=True,
                            per_utt=False):
        '''The categories of the arcs and states of one graph as `hk.arc_posteriors` takes them,
        checked on the host (`hk.check_arc_categories`).'''
        graph = self.graph if inference_graph is None else inference_graph
        src, _ = graph.out_arcs()
        return hk.check_arc_categories([len(src)], [graph.n_states], [arc_cat], [init_cat], n_cat,
                                       per_frame, per_utt)

    def decode(self, data, inference_graph=None, scale=1., predictive=False):
        '''Viterbi path mapped to pdf ids, LongTensor on the host (hmm.py:105-114).
        `predictive` (not in the reference): the emissions are the posterior-predictive
        densities (`predictive_log_likelihood` of the emission model) in place of the expected
        log-likelihoods.  The arcs of the graph are used as they stand -- fixed log-probabilities,
        or E[ln a] and E[ln pi] where they are learned: predictive arc weights are not formed.'''
        batch, pc_llhs, _ = self._search_input(data, inference_graph, scale, predictive)
        if self.durations is not None:
            return hk.duration_viterbi(batch, pc_llhs, *self._duration_tables(),
                                       map_pdf=True)[0].cpu()
        return hk.viterbi(batch, pc_llhs, map_pdf=True).cpu()

    def decode_nbest(self, data, k, inference_graph=None, scale=1.):
        '''The `k` best STATE paths mapped to pdf ids and their scores, best first: (LongTensor
        [k, T], float64 [k]) on the host.  The score of a path is the sum of its (scaled)
        log-likelihoods and the graph's initial, arc and final log-weights, in the model's
        precision; row 0 is `decode`'s path whenever its score is finite.  Ranks beyond the
        number of paths of finite score have the score -inf and a row of -1.  Not in the
        reference.  Otherwise as `decode`.'''
        self._refuse_durations('decode_nbest')
        k = hk.check_nbest(k, 'decode_nbest')
        batch, pc_llhs, _ = self._search_input(data, inference_graph, scale)
        paths, scores = hk.viterbi_nbest(batch, pc_llhs, k, map_pdf=True)
        return paths.cpu(), scores[0].cpu()

    def sample_path(self, data, inference_graph=None, scale=1., nsamples=1, generator=None):
        '''`nsamples` state paths drawn from the posterior, mapped to pdf ids: LongTensor
        [nsamples, T] on the host.  `generator`: a device torch.Generator for the uniforms
        (default: the device's global one).  Otherwise as `decode`.'''
        self._refuse_durations('sample_path')
        batch, pc_llhs, _ = self._search_input(data, inference_graph, scale)
        return hk.sample_paths(batch, pc_llhs, nsamples=nsamples, generator=generator,
                               map_pdf=True).cpu()

    def log_evidence(self, data, inference_graph=None, scale=1., per_frame=False,
                     predictive=False):
        '''ln p(x_0 .. x_{T-1}) under the model's expected log-likelihoods and the graph's
        (expected) log-transitions, summed over all state paths: a 0-d float64 tensor on the
        device, or with `per_frame` (value, [T] float64 of ln p(x_t | x_0 .. x_{t-1})).  Not in
        the reference, whose `lognorm` (graph.py:289-326) is this number.  With `predictive`
        the emissions are the posterior-predictive densities -- the held-out likelihood of a
        Bayesian model, never below the default's value; the arcs stay as they are (fixed, or
        E[ln a] / E[ln pi] where learned).  Otherwise as `decode`.'''
        # (the gather is launched here, not in `_search_input`: the refusal comes before it)
        batch, pc_all, _ = self._search_batch(data, inference_graph, predictive)
        if self.durations is not None:
            if per_frame:
                self._refuse_durations('log_evidence(per_frame=True)')
            return hk.duration_forward_backward(batch, hk.gather(batch, pc_all, scale),
                                                *self._duration_tables(), want_counts=False)[1][0]
        utt, frame = hk.log_evidence(batch, hk.gather(batch, pc_all, scale), per_frame=per_frame)
        return (utt[0], frame) if per_frame else utt[0]

    def arc_posteriors(self, data, arc_cat, init_cat, n_cat, inference_graph=None, scale=1.,
                       per_frame=True):
        '''The posteriors of the graph's arcs folded into `n_cat` categories
        (`hmm_kernels.arc_posteriors`): with `per_frame` a [T, n_cat] tensor on the device whose
        row t >= 1 holds, per category, the sum of P(s_{t-1} = i, s_t = j | x) over the arcs
        i -> j of that category and whose row 0 holds gamma_0 by `init_cat`; without it their
        sum over the frames, [n_cat] float64.  `arc_cat` follows `graph.out_arcs()`, `init_cat`
        the graph's states; entries are in [0, n_cat) or -1 (count nothing).  Not in the
        reference.  Otherwise as `decode`.'''
        self._refuse_durations('arc_posteriors')
        cats = self._checked_categories(inference_graph, arc_cat, init_cat, n_cat, per_frame,
                                        not per_frame)
        batch, pc_llhs, _ = self._search_input(data, inference_graph, scale)
        frame, utt = hk.arc_posteriors(batch, pc_llhs, *cats, n_cat, per_frame=per_frame,
                                       per_utt=not per_frame)
        return frame if per_frame else utt[0]

    def max_marginals(self, data, inference_graph=None, scale=1.):
        '''(best, [T, S]) on the device: the score of the Viterbi path (0-d float64) and, for
        every frame and state, the score of the best path through it minus `best`
        (`hmm_kernels.max_marginals`): 0 along `decode`'s path, negative off it, -inf where no
        path passes.  Not in the reference.  Otherwise as `decode`.'''
        self._refuse_durations('max_marginals')
        batch, pc_llhs, n_frames = self._search_input(data, inference_graph, scale)
        best, state, _, _ = hk.max_marginals(batch, pc_llhs)
        return best[0], state.view(n_frames, -1)

    def arc_max_marginals(self, data, arc_cat, init_cat, n_cat, inference_graph=None, scale=1.,
                          per_frame=True):
        '''(best, max-marginals of the graph's arcs folded into `n_cat` categories), on the
        device (`hmm_kernels.max_marginals`): with `per_frame` a [T, n_cat] tensor whose row
        t >= 1 holds, per category, the score of the best path that enters frame t on an arc of
        that category, minus `best`, and whose row 0 holds the same for the states by
        `init_cat`; without it their maximum over the frames, [n_cat] float64.  -inf: no such
        path.  The categories are those of `arc_posteriors`.  Not in the reference.  Otherwise
        as `decode`.'''
        self._refuse_durations('max_marginals')
        cats = self._checked_categories(inference_graph, arc_cat, init_cat, n_cat, per_frame,
                                        not per_frame)
        batch, pc_llhs, _ = self._search_input(data, inference_graph, scale)
        best, _, frame, utt = hk.max_marginals(batch, pc_llhs, *cats, n_cat, states=False,
                                               per_frame=per_frame, per_utt=not per_frame)
        return best[0], (frame if per_frame else utt[0])

    def posteriors(self, data, inference_graph=None, scale=1.0):
        'State posteriors; `scale` multiplies the statistics (hmm.py:116-121).'
        graph = self.graph if inference_graph is None else inference_graph
        stats = self.modelset.sufficient_statistics(data) * scale
        pc_all = self._emissions().expected_log_likelihood(stats)
        if getattr(getattr(graph, '_set', None), 'is_bound', False):
            self._bound_set(graph).refresh(pc_all.dtype)
        batch = self._batch_of_one(graph, len(stats), pc_all.dtype)
        if self.durations is not None:
            gamma = hk.duration_forward_backward(batch, hk.gather(batch, pc_all, 1.),
                                                 *self._duration_tables(), want_counts=False)[0]
            return gamma.view(len(stats), -1)
        gamma = hk.forward_backward(batch, hk.gather(batch, pc_all, 1.))[0]
        return gamma.view(len(stats), -1)


def unit_start_categories(graph, start_pdf, end_pdf):
    '''(arc_cat, init_cat), int32 host arrays over `graph.out_arcs()` and the graph's states, of
    the unit-start posteriors, the units numbered in `start_pdf` order: an arc i -> j with
    i != j whose destination's pdf id is `start_pdf[u]` has category u, every other arc -1;
    state j has the category of the unit whose pdf ids `start_pdf[u] .. end_pdf[u]` (the unit's
    first and LAST pdf) hold its own, -1 when there is none.  Works on the model's graph and on
    alignment graphs (a unit that is repeated in a transcription is one category).'''
    pdf = np.arange(graph.n_states, dtype=np.int64) if graph.pdf_id_mapping is None else \
        np.asarray([int(i) for i in graph.pdf_id_mapping], dtype=np.int64)
    src, dst = graph.out_arcs()
    firsts = np.asarray([int(start_pdf[u]) for u in start_pdf], dtype=np.int64)
    lasts = np.asarray([int(end_pdf[u]) for u in start_pdf], dtype=np.int64)
    top = int(max(pdf.max(initial=0), lasts.max(initial=0))) + 1
    unit_of_first = np.full(top, -1, dtype=np.int32)
    unit_of_first[firsts] = np.arange(len(firsts), dtype=np.int32)
    unit_of_pdf = np.full(top, -1, dtype=np.int32)
    for u, (a, b) in enumerate(zip(firsts, lasts)):
        unit_of_pdf[a:b + 1] = u
    arc_cat = np.where(np.asarray(src) != np.asarray(dst), unit_of_first[pdf[dst]], -1)
    return arc_cat.astype(np.int32), unit_of_pdf[pdf].astype(np.int32)


def _unit_starts(model, data, inference_graph=None, scale=1.):
    '''Unit-start posteriors [T, n_units] on the device, the units in `start_pdf` order: entry
    (t, u) is the probability that unit u BEGINS at frame t -- for t >= 1 that a path enters
    the unit's first state from another state, for t = 0 that it starts inside the unit.
    `.sum(1)` is the boundary posterior of a frame, `.sum(0)` the expected number of
    occurrences of every unit (the soft counterparts of `decode`'s boundaries and unit counts).
    A unit that can be entered at a state other than its first is not covered: such entries are
    not counted.  Otherwise as `decode`.'''
    graph = model.graph if inference_graph is None else inference_graph
    arc_cat, init_cat = unit_start_categories(graph, model.start_pdf, model.end_pdf)
    return model.arc_posteriors(data, arc_cat, init_cat, len(model.start_pdf),
                                inference_graph=inference_graph, scale=scale)


def _unit_start_margins(model, data, inference_graph=None, scale=1.):
    '''(best, [T, n_units]) on the device, the units in `start_pdf` order: the Viterbi score and
    the unit-start max-marginals -- entry (t, u) is the score lost against the best path by
    forcing unit u to BEGIN at frame t (for t >= 1: to enter the unit's first state from another
    state; for t = 0: to start inside the unit).  0 on the Viterbi segmentation, -inf where
    impossible; everything `>= -beam` is the unit-start lattice of that beam.  The max-product
    twin of `unit_starts`, with its categories.  Otherwise as `decode`.'''
    graph = model.graph if inference_graph is None else inference_graph
    arc_cat, init_cat = unit_start_categories(graph, model.start_pdf, model.end_pdf)
    return model.arc_max_marginals(data, arc_cat, init_cat, len(model.start_pdf),
                                   inference_graph=inference_graph, scale=scale)


def _checked_unit_categories(model, inference_graph):
    '(the unit-start categories of the graph, checked as `hk.segment_margins` takes them, n_units).'
    graph = model.graph if inference_graph is None else inference_graph
    arc_cat, init_cat = unit_start_categories(graph, model.start_pdf, model.end_pdf)
    n_units = len(model.start_pdf)
    return model._checked_categories(inference_graph, arc_cat, init_cat, n_units), n_units


def _unit_segments(model, data, beam=10., max_dur=None, inference_graph=None, scale=1.):
    '''(best, start, end, unit, margin) on the device: the Viterbi score (0-d float64) and the
    unit segment lattice of the beam -- every (unit, start, end) such that some path on which the
    unit BEGINS at frame `start` (as `unit_start_margins` has it) and the next unit begins at
    frame `end` + 1 (or the utterance ends with frame `end`) scores within `beam` of the best
    path; `margin` (float64, <= 0 up to rounding) is what the best such path loses against it.
    `start`, `end`, `unit` are int32, the units numbered in `start_pdf` order; sorted by
    (start, unit, end).  `max_dur`: the longest segment looked for, in frames (None: the
    utterance's length); `beam` = inf keeps every possible segment.  The Viterbi segmentation
    has margin 0.  Otherwise as `decode`.'''
    beam, max_dur = hk.check_segments(beam, max_dur, 'unit_segments')
    model._refuse_durations('the segment functions (unit_segments)')
    cats, n_units = _checked_unit_categories(model, inference_graph)
    batch, pc_llhs, n_frames = model._search_input(data, inference_graph, scale)
    best, _, frame, unit, seg = hk.segment_margins(
        batch, pc_llhs, *cats, n_units, beam, max(n_frames, 1) if max_dur is None else max_dur)
    start, end, unit, margin = hk.segments_within(frame, unit, seg, beam)
    return best[0], start.to(torch.int32), end.to(torch.int32), unit, margin


def _segment_posteriors_of(model, data, min_post, max_dur, inference_graph, scale, what):
    '`hk.segment_posteriors` of one utterance under the unit-start categories: its five outputs.'
    min_post, max_dur = hk.check_segment_posteriors(min_post, max_dur, what)
    model._refuse_durations(f'the segment functions ({what})')
    cats, n_units = _checked_unit_categories(model, inference_graph)
    batch, pc_llhs, n_frames = model._search_input(data, inference_graph, scale)
    return hk.segment_posteriors(batch, pc_llhs, *cats, n_units, min_post,
                                 max(n_frames, 1) if max_dur is None else max_dur)


def _unit_segment_posteriors(model, data, min_post=1e-3, max_dur=None, inference_graph=None,
                             scale=1.):
    '''(log_evidence, start, end, unit, post) on the device: ln p(x) (0-d float64) and the unit
    segments with their posteriors -- every (unit, start, end) such that, with probability
    `post` >= `min_post` (float64, and > 0), the unit BEGINS at frame `start` (as `unit_starts`
    has it) and the next unit begins at frame `end` + 1 (or the utterance ends with frame `end`).
    The sum-product twin of `unit_segments`: `start`, `end`, `unit` are int32, the units numbered
    in `start_pdf` order; sorted by (start, unit, end).  `max_dur`: the longest segment looked for,
    in frames (None: the utterance's length).  With `min_post` = 0 the posteriors of the segments
    that cover a frame sum to 1.  Otherwise as `decode`.'''
    evidence, _, frame, unit, seg = _segment_posteriors_of(
        model, data, min_post, max_dur, inference_graph, scale, 'unit_segment_posteriors')
    start, end, unit, post = hk.segments_above(frame, unit, seg, min_post)
    return evidence[0], start.to(torch.int32), end.to(torch.int32), unit, post


def _unit_durations(model, data, max_dur=None, inference_graph=None, scale=1.):
    '''The expected duration histogram [n_units, max_dur], float64 on the device, the units in
    `start_pdf` order: entry (u, k) is the expected number of instances of unit u that last
    exactly k + 1 frames, the sum over the start frames s of the posterior of the segment
    (u, s, s + k) -- the soft version of counting the durations on `decode`'s path.  `max_dur`
    None: the utterance's length, and row u sums to the expected count of unit u
    (`unit_starts(...).sum(0)`).  Otherwise as `decode`.'''
    _, _, _, unit, seg = _segment_posteriors_of(
        model, data, 0., max_dur, inference_graph, scale, 'unit_durations')
    hist = torch.zeros(len(model.start_pdf), seg.shape[1], dtype=torch.float64, device=seg.device)
    return hist.index_add_(0, unit.long(), seg.double())


class PhoneLoop(HMM):
    'Phone-loop HMM with a prior over the phone (unigram) weights.'
    unit_starts = _unit_starts
    unit_start_margins = _unit_start_margins
    unit_segments = _unit_segments
    unit_segment_posteriors = _unit_segment_posteriors
    unit_durations = _unit_durations

    @classmethod
    def create(cls, graph, start_pdf, end_pdf, modelset, categorical=None,
               prior_strength=1.0, train_transitions=False, transitions_prior_strength=1.,
               max_duration=0, durations_prior_strength=1.):
        '''`train_transitions` (not in the reference): learn the units' transition
        probabilities too (`HMMTransitions`: Dirichlet rows whose prior concentrations are
        `transitions_prior_strength` x the graph's transition probabilities).  `max_duration`
        D > 0 (not in the reference): explicit state durations of 1 .. D frames, as
        `HMM.create` has them.'''
        cls._check_durations_with(max_duration, train_transitions)
        tensor = modelset.mean_field_factorization()[0][0].prior._tensors()[0]
        if categorical is None:
            weights = torch.ones(len(start_pdf), dtype=tensor.dtype, device=tensor.device)
            weights /= len(start_pdf)
            categorical = Categorical.create(weights, prior_strength)
        transitions = HMMTransitions.create(
            graph.trans_log_probs, list(end_pdf.values()), list(start_pdf.values()),
            transitions_prior_strength) if train_transitions else None
        durations = StateDurations.create(graph, max_duration, durations_prior_strength) \
            if max_duration else None
        return cls(graph, modelset, start_pdf, end_pdf, categorical, transitions, durations)

    def __init__(self, graph, modelset, start_pdf, end_pdf, categorical, transitions=None,
                 durations=None):
        super().__init__(graph, modelset)
        self.start_pdf = start_pdf
        self.end_pdf = end_pdf
        self.categorical = categorical
        self.transitions = transitions
        self.durations = durations
        if durations is not None:
            self._check_durations_with(True, transitions is not None)
            self._check_units_for_durations()
        param = self.categorical.mean_field_factorization()[0][0]
        param.register_callback(self._on_weights_update)
        if transitions is not None:
            self._attach_transitions()          # (rewrites the exits too: _on_weights_update)
        else:
            self._on_weights_update()

    def _exit_states(self):
        return list(self.end_pdf.values())

    def _check_units_for_durations(self):
        '''Explicit durations count a phone where a segment of its start state begins: the start
        states must be entered from end states only, and no unit's start state is its end state
        (its one state would be entered from itself, which a duration law cannot express).'''
        starts, ends = list(self.start_pdf.values()), list(self.end_pdf.values())
        if set(starts) & set(ends):
            raise NotImplementedError(
                'explicit durations (max_duration > 0) with units whose start state is their end '
                'state are not supported: a one-state unit that follows itself is a longer stay')
        trans = self.graph.trans_log_probs.detach().to('cpu')
        arcs = torch.isfinite(trans) & (trans.exp() > 0)
        arcs.fill_diagonal_(False)
        inner = torch.ones(trans.shape[0], dtype=torch.bool)
        inner[torch.as_tensor(ends)] = False
        if bool(arcs[inner][:, torch.as_tensor(starts)].any()):
            raise ValueError('explicit durations: a unit\'s start state is entered from a state '
                             'that ends no unit; the phone counts would miss it')

    def _on_transitions_update(self):
        '''Intra-unit entries <- E[ln a], then the phone exits <- E[ln a_exit] + E[ln w]: the
        graph is the same whichever of the two callbacks the optimizer runs first.'''
        logp = self._write_transitions()
        ex, lw = self._shared_logs()
        end_cats = self.transitions.index_tensors(ex.device, self._exit_states())[5]
        ex.copy_(logp[end_cats])
        self._write_exits(ex, lw)

    _on_transitions_update.device_only = HMM._transitions_update_capturable

    def _shared_logs(self):
        '''(E[ln a_exit] of the phones' end states [P], E[ln w] of the phones [P]) for learned
        transitions: two tensors on the graph's device that stay where they are.  Each of the
        two callbacks writes its own group's half in place and reads the other half from here,
        never the other group's posterior or memo: a HIP graph recorded for one group's update
        would go on reading those after the other group has replaced them.'''
        trans = self.graph.trans_log_probs
        key = (str(trans.device), trans.dtype)
        memo = self.__dict__.get('_shared_memo')
        if memo is None or memo[0] != key:
            end_cats = self.transitions.index_tensors(trans.device, self._exit_states())[5]
            ex = self.transitions.log_probs().to(dtype=trans.dtype, device=trans.device)[end_cats]
            lw = self.categorical.log_weights().to(dtype=trans.dtype, device=trans.device).clone()
            memo = (key, ex, lw)
            self.__dict__['_shared_memo'] = memo
        return memo[1], memo[2]

    def _index_tensors(self, device):
        '''(end states, start states) of the phones as device index tensors,
        built once per device: a host -> device copy from pageable memory
        behind queued kernels blocks the host for tens of ms (it showed up as
        a 50 ms stall every time the phone weights were updated).'''
        end_idxs, start_idxs = list(self.end_pdf.values()), list(self.start_pdf.values())
        memo = self.__dict__.get('_idx_memo')
        if memo is None or memo[0] != device or memo[1] != (end_idxs, start_idxs):
            memo = (device, (end_idxs, start_idxs), torch.as_tensor(end_idxs, device=device),
                    torch.as_tensor(start_idxs, device=device))
            self.__dict__['_idx_memo'] = memo
        return memo[2], memo[3]

    def _on_weights_update(self):
        '''Rewrite the phone-exit transitions with E[ln w] (phoneloop.py:53-65).
        Host-side callback over P x P entries; the CSR copy on the device is
        rebuilt at the next inference (CompiledGraph.device_graph).'''
        trans = self.graph.trans_log_probs
        log_weights = self.categorical.log_weights().to(dtype=trans.dtype,
                                                        device=trans.device)
        if self.transitions is not None:
            # learned transitions: the residual is E[ln a_exit] of the end state, as the
            # transitions' callback last wrote it
            residuals, shared_lw = self._shared_logs()
            shared_lw.copy_(log_weights)
            self._write_exits(residuals, shared_lw)
            return
        ends, starts = self._index_tensors(trans.device)
        residuals = (1 - trans[ends, ends].exp()).log()
        self._write_exits(residuals, log_weights)

    def _write_exits(self, residuals, log_weights):
        'trans[end_i, start_j] = residuals[i] + log_weights[j], then the device image and hub.'
        trans = self.graph.trans_log_probs
        start_idxs = list(self.start_pdf.values())
        end_idxs = list(self.end_pdf.values())
        # all phones at once (the reference loops over them; same elementwise ops)
        ends, starts = self._index_tensors(trans.device)
        if len(set(end_idxs)) == len(end_idxs):
            trans[ends[:, None], starts[None, :]] = residuals[:, None] + log_weights[None, :]
        else:                                    # repeated end states: last write wins
            for i, end_idx in enumerate(end_idxs):
                trans[end_idx, start_idxs] = residuals[i] + log_weights
        self.graph.weights_rewritten()
        # the block just written is rank one: tell the graph, so that
        # forward-backward can treat the eliminated pivot state as a hub
        if len(set(end_idxs)) == len(end_idxs) and len(set(start_idxs)) == len(start_idxs):
            self.graph.set_hub(end_idxs, residuals, start_idxs, log_weights)

    # the callback is index arithmetic on device tensors when the graph lives on the GPU
    # (no host copy, no synchronisation): the update of the weights' group may then be
    # captured as a HIP graph (parameters.py: register_callback)
    def _weights_update_capturable(self):
        if not self.graph.trans_log_probs.is_cuda:
            return False
        # (the index tensors are made NOW: their host -> device copy cannot be recorded)
        self._index_tensors(self.graph.trans_log_probs.device)
        if self.transitions is not None:
            return self._transitions_update_capturable()
        return True

    _on_weights_update.device_only = _weights_update_capturable

    def mean_field_factorization(self):
        from .mixtures import _merge_groups
        mff = _merge_groups(self.modelset.mean_field_factorization(),
                            self.categorical.mean_field_factorization())
        if self.transitions is not None:
            mff = mff + self.transitions.mean_field_factorization()
        if self.durations is not None:
            mff = mff + self.durations.mean_field_factorization()
        return mff

    def phone_counts(self, xi_sum, gamma0, hub_flow=None):
        '''sum_t xi_t[ends, starts] summed over ends + gamma_0[starts] (88-95).
        `xi_sum` may be None when the graph routes every end -> start arc through
        its hub: `hub_flow` then holds the whole sum.'''
        ends, starts = self._index_tensors(gamma0.device)
        counts = gamma0[starts].to(torch.float64)
        if xi_sum is not None and xi_sum.dim() == 3:          # per frame (reference layout)
            xi_sum = xi_sum.sum(dim=0)
        if xi_sum is not None:
            counts = counts + xi_sum[:, starts][ends, :].sum(dim=0)
        if hub_flow is not None:
            counts = counts + hub_flow[starts]
        return counts

    def accumulate(self, stats, parent_msg=None):
        retval = super().accumulate(stats, parent_msg)
        wparam = self.categorical.mean_field_factorization()[0][0]
        ref = wparam.stats
        if self.cache.get('dur_entries') is not None:
            # explicit durations: a phone is counted where a segment of its start state begins
            g0, entry = self.cache['dur_entries']
            _, starts = self._index_tensors(g0.device)
            counts = (g0[starts] + entry[starts]).to(dtype=ref.dtype, device=ref.device)
            resps_stats = self.categorical.sufficient_statistics(counts.view(1, -1))
            retval.update(self.categorical.accumulate(resps_stats))
        elif 'trans_resps' in self.cache:
            first = self.cache.get('first_resps')
            counts = self.phone_counts(self.cache['trans_resps'],
                                       self.cache['resps'][0] if first is None else first,
                                       self.cache.get('hub_flow'))
            counts = counts.to(dtype=ref.dtype, device=ref.device)
            resps_stats = self.categorical.sufficient_statistics(counts.view(1, -1))
            retval.update(self.categorical.accumulate(resps_stats))
        else:
            # trained with forced alignments: the phone weights get no counts
            fake = torch.zeros(len(self.start_pdf), dtype=ref.dtype, device=ref.device)
            retval.update(self.categorical.accumulate(fake[None, :]))
        return retval


class BigramPhoneLoop(HMM):
    '''Phone-loop HMM with a bigram language model: a prior over the P x P phone
    transition weights (`CategoricalSet`: Dirichlet rows; `SBCategoricalSet`: the
    hierarchical Dirichlet process).  API and pickled attributes of
    beer/models/phoneloop.py:104-191.

    A free loop runs on the fused kernel of the declared bigram block
    (`beer_hmm_posteriors_bigram`, csrc/hmm_bigram.hip) and counts the block's
    transition posteriors only -- no first-frame term, unlike the unigram loop
    (phoneloop.py:174-186).'''
    unit_starts = _unit_starts
    unit_start_margins = _unit_start_margins
    unit_segments = _unit_segments
    unit_segment_posteriors = _unit_segment_posteriors
    unit_durations = _unit_durations

    @classmethod
    def create(cls, graph, start_pdf, end_pdf, modelset, categoricalset=None,
               prior_strength=1.0, train_transitions=False, max_duration=0):
        if max_duration:
            raise NotImplementedError('explicit durations (max_duration > 0) with a '
                                      'BigramPhoneLoop are not supported: its fused kernel has '
                                      'no duration laws')
        if train_transitions:
            raise ValueError('learned transitions (train_transitions=True) are not supported '
                             'on a bigram phone loop: its kernel does not count them')
        tensor = modelset.mean_field_factorization()[0][0].prior._tensors()[0]
        if categoricalset is None:
            weights = torch.ones(len(start_pdf), len(start_pdf), dtype=tensor.dtype,
                                 device=tensor.device)
            weights /= len(start_pdf)
            categoricalset = CategoricalSet.create(weights, prior_strength)
        return cls(graph, modelset, start_pdf, end_pdf, categoricalset)

    def __init__(self, graph, modelset, start_pdf, end_pdf, categoricalset):
        super().__init__(graph, modelset)
        self.start_pdf = start_pdf
        self.end_pdf = end_pdf
        self.categoricalset = categoricalset
        param = self.categoricalset.mean_field_factorization()[0][0]
        param.register_callback(self._on_weights_update)
        self._on_weights_update()

    _index_tensors = PhoneLoop._index_tensors

    def _emissions(self):
        # (built from a unigram loop's `modelset`, the emissions come wrapped twice, as in
        # the reference's mkphoneloopbigram: the pdf-id order is the graph's, not theirs)
        ems = self.modelset.original_modelset
        while isinstance(ems, DynamicallyOrderedModelSet):
            ems = ems.original_modelset
        return ems

    def _on_weights_update(self):
        '''trans[end_i, start_j] = ln(1 - loop_i) + L[i, j] (phoneloop.py:147-156), L the
        prior's own E[ln w] of the one-hot rows (a `CategoricalSet` gives it transposed, the
        stick-breaking set row by row: INTEGRATION.md), then the block is declared to the
        graph for the fused kernel.'''
        trans = self.graph.trans_log_probs
        cset = self.categoricalset
        # the reference's expected_log_likelihood of the one-hot rows, without the product:
        # E[ln pi]^T for Dirichlet rows, E[ln pi] row by row for the stick-breaking set
        log_weights = cset.log_weights().t() if isinstance(cset, CategoricalSet) \
            else cset.log_weights()
        log_weights = log_weights.to(dtype=trans.dtype, device=trans.device)
        start_idxs = list(self.start_pdf.values())
        end_idxs = list(self.end_pdf.values())
        ends, starts = self._index_tensors(trans.device)
        residuals = (1 - trans[ends, ends].exp()).log()
        unique = len(set(end_idxs)) == len(end_idxs) and len(set(start_idxs)) == len(start_idxs)
        if unique:
            trans[ends[:, None], starts[None, :]] = residuals[:, None] + log_weights
        else:                                    # repeated states: last write wins
            for i, end_idx in enumerate(end_idxs):
                trans[end_idx, start_idxs] = residuals[i] + log_weights[i]
        self.graph.weights_rewritten()
        if unique:
            self.graph.set_bigram_block(end_idxs, residuals, start_idxs, log_weights)

    # index arithmetic and kernels on device tensors when the graph and the weights live on
    # the GPU: the update of the weights' group may be captured as a HIP graph
    # (parameters.py: register_callback), as PhoneLoop's
    def _weights_update_capturable(self):
        if not self.graph.trans_log_probs.is_cuda:
            return False
        cset = self.categoricalset
        conc = cset.mean_field_factorization()[0][0].posterior.params.concentrations
        if not conc.is_cuda:
            return False
        if isinstance(cset, SBCategoricalSet) and not cset.ordering.is_cuda:
            return False
        self._index_tensors(self.graph.trans_log_probs.device)
        return True

    _on_weights_update.device_only = _weights_update_capturable

    def mean_field_factorization(self):
        from .mixtures import _merge_groups
        return _merge_groups(self.modelset.mean_field_factorization(),
                             self.categoricalset.mean_field_factorization())

    def declare_block(self):
        '''Declare the end -> start block to the graph if it is not (a model unpickled from
        the reference, or moved to another device, has no declaration): the block as the
        dense matrix holds it.'''
        graph = self.graph
        ends, starts = list(self.end_pdf.values()), list(self.start_pdf.values())
        hint = graph.__dict__.get('bigram')
        if hint is None or hint[0] != ends or hint[2] != starts:
            block = graph.trans_log_probs[torch.as_tensor(ends)[:, None],
                                          torch.as_tensor(starts)[None, :]]
            graph.set_bigram_block(ends, torch.zeros(len(ends), dtype=block.dtype), starts, block)

    def bigram_counts(self, xi):
        '''The end -> start block [P, P] of transition posteriors summed over time
        (`xi` [S, S], or the reference's per-frame [T-1, S, S]).'''
        ends, starts = self._index_tensors(xi.device)
        if xi.dim() == 3:
            xi = xi.sum(dim=0)
        return xi[ends[:, None], starts[None, :]]

    def expected_log_likelihood(self, stats, inference_graph=None, viterbi=False,
                                state_path=None, scale=1., utt_lengths=None, sample=False):
        '''As HMM.expected_log_likelihood; the free loop (no inference graph, no Viterbi, no
        drawn path, summed transition posteriors) runs on the fused bigram kernel as a ragged
        batch of one or of `utt_lengths` utterances.'''
        sample = hk.check_sample(sample, len(stats), viterbi, state_path)
        if inference_graph is not None or viterbi or state_path is not None or \
                sample is not None or (reference_layout_enabled() and utt_lengths is None):
            self.cache.pop('bigram_counts', None)
            self.cache.pop('trans_resps', None)
            return super().expected_log_likelihood(stats, inference_graph, viterbi, state_path,
                                                   scale, utt_lengths,
                                                   sample=False if sample is None else sample)
        dense = kernels.is_dense(stats)
        emissions = self._emissions()
        pc_all = emissions.expected_log_likelihood(stats.detach())
        self.modelset.cache['order'] = self.graph.pdf_id_mapping
        T = pc_all.shape[0]
        lengths = [T] if utt_lengths is None else [int(n) for n in utt_lengths]
        if sum(lengths) != T:
            raise ValueError('utt_lengths do not add up to the number of frames')
        self.declare_block()
        batch = hk.HmmBatch([self.graph], [0] * len(lengths), lengths, pc_all.dtype)
        state_resps, counts = hk.posteriors_bigram(batch, pc_all, scale)
        # sum_s gamma_ts * scale * l_ts per frame (hmm.py:87) from the scattered posteriors
        exp_llh = (state_resps * _hip.on_device(pc_all)).sum(dim=1)
        for key in ('resps', 'trans_resps', 'hub_flow', 'first_resps'):
            self.cache.pop(key, None)
        self.cache['bigram_counts'] = counts
        self.cache['scaled_pdf_resps'] = state_resps
        self.cache['scale'] = scale
        return self._with_gradient(stats, exp_llh, state_resps, emissions, dense)

    def accumulate(self, stats, parent_msg=None):
        retval = HMM.accumulate(self, stats, parent_msg)
        self.cache.pop('resps', None)
        counts = self.cache.get('bigram_counts')
        if counts is None and self.cache.get('trans_resps') is not None:
            counts = self.bigram_counts(self.cache['trans_resps'])
        retval.update(self.weights_accumulate(counts))
        return retval

    def weights_accumulate(self, counts):
        '''Statistics of the bigram weights from the summed block counts [P, P]; None
        (trained with alignment graphs): zero counts.  The reference crashes there
        (`CategoricalSet.accumulate` needs responsibilities, `SBCategoricalSet.accumulate`
        is not implemented); zero counts are what its code means to give.'''
        param = self.categoricalset.mean_field_factorization()[0][0]
        ref = param.posterior.params.concentrations
        P = len(self.start_pdf)
        if counts is None:
            counts = torch.zeros(P, P, dtype=ref.dtype, device=ref.device)
        counts = counts.to(dtype=ref.dtype, device=ref.device)
        cstats = self.categoricalset.sufficient_statistics(counts)
        return self.categoricalset.accumulate_from_jointresps(cstats[None])
