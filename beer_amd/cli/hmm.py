"""`beer hmm <cmd>`: the callers either side of the hot path
(beer/cli/subcommands/hmm/*.py).  Same positional arguments, options, pickled
artefacts and log lines; `accumulate` / `decode` process the whole list of
utterances as ONE ragged batch on the GPU instead of a Python loop."""

import os
import pickle
import sys
import warnings

import numpy as np
import torch
import yaml

import beer_amd as beer
from beer_amd import _hip
from . import compat

# ---------------------------------------------------------------------------
# helpers


def _load(path):
    with open(path, 'rb') as f:
        return compat.load(f)


def _dump(obj, path):
    with open(path, 'wb') as f:
        pickle.dump(obj, f)


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _utt_ids(args_utts, dataset):
    if args_utts:
        stream = sys.stdin if args_utts == '-' else open(args_utts)
        return [line.strip().split()[0] for line in stream if line.strip()]
    return [utt.id for utt in dataset.utterances(random_order=False)]


def _cpu_elbo(elbo):
    'ELBO object with every tensor on the host (portable pickle).'
    # parameters are named by their uuid (models.parameters.ParameterRef): the file
    # holds neither device tensors nor model objects, `update` reads it without a GPU
    from ..models.parameters import ParameterRef
    acc = {ParameterRef(p.uuid): s.cpu() for p, s in elbo._acc_stats.items()}
    value = elbo.value.cpu() if isinstance(elbo.value, torch.Tensor) else elbo.value
    mbsize = elbo._minibatchsize
    if isinstance(mbsize, torch.Tensor):                  # after an RCCL all-reduce
        mbsize = int(round(float(mbsize)))
    refs = [ParameterRef(p.uuid) for p in elbo._model_parameters]
    return beer.EvidenceLowerBoundInstance(value, acc, refs, mbsize, elbo._datasize)


class UnitTopology:
    """A unit's HMM topology as conf/hmm.yml writes it (a list of {start_id, end_id, trans_prob})
    held as arrays: the lowest and the highest state id are the non-emitting entry and exit, the
    ids between them emit, in order (mkphones.py:12-43).  `graph(first_pdf)` instantiates it."""

    def __init__(self, arcs_conf):
        arcs = sorted({(int(a['start_id']), int(a['end_id']), float(a['trans_prob'])) for a in arcs_conf})
        self.src, self.dst = (np.asarray([a[i] for a in arcs], dtype=np.int64) for i in (0, 1))
        self.weight = np.asarray([a[2] for a in arcs], dtype=np.float64)
        ids = np.unique(np.concatenate([self.src, self.dst]))
        if not np.array_equal(ids, np.arange(len(ids))):
            raise ValueError(f'state ids of a topology must be 0 .. n-1, got {ids.tolist()}')
        self.n_states, self.n_emitting = len(ids), len(ids) - 2

    def graph(self, first_pdf):
        g = beer.graph.Graph()
        last = self.n_states - 1
        for sid in range(self.n_states):
            g.add_state(pdf_id=None if sid in (0, last) else first_pdf + sid - 1)
        g.start_state, g.end_state = 0, last
        for s, e, w in zip(self.src.tolist(), self.dst.tolist(), self.weight.tolist()):
            g.add_arc(s, e, w)
        return g


def build_units(groups_conf, grouped_names, mean, var):
    """`beer hmm mkphones` (mkphones.py:95-113): ({unit name: Graph}, JointModelSet of one
    MixtureSet per group).  `groups_conf`: {group name: its entry of conf/hmm.yml};
    `grouped_names`: {group name: [unit names]}, pdf ids running through the groups in order."""
    units, sets, next_pdf = {}, [], 0
    for group, names in grouped_names.items():
        conf = groups_conf[group]
        topo = UnitTopology(conf['topology'])
        for name in names:
            units[name] = topo.graph(next_pdf)
            next_pdf += topo.n_emitting
        n_states = topo.n_emitting * len(names)
        pool = conf.get('shared_normal_pool')
        if pool:
            # (not in the reference) the group's states share ONE pool of `pool` Gaussians and
            # differ in their mixture weights only: a tied-mixture group
            if 'n_normal_per_state' in conf:
                warnings.warn(f'group {group!r}: n_normal_per_state is ignored, its states share '
                              f'a pool of {int(pool)} Gaussians (shared_normal_pool)', stacklevel=2)
            normals = beer.NormalSet.create(
                mean=mean, cov=var, size=int(pool), prior_strength=conf['prior_strength'],
                noise_std=conf['noise_std'], cov_type=conf['cov_type'])
            sets.append(beer.TiedMixtureSet.create(n_states, normals,
                                                   prior_strength=conf['prior_strength']))
            continue
        normals = beer.NormalSet.create(
            mean=mean, cov=var, size=n_states * conf['n_normal_per_state'],
            prior_strength=conf['prior_strength'], noise_std=conf['noise_std'],
            cov_type=conf['cov_type'], shared_cov=conf['shared_cov'])
        sets.append(beer.MixtureSet.create(n_states, normals, prior_strength=conf['prior_strength']))
    return units, beer.JointModelSet(sets)


def loop_graph(unit_names, edge_units=None):
    """`beer hmm mkphoneloopgraph` (mkphoneloopgraph.py:28-75): start, end and a pivot state, every
    unit reachable from and returning to the pivot; `edge_units` (the --start-end-group) are the
    units an utterance starts and ends with, default: the pivot itself.  `graph.symbols` maps a
    state to its unit (the reference's names for the three special states)."""
    graph = beer.graph.Graph()
    graph.start_state, graph.end_state = graph.add_state(), graph.add_state()
    pivot = graph.add_state()
    state_of = {name: graph.add_state() for name in unit_names}
    edges = [state_of[u] for u in edge_units] if edge_units else [pivot]
    for arc in [(graph.start_state, e) for e in edges] + [(e, graph.end_state) for e in edges]:
        graph.add_arc(*arc)
    for state in state_of.values():
        graph.add_arc(pivot, state)
        graph.add_arc(state, pivot)
    graph.symbols = {graph.start_state: '\\<s\\>', graph.end_state: '\\</s\\>', pivot: '#1',
                     **{state: name for name, state in state_of.items()}}
    graph.normalize()
    return graph


def _only_pdf(graph, walk):
    states = [s for s, _ in walk]
    if len(states) != 1:
        raise ValueError(f'expected only one emitting state, got: {len(states)}')
    return graph.state_from_id(states[0]).pdf_id


def decode_graph(loop, units):
    """`beer hmm mkdecodegraph` (mkdecodegraph.py:19-55): every unit state of the loop replaced by
    the unit's HMM; (graph, {unit: its first pdf}, {unit: its last pdf})."""
    state_of = {unit: state for state, unit in loop.symbols.items()}
    for unit, hmm in units.items():
        loop.replace_state(state_of[unit], hmm)
    loop.normalize()
    first = {u: _only_pdf(h, h.find_next_pdf_ids(h.start_state)) for u, h in units.items()}
    last = {u: _only_pdf(h, h.find_previous_pdf_ids(h.end_state)) for u, h in units.items()}
    return loop, first, last


PRIORS = ('dirichlet', 'dirichlet2', 'dirichlet_process', 'gamma_dirichlet_process',
          'hierarchical_dirichlet_process')
BIGRAM_PRIORS = ('dirichlet2', 'hierarchical_dirichlet_process')


def phone_loop(graph, start_pdf, end_pdf, emissions, weights_prior='gamma_dirichlet_process',
               concentration=None, train_transitions=False, transitions_prior_strength=1.,
               max_duration=0, durations_prior_strength=1.):
    '''`beer hmm mkphoneloop` (mkphoneloop.py:30-80): a `BigramPhoneLoop` for the
    bigram priors (`dirichlet2`, `hierarchical_dirichlet_process`), else a `PhoneLoop`.
    `train_transitions` (not in the reference): the units' transition probabilities are
    learned too (PhoneLoop only).  `max_duration` D > 0 (not in the reference): every state
    stays 1 .. D frames under a learned duration law (PhoneLoop only).'''
    size = len(start_pdf)
    conc = concentration if concentration else size / 2
    if max_duration and weights_prior in BIGRAM_PRIORS:
        raise NotImplementedError('explicit durations (--max-duration) with a BigramPhoneLoop '
                                  f'(--weights-prior {weights_prior}) are not supported: its '
                                  'fused kernel has no duration laws')
    if train_transitions and weights_prior in BIGRAM_PRIORS:
        raise ValueError('learned transitions (--train-transitions) are not supported on a '
                         f'bigram phone loop (--weights-prior {weights_prior})')
    if weights_prior == 'dirichlet2':
        cset = beer.CategoricalSet.create(torch.ones(size, size) / size, prior_strength=conc)
        return beer.BigramPhoneLoop.create(graph.compile(), start_pdf, end_pdf, emissions, cset)
    if weights_prior == 'hierarchical_dirichlet_process':
        root = beer.SBCategorical.create(truncation=size, prior_strength=conc)
        cset = beer.SBCategoricalSet.create(size, root, prior_strength=conc)
        return beer.BigramPhoneLoop.create(graph.compile(), start_pdf, end_pdf, emissions, cset)
    if weights_prior == 'dirichlet':
        cat = beer.Categorical.create(torch.ones(size) / size, prior_strength=conc)
    elif weights_prior == 'dirichlet_process':
        cat = beer.SBCategorical.create(truncation=size, prior_strength=conc)
    elif weights_prior == 'gamma_dirichlet_process':
        cat = beer.SBCategoricalHyperPrior.create(truncation=size, prior_strength=conc,
                                                  hyper_prior_strength=1.)
    else:
        raise ValueError(f'unknown prior over the weights: {weights_prior!r}')
    return beer.PhoneLoop.create(graph.compile(), start_pdf, end_pdf, emissions, cat,
                                 train_transitions=train_transitions,
                                 transitions_prior_strength=transitions_prior_strength,
                                 max_duration=max_duration,
                                 durations_prior_strength=durations_prior_strength)


def bigram_loop(ploop, weights_prior):
    '''`beer hmm mkphoneloopbigram` (mkphoneloopbigram.py:14-49): a bigram loop on the
    unigram loop's graph, emissions and phones.  `dirichlet2` ignores the unigram's weights
    (every concentration 1 / P); the hierarchical Dirichlet process is rooted at the
    unigram's own stick-breaking weights, with prior strength P / 2.'''
    size = len(ploop.start_pdf)
    if getattr(ploop, 'transitions', None) is not None:
        raise ValueError('learned transitions are not supported on a bigram phone loop: make '
                         'the bigram loop from a unigram loop without --train-transitions')
    if getattr(ploop, 'durations', None) is not None:
        raise NotImplementedError('explicit durations (--max-duration) with a BigramPhoneLoop are '
                                  'not supported: make the bigram loop from a unigram loop '
                                  'without --max-duration')
    if weights_prior == 'dirichlet2':
        cset = beer.CategoricalSet.create(torch.ones(size, size) / size, prior_strength=1)
    elif weights_prior == 'hierarchical_dirichlet_process':
        cset = beer.SBCategoricalSet.create(size, ploop.categorical, prior_strength=size / 2)
    else:
        raise ValueError(f'unknown prior over the bigram weights: {weights_prior!r}')
    return beer.BigramPhoneLoop.create(ploop.graph, ploop.start_pdf, ploop.end_pdf,
                                       ploop.modelset, cset)


def phones_of_path(path, start_pdf, per_frame=False):
    """A pdf-id path as unit symbols (decode.py:27-40): a new unit starts wherever the path ENTERS
    the first pdf of a unit from another pdf; `per_frame` repeats the running unit for every frame."""
    path = np.asarray(path, dtype=np.int64).reshape(-1)
    names = list(start_pdf)
    firsts = np.asarray([start_pdf[n] for n in names], dtype=np.int64)
    if path[0] not in firsts:
        raise KeyError(int(path[0]))                  # (as the reference's dictionary look-up)
    enters = np.concatenate([[True], (path[1:] != path[:-1]) & np.isin(path[1:], firsts)])
    which = {int(pdf): n for n, pdf in zip(names, firsts)}
    heads = [which[int(p)] for p in path[enters]]
    if not per_frame:
        return heads
    return [heads[i] for i in np.cumsum(enters) - 1]


# ---------------------------------------------------------------------------
# commands: each is (setup(parser), main(args, logger))

class mkphones:
    'create a set of left-to-right HMM representing "phones"'

    @staticmethod
    def setup(parser):
        group = parser.add_mutually_exclusive_group(required=True)
        group.add_argument('-d', '--dataset', help='dataset for initialization')
        group.add_argument('-D', '--dimension', type=int, help='dimension of the features')
        parser.add_argument('conf', help='configuration file')
        parser.add_argument('units', help='list of units and their group')
        parser.add_argument('out', help='output phone HMMs')

    @staticmethod
    def main(args, logger):
        with open(args.conf) as f:
            conf = yaml.safe_load(f)
        groups = {g['group_name']: g for g in conf}
        grouped = {name: [] for name in groups}
        with open(args.units) as f:
            for line in f:
                name, group = line.strip().split()
                grouped[group].append(name)
        if args.dataset:
            dataset = _load(args.dataset)
            mean, var = dataset.mean, dataset.var
        else:
            mean, var = torch.zeros(args.dimension).float(), torch.ones(args.dimension).float()
        units, emissions = build_units(groups, grouped, mean, var)
        _dump((units, emissions), args.out)
        logger.info(f'created {len(units)} HMMs for a total of {len(emissions)} emitting states')
        logger.info(f'expected features dimension: {len(mean)}')


class mkphoneloopgraph:
    'create a phone-loop graph'

    @staticmethod
    def setup(parser):
        parser.add_argument('-s', '--start-end-group', help='group starting/ending the loop')
        parser.add_argument('units', help='list of units and their group')
        parser.add_argument('out', help='output phone-loop graph')

    @staticmethod
    def main(args, logger):
        with open(args.units) as f:
            units = [tuple(line.strip().split()) for line in f if line.strip()]
        edge_units = [name for name, group in units if group == args.start_end_group] \
            if args.start_end_group else None
        graph = loop_graph([name for name, _ in units], edge_units)
        _dump(graph, args.out)
        logger.info(f'created phone-loop graph. # states: {len(list(graph.states()))} '
                    f'# arcs: {len(list(graph.arcs()))} start/end group: {args.start_end_group}')


class mkdecodegraph:
    'combine a set of HMMs with a phone-loop graph'

    @staticmethod
    def setup(parser):
        parser.add_argument('phoneloop', help='phone loop graph')
        parser.add_argument('hmms', help="phones' hmms")
        parser.add_argument('out', help='output decoding graph')

    @staticmethod
    def main(args, logger):
        graph = _load(args.phoneloop)
        units, _ = _load(args.hmms)
        graph, start_pdf, end_pdf = decode_graph(graph, units)
        _dump((graph, start_pdf, end_pdf), args.out)
        logger.info(f'created decoding graph. # states: {len(list(graph.states()))} '
                    f'# arcs: {len(list(graph.arcs()))} ')


class mkphoneloop:
    'create a phone-loop model'
    PRIORS = PRIORS

    @staticmethod
    def setup(parser):
        parser.add_argument('-c', '--concentration', type=float,
                            help='concentration of the Dirichlet Process')
        parser.add_argument('--weights-prior', default='gamma_dirichlet_process',
                            choices=mkphoneloop.PRIORS, help='prior over the phone weights')
        parser.add_argument('--train-transitions', action='store_true',
                            help='learn the transition probabilities of the units too '
                                 '(Dirichlet priors; not in the reference)')
        parser.add_argument('--transitions-prior-strength', type=float, default=1.,
                            help='prior strength of the learned transition probabilities')
        parser.add_argument('--max-duration', type=int, default=0,
                            help='explicit state durations: every state stays 1 .. D frames '
                                 'under a learned law (0: the geometric stay of the self-loops; '
                                 'not in the reference)')
        parser.add_argument('--durations-prior-strength', type=float, default=1.,
                            help='prior strength of the duration laws')
        parser.add_argument('decode_graph', help='decoding graph')
        parser.add_argument('hmms', help="phones' hmm")
        parser.add_argument('out', help='phone loop model')

    @staticmethod
    def main(args, logger):
        graph, start_pdf, end_pdf = _load(args.decode_graph)
        _, emissions = _load(args.hmms)
        size = len(start_pdf)
        ploop = phone_loop(graph, start_pdf, end_pdf, emissions, args.weights_prior,
                           args.concentration, args.train_transitions,
                           args.transitions_prior_strength, args.max_duration,
                           args.durations_prior_strength)
        _dump(ploop, args.out)
        logger.info(f'successfully created a phone-loop model with {size} phones')


class mkphoneloopbigram:
    'create a bigram phone-loop model'
    PRIORS = BIGRAM_PRIORS

    @staticmethod
    def setup(parser):
        # (the reference's default, gamma_dirichlet_process, is not one of its choices:
        # the option has to be given)
        parser.add_argument('--weights-prior', default='gamma_dirichlet_process',
                            choices=mkphoneloopbigram.PRIORS,
                            help='type of prior over the phone weights')
        parser.add_argument('phoneloop', help='unigram phone loop')
        parser.add_argument('out', help='bigram phone loop (out)')

    @staticmethod
    def main(args, logger):
        ploop = _load(args.phoneloop)
        ploop2 = bigram_loop(ploop, args.weights_prior)
        _dump(ploop2, args.out)
        logger.info('successfully created a bigram phone-loop model with '
                    f'{len(ploop.start_pdf)} phones')


class mkaligraph:
    'create the alignment graphs from transcriptions (stdin)'

    @staticmethod
    def setup(parser):
        parser.add_argument('hmms', help='hmm graph for each unit')
        parser.add_argument('outdir', help='output directory')

    @staticmethod
    def main(args, logger):
        hmm_graphs, _ = _load(args.hmms)
        uttids, seqs = [], []
        for line in sys.stdin:
            tokens = line.strip().split()
            if not tokens:
                continue
            uttid, phones = tokens[0], tokens[1:]
            if not phones:
                logger.error(f'utterance {uttid} has no transcription')
                continue
            uttids.append(uttid)
            seqs.append(phones)
        # every transcription in one native call (beer_aligraphs_compile); the
        # files keep the reference's format: a pickled dense CompiledGraph
        graphs = beer.graph.compile_alignments(seqs, hmm_graphs)
        for uttid, graph in zip(uttids, graphs):
            arr = np.empty(1, dtype=object)
            arr[0] = graph.to_dense()
            np.save(os.path.join(args.outdir, uttid + '.npy'), arr)
        logger.info(f'created alignment graphs for {len(uttids)} utterances')


class phonelist:
    "print the list of phones from a set of phones' HMM"

    @staticmethod
    def setup(parser):
        parser.add_argument('hmms', help="phones' hmms")

    @staticmethod
    def main(args, logger):
        units, _ = _load(args.hmms)
        import re
        natkey = lambda s: [int(t) if t.isdigit() else t for t in re.split(r'(\d+)', s.lower())]
        for key in sorted(units.keys(), key=natkey):
            print(key)


def _shard(model, dataset, uttids, alis, logger):
    'Features and per-utterance graphs of the utterances that exist.'
    feats, graphs, kept = [], [], []
    for uttid in uttids:
        try:
            utt = dataset[uttid]
        except KeyError:
            logger.warning(f'no utterance {uttid} in the dataset')
            continue
        graph = None
        if alis is not None:
            try:
                graph = alis[uttid][0]
            except KeyError:
                logger.warning(f'no alignment graph for utterance "{uttid}"')
        feats.append(utt.features)
        graphs.append(graph)
        kept.append(uttid)
    return feats, graphs, kept


def _shard_elbo(model, feats, graphs, datasize, scale):
    '''ELBO of a shard whose utterances may have an alignment graph (`graphs[i]`, or None).
    Utterances with one train the emissions -- and learned transitions, whose categories the
    graphs are bound to here -- but give the phone weights no counts (phoneloop.py:98-100);
    those without one go through the free phone loop and DO count phones, as the reference's
    per-utterance `inference_graph=None` does (accumulate.py:45-54): two batches, one sum.'''
    elbo = beer.evidence_lower_bound(datasize=datasize)
    aligned = [i for i, g in enumerate(graphs) if g is not None]
    free = [i for i, g in enumerate(graphs) if g is None]
    if aligned:
        use = [graphs[i] for i in aligned]
        if getattr(model, 'transitions', None) is not None:
            use = model.bind_alignment_graphs(use)
        elbo = elbo + beer.accumulate_elbo(model, [feats[i] for i in aligned], datasize=datasize,
                                           inference_graphs=use, scale=scale)
    if free:
        elbo = elbo + beer.accumulate_elbo(model, [feats[i] for i in free], datasize=datasize,
                                           scale=scale)
    return elbo


def _load_alis(path):
    '''alis.npz: one `.npy` object array [CompiledGraph] per utterance
    (mkaligraph.py:60-63, accumulate.py:35,50).  Loaded eagerly; archives
    written by the reference are remapped to beer_amd classes.'''
    if not path:
        return None
    return compat.load_npz(path)


class accumulate:
    'Accumulate the ELBO from a list of utterances given from "stdin"'

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('model', help='hmm based model')
        parser.add_argument('dataset', help='training data set')
        parser.add_argument('out', help='output accumulated ELBO')

    @staticmethod
    def main(args, logger):
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        uttids = [line.strip().split()[0] for line in sys.stdin if line.strip()]
        feats, graphs, kept = _shard(model, dataset, uttids, alis, logger)
        count = len(kept)
        elbo = _shard_elbo(model, feats, graphs, dataset.size, args.acoustic_scale)
        _dump((_cpu_elbo(elbo), count), args.out)
        norm = max(count, 1) * dataset.size
        logger.info(f'accumulated ELBO over {count} utterances: {float(elbo) / norm :.3f}.')


class update:
    'Update the parameters of the model given the set of ELBO loaded from stdin'

    @staticmethod
    def setup(parser):
        parser.add_argument('-l', '--learning-rate', default=1., type=float)
        parser.add_argument('-o', '--optim-state', help='optimizer state')
        parser.add_argument('model', help='model to update')
        parser.add_argument('out_model', help='updated model')

    @staticmethod
    def main(args, logger):
        model = _load(args.model)
        optim = beer.VBConjugateOptimizer(model.conjugate_bayesian_parameters(keepgroups=True),
                                          lrate=args.learning_rate)
        if args.optim_state and os.path.isfile(args.optim_state):
            optim.load_state_dict(torch.load(args.optim_state))
        optim.init_step()
        elbo, nutts = None, 0
        for line in sys.stdin:
            if not line.strip():
                continue
            elbo_batch, nutts_batch = _load(line.strip())
            elbo = elbo_batch if elbo is None else elbo + elbo_batch
            nutts += nutts_batch
        elbo.sync(model)
        elbo.backward()
        optim.step()
        _dump(model, args.out_model)
        if args.optim_state:
            torch.save(optim.state_dict(), args.optim_state)
        logger.info(f'accumulated ELBO={float(elbo) / (nutts * elbo._datasize):.3f}')


class train:
    'train a HMM based model on a single machine'

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-b', '--batch-size', type=int, default=-1,
                            help='utterances per update (-1: all)')
        parser.add_argument('-e', '--epochs', type=int, default=1)
        parser.add_argument('-l', '--lrate', type=float, default=1.)
        parser.add_argument('model', help='hmm based model')
        parser.add_argument('dataset', help='training data set')
        parser.add_argument('out', help='output model')

    @staticmethod
    def main(args, logger):
        # (the reference's `train` refers to an optimizer that no longer exists,
        #  train.py:34; this is the working equivalent)
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=args.lrate)
        alis = _load_alis(args.alis)
        for epoch in range(1, args.epochs + 1):
            utts = list(dataset.utterances())
            bsize = len(utts) if args.batch_size <= 0 else args.batch_size
            for b in range(0, len(utts), bsize):
                batch = utts[b:b + bsize]
                optim.init_step()
                if alis is None:
                    elbo = beer.accumulate_elbo(model, [u.features for u in batch],
                                                datasize=dataset.size)
                else:
                    feats, graphs, _ = _shard(model, dataset, [u.id for u in batch], alis, logger)
                    elbo = _shard_elbo(model, feats, graphs, dataset.size, 1.)
                elbo.backward()
                optim.step()
                logger.info(f'epoch={epoch} batch={b // bsize + 1} '
                            f'ELBO={float(elbo) / (len(batch) * dataset.size):.3f}')
        _dump(model.cpu(), args.out)
        logger.info(f'finished training after {args.epochs} epochs. '
                    f'KL(q || p) = {float(model.kl_div_posterior_prior()): .3f}')


class decode:
    '''print the most likely path of all the utterances of a dataset, or (--nsamples) paths
    drawn from the posterior, or (--mbr) the minimum-Bayes-risk one of several'''

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('--per-frame', action='store_true')
        parser.add_argument('--nsamples', type=int, default=None,
                            help='print that many paths drawn from the posterior per '
                                 'utterance, as "<uttid>-<k>", instead of the most likely one')
        parser.add_argument('--seed', type=int, default=0,
                            help='seed of the random draws (with --nsamples)')
        parser.add_argument('--nbest', type=int, default=None,
                            help='print the N best STATE paths per utterance, best first, as '
                                 '"<uttid>-<r>" (N <= 16).  They are paths over the states: many '
                                 'of them differ only by a boundary frame and spell the same '
                                 'units (see --distinct)')
        parser.add_argument('--scores', default=None,
                            help='with --nbest: write "<uttid>-<r> <score>" lines to this file')
        parser.add_argument('--distinct', action='store_true',
                            help='with --nbest: among the N state paths keep the best-scoring '
                                 'one of each unit sequence and renumber (may print fewer than N)')
        parser.add_argument('--mbr', action='store_true',
                            help='with --nbest N or --nsamples N: print, as "<uttid> <units>", '
                                 'the one of the N hypotheses with the smallest expected edit '
                                 'distance to the others (minimum Bayes risk)')
        parser.add_argument('--risks', default=None,
                            help='with --mbr: write "<uttid> <chosen> <risk> <risk of '
                                 'hypothesis 1>" lines to this file')
        parser.add_argument('--mbr-scale', default=1., type=float,
                            help='with --mbr --nbest: hypothesis r weighs '
                                 'exp(MBR_SCALE * (score_r - score_1))')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('--predictive', action='store_true',
                            help='decode with the posterior-predictive (Student-t) emission '
                                 'densities instead of the expected log-likelihoods (the most '
                                 'likely path only: not with --nbest or --nsamples)')
        parser.add_argument('-u', '--utts', help='utterances to decode ("-" for stdin)')
        parser.add_argument('model', help='hmm based model')
        parser.add_argument('dataset', help='data set')

    @staticmethod
    def check(args):
        'The option errors, raised before a model or a data set is read.'
        if args.nbest is not None:
            if args.nsamples is not None:
                raise SystemExit('--nbest and --nsamples exclude each other')
            if not 1 <= args.nbest <= _hip.NBEST_MAX:
                raise SystemExit(f'--nbest: 1 .. {_hip.NBEST_MAX}')
        elif args.scores is not None or args.distinct:
            raise SystemExit('--scores and --distinct go with --nbest')
        if getattr(args, 'predictive', False) and \
                (args.nbest is not None or args.nsamples is not None):
            raise SystemExit('--predictive decodes the most likely path: not with --nbest or '
                             '--nsamples')
        if getattr(args, 'mbr', False):
            if args.nbest is None and args.nsamples is None:
                raise SystemExit('--mbr chooses among hypotheses: give --nbest N or --nsamples N')
            if getattr(args, 'predictive', False):
                raise SystemExit('--mbr: not with --predictive')
            if args.scores is not None or args.distinct:
                raise SystemExit('--mbr prints one hypothesis: not with --scores or --distinct')
            if args.nsamples is not None and args.nsamples < 1:
                raise SystemExit('--nsamples: at least 1')
        elif getattr(args, 'risks', None) is not None:
            raise SystemExit('--risks goes with --mbr')

    @staticmethod
    def nbest_lines(uttid, paths, scores, start_pdf, per_frame=False, distinct=False):
        '''The lines of one utterance under --nbest: [(label, units, score)], best first.  Ranks
        without a path are skipped; `distinct` keeps the first (best) path of every unit
        sequence and renumbers.'''
        out, seen = [], set()
        for path, value in zip(np.asarray(paths), np.asarray(scores, dtype=np.float64)):
            if path.size and path[0] < 0:
                continue
            if distinct:
                units = tuple(phones_of_path(path, start_pdf))
                if units in seen:
                    continue
                seen.add(units)
            phones = phones_of_path(path, start_pdf, per_frame)
            out.append((f'{uttid}-{len(out) + 1}', phones, float(value)))
        return out

    @staticmethod
    def mbr(args, model, feats, use, kept, logger):
        'decode --mbr: the hypothesis of smallest expected edit distance among the N of a search.'
        if not kept:
            paths, scores = [], None
        elif args.nbest is not None:
            paths, scores = beer.decode_nbest_batch(model, feats, args.nbest, inference_graphs=use,
                                                    scale=args.acoustic_scale)
        else:
            generator = torch.Generator(device=_device())
            generator.manual_seed(args.seed)
            paths = beer.sample_paths_batch(model, feats, inference_graphs=use,
                                            scale=args.acoustic_scale, nsamples=args.nsamples,
                                            generator=generator)
            scores = None
        _, index, risk = beer.mbr_select(model, paths, scores, args.mbr_scale) if kept else \
            ([], torch.zeros(0), torch.zeros(0, 1))
        index, risk = index.cpu().tolist(), risk.cpu().numpy()
        risk_lines = []
        for n, (uttid, stack) in enumerate(zip(kept, paths)):
            path = stack[index[n]].cpu().numpy()
            phones = phones_of_path(path, model.start_pdf, args.per_frame) \
                if path.size and path[0] >= 0 else []
            print(uttid, ' '.join(phones))
            risk_lines.append(f'{uttid} {index[n] + 1} {risk[n, index[n]]:.6f} {risk[n, 0]:.6f}\n')
        if args.risks is not None:
            with open(args.risks, 'w') as f:
                f.writelines(risk_lines)
        logger.info(f'successfully chose among the hypotheses of {len(kept)} utterances.')

    @staticmethod
    def main(args, logger):
        decode.check(args)
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        feats, graphs, kept = _shard(model, dataset, _utt_ids(args.utts, dataset), alis, logger)
        use = None if alis is None else [g if g is not None else model.graph for g in graphs]
        if args.mbr:
            decode.mbr(args, model, feats, use, kept, logger)
            return
        if args.nbest is not None:
            paths, scores = beer.decode_nbest_batch(
                model, feats, args.nbest, inference_graphs=use, scale=args.acoustic_scale) \
                if kept else ([], np.zeros((0, args.nbest)))
            scores = scores.cpu().numpy() if kept else scores
            score_lines, n = [], 0
            for uttid, p, s in zip(kept, paths, scores):
                for label, phones, value in decode.nbest_lines(
                        uttid, p.cpu().numpy(), s, model.start_pdf, args.per_frame, args.distinct):
                    print(label, ' '.join(phones))
                    score_lines.append(f'{label} {value:.6f}\n')
                    n += 1
            if args.scores is not None:
                with open(args.scores, 'w') as f:
                    f.writelines(score_lines)
            logger.info(f'successfully decoded {n} paths of {len(kept)} utterances.')
            return
        if args.nsamples is not None:
            if args.nsamples < 1:
                raise SystemExit('--nsamples: at least 1')
            generator = torch.Generator(device=_device())
            generator.manual_seed(args.seed)
            draws = beer.sample_paths_batch(model, feats, inference_graphs=use,
                                            scale=args.acoustic_scale, nsamples=args.nsamples,
                                            generator=generator) if kept else []
            for uttid, paths in zip(kept, draws):
                for k, path in enumerate(paths.cpu().numpy(), start=1):
                    phones = phones_of_path(path, model.start_pdf, args.per_frame)
                    print(f'{uttid}-{k}', ' '.join(phones))
            logger.info(f'successfully drew {args.nsamples} paths for {len(kept)} utterances.')
            return
        paths = beer.decode_batch(model, feats, inference_graphs=use, scale=args.acoustic_scale,
                                  predictive=args.predictive) if kept else []
        for uttid, path in zip(kept, paths):
            phones = phones_of_path(path.cpu().numpy(), model.start_pdf, args.per_frame)
            print(uttid, ' '.join(phones))
        logger.info(f'successfully decoded {len(kept)} utterances.')


class score:
    '''print the log-evidence ln p(x) of all the utterances of a dataset under the model (the
    forward score, summed over all state paths): "<uttid> <log-evidence> <n_frames>"'''

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('--predictive', action='store_true',
                            help='score with the posterior-predictive (Student-t) emission '
                                 'densities: the held-out likelihood of the Bayesian model '
                                 '(the default scores with exp(E[ln p]), which is not a density)')
        parser.add_argument('-u', '--utts', help='utterances to score ("-" for stdin)')
        parser.add_argument('model', help='hmm based model')
        parser.add_argument('dataset', help='data set')

    @staticmethod
    def main(args, logger):
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        feats, graphs, kept = _shard(model, dataset, _utt_ids(args.utts, dataset), alis, logger)
        use = None if alis is None else [g if g is not None else model.graph for g in graphs]
        values = beer.log_evidence_batch(
            model, feats, inference_graphs=use, scale=args.acoustic_scale,
            predictive=args.predictive).cpu().tolist() if kept else []
        total, n_frames = 0., 0
        for uttid, value, utt in zip(kept, values, feats):
            print(uttid, '%.6f' % value, len(utt))
            total, n_frames = total + value, n_frames + len(utt)
        logger.info(f'scored {len(kept)} utterances: total log-evidence {total:.3f}, '
                    f'{total / max(n_frames, 1):.4f} per frame over {n_frames} frames.')


class boundaries:
    '''write the unit-start posteriors of all the utterances of a dataset, "<outdir>/<uttid>.npy"
    [T, n_units]: the probability that a unit begins at a frame (summed over the units: the
    boundary posterior of the frame); --counts also prints the expected number of occurrences of
    every unit, "<uttid> <count of unit 1> ... <count of unit U>"'''

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('-u', '--utts', help='utterances to process ("-" for stdin)')
        parser.add_argument('--counts', action='store_true',
                            help='print the expected unit counts of every utterance')
        parser.add_argument('model', help='phone-loop model')
        parser.add_argument('dataset', help='data set')
        parser.add_argument('outdir', help='output directory')

    @staticmethod
    def main(args, logger):
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        feats, graphs, kept = _shard(model, dataset, _utt_ids(args.utts, dataset), alis, logger)
        use = None if alis is None else [g if g is not None else model.graph for g in graphs]
        os.makedirs(args.outdir, exist_ok=True)
        starts = beer.unit_starts_batch(model, feats, inference_graphs=use,
                                        scale=args.acoustic_scale) if kept else []
        # (the counts in float64 from the kernel's own sums, not from the written rows)
        counts = beer.unit_counts_batch(model, feats, inference_graphs=use,
                                        scale=args.acoustic_scale).cpu().numpy() \
            if kept and args.counts else None
        total = 0.
        for n, (uttid, post) in enumerate(zip(kept, starts)):
            post = post.cpu().numpy()
            np.save(os.path.join(args.outdir, f'{uttid}.npy'), post)
            total += float(post.sum(dtype=np.float64))
            if counts is not None:
                print(uttid, ' '.join('%.6f' % c for c in counts[n]))
        logger.info(f'wrote the unit-start posteriors of {len(kept)} utterances: '
                    f'{total / max(len(kept), 1):.2f} expected units per utterance.')


def lattice_entries(margins, beam):
    '''(frame int32, unit int32, margin float64) of the entries of a [T, n_units] array of
    unit-start max-marginals that lie within `beam` of the best path, sorted by frame and then
    by unit.'''
    margins = np.asarray(margins, dtype=np.float64)
    frame, unit = np.nonzero(margins >= -beam)             # (row-major: by frame, then by unit)
    return frame.astype(np.int32), unit.astype(np.int32), margins[frame, unit]


class lattice:
    '''write the unit-start lattice of all the utterances of a dataset, "<outdir>/<uttid>.npz":
    every (frame, unit) at which the unit can begin on a path whose score is within --beam of the
    best path's, with the score lost ("margin", 0 on the Viterbi segmentation), the Viterbi
    "score" and the "units"; prints "<uttid> <score> <n_entries> <n_frames>".  --segments also
    stores the unit segments within the beam, "seg_unit" from frame "seg_start" to frame "seg_end"
    with the score lost "seg_margin", sorted by (start, unit, end), and appends their number to
    the printed line'''

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('-u', '--utts', help='utterances to process ("-" for stdin)')
        parser.add_argument('--beam', default=10., type=float,
                            help='keep what is within this score of the best path (default 10)')
        parser.add_argument('--segments', action='store_true',
                            help='also store the unit segments (unit, start, end) within the beam')
        parser.add_argument('--max-dur', default=100, type=int,
                            help='with --segments: the longest segment, in frames (default 100)')
        parser.add_argument('model', help='phone-loop model')
        parser.add_argument('dataset', help='data set')
        parser.add_argument('outdir', help='output directory')

    @staticmethod
    def main(args, logger):
        if not (args.beam >= 0. and np.isfinite(args.beam)):
            raise SystemExit(f'--beam: a finite number >= 0, not {args.beam}')
        if args.max_dur < 1:
            raise SystemExit(f'--max-dur: at least 1 frame, not {args.max_dur}')
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        feats, graphs, kept = _shard(model, dataset, _utt_ids(args.utts, dataset), alis, logger)
        use = None if alis is None else [g if g is not None else model.graph for g in graphs]
        os.makedirs(args.outdir, exist_ok=True)
        scores, margins = beer.unit_start_margins_batch(
            model, feats, inference_graphs=use, scale=args.acoustic_scale) if kept else ([], [])
        segments = beer.unit_segments_batch(
            model, feats, beam=args.beam, max_dur=args.max_dur, inference_graphs=use,
            scale=args.acoustic_scale)[1] if kept and args.segments else [None] * len(kept)
        units = np.asarray([str(u) for u in model.start_pdf])
        total = n_segments = 0
        for uttid, score, margin, segs in zip(kept, scores.cpu().tolist() if kept else [], margins,
                                              segments):
            frame, unit, value = lattice_entries(margin.cpu().numpy(), args.beam)
            more, tail = {}, ()
            if segs is not None:
                more = dict(zip(('seg_start', 'seg_end', 'seg_unit', 'seg_margin'),
                                (v.cpu().numpy() for v in segs)))
                tail = (len(more['seg_start']),)
                n_segments += tail[0]
            np.savez(os.path.join(args.outdir, f'{uttid}.npz'), frame=frame, unit=unit,
                     margin=value, score=np.float64(score), units=units, **more)
            print(uttid, '%.6f' % score, len(frame), len(margin), *tail)
            total += len(frame)
        logger.info(f'wrote the unit-start lattices of {len(kept)} utterances within a beam of '
                    f'{args.beam:g}: {total / max(len(kept), 1):.1f} entries per utterance' +
                    (f', {n_segments / max(len(kept), 1):.1f} segments' if args.segments else '') +
                    '.')


class segments:
    '''write the unit segments of all the utterances of a dataset with their posteriors,
    "<outdir>/<uttid>.npz": every "unit" that begins at frame "start" and lasts until frame "end"
    with a probability "post" of at least --min-post, sorted by (start, unit, end), the
    "log_evidence" and the "units"; prints "<uttid> <log-evidence> <n_segments> <n_frames>".
    --durations also saves the expected duration histogram of the shard, [n_units, max_dur]: how
    many instances of a unit last exactly k + 1 frames'''

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('-u', '--utts', help='utterances to process ("-" for stdin)')
        parser.add_argument('--min-post', default=1e-3, type=float,
                            help='keep the segments of at least this posterior (default 0.001)')
        parser.add_argument('--max-dur', default=None, type=int,
                            help='the longest segment, in frames (default: the utterance)')
        parser.add_argument('--durations', metavar='FILE',
                            help='save the expected duration histogram of the shard as "npy" '
                                 '(needs --max-dur)')
        parser.add_argument('model', help='phone-loop model')
        parser.add_argument('dataset', help='data set')
        parser.add_argument('outdir', help='output directory')

    @staticmethod
    def main(args, logger):
        if not 0. <= args.min_post <= 1.:
            raise SystemExit(f'--min-post: a probability in [0, 1], not {args.min_post}')
        if args.max_dur is not None and args.max_dur < 1:
            raise SystemExit(f'--max-dur: at least 1 frame, not {args.max_dur}')
        if args.durations is not None and args.max_dur is None:
            raise SystemExit('--durations needs --max-dur: the width of the histogram')
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        feats, graphs, kept = _shard(model, dataset, _utt_ids(args.utts, dataset), alis, logger)
        use = None if alis is None else [g if g is not None else model.graph for g in graphs]
        os.makedirs(args.outdir, exist_ok=True)
        evidence, segs = beer.unit_segment_posteriors_batch(
            model, feats, min_post=args.min_post, max_dur=args.max_dur, inference_graphs=use,
            scale=args.acoustic_scale) if kept else ([], [])
        units = np.asarray([str(u) for u in model.start_pdf])
        total = 0
        for uttid, value, utt, seg in zip(kept, evidence.cpu().tolist() if kept else [], feats,
                                          segs):
            start, end, unit, post = (v.cpu().numpy() for v in seg)
            np.savez(os.path.join(args.outdir, f'{uttid}.npz'), start=start, end=end, unit=unit,
                     post=post, log_evidence=np.float64(value), units=units)
            print(uttid, '%.6f' % value, len(start), len(utt))
            total += len(start)
        if args.durations is not None:
            hist = beer.unit_durations_batch(
                model, feats, args.max_dur, inference_graphs=use,
                scale=args.acoustic_scale).cpu().numpy() if kept else \
                np.zeros((len(units), args.max_dur))
            with open(args.durations, 'wb') as f:           # (np.save would append ".npy")
                np.save(f, hist)
        logger.info(f'wrote the unit segments of {len(kept)} utterances with a posterior of at '
                    f'least {args.min_post:g}: {total / max(len(kept), 1):.1f} per utterance.')


def read_utt2spk(path):
    '{utterance id: speaker} of a text file, one "<uttid> <speaker>" per line.'
    out = {}
    with open(path) as f:
        for n, line in enumerate(f, start=1):
            tokens = line.split()
            if not tokens:
                continue
            if len(tokens) != 2:
                raise SystemExit(f'{path}:{n}: expected "<uttid> <speaker>", got {line.strip()!r}')
            out[tokens[0]] = tokens[1]
    return out


def speakers_of(uttids, utt2spk):
    '''(names, index per utterance): the speakers of `uttids` in order of first appearance.  An
    utterance without a speaker is an error that names it.'''
    names, where, idx = [], {}, []
    for uttid in uttids:
        if uttid not in utt2spk:
            raise SystemExit(f'utt2spk: no speaker for utterance "{uttid}"')
        spk = utt2spk[uttid]
        if spk not in where:
            where[spk] = len(names)
            names.append(spk)
        idx.append(where[spk])
    return names, idx


class adapt:
    '''estimate one affine feature transform per speaker (constrained MLLR) under the model and
    write them as an "npz" archive ("speakers", "W" [n, D, D + 1]); prints
    "<speaker> <n_frames> <gain per frame>" per speaker, the gain of the auxiliary function
    summed over the rounds (a lower bound of the gain in log-likelihood per frame)'''

    @staticmethod
    def setup(parser):
        parser.add_argument('-a', '--alis', help='alignment graphs in a "npz" archive')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('--iters', type=int, default=3,
                            help='rounds of statistics and estimation (default 3)')
        parser.add_argument('--sweeps', type=int, default=20,
                            help='sweeps over the rows of a transform per round (default 20)')
        parser.add_argument('--min-count', type=float, default=500.,
                            help='frames a speaker needs to get a transform (default 500)')
        parser.add_argument('--init', metavar='TRANSFORMS',
                            help='transforms to start from (default: the identity)')
        parser.add_argument('-u', '--utts', help='utterances to use ("-" for stdin)')
        parser.add_argument('model', help='hmm based model')
        parser.add_argument('dataset', help='data set')
        parser.add_argument('utt2spk', help='text file, "<uttid> <speaker>" per line')
        parser.add_argument('out', help='output transforms ("npz")')

    @staticmethod
    def main(args, logger):
        if args.iters < 1 or args.sweeps < 1:
            raise SystemExit('--iters and --sweeps: at least 1')
        utt2spk = read_utt2spk(args.utt2spk)
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        alis = _load_alis(args.alis)
        feats, graphs, kept = _shard(model, dataset, _utt_ids(args.utts, dataset), alis, logger)
        names, idx = speakers_of(kept, utt2spk)
        use = None if alis is None else [g if g is not None else model.graph for g in graphs]
        init = None
        if args.init:
            # the speakers of this run, in its order: those of the file keep their transform
            old = beer.AffineTransforms.load(args.init)
            init = beer.AffineTransforms(names, old.dim)
            for n, at in enumerate(old.indices(names)):
                if at >= 0:
                    init.W[n] = old.W[at]
        frames = np.zeros(len(names), dtype=np.int64)
        for n, utt in zip(idx, feats):
            frames[n] += len(utt)
        if kept:
            transforms, gains = beer.adapt(
                model, feats, idx, names, iters=args.iters, transforms=init,
                inference_graphs=use, scale=args.acoustic_scale, sweeps=args.sweeps,
                min_count=args.min_count)
            total = np.sum(gains, axis=0)
        else:
            transforms, total = beer.AffineTransforms(names, dataset.mean.shape[0]), np.zeros(0)
        transforms.save(args.out)
        for name, count, gain in zip(names, frames.tolist(), total.tolist()):
            print(name, count, '%.6f' % gain)
        logger.info(f'estimated the transforms of {len(names)} speakers from {len(kept)} '
                    f'utterances ({int(frames.sum())} frames).')


class posteriors:
    'state / phone posteriors of all the utterances of a dataset'
    EPS = 1e-5

    @staticmethod
    def setup(parser):
        parser.add_argument('-S', '--state', action='store_true', help='state level')
        parser.add_argument('-l', '--log', action='store_true', help='log domain')
        parser.add_argument('-s', '--acoustic-scale', default=1., type=float)
        parser.add_argument('-u', '--utts', help='utterances ("-" for stdin)')
        parser.add_argument('model', help='hmm based model')
        parser.add_argument('dataset', help='data set')
        parser.add_argument('outdir', help='output directory')

    @staticmethod
    def main(args, logger):
        model = _load(args.model).to(_device())
        dataset = _load(args.dataset)
        count = 0
        for uttid in _utt_ids(args.utts, dataset):
            try:
                utt = dataset[uttid]
            except KeyError:
                logger.warning(f'no data for utterance {uttid}')
                continue
            posts = model.posteriors(utt.features, scale=args.acoustic_scale).cpu().numpy()
            if not args.state:
                out = np.zeros((len(posts), len(model.start_pdf)))
                for i, unit in enumerate(model.start_pdf):
                    out[:, i] = posts[:, model.start_pdf[unit]:model.end_pdf[unit]].sum(axis=-1)
                posts = out
            if args.log:
                posts = np.log(posteriors.EPS + posts)
            np.save(os.path.join(args.outdir, f'{uttid}.npy'), posts)
            count += 1
        logger.info(f'successfully computed the posteriors for {count} utterances.')


def read_alignments(path):
    'A file of per-frame alignments "<uttid> <label per frame ...>" as {uttid: [labels]}, in order.'
    alis = {}
    with open(path) as f:
        for line in f:
            tokens = line.split()
            if tokens:
                alis[tokens[0]] = tokens[1:]
    return alis


def _merge_repeats(labels):
    labels = np.asarray(labels, dtype=np.int64)
    return labels[np.concatenate([[True], labels[1:] != labels[:-1]])] if labels.size else labels


class evaluate:
    '''score per-frame unit alignments against reference alignments (the recipe's score_aud):
    every unit is mapped to the reference label it shares most frames with, then the equivalent
    phone error rate (repeats merged on both sides; edit distances on the GPU), the normalised
    mutual information, the entropy rate of the units and the recall / precision / F-score of
    the unit boundaries are printed as "key value" lines'''

    KEYS = ('PER', 'sub', 'del', 'ins', 'NMI', 'entropy_rate', 'perplexity', 'recall',
            'precision', 'fscore', 'n_units')

    @staticmethod
    def setup(parser):
        parser.add_argument('--delta', default=2, type=int,
                            help='frames a unit boundary may lie from a reference boundary and '
                                 'still hit it')
        parser.add_argument('--mapping', default=None,
                            help='write the "<unit> <reference label>" mapping to this file')
        parser.add_argument('--lists', action='store_true',
                            help='the hypothesis file holds lists, "<uttid>-<r> <labels>" '
                                 '(decode --nbest / --nsamples --per-frame): the scores are '
                                 'those of every utterance\'s first hypothesis, and closest_PER '
                                 'that of the closest one of its list')
        parser.add_argument('ref_ali', help='reference per-frame alignments')
        parser.add_argument('hyp_ali', help='per-frame alignments to score')

    @staticmethod
    def collect(ref, hyp, lists):
        '''(uttids, reference labels, hypothesis lists) of the utterances both sides have, in the
        reference's order, and the number skipped; SystemExit naming an utterance whose sides
        differ in length.'''
        if lists:
            grouped = {}
            for label, frames in hyp.items():
                uttid, _, rank = label.rpartition('-')
                if not uttid or not rank.isdigit():
                    raise SystemExit(f'--lists: "{label}" is not "<uttid>-<r>"')
                grouped.setdefault(uttid, []).append((int(rank), frames))
            hyp = {u: [frames for _, frames in sorted(h, key=lambda e: e[0])]
                   for u, h in grouped.items()}
        else:
            hyp = {u: [frames] for u, frames in hyp.items()}
        uttids = [u for u in ref if u in hyp]
        skipped = len(ref) - len(uttids) + sum(1 for u in hyp if u not in ref)
        for u in uttids:
            for frames in hyp[u]:
                if len(frames) != len(ref[u]):
                    raise SystemExit(f'{u}: {len(ref[u])} reference frames, {len(frames)} in '
                                     'the hypothesis')
        return uttids, [ref[u] for u in uttids], [hyp[u] for u in uttids], skipped

    @staticmethod
    def scores(ref, hyps, delta=2):
        '''The scores as (key, text) lines, the unit -> reference label mapping and, for lists,
        the line of the closest hypotheses: `ref` one list of labels per utterance, `hyps` one
        list of such lists per utterance.'''
        ref_names = sorted({l for utt in ref for l in utt})
        hyp_names = sorted({l for lst in hyps for utt in lst for l in utt})
        ref_id = {l: i for i, l in enumerate(ref_names)}
        hyp_id = {l: i for i, l in enumerate(hyp_names)}
        R = [np.asarray([ref_id[l] for l in utt], dtype=np.int64) for utt in ref]
        H = [[np.asarray([hyp_id[l] for l in utt], dtype=np.int64) for utt in lst] for lst in hyps]
        first = [lst[0] for lst in H]
        counts = beer.contingency(R, first) if R else np.zeros((0, 0), dtype=np.int64)
        if counts.shape[0] < len(hyp_names):          # (units only later ranks use: no overlap)
            counts = np.concatenate([counts, np.zeros((len(hyp_names) - counts.shape[0],
                                                       counts.shape[1]), dtype=np.int64)])
        mapping = beer.maxoverlap_mapping(counts)
        refs = [_merge_repeats(r) for r in R]
        errors = beer.token_error_rate(refs, [_merge_repeats(mapping[h]) for h in first])
        nmi = beer.normalized_mutual_information(counts)
        entropy, perplexity = beer.entropy_rate(first)
        bounds = beer.boundary_scores(R, first, delta=delta)

        def percent(n):
            return '%.2f' % (100. * n / errors.n_ref if errors.n_ref else 0.)
        lines = [('PER', '%.2f' % errors.rate), ('sub', percent(errors.sub)),
                 ('del', percent(errors.dele)), ('ins', percent(errors.ins)),
                 ('NMI', '%.2f' % nmi), ('entropy_rate', '%.2f' % entropy),
                 ('perplexity', '%.2f' % perplexity), ('recall', '%.2f' % bounds.recall),
                 ('precision', '%.2f' % bounds.precision), ('fscore', '%.2f' % bounds.fscore),
                 ('n_units', str(len(hyp_names)))]
        closest = beer.closest_error_rate(refs, [[_merge_repeats(mapping[h]) for h in lst]
                                               for lst in H])
        named = [(u, ref_names[int(mapping[i])]) for i, u in enumerate(hyp_names)] \
            if ref_names else []
        return lines, named, ('closest_PER', '%.2f' % closest.rate)

    @staticmethod
    def main(args, logger):
        ref, hyp = read_alignments(args.ref_ali), read_alignments(args.hyp_ali)
        uttids, R, H, skipped = evaluate.collect(ref, hyp, args.lists)
        lines, mapping, closest = evaluate.scores(R, H, args.delta)
        for key, text in lines + ([closest] if args.lists else []):
            print(key, text)
        if args.mapping is not None:
            with open(args.mapping, 'w') as f:
                f.writelines(f'{unit} {label}\n' for unit, label in mapping)
        logger.info(f'scored {len(uttids)} utterances; {skipped} without a counterpart were '
                    'skipped.')


def duration_lines(model):
    '''The lines of `beer hmm durations`: "<unit> <state> <mean frames> <mode> <p(1)> .. <p(D)>"
    per state of every unit (the states of a unit counted from 0), from the posterior means of
    the duration laws.'''
    if getattr(model, 'durations', None) is None:
        raise SystemExit('the model has no explicit durations (mkphoneloop --max-duration)')
    probs, means = model.durations.expected_durations()
    lines = []
    for unit in model.start_pdf:
        for k, pdf in enumerate(range(int(model.start_pdf[unit]), int(model.end_pdf[unit]) + 1)):
            row = probs[pdf]
            lines.append(' '.join([str(unit), str(k), '%.4f' % float(means[pdf]),
                                   str(int(row.argmax()) + 1)] + ['%.6f' % float(p) for p in row]))
    return lines


class durations:
    '''print the learned duration laws of a model made with --max-duration:
    "<unit> <state> <mean frames> <mode> <p(1)> .. <p(D)>" per unit state'''

    @staticmethod
    def setup(parser):
        parser.add_argument('model', help='phone-loop model with explicit durations')

    @staticmethod
    def main(args, logger):
        for line in duration_lines(_load(args.model)):
            print(line)


COMMANDS = [accumulate, decode, mkaligraph, mkdecodegraph, mkphoneloop, mkphoneloopbigram,
            mkphoneloopgraph, mkphones, posteriors, phonelist, train, update, score, lattice,
            segments, adapt, durations, evaluate, boundaries]
