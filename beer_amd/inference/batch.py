"""Batched E-step: the MI355X-first counterpart of the reference's
per-utterance accumulation loop.

The reference's data-parallel "map" step (`beer hmm accumulate`,
beer/cli/subcommands/hmm/accumulate.py:39-59) calls `evidence_lower_bound`
once per utterance -- a Python loop over ~300-frame utterances with tens of
torch ops each.  `accumulate_elbo` does the same work for a whole shard in a
handful of kernel launches over a ragged batch and returns the SAME object the
loop would have produced:

    elbo = evidence_lower_bound(datasize=N)
    for utt in shard:
        elbo += evidence_lower_bound(model, utt, datasize=N, ...)

i.e. value = sum_u (N / T_u) sum_t l_ut - U * KL(q || p)   (quirk Q1),
acc_stats = sum_u acc_u, minibatchsize = sum_u T_u.  The KL term is computed
once.  Sufficient statistics are accumulated in fp64 across the whole shard.
"""

import os
import threading

import torch

from .. import _hip, hmm_kernels as hk, kernels
from ..models.gaussians import NormalSet
from ..models.mixtures import Mixture, MixtureSet, TiedMixtureSet
from ..models.modelset import JointModelSet
from ..models.sequence import HMM, BigramPhoneLoop, PhoneLoop, unit_start_categories
from ..models.vae import VAE
from ..stats import FrameStats
from .objectives import EvidenceLowerBoundInstance

__all__ = ['accumulate_elbo', 'pack_utterances', 'decode_batch', 'sample_paths_batch',
           'log_evidence_batch', 'unit_starts_batch', 'unit_counts_batch',
           'unit_start_margins_batch', 'unit_segments_batch', 'ShardStatics',
           'decode_nbest_batch', 'unit_segment_posteriors_batch', 'unit_durations_batch']

# Scratch of one sub-batch (responsibilities, per-state likelihoods, trellis): up to
# three sub-batches are in flight, so a sub-batch may take an eighth of what is free on
# the device when the first batch is cut, at most 48 GB (a 288 GB MI355X to itself:
# 36 GB -- the 10 M frames of BASELINE config 3 are then ONE launch of every kernel, 29 GB
# of scratch; a smaller or shared device: less).  BEER_SCRATCH_GB overrides.
_SCRATCH_CAP = 48 << 30
_scratch_bytes = [int(os.environ['BEER_SCRATCH_GB']) << 30 if 'BEER_SCRATCH_GB' in os.environ
                  else None]


def _scratch_budget():
    if _scratch_bytes[0] is None:
        try:
            free, _ = torch.cuda.mem_get_info()
            _scratch_bytes[0] = max(1 << 28, min(_SCRATCH_CAP, free // 8))
        except Exception:                                   # no device: the caller raises later
            _scratch_bytes[0] = _SCRATCH_CAP
    return _scratch_bytes[0]


class ShardStatics:
    '''What `accumulate_elbo` derives from the utterance LENGTHS and the data-set size alone
    -- offsets, the per-utterance weights datasize / T_u on the device, the cut into
    sub-batches -- kept by the caller across the iterations over one shard (like
    `FrameImages` for the frames: nothing is cached behind the caller's back).  One object
    per (utterances, datasize) pair; a call whose lengths do not match what the object was
    filled with refills it.  Without one these are rebuilt per call: a 33 k-element host
    loop and two small uploads per iteration, and -- uploads cannot be recorded -- no
    capture of the iteration as a HIP graph (`CapturedIteration`).'''

    def __init__(self):
        self.key, self.items, self.lengths, self.mark = None, {}, None, None

    def bind(self, lengths):
        '''The shard these statics belong to: the same list object (the usual case: O(1)) or
        an equal one keeps them, anything else empties them.'''
        n = len(lengths)
        mark = (n, lengths[0], lengths[n // 2], lengths[-1]) if n else (0,)
        if self.lengths is not lengths or self.mark != mark:
            # (the same list edited in place is caught where it is cheap to look: its length
            #  and three of its entries)
            if self.mark != mark or self.lengths != lengths:
                self.key, self.items = None, {}
            self.lengths, self.mark = lengths, mark

    def entry(self, key, name, make):
        if self.key != key:
            self.key, self.items = key, {}
        if name not in self.items:
            self.items[name] = make()
        return self.items[name]


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def pack_utterances(utterances):
    '''(X [sum T_u, D] on the GPU, lengths list).  Accepts a list of [T_u, D]
    tensors or an already packed `(X, lengths)` pair.'''
    if isinstance(utterances, tuple) and len(utterances) == 2 and \
            isinstance(utterances[0], torch.Tensor):
        X, lengths = utterances
        # (a list of Python ints is handed through as it is: `ShardStatics` recognises the
        # caller's list by identity)
        if not (isinstance(lengths, list) and set(map(type, lengths)) <= {int}):
            lengths = [int(n) for n in lengths]
        return _hip.on_device(X), lengths
    utterances = list(utterances)
    lengths = [len(u) for u in utterances]
    dev = _hip.require_device()
    X = torch.cat([u.to(dev) for u in utterances], dim=0).contiguous()
    return X, lengths


def _groups(emissions):
    '''Flatten an emission model into [(MixtureSet | TiedMixtureSet | NormalSet, S, G)].  A
    nested MixtureSet is one group of S mixtures of its G leaves
    (`MixtureSet.leaf_log_weights`); a TiedMixtureSet one of S mixtures of the G = K Gaussians
    of its pool, which it does not own S times: `_n_gaussians`.'''
    if isinstance(emissions, JointModelSet):
        out = []
        for m in emissions.modelsets:
            out += _groups(m)
        return out
    if isinstance(emissions, MixtureSet):
        return [(emissions, len(emissions), emissions.n_leaves_per_mixture)]
    if isinstance(emissions, TiedMixtureSet):
        return [(emissions, len(emissions), len(emissions.modelset))]
    if isinstance(emissions, NormalSet):
        return [(emissions, len(emissions), 1)]
    raise NotImplementedError(f'unsupported emission model {type(emissions).__name__}')


def _normalset(group):
    return group.normalset if isinstance(group, (MixtureSet, TiedMixtureSet)) else group


def _n_gaussians(group, S, G):
    'Rows of the group\'s Gaussian statistics: S x G, or the K of a tied group\'s one pool.'
    return G if isinstance(group, TiedMixtureSet) else S * G


def _sub_batches(lengths, bytes_per_frame, max_frames):
    '''Split utterance indices into runs whose scratch fits the budget.  The
    runs are balanced (same number of frames, within an utterance) rather than
    filled greedily: equal-sized scratch tensors are recycled by the caching
    allocator, unequal ones make it hipMalloc / hipFree gigabytes every
    iteration (25 ms stalls at config 3).'''
    budget = max(1, min(max_frames, _scratch_budget() // max(1, bytes_per_frame)))
    total = sum(lengths)
    n_runs = max(1, -(-total // budget))
    target = -(-total // n_runs)
    runs, cur, n = [], [], 0
    for u, T in enumerate(lengths):
        if cur and (n + T > budget or (n >= target and len(runs) < n_runs - 1)):
            runs.append(cur)
            cur, n = [], 0
        cur.append(u)
        n += T
    if cur:
        runs.append(cur)
    return runs


# Per host thread (a thread drives its own stream of sub-batches: two training loops in two
# threads must not pop each other's events) -- the throttle's queue and the KL side streams.
_local = threading.local()


def _throttle(depth=2):
    '''Keep the host at most `depth` sub-batches ahead of the GPU.  Every
    sub-batch allocates gigabytes of scratch (responsibilities, per-state
    likelihoods); a host that queues many of them before the first has run
    makes the caching allocator hipMalloc new blocks instead of recycling --
    tens of ms each, and the stream waits for them.'''
    if _capturing():
        return torch.cuda.Event()             # (a recording does not run: nothing to wait for)
    in_flight = _local.__dict__.setdefault('in_flight', [])
    while len(in_flight) >= depth:
        in_flight.pop(0).synchronize()
    ev = torch.cuda.Event()
    in_flight.append(ev)
    return ev


def _cached_batch(graph, run_lengths, dtype):
    '''Batch descriptor of utterances that all use `graph` (the free phone
    loop).  Training iterates over the same shard again and again: the
    descriptor is kept on the graph and reused as long as the graph's device
    image is the same object (its weights are refreshed in place), so the
    steady-state iteration has no host -> device copy at all.'''
    cache = graph.__dict__.setdefault('_batch_cache', {})
    key = (dtype, tuple(run_lengths))
    dg = graph.device_graph(dtype)
    hit = cache.get(key)
    if hit is not None and hit.dgraphs[0] is dg:
        return hit
    if len(cache) >= 8:
        cache.clear()
    batch = hk.HmmBatch([graph], [0] * len(run_lengths), run_lengths, dtype)
    cache[key] = batch
    return batch


_KL_BESIDE = os.environ.get('BEER_KL_SIDE_STREAM', '1') != '0'


def _kl_beside_the_estep(model, device):
    '''KL(q || p) of the model's parameters on a side stream: a dozen small launches
    (expected statistics and log-normalisers of the Dirichlets, the KL kernels, their
    sums) that depend on the parameters only, not on the frames -- queued beside the
    E-step kernels instead of in front of them.  Returns (kl, event or None); the
    caller makes its stream wait for the event before it uses `kl`.  The side stream
    starts behind everything queued so far (the previous M-step), and the next call
    starts behind this one's consumers: tensors it allocates are not recycled early.'''
    if not _KL_BESIDE or isinstance(model, VAE) or device.type != 'cuda' or _capturing():
        return torch.as_tensor(model.kl_div_posterior_prior()), None
    main = torch.cuda.current_stream(device)
    # Everything the distributions memoise -- expected statistics (which the E-step
    # reads: `natural_form()`), log-normalisers, natural parameters -- is produced HERE,
    # on the main stream: a memo entry written by a side-stream kernel would be picked up
    # by the main stream's E-step with nothing ordering the two.  What is left for the
    # side stream are the KL kernels and their sums, whose results nobody reads before
    # the caller has waited for the event.
    for param in model.bayesian_parameters():
        for dist in (getattr(param, 'posterior', None), getattr(param, 'prior', None)):
            if dist is not None and hasattr(dist, 'expected_sufficient_statistics'):
                dist.expected_sufficient_statistics()
                dist.log_norm()
                dist.natural_parameters()
    side_streams = _local.__dict__.setdefault('side_streams', {})
    side = side_streams.get(device)
    if side is None:
        side = side_streams[device] = torch.cuda.Stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        kl = torch.as_tensor(model.kl_div_posterior_prior())
        done = side.record_event()
    return kl, done


def _finish(model, value_terms, kl, nutt, acc, datasize, total_frames):
    value = value_terms - float(nutt) * kl.to(value_terms.device, torch.float64)
    return EvidenceLowerBoundInstance(value, acc, model.bayesian_parameters(),
                                      total_frames, datasize)


def _like(param, t):
    return t.to(dtype=param.stats.dtype, device=param.stats.device)


def _mixture_batch(model, X, lengths, datasize, labels, max_frames, statics=None):
    ns = model.normalset
    K, cov = len(ns), ns.cov_type
    dev, dtype = X.device, X.dtype
    exp_T = ns.means_precisions.natural_form()
    lw = model._log_weights().view(1, K)
    Q = FrameStats(X[:1], cov).shape[1]
    acc = torch.zeros(K, Q, dtype=torch.float64, device=dev)
    utt_llh = torch.zeros(len(lengths), dtype=torch.float64, device=dev)

    def offsets_and_scales():
        off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)
        # every host -> device copy happens here, BEFORE the first big kernel: a copy
        # from pageable memory makes the host wait for the stream, and one issued
        # after the E-step kernels would keep the host from queueing the M-step
        # launches while those kernels run
        up = _hip.upload({'off': off, 'scales': torch.as_tensor(
            [datasize / float(T) for T in lengths], dtype=torch.float64)}, dev)
        return off, up['off'], up['scales']
    statics = statics if statics is not None else ShardStatics()
    statics.bind(lengths)
    skey = ('mixture', len(lengths), float(datasize), str(dev))
    off, off_dev, scales = statics.entry(skey, 'offsets', offsets_and_scales)
    lab_dev = None if labels is None else \
        _hip.on_device(torch.as_tensor(labels)).to(torch.int64).contiguous()
    if lab_dev is not None and model.nested:
        # labels name the outer components: M mixtures of their leaves, one-hot state
        # responsibilities (Mixture._nested_expected_log_likelihood)
        M = len(model.modelset)
        lw_sets = model.modelset.leaf_log_weights()
    for run in _sub_batches(lengths, K * X.element_size(), max_frames):
        done = _throttle()
        f0, f1 = int(off[run[0]]), int(off[run[-1] + 1])
        stats = FrameStats(X[f0:f1], cov)
        lab = None if lab_dev is None else lab_dev[f0:f1]
        wide = kernels.wide_mixture_split(stats, K, cov) if lab is None else None
        seg = off_dev[run[0]:run[-1] + 2] - f0
        if lab is not None and model.nested:
            set_norm, resps = kernels.mixtureset_estep(stats, exp_T, lw_sets, M, K // M, cov)
            onehot = torch.zeros_like(set_norm).scatter_(1, lab.view(-1, 1), 1.)
            hk.segment_sum(kernels.rowdot(set_norm, onehot), seg, len(run),
                           out=utt_llh[run[0]:run[-1] + 1])
            kernels.normal_accumulate(stats, resps, onehot, M, K // M, cov, acc=acc)
            done.record()
            continue
        if lab is None and kernels.packed_path_ok(stats, K, cov):
            # responsibilities go to the accumulation already split for its fp16 products
            log_norm, resps = kernels.mixture_estep_packed(stats, exp_T, lw, K, cov)
        elif wide:
            # K > 256: blocks of components on the mixture-set kernels, two-level softmax
            log_norm, resps = kernels.wide_mixture_estep(stats, exp_T, lw, K, cov, wide)
        else:
            log_norm, resps = kernels.mixtureset_estep(stats, exp_T, lw, 1, K, cov, labels=lab)
        hk.segment_sum(log_norm.view(-1), seg, len(run), out=utt_llh[run[0]:run[-1] + 1])
        kernels.normal_accumulate(stats, resps, None, K, 1, cov, acc=acc)
        done.record()
    value_terms = (scales * utt_llh).sum()
    out = {**model._weights_accumulate(acc), ns.means_precisions: _like(ns.means_precisions, acc)}
    return value_terms, out


def _emission_estep(groups, stats, dtype, for_accumulate=False):
    '''pc_all [T, S_total] + per group what its accumulation needs: the component
    responsibilities [T, S*G] (float32 matrix, or `PackedResps` where
    `kernels.packed_sets_ok`), or -- where the accumulation recomputes them from
    the frames (`kernels.fused_accumulate_ok`) -- the group's log-normalisers.'''
    cols, comps = [], []
    for grp, S, G in groups:
        ns = _normalset(grp)
        gstats = stats.as_cov(ns.cov_type)
        if isinstance(grp, TiedMixtureSet):
            # the pool's K log-likelihoods once, the S columns by `beer_tied_lognorm`
            tied = grp.estep(gstats)
            cols.append(tied[2])
            comps.append(('tied',) + tied)
            continue
        lw = grp.leaf_log_weights() if isinstance(grp, MixtureSet) else None
        fused = for_accumulate and G > 1 and \
            kernels.fused_accumulate_ok(gstats, S, G, ns.cov_type)
        if for_accumulate and G > 1 and not fused and \
                kernels.packed_sets_ok(gstats, S, G, ns.cov_type):
            # full covariance: responsibilities as the accumulation kernel's tiles
            log_norm, packed = kernels.mixtureset_estep_packed(
                gstats, ns.means_precisions.natural_form(), lw, S, G, ns.cov_type)
            cols.append(log_norm)
            comps.append(packed)
            continue
        log_norm, resps = kernels.mixtureset_estep(
            gstats, ns.means_precisions.natural_form(), lw, S, G, ns.cov_type,
            want_resps=for_accumulate and G > 1 and not fused)
        cols.append(log_norm)
        comps.append(('fused', log_norm, lw) if fused else resps)
    pc_all = cols[0] if len(cols) == 1 else torch.cat(cols, dim=-1)
    return pc_all, comps


def _emission_predictive(groups, stats):
    '''pc_all [T, S_total] of posterior-predictive log-densities: the predictive twin of
    `_emission_estep` for the searches (Student-t densities of the Gaussians under the
    logarithm of the MEAN weights; nothing is kept for an accumulation).'''
    cols = []
    for grp, S, G in groups:
        if isinstance(grp, TiedMixtureSet):
            grp.predictive_log_likelihood(stats)            # raises: not supported
        ns = _normalset(grp)
        lmw = grp.leaf_log_mean_weights() if isinstance(grp, MixtureSet) else None
        cols.append(kernels.mixtureset_predictive(
            stats.as_cov(ns.cov_type), ns.means_precisions.posterior.predictive_table(), lmw,
            S, G, ns.cov_type))
    return cols[0] if len(cols) == 1 else torch.cat(cols, dim=-1)


def _hmm_batch(model, X, lengths, datasize, graphs, scale, viterbi, state_paths, max_frames,
               frame_images=None, statics=None, sample=None):
    emissions = model._emissions()
    groups = _groups(emissions)
    S_total = sum(S for _, S, _ in groups)
    dev, dtype = X.device, X.dtype
    free_loop = graphs is None
    accs, tied_counts = [], []
    for grp, S, G in groups:
        ns = _normalset(grp)
        Q = FrameStats(X[:1], ns.cov_type).shape[1]
        accs.append(torch.zeros(_n_gaussians(grp, S, G), Q, dtype=torch.float64, device=dev))
        # a tied group's weight statistics do not follow from its Gaussians': [S, K] of their own
        tied_counts.append(torch.zeros(S, G, dtype=torch.float64, device=dev)
                      if isinstance(grp, TiedMixtureSet) else None)
    nutt = len(lengths)
    utt_llh = torch.zeros(nutt, dtype=torch.float64, device=dev)

    def offsets_and_scales():
        off = torch.zeros(nutt + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)
        return off, _hip.to_device(torch.as_tensor([datasize / float(T) for T in lengths],
                                                   dtype=torch.float64), dev)
    statics = statics if statics is not None else ShardStatics()
    statics.bind(lengths)
    skey = ('hmm', nutt, float(datasize), str(dev))
    off, scales = statics.entry(skey, 'offsets', offsets_and_scales)
    xi_tot = g0_tot = flow_tot = None
    # learned transition probabilities (HMM.transitions): their counts come out of the
    # forward-backward launches, summed over the sub-batches in arc / state order
    learned = model.transitions is not None
    if learned and not free_loop:
        # bound alignment graphs only (`HMM.bind_alignment_graphs`): E[ln a] on every arc of
        # their image before the first recursion, counts by category out of the launches
        model._bound_set(graphs).refresh(dtype)
    tcounts_tot = None
    # explicit durations (HMM.durations): their own forward-backward over (state, duration)
    durations = model.durations is not None
    if durations and (viterbi or state_paths is not None or sample is not None):
        model._refuse_durations('viterbi=, state_paths= or sample= training')
    dur_tot = ent_tot = None
    bigram = free_loop and isinstance(model, BigramPhoneLoop)
    counts_tot = None
    max_S = model.graph.n_states if free_loop else max(g.n_states for g in graphs)
    # scratch per frame: the responsibilities of the groups whose accumulation does
    # not recompute them, per-state likelihoods / posteriors, the trellis
    # (a tied group: the pool's log-likelihoods and responsibilities, 2 K)
    K_scratch = sum(2 * G if isinstance(grp, TiedMixtureSet) else S * G
                    for grp, S, G in groups
                    if isinstance(grp, TiedMixtureSet) or (G > 1 and not kernels.fused_accumulate_ok(
                        FrameStats(X, _normalset(grp).cov_type), S, G, _normalset(grp).cov_type)))
    bpf = (K_scratch + 2 * S_total) * X.element_size() + max_S * (3 * X.element_size() + 8)
    if sample is not None:
        bpf += 16                                 # the uniform and the drawn state of a frame
    if durations:
        bpf += 16 * max_S + 16                    # the beg / end trellises and two offsets a frame
    if bigram:
        model.declare_block()
        bpf += 16 * len(model.start_pdf)          # the u / v rows the bigram counts come from
    if frame_images is None or not frame_images.covers(X):
        # frame fragment images built per sub-batch and freed with it (the caller keeps none)
        bpf += max((_hip.lib().beer_frame_image_bytes(
            _hip.COV_CODE[_normalset(grp).cov_type], 1 << 20, X.shape[1]) >> 20)
            for grp, _, _ in groups) if X.dtype == torch.float32 else 0
    runs = statics.entry(skey, ('runs', bpf, max_frames), lambda: [
        (run, int(off[run[0]]), int(off[run[-1] + 1]), [lengths[u] for u in run])
        for run in _sub_batches(lengths, bpf, max_frames)])
    for run_index, (run, f0, f1, run_lengths) in enumerate(runs):
        done = _throttle()
        # the emission E-step is queued first: building the batch descriptor (host
        # work + one asynchronous copy from pinned memory) overlaps with it
        stats = FrameStats(X[f0:f1], _normalset(groups[0][0]).cov_type, images=frame_images)
        pc_all, comps = _emission_estep(groups, stats, dtype, for_accumulate=True)
        if free_loop:
            batch = _cached_batch(model.graph, run_lengths, dtype)
        else:
            def images_of(uniq):
                """What a cached descriptor's struct pointers point into: one blob per GraphSet
                (alignment graphs compiled together share it), the memoised device image of every
                other graph (rebuilt -- a NEW object -- when its tensors are replaced or rewritten)."""
                sets, out = {}, []
                for g in uniq:
                    owner = getattr(g, '_set', None)
                    if owner is None:
                        out.append(g.device_graph(dtype))
                    elif id(owner) not in sets:
                        sets[id(owner)] = True
                        out.append(owner.device_image(dtype)[0])
                return out

            def make_batch():
                uniq, ids, seen = [], [], {}
                for u in run:
                    g = graphs[u]
                    if id(g) not in seen:
                        seen[id(g)] = len(uniq)
                        uniq.append(g)
                    ids.append(seen[id(g)])
                return hk.HmmBatch(uniq, ids, run_lengths, dtype), graphs, uniq, images_of(uniq)
            # (the descriptor of a run's alignment graphs -- thousands of graph structs, one
            # upload -- is the caller's to keep with the shard.  Its key names everything the cut
            # into runs depends on (bytes per frame, max_frames) and the list of graphs (identity,
            # length, the run's first and last graph); a hit is still checked against the device
            # images its struct pointers were taken from)
            bkey = ('batch', run_index, bpf, max_frames, id(graphs), len(graphs),
                    id(graphs[run[0]]), id(graphs[run[-1]]), str(dtype))
            batch, _, uniq, images = statics.entry(skey, bkey, make_batch)
            if not all(a is b for a, b in zip(images, images_of(uniq))):
                statics.items.pop(bkey)
                batch, _, uniq, images = statics.entry(skey, bkey, make_batch)
        hard = viterbi or state_paths is not None or sample is not None
        if durations:
            # gather, forward-backward over (state, duration), scatter; the counts are summed
            # over the sub-batches
            pc_llhs = hk.gather(batch, pc_all, scale)
            gamma, _, dc, entry, g0 = hk.duration_forward_backward(
                batch, pc_llhs, *model._duration_tables())
            sr, _ = hk.scatter(batch, pc_llhs, gamma, S_total, scale, want_exp_llh=False,
                               utt_llh=utt_llh[run[0]:run[-1] + 1])
            dur_tot = dc if dur_tot is None else dur_tot + dc
            if free_loop:
                ent_tot = entry if ent_tot is None else ent_tot + entry
                g0_tot = g0 if g0_tot is None else g0_tot + g0
            _accumulate_emissions(groups, comps, accs, sr, stats, tied_counts)
            done.record()
            continue
        if bigram and not hard:
            # the fused bigram kernel (the general path when the block does not qualify)
            sr, counts = hk.posteriors_bigram(batch, pc_all, scale,
                                              utt_llh=utt_llh[run[0]:run[-1] + 1])
            counts_tot = counts if counts_tot is None else counts_tot + counts
            _accumulate_emissions(groups, comps, accs, sr, stats, tied_counts)
            done.record()
            continue
        # phone counts come from the flows through the loop's hub (the eliminated
        # pivot); a loop whose end -> start arcs stayed ordinary arcs needs xi
        need_counts = free_loop and isinstance(model, PhoneLoop)
        hubbed = need_counts and getattr(getattr(batch.dgraphs[0], 'lowdeg', None), 'n_hubs', 0) >= 1
        if learned and not hard and hk.fused_ok(batch) and (hubbed or not need_counts):
            # the same launch with the transition counts
            sr, g0, flow, tc = hk.posteriors_fused(batch, pc_all, scale, want_counts=need_counts,
                                                   utt_llh=utt_llh[run[0]:run[-1] + 1],
                                                   want_transitions=True)
            xi = None
        elif learned and not hard:
            # the one-wave kernels' counts, or -- graphs beyond them -- the general kernel's
            # dense xi (hub arcs in the matrix) and the last frames' posteriors
            pc_llhs = hk.gather(batch, pc_all, scale)
            gamma, g0, flow, xi, tc = hk.forward_backward_counts(batch, pc_llhs)
            sr, _ = hk.scatter(batch, pc_llhs, gamma, S_total, scale, want_exp_llh=False,
                               utt_llh=utt_llh[run[0]:run[-1] + 1])
        elif not hard and hk.fused_ok(batch) and (hubbed or not need_counts):
            # gather + forward-backward + scatter in one launch, one wave per utterance
            sr, g0, flow = hk.posteriors_fused(batch, pc_all, scale, want_counts=need_counts,
                                               utt_llh=utt_llh[run[0]:run[-1] + 1])
            xi = None
        else:
            pc_llhs = hk.gather(batch, pc_all, scale)
            if hard:
                if sample is not None:
                    # a path drawn from the posterior (forward filtering, backward sampling)
                    path = hk.sample_paths(batch, pc_llhs, None if sample is True
                                           else sample.reshape(1, -1)[:, f0:f1])[0]
                elif state_paths is None:
                    path = hk.viterbi(batch, pc_llhs)
                else:
                    path = torch.cat([torch.as_tensor(state_paths[u]).reshape(-1) for u in run])
                gamma, xi, g0 = hk.path_posteriors(batch, path, want_xi=free_loop)
                flow = None
                if learned:
                    tc = hk.path_counts(batch, path, xi)
            else:
                gamma, xi, g0, _, flow = hk.forward_backward(batch, pc_llhs, want_xi=free_loop)
            sr, _ = hk.scatter(batch, pc_llhs, gamma, S_total, scale, want_exp_llh=False,
                               utt_llh=utt_llh[run[0]:run[-1] + 1])
        if learned:
            tc = model.transition_counts(batch.dgraphs[0], tc)
            tcounts_tot = tc if tcounts_tot is None else tcounts_tot + tc
        if free_loop:
            if xi is not None:
                xi_tot = xi if xi_tot is None else xi_tot + xi
            if g0 is not None:
                g0_tot = g0 if g0_tot is None else g0_tot + g0
            if flow is not None:
                flow_tot = flow if flow_tot is None else flow_tot + flow
        _accumulate_emissions(groups, comps, accs, sr, stats, tied_counts)
        done.record()
    value_terms = (scales * utt_llh).sum()
    out = {}
    for (grp, S, G), acc, cnt in zip(groups, accs, tied_counts):
        ns = _normalset(grp)
        out[ns.means_precisions] = _like(ns.means_precisions, acc)
        if isinstance(grp, MixtureSet):
            out.update(grp.weights_accumulate(acc))
        elif isinstance(grp, TiedMixtureSet):
            out.update(grp.weights_accumulate(cnt))
    if learned:
        out.update(model.transitions.accumulate_counts(tcounts_tot))
    if durations:
        out.update(model.durations.accumulate_counts(dur_tot))
    if isinstance(model, BigramPhoneLoop):
        if bigram and counts_tot is None and xi_tot is not None:       # (Viterbi training)
            counts_tot = model.bigram_counts(xi_tot)
        # (alignment graphs: zero counts -- INTEGRATION.md)
        out.update(model.weights_accumulate(counts_tot if bigram else None))
    if isinstance(model, PhoneLoop):
        wparam = model.categorical.mean_field_factorization()[0][0]
        ref = wparam.stats
        if free_loop:
            if durations:
                # a phone is counted where a segment of its start state begins
                _, starts = model._index_tensors(g0_tot.device)
                counts = g0_tot[starts] + ent_tot[starts]
            else:
                counts = model.phone_counts(xi_tot, g0_tot, flow_tot)
            counts = counts.to(dtype=ref.dtype, device=ref.device)
            # per-utterance `sufficient_statistics` (last <- sum) then sum over
            # utterances == the same map applied to the summed counts.
            cstats = model.categorical.sufficient_statistics(counts.view(1, -1))
            out.update(model.categorical.accumulate(cstats))
        else:
            fake = torch.zeros(len(model.start_pdf), dtype=ref.dtype, device=ref.device)
            out.update(model.categorical.accumulate(fake[None, :]))
    return value_terms, out


def _accumulate_emissions(groups, comps, accs, sr, stats, counts=None):
    '''The emissions' statistics of a sub-batch from its posteriors at the pdf ids (`counts`:
    per group, the [S, K] weight counts of a tied one).'''
    first = 0
    for n, ((grp, S, G), comp, acc) in enumerate(zip(groups, comps, accs)):
        ns = _normalset(grp)
        sr_g = sr if len(groups) == 1 else sr[:, first:first + S].contiguous()
        first += S
        gstats = stats.as_cov(ns.cov_type)
        if isinstance(grp, TiedMixtureSet):
            # pool responsibilities [T, K] + weight counts, then the pool as K Gaussians
            r, _ = kernels.tied_accumulate(*comp[1:], sr_g, counts=counts[n])
            kernels.normal_accumulate(gstats, r, None, G, 1, ns.cov_type, acc=acc)
        elif G == 1:
            kernels.normal_accumulate(gstats, sr_g, None, S, 1, ns.cov_type, acc=acc)
        elif isinstance(comp, tuple):
            # responsibilities recomputed inside the accumulation: no [T, K] matrix
            kernels.mixtureset_accumulate_fused(
                gstats, ns.means_precisions.natural_form(), comp[2], comp[1], sr_g, S, G,
                ns.cov_type, acc=acc)
        else:
            kernels.normal_accumulate(gstats, comp, sr_g, S, G, ns.cov_type, acc=acc)


def _vae_batch(model, X, lengths, datasize, nsamples, llh_weight, kl_weight):
    '''One minibatch of utterances through a VAE: the encoder / decoder see
    the packed frames, an HMM prior sees them as a ragged batch.  The value
    keeps its autograd graph (`elbo.backward()` reaches the networks).'''
    kwargs = {'utt_lengths': lengths} if isinstance(model.prior, HMM) else {}
    broadcast, model.reference_broadcast = model.reference_broadcast, False
    try:
        per_frame = model.expected_log_likelihood(X, nsamples=nsamples, llh_weight=llh_weight,
                                                  kl_weight=kl_weight, **kwargs)
    finally:
        model.reference_broadcast = broadcast
    # frame weights datasize / T_u (times T_u with the reference's [T, T] quirk)
    w = [float(datasize) if broadcast else datasize / float(T) for T in lengths]
    weights = torch.repeat_interleave(
        torch.as_tensor(w, dtype=torch.float64, device=per_frame.device),
        torch.as_tensor(lengths, device=per_frame.device))
    value_terms = (weights * per_frame.to(torch.float64)).sum()
    return value_terms, model.accumulate(None)


def accumulate_elbo(model, utterances, datasize=-1, inference_graphs=None, scale=1.,
                    viterbi=False, state_paths=None, labels=None, max_frames=1 << 24,
                    nsamples=1, llh_weight=1., kl_weight=1., frame_images=None, statics=None,
                    sample=False):
    '''ELBO + accumulated statistics of a shard of utterances, identical to the
    sum of per-utterance `evidence_lower_bound(model, utt, datasize=datasize,
    inference_graph=..., scale=..., viterbi=...)` calls.

    Args:
        model: `Mixture` (nested ones included), `HMM` or `PhoneLoop`.
        utterances: list of [T_u, D] tensors, or `(X_packed, lengths)`.
        datasize: frames in the whole training set (<= 0: this shard).
        inference_graphs: optional list of per-utterance `CompiledGraph`
            (alignment graphs); None = the model's own graph.
        scale: acoustic scale (HMM only).
        viterbi / state_paths: hard-alignment training branches (HMM only).
        sample: True, or a float64 tensor of one uniform in [0, 1) per packed frame (HMM
            only): every utterance is trained on a state path drawn from its posterior
            (`hk.sample_paths`), through the branch `state_paths` takes.
        labels: optional int64 [sum T_u] component labels (Mixture only; the outer
            components of a nested one).
        nsamples, llh_weight, kl_weight: `VAE.expected_log_likelihood`
            arguments (VAE only; the batch is one minibatch, its value keeps
            the autograd graph of the networks).
        frame_images: optional `FrameImages` of the packed frames (HMM only; the
            caller's, kept across iterations over the same shard).  Without it the
            images of a sub-batch live for this call only.
        statics: optional `ShardStatics` (Mixture, HMM): what depends on the utterance
            lengths and `datasize` only, kept by the caller across iterations.
    '''
    if sample is not None and sample is not False:
        # (refused on the host, before the frames go to the device)
        packed = isinstance(utterances, tuple) and len(utterances) == 2 and \
            isinstance(utterances[0], torch.Tensor)
        if not packed:
            utterances = list(utterances)
        sample = hk.check_sample(sample, sum(int(n) for n in utterances[1]) if packed
                                 else sum(len(u) for u in utterances), viterbi, state_paths)
        if not isinstance(model, HMM):
            raise ValueError('sample: HMM models only')
    else:
        sample = None
    X, lengths = pack_utterances(utterances)
    if any(T <= 0 for T in lengths):
        raise ValueError('empty utterance in the batch')
    total = sum(lengths)
    if datasize <= 0:
        datasize = total
    if len(lengths) == 0:
        return EvidenceLowerBoundInstance(0., {}, [], 0, datasize)
    kl, kl_done = _kl_beside_the_estep(model, X.device)
    if isinstance(model, Mixture):
        value_terms, acc = _mixture_batch(model, X, lengths, datasize, labels, max_frames, statics)
    elif isinstance(model, HMM):
        value_terms, acc = _hmm_batch(model, X, lengths, datasize, inference_graphs, scale,
                                      viterbi, state_paths, max_frames, frame_images, statics,
                                      sample)
    elif isinstance(model, VAE):
        value_terms, acc = _vae_batch(model, X, lengths, datasize, nsamples, llh_weight,
                                      kl_weight)
    else:
        raise NotImplementedError(f'no batched E-step for {type(model).__name__}')
    model.clear_cache()
    if kl_done is not None:
        torch.cuda.current_stream(X.device).wait_event(kl_done)
    return _finish(model, value_terms, kl, len(lengths), acc, datasize, total)


def _no_durations(model, what):
    'NotImplementedError for the searches explicit durations (HMM.durations) do not cover.'
    if getattr(model, 'durations', None) is not None:
        model._refuse_durations(what)


def _shard_args(what, utterances, inference_graphs):
    '''The utterances of a shard as `pack_utterances` takes them -- a packed (X, lengths) pair as
    it is, anything else as a list -- once there is one inference graph per utterance (ValueError
    if not).'''
    packed = isinstance(utterances, tuple) and len(utterances) == 2 and \
        isinstance(utterances[0], torch.Tensor)
    if not packed:
        utterances = list(utterances)
    if inference_graphs is not None:
        nutt = len(utterances[1]) if packed else len(utterances)
        if len(inference_graphs) != nutt:
            raise ValueError(f'{what}: {len(inference_graphs)} inference graphs for {nutt} '
                             'utterances')
    return utterances


def _unit_shard(what, model):
    '''(n_units, categories) of a phone loop, ValueError for a model without units:
    `categories(batch)` are the unit-start categories of a sub-batch's distinct graphs, (one
    arc_cat per graph, one init_cat per graph), every graph's built once for as long as the
    caller keeps the function.'''
    if not hasattr(model, 'start_pdf'):
        raise ValueError(f'{what}: a phone loop (a model with units), not '
                         f'{type(model).__name__}')
    cats = {}

    def categories(batch):
        for graph in batch.distinct_graphs:
            if id(graph) not in cats:
                cats[id(graph)] = unit_start_categories(graph, model.start_pdf, model.end_pdf)
        pairs = [cats[id(graph)] for graph in batch.distinct_graphs]
        return [p[0] for p in pairs], [p[1] for p in pairs]

    return len(model.start_pdf), categories


def _split_segments(batch, run_lengths, start, end, unit, value):
    '''The segments of a sub-batch, sorted by start frame, as one (start, end, unit, value) per
    utterance, the frames counted from the utterance's first.'''
    first = batch.bufs['frame_off']
    utt = torch.searchsorted(first[1:].contiguous(), start, right=True)
    counts = torch.bincount(utt, minlength=len(run_lengths)).tolist()
    start, end = start - first[utt], end - first[utt]
    return list(zip(*(torch.split(v, counts) for v in
                      (start.to(torch.int32), end.to(torch.int32), unit, value))))


def _cat_or_empty(parts, *shape):
    'The float64 results of the sub-batches as one tensor; [0, *shape] for a shard of none.'
    return torch.cat(parts) if parts else \
        torch.zeros(0, *shape, dtype=torch.float64, device=_hip.require_device())


def decode_batch(model, utterances, inference_graphs=None, scale=1., max_frames=1 << 20,
                 predictive=False):
    '''Viterbi pdf-id paths for a shard: list of int64 tensors, one per
    utterance (`HMM.decode`, beer/models/hmm.py:105-114, batched).  `predictive`: the
    emissions are the posterior-predictive densities; the arcs of the graphs are used as
    they stand (fixed, or E[ln a] / E[ln pi] where learned), as in `HMM.decode`.'''
    if getattr(model, 'durations', None) is not None:
        # explicit durations: back-pointers (source, duration) in two doubles per state
        tables = model._duration_tables()
        return _paths_batch(model, utterances, inference_graphs, scale, max_frames, 16,
                            lambda batch, pc_llhs: hk.duration_viterbi(
                                batch, pc_llhs, *tables, map_pdf=True)[0],
                            trellis_bytes=16, predictive=predictive)
    return _paths_batch(model, utterances, inference_graphs, scale, max_frames, 0,
                        lambda batch, pc_llhs: hk.viterbi(batch, pc_llhs, map_pdf=True),
                        predictive=predictive)


def sample_paths_batch(model, utterances, inference_graphs=None, scale=1., nsamples=1,
                       generator=None, max_frames=1 << 20):
    '''`nsamples` pdf-id paths per utterance drawn from the posterior: list of int64
    [nsamples, T_u] tensors, one per utterance (`HMM.sample_path`, batched).  `generator`: a
    device torch.Generator for the uniforms.'''
    _no_durations(model, 'sample_paths_batch')
    nsamples = int(nsamples)
    if nsamples < 1:
        raise ValueError('sample_paths_batch: at least one sample')
    # beside decode_batch's scratch: the fp64 trellis in place of the int32 back-pointers, and
    # a uniform and a state per sample and frame
    return _paths_batch(model, utterances, inference_graphs, scale, max_frames, 16 * nsamples,
                        lambda batch, pc_llhs: hk.sample_paths(
                            batch, pc_llhs, nsamples=nsamples, generator=generator, map_pdf=True),
                        trellis_bytes=8)


def decode_nbest_batch(model, utterances, k, inference_graphs=None, scale=1.,
                       max_frames=1 << 20):
    '''The `k` best state paths of every utterance of a shard as pdf ids, and their scores
    (`HMM.decode_nbest`, batched): (list of int64 [k, T_u] tensors, float64 [nutt, k]) on the
    device, best first; ranks without a path of finite score hold -1 and -inf.'''
    k = hk.check_nbest(k, 'decode_nbest_batch')
    _no_durations(model, 'decode_nbest_batch')
    scores = []

    def search(batch, pc_llhs):
        paths, batch_scores = hk.viterbi_nbest(batch, pc_llhs, k, map_pdf=True)
        scores.append(batch_scores)
        return paths

    # decode_batch's scratch with k back-pointers per state, and the k paths of a frame besides
    paths = _paths_batch(model, utterances, inference_graphs, scale, max_frames, 8 * k, search,
                         trellis_bytes=4 * k)
    return paths, torch.cat(scores)


def log_evidence_batch(model, utterances, inference_graphs=None, scale=1., per_frame=False,
                       max_frames=1 << 20, predictive=False):
    '''ln p(x) of every utterance of a shard under the model, summed over all state paths:
    float64 [nutt] on the device (`HMM.log_evidence`, batched); with `per_frame` also a list of
    float64 [T_u] tensors, the terms ln p(x_t | x_0 .. x_{t-1}) of every utterance.
    `predictive`: the emissions are the posterior-predictive densities (held-out likelihood);
    the arcs of the graphs are used as they stand (fixed, or E[ln a] / E[ln pi] where
    learned), as in `HMM.log_evidence`.'''
    utterances = _shard_args('log_evidence_batch', utterances, inference_graphs)
    totals, frames = [], []
    if getattr(model, 'durations', None) is not None:
        if per_frame:
            model._refuse_durations('log_evidence_batch(per_frame=True)')
        tables = model._duration_tables()
        # (a packed shard is still the tuple it came as; anything else is a list by now)
        trellis = 16 + utterances[0].element_size() if isinstance(utterances, tuple) else 24
        for batch, pc_llhs, _ in _search_batches(model, utterances, inference_graphs, scale,
                                                 max_frames, 16, trellis, predictive=predictive):
            totals.append(hk.duration_forward_backward(batch, pc_llhs, *tables,
                                                       want_counts=False)[1])
        return _cat_or_empty(totals)
    # decode_batch's scratch without the trellis; a float64 per frame besides
    for batch, pc_llhs, run_lengths in _search_batches(model, utterances, inference_graphs, scale,
                                                       max_frames, 8 if per_frame else 0, 0,
                                                       predictive=predictive):
        utt, frame = hk.log_evidence(batch, pc_llhs, per_frame=per_frame)
        totals.append(utt)
        if per_frame:
            frames += list(torch.split(frame, run_lengths))
    total = _cat_or_empty(totals)
    return (total, frames) if per_frame else total


def unit_starts_batch(model, utterances, inference_graphs=None, scale=1., max_frames=1 << 20):
    '''Unit-start posteriors of every utterance of a shard: a list of [T_u, n_units] tensors on
    the device, the units in `model.start_pdf` order (`PhoneLoop.unit_starts`, batched).'''
    return _unit_arcs_batch('unit_starts_batch', model, utterances, inference_graphs, scale,
                            max_frames, True)


def unit_counts_batch(model, utterances, inference_graphs=None, scale=1., max_frames=1 << 20):
    '''Expected number of occurrences of every unit in every utterance of a shard: float64
    [nutt, n_units] on the device, the sums over the frames of `unit_starts_batch` -- a soft bag
    of units.'''
    return _unit_arcs_batch('unit_counts_batch', model, utterances, inference_graphs, scale,
                            max_frames, False)


def unit_start_margins_batch(model, utterances, inference_graphs=None, scale=1.,
                             max_frames=1 << 20):
    '''The Viterbi score and the unit-start max-marginals of every utterance of a shard:
    (float64 [nutt], list of [T_u, n_units] tensors) on the device, the units in
    `model.start_pdf` order (`PhoneLoop.unit_start_margins`, batched): entry (t, u) is the score
    lost against the best path by forcing unit u to begin at frame t.'''
    return _unit_arcs_batch('unit_start_margins_batch', model, utterances, inference_graphs,
                            scale, max_frames, True, margins=True)


def unit_segments_batch(model, utterances, beam=10., max_dur=None, inference_graphs=None,
                        scale=1., max_frames=1 << 20):
    '''The Viterbi score and the unit segment lattice of every utterance of a shard: (float64
    [nutt], list of (start, end, unit, margin) per utterance) on the device
    (`PhoneLoop.unit_segments`, batched): the segments within `beam` of the best path, frames
    counted from the utterance's first, sorted by (start, unit, end).  `max_dur` None: the
    length of the longest utterance of a sub-batch, which cuts nothing.'''
    what = 'unit_segments_batch'
    beam, max_dur = hk.check_segments(beam, max_dur, what)
    _no_durations(model, what)
    utterances = _shard_args(what, utterances, inference_graphs)
    n_units, categories = _unit_shard(what, model)
    out, bests = [], []
    # decode_batch's scratch with two fp64 trellises (d and X) in place of the back-pointers; a
    # row of start margins per frame besides (sized for float64).  The segment rows of the
    # entries within the beam come on top: n_entries * max_dur values.
    for batch, pc_llhs, run_lengths in _search_batches(model, utterances, inference_graphs, scale,
                                                       max_frames, 8 + 8 * n_units, 16):
        dur = max(max(run_lengths), 1) if max_dur is None else max_dur
        best, _, frame, unit, seg = hk.segment_margins(batch, pc_llhs, *categories(batch),
                                                       n_units, beam, dur)
        bests.append(best)
        out += _split_segments(batch, run_lengths, *hk.segments_within(frame, unit, seg, beam))
    return _cat_or_empty(bests), out


def _segment_posteriors_batches(what, model, utterances, min_post, max_dur, inference_graphs,
                                scale, max_frames):
    '''(batch, lengths, `hk.segment_posteriors`' outputs) per sub-batch of a shard, under the
    unit-start categories; the arguments are checked before the first sub-batch is built.'''
    _no_durations(model, what)
    utterances = _shard_args(what, utterances, inference_graphs)
    n_units, categories = _unit_shard(what, model)
    # decode_batch's scratch with two fp64 trellises (â and Y) in place of the back-pointers; a
    # normaliser and a row of start posteriors per frame besides (sized for float64).  The
    # segment rows of the entries come on top: n_entries * max_dur values.
    for batch, pc_llhs, run_lengths in _search_batches(model, utterances, inference_graphs, scale,
                                                       max_frames, 8 + 8 * n_units, 16):
        dur = max(max(run_lengths), 1) if max_dur is None else max_dur
        yield batch, run_lengths, hk.segment_posteriors(batch, pc_llhs, *categories(batch),
                                                        n_units, min_post, dur)


def unit_segment_posteriors_batch(model, utterances, min_post=1e-3, max_dur=None,
                                  inference_graphs=None, scale=1., max_frames=1 << 20):
    '''The log-evidence and the unit segments with their posteriors of every utterance of a
    shard: (float64 [nutt], list of (start, end, unit, post) per utterance) on the device
    (`PhoneLoop.unit_segment_posteriors`, batched): the segments whose posterior is >= `min_post`
    (and > 0), frames counted from the utterance's first, sorted by (start, unit, end).  `max_dur`
    None: the length of the longest utterance of a sub-batch, which cuts nothing.'''
    what = 'unit_segment_posteriors_batch'
    min_post, max_dur = hk.check_segment_posteriors(min_post, max_dur, what)
    out, totals = [], []
    for batch, run_lengths, (evidence, _, frame, unit, seg) in _segment_posteriors_batches(
            what, model, utterances, min_post, max_dur, inference_graphs, scale, max_frames):
        totals.append(evidence)
        out += _split_segments(batch, run_lengths, *hk.segments_above(frame, unit, seg, min_post))
    return _cat_or_empty(totals), out


def unit_durations_batch(model, utterances, max_dur, inference_graphs=None, scale=1.,
                         max_frames=1 << 20):
    '''The expected duration histogram of a shard: float64 [n_units, max_dur] on the device, the
    sum over the utterances of `PhoneLoop.unit_durations` -- entry (u, k) is the expected number of
    instances of unit u that last exactly k + 1 frames.  `max_dur` is required: the shard's
    utterances share the histogram's width; instances longer than it are left out.'''
    what = 'unit_durations_batch'
    _, max_dur = hk.check_segment_posteriors(0., max_dur, what)
    if max_dur is None:
        raise ValueError(f'{what}: max_dur is an integer >= 1, not None')
    hist = None
    for _, _, (_, _, _, unit, seg) in _segment_posteriors_batches(
            what, model, utterances, 0., max_dur, inference_graphs, scale, max_frames):
        if hist is None:
            hist = torch.zeros(len(model.start_pdf), max_dur, dtype=torch.float64,
                               device=seg.device)
        hist.index_add_(0, unit.long(), seg.double())
    if hist is None:                                        # (no utterance)
        hist = torch.zeros(len(model.start_pdf), max_dur, dtype=torch.float64,
                           device=_hip.require_device())
    return hist


def _unit_arcs_batch(what, model, utterances, inference_graphs, scale, max_frames, per_frame,
                     margins=False):
    _no_durations(model, what)
    utterances = _shard_args(what, utterances, inference_graphs)
    n_units, categories = _unit_shard(what, model)
    out, bests = [], []
    # decode_batch's scratch with the fp64 trellis in place of the back-pointers; a normaliser
    # and the output row per frame besides (sized for float64)
    row = 8 * n_units if per_frame else 0
    for batch, pc_llhs, run_lengths in _search_batches(model, utterances, inference_graphs, scale,
                                                       max_frames, 8 + row, 8):
        if margins:
            best, _, frame, utt = hk.max_marginals(batch, pc_llhs, *categories(batch), n_units,
                                                   states=False, per_frame=True)
            bests.append(best)
        else:
            frame, utt = hk.arc_posteriors(batch, pc_llhs, *categories(batch), n_units,
                                           per_frame=per_frame, per_utt=not per_frame)
        if per_frame:
            out += list(torch.split(frame, run_lengths))
        else:
            out.append(utt)
    if margins:
        return _cat_or_empty(bests), out
    if per_frame:
        return out
    return _cat_or_empty(out, n_units)


def _paths_batch(model, utterances, inference_graphs, scale, max_frames, extra_bytes, search,
                 trellis_bytes=4, predictive=False):
    '''`search(batch, pc_llhs)` -> paths [..., n_frames] over sub-batches of the shard, split by
    utterance along the last dimension.  Scratch per frame: decode_batch's, with `trellis_bytes`
    per state for the search's own workspace and `extra_bytes` besides.'''
    paths = []
    for batch, pc_llhs, run_lengths in _search_batches(model, utterances, inference_graphs, scale,
                                                       max_frames, extra_bytes, trellis_bytes,
                                                       predictive=predictive):
        paths += list(torch.split(search(batch, pc_llhs), run_lengths, dim=-1))
    return paths


def _search_batches(model, utterances, inference_graphs, scale, max_frames, extra_bytes,
                    trellis_bytes, predictive=False):
    '''The sub-batches of a shard for a search over its utterances: yields (HmmBatch, gathered
    pc_llhs, lengths) per sub-batch.  Scratch per frame: the emissions' E-step, the gathered
    log-likelihoods, `trellis_bytes` per state and `extra_bytes` besides.  `predictive`: the
    emissions' posterior-predictive densities (`_emission_predictive`) in place of the E-step.'''
    X, lengths = pack_utterances(utterances)
    groups = _groups(model._emissions())
    S_total = sum(S for _, S, _ in groups)
    K_max = sum(2 * G if isinstance(grp, TiedMixtureSet) else S * G for grp, S, G in groups)
    off = [0]
    for T in lengths:
        off.append(off[-1] + T)
    max_S = model.graph.n_states if inference_graphs is None \
        else max(g.n_states for g in inference_graphs)
    if inference_graphs is not None and len(inference_graphs) and \
            getattr(getattr(inference_graphs[0], '_set', None), 'is_bound', False):
        # graphs bound to learned transitions: E[ln a] on their arcs before the search
        model._bound_set(inference_graphs).refresh(X.dtype)
    bpf = (K_max + S_total) * X.element_size() + max_S * (X.element_size() + trellis_bytes) + \
        extra_bytes
    for run in _sub_batches(lengths, bpf, max_frames):
        f0, f1 = off[run[0]], off[run[-1] + 1]
        stats = FrameStats(X[f0:f1], _normalset(groups[0][0]).cov_type)
        if predictive:
            pc_all = _emission_predictive(groups, stats)
        else:
            pc_all, _ = _emission_estep(groups, stats, X.dtype)
        run_lengths = [lengths[u] for u in run]
        if inference_graphs is None:
            uniq = [model.graph]
            batch = hk.HmmBatch(uniq, [0] * len(run), run_lengths, X.dtype)
        else:
            uniq, ids, seen = [], [], {}
            for u in run:
                g = inference_graphs[u]
                if id(g) not in seen:
                    seen[id(g)] = len(uniq)
                    uniq.append(g)
                ids.append(seen[id(g)])
            batch = hk.HmmBatch(uniq, ids, run_lengths, X.dtype)
        batch.distinct_graphs = uniq
        yield batch, hk.gather(batch, pc_all, scale), run_lengths
