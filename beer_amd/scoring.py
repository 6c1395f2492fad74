'''Comparing transcriptions: unit sequences of decoded paths, edit distances and token error
rates on the GPU, minimum-Bayes-risk selection among the N best or sampled paths of an
utterance, and the scores of acoustic unit discovery (the recipe's `score_aud`: max-overlap
mapping, normalised mutual information, entropy rate, boundary recall / precision / F-score).

The distances are `beer_edit_distance` (csrc/editdist.hip): integers, exact.  The AUD scores
are host numpy: their inputs are label files.'''

import collections

import numpy as np
import torch

from . import _hip
from . import kernels
from .inference.batch import (_no_durations, _unit_shard, decode_nbest_batch,
                              sample_paths_batch)

__all__ = ['unit_sequences_batch', 'edit_distances', 'token_error_rate', 'closest_error_rate',
           'mbr_decode_batch', 'mbr_select', 'contingency', 'maxoverlap_mapping',
           'normalized_mutual_information', 'entropy_rate', 'boundary_scores', 'TokenErrors',
           'BoundaryScores']


class TokenErrors(collections.namedtuple('TokenErrors', 'errors sub dele ins n_ref n_utts')):
    '''Substitutions, deletions (reference tokens the hypothesis lacks) and insertions summed
    over `n_utts` utterances of `n_ref` reference tokens; `errors` is their sum.'''
    __slots__ = ()

    @property
    def rate(self):
        'The error rate in percent (0 for an empty reference).'
        return 100. * self.errors / self.n_ref if self.n_ref else 0.


BoundaryScores = collections.namedtuple('BoundaryScores',
                                        'recall precision fscore hits n_ref n_hyp')


# ---------------------------------------------------------------------------
# sequences on the device

def _unit_table(model):
    'unit_of_pdf of `beer_unit_sequences`: the index (in `start_pdf` order) of the unit a pdf begins.'
    firsts = [int(pdf) for pdf in model.start_pdf.values()]
    n_pdf = max(firsts + [int(pdf) for pdf in model.end_pdf.values()]) + 1
    table = np.full(n_pdf, -1, dtype=np.int32)
    for unit, pdf in enumerate(firsts):
        table[pdf] = unit
    return torch.from_numpy(table)


def _pack_rows(tensors, dtype):
    '''Tensors of one or two dimensions as one packed tensor of their rows on the device, the
    rows' starts and lengths (host int64), and the number of rows of every tensor (None: it had
    one dimension).'''
    dev = _hip.require_device()
    rows, lens = [], []
    for t in tensors:
        t = torch.as_tensor(t)
        if t.dim() not in (1, 2):
            raise ValueError(f'a sequence or a stack of sequences, not a tensor of shape '
                             f'{tuple(t.shape)}')
        rows.append(None if t.dim() == 1 else t.shape[0])
        lens += [t.shape[-1]] * (1 if t.dim() == 1 else t.shape[0])
    flat = [torch.as_tensor(t).to(dev).to(dtype).reshape(-1) for t in tensors]
    packed = torch.cat(flat) if flat else torch.zeros(0, dtype=dtype, device=dev)
    lens = torch.tensor(lens, dtype=torch.int64)
    start = torch.cumsum(lens, 0) - lens
    return packed, start, lens, rows


def _unit_rows(model, paths, what, per_frame=False):
    '''The kernel's outputs for the rows of `paths` (a list of [T_u] or [N, T_u] pdf-id paths):
    (units, n_units (host), frame units or None, start, lens, rows).  KeyError for a path that
    holds a pdf the units do not have, or that begins inside a unit, as `phones_of_path`.'''
    if not hasattr(model, 'start_pdf'):
        _unit_shard(what, model)
    packed, start, lens, rows = _pack_rows(paths, torch.int64)
    units, n_units, frames = kernels.unit_sequences(packed, start, lens, _unit_table(model),
                                                    per_frame=per_frame)
    n_units = n_units.cpu()
    bad = torch.nonzero(n_units == -2).reshape(-1)
    if bad.numel():
        first = int(packed[int(start[int(bad[0])])])
        raise KeyError(first)
    return units, n_units, frames, start, lens, rows


def _split_rows(values, start, counts, rows):
    'Per input tensor: the slice of `values` of its row, or the list of those of its rows.'
    out, q = [], 0
    for n in rows:
        got = []
        for _ in range(1 if n is None else n):
            c = int(counts[q])
            got.append(None if c < 0 else values[int(start[q]):int(start[q]) + c])
            q += 1
        out.append(got[0] if n is None else got)
    return out


def unit_sequences_batch(model, paths, per_frame=False):
    '''The unit sequences of pdf-id paths (`beer_unit_sequences`): `paths` is a list of [T_u] or
    [N, T_u] int64 tensors, as `decode_batch`, `decode_nbest_batch` and `sample_paths_batch`
    return them; the result has an int32 tensor of unit indices (in `model.start_pdf` order) on
    the device for every [T_u] path, and a list of N of them for every [N, T_u] stack -- None for
    a rank without a path (a row of -1).  `per_frame`: the running unit of every frame instead.
    ValueError for a model without units; KeyError for a path that begins inside a unit.'''
    units, n_units, frames, start, lens, rows = _unit_rows(model, paths, 'unit_sequences_batch',
                                                           per_frame)
    if per_frame:
        return _split_rows(frames, start, torch.where(n_units < 0, n_units, lens.to(n_units.dtype)),
                           rows)
    return _split_rows(units, start, n_units, rows)


def _pack_sequences(seqs):
    flat = [np.asarray(s.cpu() if torch.is_tensor(s) else s).reshape(-1) for s in seqs]
    for s in flat:
        if s.size and not np.issubdtype(s.dtype, np.integer):
            raise ValueError(f'integer sequences, not {s.dtype}')
    lens = np.asarray([len(s) for s in flat], dtype=np.int64)
    packed = np.concatenate(flat).astype(np.int32) if flat and lens.sum() else \
        np.zeros(0, dtype=np.int32)
    return torch.from_numpy(packed), torch.from_numpy(lens)


def edit_distances(refs, hyps, ops=False):
    '''Levenshtein distances of `refs[i]` and `hyps[i]`, two lists of integer sequences (lists,
    arrays or tensors): int32 [n] on the device; with `ops` also int32 [n, 3], the
    (substitutions, deletions, insertions) of the cheapest alignment with the smallest such
    triple -- a deletion is a reference token the hypothesis lacks.'''
    refs, hyps = list(refs), list(hyps)
    if len(refs) != len(hyps):
        raise ValueError(f'edit_distances: {len(refs)} references for {len(hyps)} hypotheses')
    sym, lens = _pack_sequences(refs + hyps)
    n = len(refs)
    index = torch.arange(n, dtype=torch.int32)
    return kernels.edit_distance(sym, torch.cumsum(lens, 0) - lens, lens, index, index + n, ops=ops)


def _errors(moves, lens_ref, n_utts):
    sub, dele, ins = (int(v) for v in moves.sum(0).tolist()) if len(moves) else (0, 0, 0)
    return TokenErrors(sub + dele + ins, sub, dele, ins, int(lens_ref), n_utts)


def token_error_rate(refs, hyps):
    '''`TokenErrors` (errors, sub, dele, ins, n_ref, n_utts) of the hypotheses against the
    references, two lists of integer sequences; `.rate` is the error rate in percent.'''
    refs = list(refs)
    _, moves = edit_distances(refs, hyps, ops=True)
    return _errors(moves.cpu().to(torch.int64), sum(len(r) for r in refs), len(refs))


def closest_error_rate(refs, hyp_lists):
    '''`token_error_rate` with, for every utterance, the hypothesis of its list that is closest
    to the reference (the first of the closest).'''
    refs, hyp_lists = list(refs), [list(h) for h in hyp_lists]
    if len(refs) != len(hyp_lists):
        raise ValueError(f'closest_error_rate: {len(refs)} references for {len(hyp_lists)} lists')
    if any(len(h) == 0 for h in hyp_lists):
        raise ValueError('closest_error_rate: an utterance without a hypothesis')
    owner = [u for u, h in enumerate(hyp_lists) for _ in h]
    dist, moves = edit_distances([refs[u] for u in owner], [s for h in hyp_lists for s in h],
                                 ops=True)
    dist, moves = dist.cpu().numpy(), moves.cpu().to(torch.int64)
    pick, lo = [], 0
    for h in hyp_lists:
        pick.append(lo + int(np.argmin(dist[lo:lo + len(h)])))
        lo += len(h)
    return _errors(moves[pick], sum(len(r) for r in refs), len(refs))


def mbr_decode_batch(model, utterances, nbest=None, nsamples=None, generator=None,
                     inference_graphs=None, scale=1., weight_scale=1., max_frames=1 << 20):
    '''Minimum-Bayes-risk unit sequences of a shard: among the hypotheses of an utterance -- its
    `nbest` best state paths or `nsamples` paths drawn from the posterior (exactly one of the two
    is given) -- the one whose expected edit distance to the others is smallest.
    Returns (units, index, risk): risk [nutt, N] float64 on the device,
    risk[u, i] = sum_j w_j d(i, j) with d the edit distance of the unit sequences, w uniform
    under `nsamples` and proportional to exp(weight_scale * (score_r - score_0)) over the ranks
    that have a path under `nbest` (+inf for a rank without one); index [nutt] int64 the
    smallest index of the smallest risk; units a list of int32 tensors, that hypothesis (None
    for an utterance without any path).  `max_frames`, `scale`, `inference_graphs`, `generator`:
    as `decode_nbest_batch` / `sample_paths_batch`.'''
    if (nbest is None) == (nsamples is None):
        raise ValueError('mbr_decode_batch: exactly one of nbest and nsamples')
    _no_durations(model, 'mbr_decode_batch')
    _unit_shard('mbr_decode_batch', model)
    if nbest is not None:
        paths, scores = decode_nbest_batch(model, utterances, nbest, inference_graphs=inference_graphs,
                                           scale=scale, max_frames=max_frames)
    else:
        paths = sample_paths_batch(model, utterances, inference_graphs=inference_graphs,
                                   scale=scale, nsamples=nsamples, generator=generator,
                                   max_frames=max_frames)
        scores = None
    return mbr_select(model, paths, scores, weight_scale)


def mbr_select(model, paths, scores=None, weight_scale=1.):
    '''`mbr_decode_batch` on hypotheses that exist already: `paths` a list of [N, T_u] pdf-id
    paths, `scores` [nutt, N] their scores (None: uniform weights).'''
    if not hasattr(model, 'start_pdf'):
        _unit_shard('mbr_select', model)
    dev = _hip.require_device()
    nutt = len(paths)
    if nutt == 0:
        return [], torch.zeros(0, dtype=torch.int64, device=dev), \
            torch.zeros(0, 0, dtype=torch.float64, device=dev)
    N = paths[0].shape[0]
    units, n_units, _, start, lens, _ = _unit_rows(model, paths, 'mbr_decode_batch')
    counts = n_units.to(dev).reshape(nutt, N)
    have = counts >= 0
    # the N (N - 1) / 2 pairs i < j of every utterance; a rank without a path is an empty sequence
    i, j = torch.triu_indices(N, N, 1, device=dev)
    base = (torch.arange(nutt, device=dev) * N).unsqueeze(1)
    D = torch.zeros(nutt, N, N, dtype=torch.float64, device=dev)
    if i.numel():
        dist = kernels.edit_distance(units, start, counts.clamp(min=0).reshape(-1),
                                     (base + i).reshape(-1), (base + j).reshape(-1))
        D[:, i, j] = dist.reshape(nutt, -1).to(torch.float64)
        D = D + D.transpose(1, 2)
    if scores is None:
        w = have.to(torch.float64)
    else:
        scores = scores.to(dev)
        rel = torch.where(have, weight_scale * (scores - scores[:, :1]), torch.zeros_like(scores))
        w = torch.where(have, torch.exp(rel), torch.zeros_like(rel))
    w = w / w.sum(1, keepdim=True).clamp(min=1e-300)
    risk = (D * w.unsqueeze(1)).sum(2)
    risk = torch.where(have, risk, torch.full_like(risk, float('inf')))
    lowest = risk == risk.min(1, keepdim=True).values
    ranks = torch.arange(N, device=dev).expand(nutt, N)
    index = torch.where(lowest, ranks, torch.full_like(ranks, N)).min(1).values
    chosen = (torch.arange(nutt) * N + index.cpu()).tolist()
    out = []
    for q in chosen:
        c = int(n_units[q])
        out.append(None if c < 0 else units[int(start[q]):int(start[q]) + c])
    return out, index, risk


# ---------------------------------------------------------------------------
# the scores of acoustic unit discovery (host numpy)

def _flat_labels(labels):
    if isinstance(labels, (list, tuple)) and len(labels) and not np.isscalar(labels[0]):
        labels = np.concatenate([np.asarray(l).reshape(-1) for l in labels])
    labels = np.asarray(labels).reshape(-1)
    if labels.size and (not np.issubdtype(labels.dtype, np.integer) or labels.min() < 0):
        raise ValueError('labels are non-negative integers')
    return labels.astype(np.int64)


def contingency(ref_labels, hyp_labels):
    '''Frame counts int64 [n_hyp, n_ref]: entry (h, r) is the number of frames the hypothesis
    labels h and the reference r.  Both are per-frame label indices, flat or one array per
    utterance.'''
    ref, hyp = _flat_labels(ref_labels), _flat_labels(hyp_labels)
    if ref.size != hyp.size:
        raise ValueError(f'contingency: {ref.size} reference and {hyp.size} hypothesis frames')
    n_ref, n_hyp = (int(v.max()) + 1 if v.size else 0 for v in (ref, hyp))
    counts = np.zeros((n_hyp, n_ref), dtype=np.int64)
    np.add.at(counts, (hyp, ref), 1)
    return counts


def maxoverlap_mapping(counts):
    '''For every hypothesis label the reference label it shares most frames with (int64
    [n_hyp]); the first of several maxima wins.'''
    counts = np.asarray(counts)
    if counts.shape[1] == 0:
        return np.zeros(counts.shape[0], dtype=np.int64)
    return np.argmax(counts, axis=1).astype(np.int64)


def _entropy_bits(p):
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


def normalized_mutual_information(counts):
    '''200 (H_Y - H_{Y|X}) / (H_X + H_Y) in bits, X the hypothesis label of a frame (the rows of
    `counts`) and Y the reference label (the columns), with 0 log 0 = 0; 0 when both entropies
    vanish.'''
    counts = np.asarray(counts, dtype=np.float64)
    total = counts.sum()
    if total <= 0:
        return 0.
    p = counts / total
    h_x, h_y = _entropy_bits(p.sum(1)), _entropy_bits(p.sum(0))
    if h_x + h_y <= 0:
        return 0.
    h_y_given_x = _entropy_bits(p.reshape(-1)) - h_x            # H(X, Y) - H(X)
    return 200. * (h_y - h_y_given_x) / (h_x + h_y)


def _merged(seq):
    seq = np.asarray(seq).reshape(-1)
    return seq[np.concatenate([[True], seq[1:] != seq[:-1]])] if seq.size else seq


def entropy_rate(seqs):
    '''(entropy, perplexity): the unigram entropy in bits of the tokens of the sequences once
    repeats are merged, and 2 ** entropy.'''
    tokens = [_merged(s) for s in seqs]
    tokens = np.concatenate(tokens) if tokens else np.zeros(0, dtype=np.int64)
    if tokens.size == 0:
        return 0., 1.
    _, counts = np.unique(tokens, return_counts=True)
    entropy = _entropy_bits(counts / counts.sum())
    return entropy, 2. ** entropy


def _boundaries(labels):
    labels = np.asarray(labels).reshape(-1)
    return np.nonzero(labels[1:] != labels[:-1])[0] + 1


def boundary_scores(ref, hyp, delta=2):
    '''`BoundaryScores` (recall, precision, fscore in percent; hits, n_ref, n_hyp) of the
    hypothesis boundaries of the utterances against the reference's.  `ref` / `hyp`: one array
    of per-frame labels per utterance.  A boundary is a frame whose label differs from the
    previous frame's.  The hypothesis boundaries are taken in order; each hits the nearest
    reference boundary not yet used (the first of the nearest) if it lies within `delta`
    frames.'''
    ref, hyp = list(ref), list(hyp)
    if len(ref) != len(hyp):
        raise ValueError(f'boundary_scores: {len(ref)} reference and {len(hyp)} hypothesis '
                         'utterances')
    hits = n_ref = n_hyp = 0
    for r, h in zip(ref, hyp):
        rb, hb = _boundaries(r), _boundaries(h)
        n_ref, n_hyp = n_ref + len(rb), n_hyp + len(hb)
        free = np.ones(len(rb), dtype=bool)
        for b in hb:
            if not free.any():
                break
            gap = np.where(free, np.abs(rb - b), np.iinfo(np.int64).max)
            k = int(np.argmin(gap))
            if gap[k] <= delta:
                hits += 1
                free[k] = False
    recall = hits / n_ref if n_ref else 0.
    precision = hits / n_hyp if n_hyp else 0.
    fscore = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.
    return BoundaryScores(100. * recall, 100. * precision, 100. * fscore, hits, n_ref, n_hyp)
