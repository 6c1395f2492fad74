"""Python faces of the HMM entry points of include/beer_hip.h: ragged-batch
descriptors, pdf-id gather / scatter, forward-backward, Viterbi."""

import ctypes
import threading

import numpy as np
import torch

from . import _hip

__all__ = ['HmmBatch', 'gather', 'forward_backward', 'viterbi', 'path_posteriors',
           'scatter', 'gather_columns', 'scatter_columns', 'segment_sum', 'fused_ok',
           'posteriors_fused', 'trans_posteriors_dense', 'counting_log_space', 'bigram_ok',
           'posteriors_bigram', 'lowdeg_arcs', 'forward_backward_counts', 'path_counts',
           'last_frame_sum', 'sample_paths', 'sample_route', 'check_sample', 'sample_uniforms',
           'log_evidence', 'evidence_route', 'arc_posteriors', 'arcs_route',
           'check_arc_categories', 'viterbi_nbest', 'nbest_route', 'check_nbest',
           'max_marginals', 'maxmarg_route', 'SegmentMap', 'segment_map', 'segments_route',
           'segment_margins', 'segments_within', 'check_segments', 'segposts_route',
           'segment_posteriors', 'segments_above', 'check_segment_posteriors',
           'check_durations', 'duration_route', 'duration_forward_backward', 'duration_viterbi',
           'duration_arcs_route', 'duration_arc_posteriors']


class HmmBatch:
    '''beer_batch descriptor: `graphs` are the distinct CompiledGraph objects
    of the batch, `graph_ids[u]` the one utterance u uses, `lengths[u]` its
    number of frames.  Packed per-state buffers hold utterance u at element
    offset `llh_off[u]` as a row-major [T_u, S_u] block.'''

    def __init__(self, graphs, graph_ids, lengths, dtype, with_pdf_ids=True, lowdeg=True):
        dev = _hip.require_device()
        self.dtype, self.device = dtype, dev
        self.nutt = len(lengths)
        lengths_t = torch.as_tensor(lengths, dtype=torch.int64)
        gid_t = torch.as_tensor(graph_ids, dtype=torch.int64)
        self.source_graphs = list(graphs)
        gset = getattr(graphs[0], '_set', None) if len(graphs) > 1 else None
        if gset is not None and all(getattr(g, '_set', None) is gset for g in graphs):
            # graphs of one natively compiled GraphSet: their descriptors are rows
            # of one array -- slice it with numpy instead of building thousands of
            # Python objects per batch (each batch used to cost a 40 ms gen-2
            # garbage collection at 3000 utterances)
            idx = np.fromiter((g._i for g in graphs), dtype=np.int64, count=len(graphs))
            _, structs = gset.device_image(dtype)
            size = ctypes.sizeof(_hip.Graph)
            raw = np.frombuffer(structs, dtype=np.uint8).reshape(-1, size)[idx]
            head = np.ascontiguousarray(raw[:, :16]).view(np.int32)      # n_states, n_arcs, segs
            has_lowdeg = np.ascontiguousarray(raw[:, size - 8:]).view(np.int64).reshape(-1) != 0
            n_states = head[:, 0].tolist()
            n_arcs = head[:, 1].tolist()
            max_arcs = int(head[:, 1].max())
            max_segs = int(head[:, 2:4].max())
            all_lowdeg = bool(has_lowdeg.all())
            graph_bytes = torch.from_numpy(np.ascontiguousarray(raw).reshape(-1))
            so = gset.state_off
            counts = (so[idx + 1] - so[idx]).astype(np.int64)
            pdf_off = np.concatenate([[0], np.cumsum(counts)])
            if with_pdf_ids:
                start = np.repeat(so[idx] - pdf_off[:-1], counts)
                pdf_ids = gset.pdf_ids[start + np.arange(pdf_off[-1])]
            else:
                pdf_ids = (np.arange(pdf_off[-1]) - np.repeat(pdf_off[:-1], counts)).astype(np.int32)
            self.dgraphs = [gset]                               # keeps the image alive
            ld_info = (gset.max_degree, 0, 0)                   # alignment chains: no hub
        else:
            self.dgraphs = [g.device_graph(dtype) for g in graphs]
            n_states = [dg.n_states for dg in self.dgraphs]
            parts = [np.asarray(g.pdf_id_mapping, dtype=np.int32)
                     if (with_pdf_ids and g.pdf_id_mapping is not None)
                     else np.arange(g.n_states, dtype=np.int32) for g in graphs]
            pdf_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]) if parts else [0]
            pdf_ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
            arr = (_hip.Graph * len(graphs))(*[dg.struct for dg in self.dgraphs])
            graph_bytes = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            n_arcs = [dg.n_arcs for dg in self.dgraphs]
            max_arcs = max(n_arcs + [1])
            max_segs = max([max(dg.n_in_seg, dg.n_out_seg) for dg in self.dgraphs] + [1])
            all_lowdeg = bool(self.dgraphs) and \
                all(getattr(dg, 'lowdeg', None) is not None for dg in self.dgraphs)
            infos = [getattr(dg, 'lowdeg_info', (0, 0, 0)) for dg in self.dgraphs] or [(0, 0, 0)]
            known = all(i[0] > 0 for i in infos)
            ld_info = tuple(max(i[k] for i in infos) if known else 0 for k in range(3))
        states_t = torch.as_tensor(n_states, dtype=torch.int64)[gid_t] \
            if self.nutt else torch.zeros(0, dtype=torch.int64)
        frame_off = torch.zeros(self.nutt + 1, dtype=torch.int64)
        frame_off[1:] = torch.cumsum(lengths_t, 0)
        sizes = lengths_t * states_t
        llh_off = torch.zeros(self.nutt + 1, dtype=torch.int64)
        llh_off[1:] = torch.cumsum(sizes, 0)
        self.n_frames = int(frame_off[-1])
        self.n_elems = int(llh_off[-1])
        self.frame_off_h, self.llh_off_h = frame_off, llh_off
        self.n_states = n_states
        self.n_arcs = n_arcs                        # arcs of the full CSR of every distinct graph
        self.graph_ids = list(graph_ids)
        # longest utterance first: the waves of a workgroup of the one-wave kernels then
        # finish together, and a launch ends with its shortest utterances
        order = torch.argsort(lengths_t, descending=True, stable=True).to(torch.int32) \
            if self.nutt else torch.zeros(0, dtype=torch.int32)
        # graphs bound to a model's learned transitions (`BoundGraphSet`): the category maps of
        # beer_cat_map, every graph of the batch at its offsets in the set's arrays
        owner = getattr(graphs[0], '_set', None) if len(graphs) else None
        self.bound_set = owner if getattr(owner, 'is_bound', False) and \
            all(getattr(g, '_set', None) is owner for g in graphs) else None
        extra = {}
        if self.bound_set is not None:
            at = np.fromiter((g._i for g in graphs), dtype=np.int64, count=len(graphs))
            extra = dict(cat_arc_off=torch.from_numpy(np.ascontiguousarray(owner.arc_off[at])),
                         cat_state_off=torch.from_numpy(np.ascontiguousarray(owner.state_off[at])))
        self.bufs = _hip.upload(dict(
            frame_off=frame_off, llh_off=llh_off[:-1], graph_id=gid_t.to(torch.int32),
            order=order,
            graphs=graph_bytes,
            pdf_off=torch.as_tensor(np.asarray(pdf_off), dtype=torch.int32),
            pdf_ids=torch.as_tensor(pdf_ids, dtype=torch.int32), **extra), dev)
        b = self.bufs
        self.struct = _hip.Batch(
            self.nutt, max(n_states) if n_states else 1, max(max_arcs, 1), max(max_segs, 1),
            1 if (lowdeg and all_lowdeg) else 0, len(graphs),
            b['frame_off'].data_ptr(), b['llh_off'].data_ptr(), b['graph_id'].data_ptr(),
            b['graphs'].data_ptr(), b['pdf_off'].data_ptr(), b['pdf_ids'].data_ptr(),
            *(ld_info if all_lowdeg else (0, 0, 0)), 0, b['order'].data_ptr())
        self.shared_graph = len(graphs) == 1
        if self.bound_set is not None:
            arc_cat, last_cat = owner.cat_maps()
            self.cat_map = _hip.CatMap(arc_cat.data_ptr(), last_cat.data_ptr(),
                                       b['cat_arc_off'].data_ptr(), b['cat_state_off'].data_ptr())
        self._pdf_ids_h, self._pdf_off_h = np.asarray(pdf_ids), np.asarray(pdf_off)
        self._profile = {}

    def pdf_ids_profile(self, S_total):
        '''(some graph repeats a pdf id, every graph's ids are exactly 0 .. S_total-1):
        what decides between atomic adds, plain stores into a zero-filled array and
        plain stores into an uninitialised one when posteriors go back to pdf ids.'''
        hit = self._profile.get(S_total)
        if hit is None:
            ids, off = self._pdf_ids_h, self._pdf_off_h
            n = len(off) - 1
            counts = np.diff(off)
            gidx = np.repeat(np.arange(n), counts)
            key = gidx.astype(np.int64) * (int(ids.max()) + 1 if len(ids) else 1) + ids
            distinct = len(np.unique(key)) == len(key)
            covers = distinct and bool((counts == S_total).all()) and \
                (len(ids) == 0 or int(ids.max()) < S_total)
            hit = self._profile[S_total] = (not distinct, covers)
        return hit

    def ref(self):
        return ctypes.byref(self.struct)


def gather(batch, pc_all, scale=1.):
    'pc_llhs (packed, [n_elems]) = scale * pc_all[frame, pdf_id].'
    pc_all = _hip.on_device(pc_all, batch.dtype)
    out = torch.empty(batch.n_elems, dtype=batch.dtype, device=batch.device)
    _hip.call('beer_hmm_gather', _hip.dtype_code(batch.dtype), batch.ref(), pc_all.shape[1],
              _hip.ptr(pc_all), float(scale), _hip.ptr(out))
    return out


def _route(dtype, desc, want_xi, have_hub_flow):
    'beer_hmm_fb_route: the kernel family (and its launch shape) the C entry points pick.'
    return _hip.lib().beer_hmm_fb_route(_hip.dtype_code(dtype), ctypes.byref(desc),
                                        int(want_xi), int(have_hub_flow))


def _route_or_refuse(query, batch, args, refusal):
    '''What the C route query `query` answers for the batch and the scalars `args`: the form the
    family's kernels take.  HipInvalid with the text `refusal()` builds where C refuses.'''
    route = getattr(_hip.lib(), query)(_hip.dtype_code(batch.dtype), batch.ref(), *args)
    if route == _hip.EINVAL:
        raise _hip.HipInvalid(refusal())
    return route


def _workspace(batch, desc=None, want_xi=False, packed=True):
    '''(packed gamma or None, alpha, hub_ws).  `hub_ws`: hub values per frame, or -- `desc` may take
    the general kernel with arc lists too long for LDS -- that kernel's per-arc scratch.'''
    dev, f64 = batch.device, torch.float64
    n_ws = 0 if desc is None else _hip.lib().beer_hmm_fb_scratch_doubles(
        _hip.dtype_code(batch.dtype), ctypes.byref(desc), int(want_xi))
    return (torch.empty(batch.n_elems, dtype=batch.dtype, device=dev) if packed else None,
            torch.empty(batch.n_elems, dtype=f64, device=dev),
            torch.empty(max(_hip.MAX_HUBS * batch.n_frames, n_ws), dtype=f64, device=dev))


def _note_alpha(batch, alpha, route, hub_ws):
    '''What a call on `route` left in `alpha` (for `trans_posteriors_dense`; None: the fused launch
    keeps nothing): the one-wave kernels SCALED PROBABILITIES, the others logarithms.'''
    batch.last_alpha = alpha
    batch.last_alpha_is_log = _hip.fb_family(route) != _hip.FB_WAVE
    if not batch.last_alpha_is_log:
        counting_log_space.note(batch, hub_ws)


def forward_backward(batch, pc_llhs, want_xi=False, want_lognorm=False, dense_xi=False):
    '''(gamma packed, xi_sum [S,S] fp64 or None, gamma0_sum [S] fp64 or None,
    lognorm_mean [nutt] or None, hub_flow [S] fp64 or None).  xi / gamma0 need
    a batch sharing one graph.  When the graph carries a hub (phone loop) the
    transition posteriors through it come back summed over its sources in
    `hub_flow`; `dense_xi=True` forces the general kernel and a complete
    [S, S] matrix.'''
    dt, dev = batch.dtype, batch.device
    desc = batch.struct
    if dense_xi:
        # the general kernel: a complete [S, S] matrix and log-space forward values in `alpha`.
        # On a copy: the batch's descriptor is shared with later calls and other host threads.
        desc = _hip.Batch.from_buffer_copy(desc)
        desc.all_lowdeg = 0
    xi = g0 = ln = flow = None
    if want_xi:
        if not batch.shared_graph:
            raise ValueError('transition posteriors need one graph for the whole batch')
        S = batch.n_states[0]
        xi = torch.zeros(S, S, dtype=torch.float64, device=dev)
        g0 = torch.zeros(S, dtype=torch.float64, device=dev)
        flow = torch.zeros(S, dtype=torch.float64, device=dev)
    if want_lognorm:
        ln = torch.empty(batch.nutt, dtype=dt, device=dev)
    route = _route(dt, desc, want_xi, 1)
    if route == _hip.EINVAL and not desc.all_lowdeg:
        err = _hip.HipError(
            f'forward-backward: a graph of the batch has {desc.max_states} states; the general '
            "kernel keeps five per-state arrays in the CU's 160 KB of LDS (about 4000 states). "
            'Graphs with at most 8 arcs per state besides a declared hub '
            '(CompiledGraph.set_hub) run at any size')
        err.rc = route
        raise err
    gamma, alpha, hub_ws = _workspace(batch, desc, want_xi)
    _hip.call('beer_hmm_forward_backward', _hip.dtype_code(dt), ctypes.byref(desc),
              _hip.ptr(pc_llhs), _hip.ptr(alpha), _hip.ptr(hub_ws), _hip.ptr(gamma),
              _hip.ptr(xi), _hip.ptr(g0), _hip.ptr(flow), _hip.ptr(ln))
    _note_alpha(batch, alpha, route, hub_ws)
    return gamma, xi, g0, ln, flow


def trans_posteriors_dense(batch, pc_llhs, gamma, trans_log_probs):
    '''Per-frame transition posteriors [T-1, S, S] of a ONE-utterance batch whose
    forward-backward call has just run (`beer_hmm_trans_posteriors`): the
    reference's layout, graph.py:308-323.'''
    if batch.nutt != 1:
        raise ValueError('per-frame transition posteriors: one utterance at a time')
    if not getattr(batch, 'last_alpha_is_log', False):
        raise ValueError('per-frame transition posteriors read log-space forward values: run '
                         'forward_backward(..., dense_xi=True) on this batch first')
    S, T = batch.n_states[0], batch.n_frames
    trans = _hip.on_device(trans_log_probs, batch.dtype)
    xi = torch.zeros(max(T - 1, 0), S, S, dtype=batch.dtype, device=batch.device)
    _hip.call('beer_hmm_trans_posteriors', _hip.dtype_code(batch.dtype), T, S,
              _hip.ptr(batch.last_alpha), _hip.ptr(pc_llhs), _hip.ptr(gamma), _hip.ptr(trans),
              _hip.ptr(xi))
    return xi


class counting_log_space:
    '''Context manager (per host thread): while active, every one-wave forward-backward
    launch adds the number of utterances it ran in LOG SPACE to `.count` (0-dim int64
    device tensor; `beer_hmm_fb_log_count`).  The one-wave kernels work on scaled
    probabilities and hand an utterance over to their log-space twin when a column or a
    frame's normaliser leaves fp64's range or a log-likelihood is NaN (the reference is
    log-space throughout, graph.py:270-326); `.launches` counts the launches seen.'''
    _tls = threading.local()

    def __enter__(self):
        self.count = torch.zeros((), dtype=torch.int64, device=_hip.require_device())
        self.launches = 0
        self._outer = getattr(self._tls, 'active', None)
        self._tls.active = self
        return self

    def __exit__(self, *exc):
        self._tls.active = self._outer
        return False

    @classmethod
    def note(cls, batch, hub_ws):
        self = getattr(cls._tls, 'active', None)
        if self is not None and fused_ok(batch):
            _hip.call('beer_hmm_fb_log_count', batch.ref(), _hip.ptr(hub_ws),
                      _hip.ptr(self.count))
            self.launches += 1


def fused_ok(batch):
    '''True when `posteriors_fused` takes the batch: low-degree graphs of <= 256
    states with at most one hub of <= 64 members a side (wave_fb_ok of csrc/hmm.hip).'''
    # (= wave_fb_ok: nothing else decides without xi, and no HmmBatch is refused: 1..32767 states)
    if not hasattr(batch, '_fused'):                 # (asked once per descriptor)
        batch._fused = _hip.fb_family(_route(batch.dtype, batch.struct, 0, 0)) == _hip.FB_WAVE
    return batch._fused


FUSED_ROW_MAX = 512          # kWvRowMax of hmm.hip: pdf ids of a set that fit a wave's LDS row


def posteriors_fused(batch, pc_all, scale=1., want_counts=False, utt_llh=None, frame_llh=None,
                     want_transitions=False, gamma0_sum=None):
    '''Gather + forward-backward + scatter of a shard in one launch
    (`beer_hmm_posteriors_fused`): (state_resps [n_frames, S_total] = scale *
    gamma at the pdf ids, gamma0_sum [S] or None, hub_flow [S] or None);
    `utt_llh` [nutt] fp64 += sum_t sum_s gamma * scale * pc; `frame_llh` [n_frames]
    (the batch's dtype) receives that sum per frame (hmm.py:87).  `want_counts`
    (one graph for the whole batch): the posteriors of the first frame and the
    flows through the graph's hub -- what PhoneLoop counts (phoneloop.py:88-95).
    `want_transitions` (one graph): the same launch also counts the transitions of learned
    transition probabilities (`beer_hmm_posteriors_fused_counts`, every other output bit for
    bit the same) and a fourth value is returned: ('arcs', arc_counts, src_flow) -- see
    `transition_counts`.  A batch of graphs bound to the model (`HMM.bind_alignment_graphs`,
    any graph per utterance) gives ('cat', counts by category, None) instead
    (`beer_hmm_posteriors_fused_cat`).  `gamma0_sum` ([max states] fp64, +=): the first-frame
    posteriors by state index into the caller's buffer, for batches of several graphs too.'''
    dt, dev = batch.dtype, batch.device
    pc_all = _hip.on_device(pc_all, dt)
    S_total = pc_all.shape[1]
    repeats, covers = batch.pdf_ids_profile(S_total)
    # how the posteriors go back to pdf ids (include/beer_hip.h): whole rows through LDS when a
    # graph repeats ids or leaves some out (alignment graphs) and a row fits; else atomic adds
    # into / plain stores over a zero-filled array; plain stores when the ids are a permutation
    out_mode = 2 if (repeats or not covers) and S_total <= FUSED_ROW_MAX else (1 if repeats else 0)
    make = torch.empty if (out_mode == 2 or (not repeats and covers)) else torch.zeros
    sr = make(batch.n_frames, S_total, dtype=dt, device=dev)
    _, alpha, hub_ws = _workspace(batch, packed=False)
    g0 = flow = None
    if want_counts:
        if not batch.shared_graph:
            raise ValueError('first-frame posteriors / hub flows need one graph for the batch')
        S = batch.n_states[0]
        g0 = torch.zeros(S, dtype=torch.float64, device=dev)
        flow = torch.zeros(S, dtype=torch.float64, device=dev)
    elif gamma0_sum is not None:
        if gamma0_sum.dtype != torch.float64 or gamma0_sum.numel() < max(batch.n_states):
            raise ValueError('gamma0_sum: an fp64 buffer of at least the largest graph\'s states')
        g0 = gamma0_sum
    if frame_llh is not None and (frame_llh.dtype != dt or frame_llh.numel() != batch.n_frames or
                                  not frame_llh.is_contiguous() or frame_llh.device != sr.device):
        raise ValueError('frame_llh: a contiguous [n_frames] tensor of the batch\'s dtype and device')
    args = (_hip.dtype_code(dt), batch.ref(), S_total, _hip.ptr(pc_all), float(scale),
            _hip.ptr(alpha), _hip.ptr(hub_ws), _hip.ptr(sr), out_mode, _hip.ptr(g0),
            _hip.ptr(flow), _hip.ptr(utt_llh), _hip.ptr(frame_llh))
    counts = ()
    if want_transitions and batch.bound_set is not None:
        # alignment graphs bound to the model: the counts by category, any graph per utterance
        cat_counts = _cat_buffer(batch)
        _hip.call('beer_hmm_posteriors_fused_cat', *args[:9], _hip.ptr(g0), *args[11:],
                  ctypes.byref(batch.cat_map), _hip.ptr(cat_counts))
        counts = (('cat', cat_counts, None),)
    elif want_transitions:
        arc_counts, src_flow = _count_buffers(batch)
        _hip.call('beer_hmm_posteriors_fused_counts', *args, _hip.ptr(arc_counts),
                  _hip.ptr(src_flow))
        counts = (('arcs', arc_counts, src_flow),)
    else:
        _hip.call('beer_hmm_posteriors_fused', *args)
    _note_alpha(batch, None, _hip.FB_WAVE, hub_ws)
    return (sr, g0, flow) + counts


def lowdeg_arcs(batch):
    '''(source, destination) int64 device tensors of the arcs of the batch's ONE graph's
    low-degree image, in its out-CSR order: what `arc_counts` of the count kernels are
    indexed by (hub arcs are not in it).'''
    if not batch.shared_graph or getattr(batch.dgraphs[0], 'lowdeg', None) is None:
        raise ValueError('transition counts need one graph with a low-degree image for the batch')
    return batch.dgraphs[0].lowdeg_arcs()


def _cat_buffer(batch):
    return torch.zeros(batch.bound_set.n_categories, dtype=torch.float64, device=batch.device)


def _count_buffers(batch):
    if not batch.shared_graph or not fused_ok(batch):
        raise ValueError('the one-wave transition counts: one graph for the whole batch, of at '
                         f'most 256 states with at most {_hip.SEG} arcs a state '
                         'besides one declared hub of at most 64 phones')
    dev = batch.device
    S = batch.n_states[0]
    n_arcs = batch.dgraphs[0].lowdeg.n_arcs
    return (torch.zeros(max(n_arcs, 1), dtype=torch.float64, device=dev),
            torch.zeros(S, dtype=torch.float64, device=dev))


def last_frame_sum(batch, gamma, out=None):
    '''sum over the utterances of the posteriors of their last frame, [S] fp64
    (`beer_hmm_last_frame_sum`; one graph for the batch).'''
    if not batch.shared_graph:
        raise ValueError('last-frame posteriors need one graph for the batch')
    if out is None:
        out = torch.zeros(batch.n_states[0], dtype=torch.float64, device=batch.device)
    _hip.call('beer_hmm_last_frame_sum', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(gamma), _hip.ptr(out))
    return out


def forward_backward_counts(batch, pc_llhs):
    '''Forward-backward with the transition counts of learned transition probabilities, for
    every batch of one graph that `forward_backward` takes: (gamma packed, gamma0_sum [S],
    hub_flow [S] or None, xi_sum [S, S] or None, counts).  On the one-wave kernels
    (`beer_hmm_forward_backward_counts`, `fused_ok`) counts = ('arcs', arc_counts, src_flow)
    and the phone counts come from hub_flow; beyond them (more than 256 states, hubs of more
    than 64 phones) the general kernel's dense xi_sum -- hub arcs in the matrix -- and the
    posteriors of the last frames: counts = ('dense', xi_sum, last).  See `transition_counts`.'''
    dt, dev = batch.dtype, batch.device
    if batch.bound_set is not None:
        # alignment graphs bound to the model (`beer_hmm_forward_backward_cat`): any graph per
        # utterance, the one-wave kernels or -- beyond 256 states -- the workgroup kernels
        cat_counts = _cat_buffer(batch)
        gamma, alpha, hub_ws = _workspace(batch, batch.struct, want_xi=True)
        _hip.call('beer_hmm_forward_backward_cat', _hip.dtype_code(dt), batch.ref(),
                  _hip.ptr(pc_llhs), _hip.ptr(alpha), _hip.ptr(hub_ws), _hip.ptr(gamma), None,
                  ctypes.byref(batch.cat_map), _hip.ptr(cat_counts), None)
        _note_alpha(batch, alpha, _route(dt, batch.struct, 1, 1), hub_ws)
        return gamma, None, None, None, ('cat', cat_counts, None)
    if not batch.shared_graph:
        raise ValueError('transition counts need one graph for the whole batch')
    if not fused_ok(batch):
        gamma, xi, g0, _, _ = forward_backward(batch, pc_llhs, want_xi=True, dense_xi=True)
        return gamma, g0, None, xi, ('dense', xi, last_frame_sum(batch, gamma))
    arc_counts, src_flow = _count_buffers(batch)
    S = batch.n_states[0]
    gamma, alpha, hub_ws = _workspace(batch)
    g0 = torch.zeros(S, dtype=torch.float64, device=dev)
    flow = torch.zeros(S, dtype=torch.float64, device=dev)
    _hip.call('beer_hmm_forward_backward_counts', _hip.dtype_code(dt), batch.ref(),
              _hip.ptr(pc_llhs), _hip.ptr(alpha), _hip.ptr(hub_ws), _hip.ptr(gamma),
              _hip.ptr(g0), _hip.ptr(flow), _hip.ptr(arc_counts), _hip.ptr(src_flow), None)
    _note_alpha(batch, alpha, _hip.FB_WAVE, hub_ws)
    return gamma, g0, flow, None, ('arcs', arc_counts, src_flow)


def path_counts(batch, path, xi):
    '''The hard counts of a state path, ('dense', xi, last): the dense xi_sum of
    `path_posteriors(want_xi=True)` and how often each state ends an utterance.'''
    path = _hip.on_device(torch.as_tensor(path)).to(torch.int64).reshape(-1)
    if batch.bound_set is not None:
        # alignment graphs bound to the model: +1 at the category of every arc of the path
        cat_counts = _cat_buffer(batch)
        _hip.call('beer_hmm_path_counts_cat', batch.ref(), _hip.ptr(path.contiguous()),
                  ctypes.byref(batch.cat_map), _hip.ptr(cat_counts))
        return ('cat', cat_counts, None)
    last = torch.zeros(xi.shape[0], dtype=torch.float64, device=xi.device)
    if path.numel():
        # an utterance of no frames ends in no state: it counts 0 (at whatever index)
        off = batch.bufs['frame_off']
        ends = (off[1:] - 1).clamp_(min=0)
        last.index_add_(0, path[ends], (off[1:] > off[:-1]).to(torch.float64))
    return ('dense', xi, last)


def bigram_ok(batch):
    '''True when `posteriors_bigram` takes the batch on its kernel: one graph for every
    utterance, with a declared bigram block (CompiledGraph.set_bigram_block) of at most
    128 phones on at most 512 states, every other state with at most 8 arcs a side.
    Chosen by the declared block, not by the graph's degree.'''
    graphs = getattr(batch, 'source_graphs', None)
    if not batch.shared_graph or not graphs or not hasattr(graphs[0], 'bigram_image'):
        return False
    return graphs[0].bigram_image(batch.dtype) is not None


def posteriors_bigram(batch, pc_all, scale=1., utt_llh=None):
    '''Gather + forward-backward + scatter of a free bigram loop in one launch
    (`beer_hmm_posteriors_bigram`): (state_resps [n_frames, S_total] = scale * gamma at
    the pdf ids, counts [P, P] fp64 = sum over utterances and frames of the transition
    posteriors of the block, row i = source src_i).  `utt_llh` [nutt] fp64 +=
    sum_t sum_s gamma * scale * pc.  Batches the kernel does not take (`bigram_ok`), and
    sub-batches in which an utterance left fp64's range, go through the general
    log-space path (`forward_backward(want_xi=True)`), with the same results.'''
    dt, dev = batch.dtype, batch.device
    pc_all = _hip.on_device(pc_all, dt)
    S_total = pc_all.shape[1]
    graph = batch.source_graphs[0] if getattr(batch, 'source_graphs', None) else None
    img = graph.bigram_image(dt) if (graph is not None and batch.shared_graph) else None
    if img is not None and torch.cuda.is_current_stream_capturing():
        # (the flags are read on the host below: such an E-step cannot be recorded)
        raise _hip.HipInvalid('posteriors_bigram reads its range flags on the host: '
                              'not recordable as a HIP graph')
    if img is not None:
        if len(batch._pdf_ids_h) and int(batch._pdf_ids_h.max()) >= S_total:
            raise ValueError(f'posteriors_bigram: a pdf id of the graph is not below {S_total}')
        repeats, covers = batch.pdf_ids_profile(S_total)
        atomic = repeats or not covers
        sr = (torch.zeros if atomic else torch.empty)(batch.n_frames, S_total, dtype=dt,
                                                      device=dev)
        P, N = img.n_phones, batch.n_frames
        alpha = torch.empty(N * img.n_states, dtype=torch.float64, device=dev)
        uv = torch.empty(2, N, P, dtype=torch.float64, device=dev)
        llh = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
        flags = torch.empty(batch.nutt, dtype=torch.int32, device=dev)
        b = batch.bufs
        _hip.call('beer_hmm_posteriors_bigram', _hip.dtype_code(dt), ctypes.byref(img.struct),
                  batch.nutt, N, _hip.ptr(b['frame_off']), _hip.ptr(b['order']), S_total,
                  _hip.ptr(pc_all), float(scale), _hip.ptr(alpha), _hip.ptr(uv), _hip.ptr(sr),
                  1 if atomic else 0, _hip.ptr(llh), _hip.ptr(flags))
        # (one look at the flags per sub-batch: an utterance the linear-domain recursion
        #  could not hold is redone, with the whole sub-batch, in log space below)
        if not bool(flags.any()):
            counts = img.block_weights() * (uv[0].t() @ uv[1])
            if utt_llh is not None:
                utt_llh += llh
            return sr, counts
    # the general path: log-space forward-backward with the summed transition posteriors
    if graph is None or graph.__dict__.get('bigram') is None:
        raise ValueError('posteriors_bigram: one graph with a declared bigram block '
                         '(CompiledGraph.set_bigram_block)')
    pc_llhs = gather(batch, pc_all, scale)
    gamma, xi, _, _, flow = forward_backward(batch, pc_llhs, want_xi=True, dense_xi=True)
    sr, _ = scatter(batch, pc_llhs, gamma, S_total, scale, want_exp_llh=False, utt_llh=utt_llh)
    src, _, dst, _ = graph.bigram
    src_t = torch.as_tensor(src, device=dev)
    dst_t = torch.as_tensor(dst, device=dev)
    return sr, xi[src_t[:, None], dst_t[None, :]]


def viterbi(batch, pc_llhs, map_pdf=False):
    'int64 state (or pdf id) path for every frame of the batch.'
    bt = torch.empty(batch.n_elems, dtype=torch.int32, device=batch.device)
    path = torch.empty(batch.n_frames, dtype=torch.int64, device=batch.device)
    _hip.call('beer_hmm_viterbi', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(pc_llhs), _hip.ptr(bt), _hip.ptr(path), 1 if map_pdf else 0)
    return path


def check_nbest(k, what):
    'k of an n-best search, checked on the host before any device work.'
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f'{what}: k is an integer, not {k!r}')
    if not 1 <= k <= _hip.NBEST_MAX:
        raise ValueError(f'{what}: k = {k} is outside 1 .. {_hip.NBEST_MAX}')
    return int(k)


def nbest_route(batch, k):
    '''beer_hmm_nbest_route: the form `viterbi_nbest` runs on (the frames of back-pointers the
    back-trace stages at a time, arcs in LDS or not); HipInvalid where it refuses.'''
    k = check_nbest(k, 'nbest_route')
    return _route_or_refuse('beer_hmm_nbest_route', batch, (k,), lambda: (
        f'viterbi_nbest: {k} paths on graphs of up to {batch.struct.max_states} states: at '
        'most 32767 states, and two score columns [S][k] with two frames of back-pointers '
        "[S][k] in the CU's 160 KB of LDS"))


def viterbi_nbest(batch, pc_llhs, k, map_pdf=False):
    '''The `k` best state paths of every utterance and their scores (`beer_hmm_viterbi_nbest`):
    (paths int64 [k, n_frames] -- state indices, or pdf ids with `map_pdf` --, scores float64
    [nutt, k]) on the device, best first.  Ranks beyond the number of finite-score paths of an
    utterance have the score -inf and a path of -1.'''
    k = check_nbest(k, 'viterbi_nbest')
    nbest_route(batch, k)
    dev = batch.device
    bt = torch.empty(k * batch.n_elems, dtype=torch.int32, device=dev)
    paths = torch.empty(k, batch.n_frames, dtype=torch.int64, device=dev)
    scores = torch.empty(batch.nutt, k, dtype=torch.float64, device=dev)
    _hip.call('beer_hmm_viterbi_nbest', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(pc_llhs), k, _hip.ptr(bt), _hip.ptr(paths), _hip.ptr(scores),
              1 if map_pdf else 0)
    return paths, scores


def check_sample(sample, n_frames, viterbi=False, state_path=None):
    '''The `sample` argument of the training entry points, checked on the host before any
    device work: None (False: no draw), True (uniforms from the device's default generator)
    or the float64 tensor of `n_frames` uniforms.'''
    if sample is None or sample is False:
        return None
    if viterbi or state_path is not None:
        raise ValueError('sample: a drawn path excludes viterbi=True and state_path=')
    if sample is True:
        return True
    if not torch.is_tensor(sample) or sample.dtype != torch.float64:
        raise ValueError('sample: True or a float64 tensor of one uniform in [0, 1) per frame')
    if sample.numel() != n_frames:
        raise ValueError(f'sample: {sample.numel()} uniforms for {n_frames} frames')
    return sample


def sample_uniforms(sample):
    'The `uniforms` argument of `sample_paths` for a checked `sample` (True: drawn there).'
    return None if sample is True else sample.reshape(1, -1)


def sample_route(batch, nsamples=1):
    '''beer_hmm_sample_route: the forms `sample_paths` runs on (frame chunk, arcs in LDS, four
    lanes per state in the forward pass, samples per workgroup); HipInvalid where it refuses.'''
    return _route_or_refuse('beer_hmm_sample_route', batch, (int(nsamples),), lambda: (
        f'sample_paths: {nsamples} samples on graphs of up to {batch.struct.max_states} '
        "states: at least one sample, and two fp64 trellis rows in the CU's 160 KB of LDS "
        '(about 10000 states)'))


def sample_paths(batch, pc_llhs, uniforms=None, nsamples=1, generator=None, map_pdf=False,
                 return_trellis=False):
    '''`nsamples` state paths per utterance drawn from the posterior, int64 [nsamples, n_frames]
    (state indices, or pdf ids with `map_pdf`): forward filtering, backward sampling
    (`beer_hmm_sample_paths`).  `uniforms`: float64 [nsamples, n_frames] in [0, 1), one per
    sample and frame; default torch.rand on the device with `generator`.  `return_trellis`: also
    the normalised log-space forward values, fp64 packed like `pc_llhs`.'''
    dev = batch.device
    if uniforms is None:
        nsamples = int(nsamples)
        if nsamples < 1:
            raise ValueError('sample_paths: at least one sample')
        uniforms = torch.rand(nsamples, batch.n_frames, dtype=torch.float64, device=dev,
                              generator=generator)
    else:
        if not torch.is_tensor(uniforms) or uniforms.dtype != torch.float64 or \
                uniforms.dim() != 2 or uniforms.shape[0] < 1 or \
                uniforms.shape[1] != batch.n_frames:
            raise ValueError('sample_paths: uniforms are float64 [nsamples, n_frames]')
        nsamples = uniforms.shape[0]
        uniforms = _hip.on_device(uniforms)
    sample_route(batch, nsamples)
    alpha = torch.empty(batch.n_elems, dtype=torch.float64, device=dev)
    path = torch.empty(nsamples, batch.n_frames, dtype=torch.int64, device=dev)
    _hip.call('beer_hmm_sample_paths', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(pc_llhs), _hip.ptr(uniforms), nsamples, _hip.ptr(alpha), _hip.ptr(path),
              1 if map_pdf else 0)
    return (path, alpha) if return_trellis else path


def evidence_route(batch):
    '''beer_hmm_evidence_route: the form `log_evidence` runs on (one wave per utterance with
    1 / 2 / 4 states a lane, or one workgroup per utterance with its arcs in LDS and four lanes
    per state or not); HipInvalid where it refuses.'''
    return _route_or_refuse('beer_hmm_evidence_route', batch, (), lambda: (
        f'log_evidence: graphs of up to {batch.struct.max_states} states: two fp64 rows '
        "must fit the CU's 160 KB of LDS (about 10000 states)"))


def log_evidence(batch, pc_llhs, per_frame=False):
    '''(utt [nutt] fp64, frame [n_frames] fp64 or None), on the device: ln p(x) of every
    utterance under its graph, summed over all state paths, and with `per_frame` the terms
    ln p(x_t | x_0 .. x_{t-1}) it is made of, without the final weights
    (`beer_hmm_log_evidence`: the forward pass alone, no trellis).'''
    dev = batch.device
    evidence_route(batch)
    utt = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
    frame = torch.empty(batch.n_frames, dtype=torch.float64, device=dev) if per_frame else None
    _hip.call('beer_hmm_log_evidence', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(pc_llhs), _hip.ptr(utt), _hip.ptr(frame))
    return utt, frame


def arcs_route(batch, n_cat, per_frame=True):
    '''beer_hmm_arcs_route: the form `arc_posteriors` runs on (arcs in LDS or not, a frame's
    bins in LDS or not, the utterance's bins in LDS or not); HipInvalid where it refuses.'''
    args = (int(n_cat), 1 if per_frame else 0)
    return _route_or_refuse('beer_hmm_arcs_route', batch, args, lambda: (
        f'arc_posteriors: {n_cat} categories on graphs of up to {batch.struct.max_states} '
        "states: at least one category, and two fp64 rows in the CU's 160 KB of LDS (about "
        '10000 states)'))


def check_arc_categories(n_arcs, n_states, arc_cat, init_cat, n_cat, per_frame=True,
                         per_utt=False):
    '''The category arguments of `arc_posteriors`, checked on the host before any device work:
    `n_arcs` / `n_states` are the arc and state counts of the distinct graphs of a batch,
    `arc_cat` / `init_cat` one integer array per graph (host or device) or, already concatenated,
    one tensor each.  Returns (all arc categories, all init categories) as int32 tensors (on the
    host unless the caller's were on the device).  ValueError: neither output asked for,
    n_cat < 1, lengths that do not match the graphs, categories >= n_cat or < -1.'''
    if not (per_frame or per_utt):
        raise ValueError('arc_posteriors: neither per_frame nor per_utt is asked for')
    n_cat = int(n_cat)
    if n_cat < 1:
        raise ValueError(f'arc_posteriors: {n_cat} categories')
    out = []
    for what, cats, counts in (('arc_cat', arc_cat, n_arcs), ('init_cat', init_cat, n_states)):
        if torch.is_tensor(cats):
            if cats.dim() != 1 or cats.numel() != sum(counts):
                raise ValueError(f'arc_posteriors: {what} has {cats.numel()} entries, the graphs '
                                 f'of the batch {sum(counts)}')
            flat = cats
        else:
            cats = [torch.as_tensor(np.asarray(c.cpu() if torch.is_tensor(c) else c))
                    for c in cats]
            if len(cats) != len(counts):
                raise ValueError(f'arc_posteriors: {len(cats)} {what} arrays for {len(counts)} '
                                 'distinct graphs')
            for i, (c, n) in enumerate(zip(cats, counts)):
                if c.dim() != 1 or c.numel() != n:
                    raise ValueError(f'arc_posteriors: {what} of graph {i} has {c.numel()} '
                                     f'entries, the graph {n}')
            flat = torch.cat(cats) if cats else torch.zeros(0, dtype=torch.int32)
        if flat.dtype.is_floating_point or flat.dtype == torch.bool:
            raise ValueError(f'arc_posteriors: {what} must be integers, not {flat.dtype}')
        if flat.numel() and (int(flat.max()) >= n_cat or int(flat.min()) < -1):
            raise ValueError(f'arc_posteriors: {what} outside [-1, {n_cat}): '
                             f'{int(flat.min())} .. {int(flat.max())}')
        out.append(flat.to(torch.int32).contiguous())
    return tuple(out)


def _arc_map(batch, arcs, inits):
    '''(beer_arc_map, keep) of the checked categories `arcs` / `inits` (`check_arc_categories`):
    the offsets of every distinct graph and whichever of the two arrays is still on the host go
    to the device in one upload; an empty arc array gets an element, so that its pointer is not
    NULL.  `keep` holds the tensors the structure points into: the caller keeps it until the
    launch that reads the structure has been queued.'''
    arc_off = np.concatenate([[0], np.cumsum(batch.n_arcs)[:-1]]).astype(np.int64)
    state_off = np.concatenate([[0], np.cumsum(batch.n_states)[:-1]]).astype(np.int64)
    host = {'arc_off': torch.from_numpy(arc_off), 'state_off': torch.from_numpy(state_off)}
    if arcs.device.type != 'cuda':
        host['arcs'] = arcs if arcs.numel() else torch.zeros(1, dtype=torch.int32)
    if inits.device.type != 'cuda':
        host['inits'] = inits
    up = _hip.upload(host, batch.device)
    arcs, inits = up.get('arcs', arcs), up.get('inits', inits)
    amap = _hip.ArcMap(arcs.data_ptr(), inits.data_ptr(), up['arc_off'].data_ptr(),
                       up['state_off'].data_ptr())
    return amap, (up, arcs, inits)


def arc_posteriors(batch, pc_llhs, arc_cat, init_cat, n_cat, per_frame=True, per_utt=False):
    '''(frame_out [n_frames, n_cat] of the batch's dtype or None, utt_out [nutt, n_cat] fp64 or
    None), on the device: the posterior of every arc at every frame folded into categories
    (`beer_hmm_arc_posteriors`).  Row t >= 1 of an utterance holds, per category c, the sum of
    P(s_{t-1} = i, s_t = j | x) over the arcs i -> j with `arc_cat` = c; row 0 the sum of
    gamma_0(j) over the states with `init_cat` = c; `utt_out` the sum of an utterance's rows.
    `arc_cat` follows the full out-CSR of every distinct graph of the batch (`out_arcs()` of the
    graph classes gives its (src, dst) pairs), `init_cat` its states; both are one int array per
    distinct graph or already concatenated tensors, with entries in [0, n_cat) or -1 (count
    nothing).  An utterance whose evidence is -inf gets zeros.'''
    arcs, inits = check_arc_categories(batch.n_arcs, batch.n_states, arc_cat, init_cat, n_cat,
                                       per_frame, per_utt)
    n_cat = int(n_cat)
    dev = batch.device
    arcs_route(batch, n_cat, per_frame)
    if batch.nutt == 0:
        return (torch.empty(0, n_cat, dtype=batch.dtype, device=dev) if per_frame else None,
                torch.empty(0, n_cat, dtype=torch.float64, device=dev) if per_utt else None)
    dcode = _hip.dtype_code(batch.dtype)
    amap, keep = _arc_map(batch, arcs, inits)               # (`keep` lives until the call)
    extra = _hip.lib().beer_hmm_arcs_scratch_doubles(dcode, batch.ref())
    ws = torch.empty(batch.n_frames + batch.n_elems + extra, dtype=torch.float64, device=dev)
    frame = torch.empty(batch.n_frames, n_cat, dtype=batch.dtype, device=dev) \
        if per_frame else None
    utt = torch.empty(batch.nutt, n_cat, dtype=torch.float64, device=dev) if per_utt else None
    _hip.call('beer_hmm_arc_posteriors', dcode, batch.ref(), _hip.ptr(pc_llhs),
              ctypes.byref(amap), n_cat, _hip.ptr(ws), _hip.ptr(frame), _hip.ptr(utt))
    return frame, utt


def maxmarg_route(batch, n_cat=0, states=True, per_frame=False, per_utt=False):
    '''beer_hmm_maxmarg_route: the form `max_marginals` runs on (arcs in LDS or not, the bins in
    LDS or in the output rows); HipInvalid where it refuses.'''
    args = (int(n_cat), 1 if states else 0, 1 if per_frame else 0, 1 if per_utt else 0)
    return _route_or_refuse('beer_hmm_maxmarg_route', batch, args, lambda: (
        f'max_marginals: {n_cat} categories on graphs of up to {batch.struct.max_states} '
        'states: at least one output, at least one category for the outputs by category, '
        "and two fp64 rows in the CU's 160 KB of LDS (about 10000 states)"))


def max_marginals(batch, pc_llhs, arc_cat=None, init_cat=None, n_cat=0, states=True,
                  per_frame=False, per_utt=False):
    '''(best [nutt] fp64, state [n_elems] of the batch's dtype or None, frame [n_frames, n_cat]
    of the batch's dtype or None, utt [nutt, n_cat] fp64 or None), on the device: the Viterbi
    max-marginals (`beer_hmm_max_marginals`).  `best` is the score of the best path; `state`,
    packed like `pc_llhs`, holds for every frame and state the score of the best path through
    it minus `best` (0 on the Viterbi path, -inf where no path passes); row t >= 1 of `frame`
    holds, per category c, the maximum of the same quantity over the arcs i -> j entering frame
    t with `arc_cat` = c, row 0 that of the states with `init_cat` = c, `utt` the maximum over an
    utterance's rows; a category with no member holds -inf.  The categories are those of
    `arc_posteriors` and are needed for `per_frame` / `per_utt` only.  An utterance without a
    path of finite score has best = -inf and -inf everywhere.'''
    cats = per_frame or per_utt
    if not (states or cats):
        raise ValueError('max_marginals: none of states, per_frame and per_utt is asked for')
    if cats and (arc_cat is None or init_cat is None):
        raise ValueError('max_marginals: per_frame / per_utt need arc_cat and init_cat')
    arcs = inits = None
    if arc_cat is not None or init_cat is not None:
        if arc_cat is None or init_cat is None:
            raise ValueError('max_marginals: arc_cat and init_cat come together')
        arcs, inits = check_arc_categories(batch.n_arcs, batch.n_states, arc_cat, init_cat, n_cat,
                                           True, False)
    n_cat = int(n_cat) if arcs is not None else 0
    dev = batch.device
    maxmarg_route(batch, n_cat, states, per_frame, per_utt)
    best = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
    state = torch.empty(batch.n_elems, dtype=batch.dtype, device=dev) if states else None
    frame = torch.empty(batch.n_frames, n_cat, dtype=batch.dtype, device=dev) \
        if per_frame else None
    utt = torch.empty(batch.nutt, n_cat, dtype=torch.float64, device=dev) if per_utt else None
    if batch.nutt == 0:
        return best, state, frame, utt
    dcode = _hip.dtype_code(batch.dtype)
    amap = keep = None                                      # (no categories: no map)
    if arcs is not None:
        amap, keep = _arc_map(batch, arcs, inits)           # (`keep` lives until the call)
        amap = ctypes.byref(amap)
    extra = _hip.lib().beer_hmm_maxmarg_scratch_doubles(dcode, batch.ref())
    ws = torch.empty(max(batch.n_elems + extra, 1), dtype=torch.float64, device=dev)
    _hip.call('beer_hmm_max_marginals', dcode, batch.ref(), _hip.ptr(pc_llhs), amap, n_cat,
              _hip.ptr(ws), _hip.ptr(state), _hip.ptr(frame), _hip.ptr(utt), _hip.ptr(best))
    return best, state, frame, utt


class SegmentMap:
    '''beer_seg_map on the host: the closures of every (graph, category) as int32 numpy arrays
    (`mem_ptr`, `members`, `mem_init`, `in_ptr`, `in_src`, `in_arc`, `ent_ptr`, `ent_src`,
    `ent_arc`), `max_closure`, `n_cat` and `n_graphs`; `closure(g, c)` gives the member states of
    one.  `struct(device)` uploads it once and returns the ctypes structure.'''
    FIELDS = ('mem_ptr', 'members', 'mem_init', 'in_ptr', 'in_src', 'in_arc', 'ent_ptr',
              'ent_src', 'ent_arc')

    def __init__(self, n_graphs, n_cat, max_closure, **arrays):
        self.n_graphs, self.n_cat, self.max_closure = n_graphs, n_cat, max_closure
        for name in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=np.int32))
        self._dev = {}

    def closure(self, g, c):
        k = g * self.n_cat + c
        return self.members[self.mem_ptr[k]:self.mem_ptr[k + 1]]

    def struct(self, device):
        hit = self._dev.get(device)
        if hit is None:
            # (an empty array still gets an address: no member of the structure is NULL)
            up = _hip.upload({name: torch.from_numpy(getattr(self, name)) if
                              getattr(self, name).size else torch.zeros(1, dtype=torch.int32)
                              for name in self.FIELDS}, device)
            hit = self._dev[device] = (_hip.SegMap(*[up[name].data_ptr() for name in self.FIELDS],
                                                   self.max_closure, 0), up)
        return hit[0]


def _arcs_of(graph):
    '(src, dst, n_states) of a graph object (`out_arcs()`, `n_states`) or of such a triple.'
    if isinstance(graph, tuple):
        src, dst, n_states = graph
    else:
        (src, dst), n_states = graph.out_arcs(), graph.n_states
    return np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), int(n_states)


def segment_map(graphs, arc_cat, init_cat, n_cat):
    '''The closures `segment_margins` walks, built on the host (no device needed): a
    `SegmentMap`.  `graphs` are the distinct graphs of a batch (objects with `out_arcs()` and
    `n_states`, or (src, dst, n_states) triples in out-CSR order), `arc_cat` / `init_cat` one
    integer array per graph as for `arc_posteriors`.  The closure of category c in a graph is
    the set of states reachable from the destinations of the arcs of category c and from the
    states with `init_cat` = c through arcs of category -1 (a breadth-first search): on a phone
    loop with `unit_start_categories` the unit's own states, on an alignment graph the union of
    the instances of a repeated unit.'''
    triples = [_arcs_of(g) for g in graphs]
    arcs, inits = check_arc_categories([len(t[0]) for t in triples], [t[2] for t in triples],
                                       arc_cat, init_cat, n_cat)
    n_cat = int(n_cat)
    arcs, inits = arcs.cpu().numpy(), inits.cpu().numpy()
    counts = np.zeros(len(triples) * n_cat, dtype=np.int64)
    parts = {name: [] for name in SegmentMap.FIELDS[1:]}
    n_in = n_ent = a0 = s0 = 0
    in_counts, ent_counts = [], []
    for g, (src, dst, S) in enumerate(triples):
        A = len(src)
        acat, icat = arcs[a0:a0 + A], inits[s0:s0 + S]
        a0, s0 = a0 + A, s0 + S
        free = np.nonzero(acat == -1)[0]
        fsrc, fdst = src[free], dst[free]
        for c in np.union1d(acat[acat >= 0], icat[icat >= 0]):
            enter = np.nonzero(acat == c)[0]
            inside = np.zeros(S, dtype=bool)
            inside[dst[enter]] = True
            inside[icat == c] = True
            while True:                                     # breadth-first over the -1 arcs
                reach = fdst[inside[fsrc]]
                if inside[reach].all():
                    break
                inside[reach] = True
            members = np.nonzero(inside)[0]
            local = np.full(S, -1, dtype=np.int64)
            local[members] = np.arange(len(members))
            counts[g * n_cat + c] = len(members)
            parts['members'].append(members)
            parts['mem_init'].append(icat[members] == c)
            for name, arc_ids, source in (('in', free[inside[fsrc]], 'local'),
                                          ('ent', enter, 'state')):
                # a member's arcs together, in out-CSR order (the sort is stable)
                arc_ids = arc_ids[np.argsort(local[dst[arc_ids]], kind='stable')]
                per_member = np.bincount(local[dst[arc_ids]], minlength=len(members))
                (in_counts if name == 'in' else ent_counts).append(per_member)
                parts[name + '_src'].append(local[src[arc_ids]] if source == 'local'
                                            else src[arc_ids])
                parts[name + '_arc'].append(arc_ids)

    def cat(chunks):
        return np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int64)

    def ptr(chunks):
        return np.concatenate([[0], np.cumsum(cat(chunks))])

    mem_ptr = np.concatenate([[0], np.cumsum(counts)])
    in_ptr, ent_ptr = ptr(in_counts), ptr(ent_counts)
    if max(mem_ptr[-1], in_ptr[-1], ent_ptr[-1]) >= 2 ** 31:
        raise ValueError('segment_map: the closures of these categories hold more than 2^31 '
                         'members or arcs')
    return SegmentMap(len(triples), n_cat, int(counts.max(initial=0)), mem_ptr=mem_ptr,
                      members=cat(parts['members']), mem_init=cat(parts['mem_init']),
                      in_ptr=in_ptr, in_src=cat(parts['in_src']), in_arc=cat(parts['in_arc']),
                      ent_ptr=ent_ptr, ent_src=cat(parts['ent_src']),
                      ent_arc=cat(parts['ent_arc']))


def segments_route(batch, n_cat, max_closure=0):
    '''beer_hmm_segments_route: the form `segment_margins` runs on (the trellis kernel's arcs
    and bins in LDS or not, and in the low bits the team size of the expand kernel,
    `_hip.segments_team`); HipInvalid where it refuses.'''
    args = (int(n_cat), int(max_closure))
    return _route_or_refuse('beer_hmm_segments_route', batch, args, lambda: (
        f'segment_margins: {n_cat} categories with closures of up to {max_closure} states on '
        f'graphs of up to {batch.struct.max_states} states: at least one category, two fp64 '
        "rows of the graph in the CU's 160 KB of LDS (about 10000 states), and two fp64 rows "
        'of the largest closure in 64 KB (4095 states)'))


def _check_max_dur(max_dur, what):
    'max_dur as an int, or None where it is; ValueError unless it is an integer >= 1.'
    if max_dur is None:
        return None
    if int(max_dur) != max_dur or max_dur < 1:
        raise ValueError(f'{what}: max_dur is an integer >= 1, not {max_dur}')
    return int(max_dur)


def check_segments(beam, max_dur, what='segment_margins'):
    '(beam as a float, max_dur as an int); ValueError for a negative or NaN beam, max_dur < 1.'
    beam = float(beam)
    if not beam >= 0.:
        raise ValueError(f'{what}: the beam is a number >= 0 (inf: everything), not {beam}')
    return beam, _check_max_dur(max_dur, what)


def _within(values, beam):
    'values >= -beam, and finite (beam = inf keeps every finite cell).'
    return (values >= -beam) & (values > -float('inf'))


def _segment_args(what, batch, arc_cat, init_cat, n_cat, max_dur, seg_map):
    '''(arcs, inits, n_cat, seg_map) of `segment_margins` / `segment_posteriors`, checked on the
    host in this order: `max_dur` is given, the categories (`check_arc_categories`), the segment
    map -- built here when None -- is of the batch's graphs and these categories.'''
    if max_dur is None:
        raise ValueError(f'{what}: max_dur is an integer >= 1, not None')
    arcs, inits = check_arc_categories(batch.n_arcs, batch.n_states, arc_cat, init_cat, n_cat)
    n_cat = int(n_cat)
    if seg_map is None:
        seg_map = segment_map(batch.source_graphs, arcs.cpu(), inits.cpu(), n_cat)
    if seg_map.n_cat != n_cat or seg_map.n_graphs != len(batch.n_states):
        raise ValueError(f'{what}: a segment map of {seg_map.n_graphs} graphs and '
                         f'{seg_map.n_cat} categories for {len(batch.n_states)} and {n_cat}')
    return arcs, inits, n_cat, seg_map


def _no_entries(batch, max_dur):
    '(entry_frame, entry_cat, seg) of a batch without utterances.'
    dev = batch.device
    return (torch.empty(0, dtype=torch.int64, device=dev),
            torch.empty(0, dtype=torch.int32, device=dev),
            torch.empty(0, max_dur, dtype=batch.dtype, device=dev))


def _entries_of(at):
    '(entry_frame int64, entry_cat int32) of the rows `torch.nonzero` found in `starts`.'
    return at[:, 0].contiguous(), at[:, 1].to(torch.int32)


def _entry_rows(batch, entry_frame, max_dur):
    '''(entry_off [nutt + 1]: where the entries of every utterance begin, seg [n_entries, max_dur]
    of the batch's dtype, to be filled) for entries sorted by frame.'''
    return (torch.searchsorted(entry_frame, batch.bufs['frame_off']),
            torch.empty(len(entry_frame), max_dur, dtype=batch.dtype, device=batch.device))


def _segments_where(keep, entry_frame, entry_cat, seg):
    '(start, end, unit, value float64) of the cells of `seg` that `keep` marks, in row-major order.'
    at = torch.nonzero(keep)
    start = entry_frame[at[:, 0]]
    return start, start + at[:, 1], entry_cat[at[:, 0]], seg[at[:, 0], at[:, 1]].double()


def segment_margins(batch, pc_llhs, arc_cat, init_cat, n_cat, beam, max_dur, seg_map=None):
    '''(best [nutt] fp64, starts [n_frames, n_cat], entry_frame [n_entries] int64, entry_cat
    [n_entries] int32, seg [n_entries, max_dur]) on the device, `starts` and `seg` of the batch's
    dtype: the unit segment lattice (`beer_hmm_segment_trellis`, `beer_hmm_segment_margins`).
    `best` and `starts` are `max_marginals`' best and per-frame rows, bit for bit.  The entries are
    the cells (frame, category) of `starts` that are >= -beam, in row-major order (`beam` = inf:
    every finite cell); seg[n, k] is the score of the best path on which category entry_cat[n]
    begins at frame entry_frame[n] (indexed as in the batch's frame offsets) and lasts exactly k
    more frames -- the next boundary, or the utterance's end, follows frame entry_frame[n] + k --
    minus `best`; -inf where there is no such path or the segment would pass the utterance's end.
    A segment ends where an arc of a category >= 0 is taken: the categories are those of
    `arc_posteriors`.  `seg_map`: `segment_map` of the batch's distinct graphs and these
    categories, built here when not given.  The entry selection is one `torch.nonzero`, which
    waits for the device.  ValueError, before any device work: a negative or NaN beam,
    max_dur < 1, bad categories.'''
    beam, max_dur = check_segments(beam, max_dur)
    arcs, inits, n_cat, seg_map = _segment_args('segment_margins', batch, arc_cat, init_cat,
                                                n_cat, max_dur, seg_map)
    dev, dt = batch.device, batch.dtype
    segments_route(batch, n_cat, seg_map.max_closure)
    best = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
    starts = torch.empty(batch.n_frames, n_cat, dtype=dt, device=dev)
    if batch.nutt == 0:
        return (best, starts) + _no_entries(batch, max_dur)
    dcode = _hip.dtype_code(dt)
    amap, keep = _arc_map(batch, arcs, inits)               # (`keep` lives until the call)
    extra = _hip.lib().beer_hmm_segments_scratch_doubles(dcode, batch.ref())
    trellis = torch.empty(2 * batch.n_elems + extra + 1, dtype=torch.float64, device=dev)
    d, x, ws = trellis[:batch.n_elems], trellis[batch.n_elems:2 * batch.n_elems], \
        trellis[2 * batch.n_elems:]
    _hip.call('beer_hmm_segment_trellis', dcode, batch.ref(), _hip.ptr(pc_llhs),
              ctypes.byref(amap), n_cat, _hip.ptr(d), _hip.ptr(x), _hip.ptr(ws), _hip.ptr(starts),
              _hip.ptr(best))
    # (row-major; waits for the device)
    entry_frame, entry_cat = _entries_of(torch.nonzero(_within(starts, beam)))
    entry_off, seg = _entry_rows(batch, entry_frame, max_dur)
    _hip.call('beer_hmm_segment_margins', dcode, batch.ref(), _hip.ptr(pc_llhs),
              ctypes.byref(seg_map.struct(dev)), n_cat, _hip.ptr(d), _hip.ptr(x), _hip.ptr(best),
              _hip.ptr(entry_frame), _hip.ptr(entry_cat), _hip.ptr(entry_off), len(entry_frame),
              max_dur, _hip.ptr(seg))
    return best, starts, entry_frame, entry_cat, seg


def segments_within(entry_frame, entry_cat, seg, beam):
    '''(start int64, end int64, unit int32, margin float64) of the cells of `segment_margins`'
    `seg` that are >= -beam, sorted by (start, unit, end); the frames indexed as `entry_frame`.'''
    return _segments_where(_within(seg, float(beam)), entry_frame, entry_cat, seg)


def segposts_route(batch, n_cat, max_closure=0):
    '''beer_hmm_segposts_route: the form `segment_posteriors` runs on (the trellis kernel's arcs
    and bins in LDS or not, and in the low bits the team size of the expand kernel,
    `_hip.segposts_team`); HipInvalid where it refuses.'''
    args = (int(n_cat), int(max_closure))
    return _route_or_refuse('beer_hmm_segposts_route', batch, args, lambda: (
        f'segment_posteriors: {n_cat} categories with closures of up to {max_closure} states '
        f'on graphs of up to {batch.struct.max_states} states: at least one category, two '
        "fp64 rows of the graph in the CU's 160 KB of LDS (about 10000 states), and four fp64 "
        'rows of the largest closure in 64 KB (2046 states)'))


def check_segment_posteriors(min_post, max_dur, what='segment_posteriors'):
    '''(min_post as a float, max_dur as an int or None); ValueError for a min_post that is
    negative, NaN or above 1, and for max_dur < 1.'''
    min_post = float(min_post)
    if not 0. <= min_post <= 1.:
        raise ValueError(f'{what}: min_post is a probability in [0, 1], not {min_post}')
    return min_post, _check_max_dur(max_dur, what)


def _above(values, min_post):
    'values >= min_post, and > 0 (min_post = 0 keeps every possible cell).'
    return (values >= min_post) & (values > 0)


def _check_entries(entries, n_frames, n_cat, what):
    '(entry_frame int64, entry_cat int32) of the caller; ValueError when unsorted or out of range.'
    if not isinstance(entries, (tuple, list)) or len(entries) != 2:
        raise ValueError(f'{what}: entries is a pair (entry_frame, entry_cat)')
    frame, cat = (e if torch.is_tensor(e) else torch.as_tensor(np.asarray(e)) for e in entries)
    if frame.dim() != 1 or cat.dim() != 1 or len(frame) != len(cat):
        raise ValueError(f'{what}: entry_frame and entry_cat are two vectors of one length')
    if frame.dtype.is_floating_point or cat.dtype.is_floating_point:
        raise ValueError(f'{what}: entries are integers')
    if len(frame):
        f, c = frame.cpu().numpy().astype(np.int64), cat.cpu().numpy().astype(np.int64)
        if f.min() < 0 or f.max() >= n_frames or c.min() < 0 or c.max() >= n_cat:
            raise ValueError(f'{what}: an entry outside the batch\'s {n_frames} frames or its '
                             f'{n_cat} categories')
        if (np.diff(f) < 0).any():
            raise ValueError(f'{what}: the entries are not sorted by frame')
    return frame.to(torch.int64), cat.to(torch.int32)


def segment_posteriors(batch, pc_llhs, arc_cat, init_cat, n_cat, min_post, max_dur, seg_map=None,
                       entries=None):
    '''(evidence [nutt] fp64, starts [n_frames, n_cat], entry_frame [n_entries] int64, entry_cat
    [n_entries] int32, seg [n_entries, max_dur]) on the device, `starts` and `seg` of the batch's
    dtype: the segment posteriors (`beer_hmm_segpost_trellis`, `beer_hmm_segment_posteriors`), the
    sum-product twin of `segment_margins`.  `evidence` is ln p(x) of every utterance, `starts`
    the start posteriors (`arc_posteriors`' per-frame rows).  The entries are the cells (frame,
    category) of `starts` that are >= `min_post` and > 0, in row-major order, or with
    `entries=(entry_frame, entry_cat)` the caller's, sorted by frame (those `segment_margins`
    returned, for instance: a lattice's arcs then get their posteriors).  seg[n, k] is the
    probability that category entry_cat[n] begins at frame entry_frame[n] (indexed as in the
    batch's frame offsets) and lasts exactly k more frames -- the next boundary, or the utterance's
    end, follows frame entry_frame[n] + k; 0 where that is impossible or the segment would pass the
    utterance's end.  With max_dur >= T a row sums to its entry's start posterior.  `seg_map`:
    `segment_map` of the batch's distinct graphs and these categories, built here when not given.
    The entry selection is one `torch.nonzero`, which waits for the device.  ValueError, before
    any device work: a min_post that is negative, NaN or above 1, max_dur < 1 or None, bad
    categories, a segment map of another shape, unsorted or out-of-range entries.'''
    what = 'segment_posteriors'
    min_post, max_dur = check_segment_posteriors(min_post, max_dur)
    arcs, inits, n_cat, seg_map = _segment_args(what, batch, arc_cat, init_cat, n_cat, max_dur,
                                                seg_map)
    if entries is not None:
        entries = _check_entries(entries, batch.n_frames, n_cat, what)
    dev, dt = batch.device, batch.dtype
    segposts_route(batch, n_cat, seg_map.max_closure)
    evidence = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
    starts = torch.empty(batch.n_frames, n_cat, dtype=dt, device=dev)
    if batch.nutt == 0:
        return (evidence, starts) + _no_entries(batch, max_dur)
    dcode = _hip.dtype_code(dt)
    amap, keep = _arc_map(batch, arcs, inits)               # (`keep` lives until the call)
    # the two trellises and the normalisers (an element more: no pointer is NULL)
    trellis = torch.empty(2 * batch.n_elems + batch.n_frames + 1, dtype=torch.float64, device=dev)
    alpha, y, norm = trellis[:batch.n_elems], trellis[batch.n_elems:2 * batch.n_elems], \
        trellis[2 * batch.n_elems:]
    _hip.call('beer_hmm_segpost_trellis', dcode, batch.ref(), _hip.ptr(pc_llhs),
              ctypes.byref(amap), n_cat, _hip.ptr(alpha), _hip.ptr(y), _hip.ptr(norm),
              _hip.ptr(starts), _hip.ptr(evidence))
    if entries is None:
        # (row-major; waits for the device)
        entry_frame, entry_cat = _entries_of(torch.nonzero(_above(starts, min_post)))
    else:
        entry_frame, entry_cat = (e.to(dev).contiguous() for e in entries)
    entry_off, seg = _entry_rows(batch, entry_frame, max_dur)
    _hip.call('beer_hmm_segment_posteriors', dcode, batch.ref(), _hip.ptr(pc_llhs),
              ctypes.byref(seg_map.struct(dev)), n_cat, _hip.ptr(alpha), _hip.ptr(y),
              _hip.ptr(norm), _hip.ptr(evidence), _hip.ptr(entry_frame), _hip.ptr(entry_cat),
              _hip.ptr(entry_off), len(entry_frame), max_dur, _hip.ptr(seg))
    return evidence, starts, entry_frame, entry_cat, seg


def segments_above(entry_frame, entry_cat, seg, min_post):
    '''(start int64, end int64, unit int32, post float64) of the cells of `segment_posteriors`'
    `seg` that are >= min_post and > 0, sorted by (start, unit, end); the frames indexed as
    `entry_frame`.'''
    return _segments_where(_above(seg, float(min_post)), entry_frame, entry_cat, seg)


def check_durations(log_dur, S_total, leave_w=None):
    '''The duration table of the explicit-duration entry points, checked on the host before any
    launch: `log_dur` a float64 tensor [S_total, D] with 1 <= D <= BEER_HSMM_MAX_DUR, no NaN and
    no +inf (-inf is legal); `leave_w` None or float64 [S_total], finite.  Returns D.'''
    if not torch.is_tensor(log_dur) or log_dur.dtype != torch.float64 or log_dur.dim() != 2:
        raise ValueError('durations: log_dur is a float64 tensor [S_total, D]')
    if log_dur.shape[0] != int(S_total):
        raise ValueError(f'durations: log_dur has {log_dur.shape[0]} rows for {S_total} pdf ids')
    D = int(log_dur.shape[1])
    if not 1 <= D <= _hip.HSMM_MAX_DUR:
        raise ValueError(f'durations: D = {D} is outside 1 .. {_hip.HSMM_MAX_DUR} '
                         '(BEER_HSMM_MAX_DUR)')
    if bool(torch.isnan(log_dur).any()) or bool((log_dur == float('inf')).any()):
        raise ValueError('durations: log_dur holds NaN or +inf')
    if leave_w is not None:
        if not torch.is_tensor(leave_w) or leave_w.dtype != torch.float64 or \
                tuple(leave_w.shape) != (int(S_total),):
            raise ValueError(f'durations: leave_w is a float64 tensor [{S_total}]')
        if not bool(torch.isfinite(leave_w).all()):
            raise ValueError('durations: leave_w must be finite')
    return D


def duration_route(batch, D):
    '''beer_hsmm_route: the form the explicit-duration kernels take for this batch and D (the
    team of lanes per state, ring in LDS or not, low-degree images or the full CSR); HipInvalid
    -- naming the limit -- where they refuse.'''
    return _route_or_refuse('beer_hsmm_route', batch, (int(D),), lambda: (
        f'explicit durations: D = {D} on graphs of up to {batch.struct.max_states} states: at '
        f'most {_hip.HSMM_MAX_DUR} frames a stay (BEER_HSMM_MAX_DUR) and '
        f'{_hip.HSMM_MAX_STATES} states a graph (BEER_HSMM_MAX_STATES)'))


def _duration_args(batch, pc_llhs, log_dur, leave_w, scratch='beer_hsmm_scratch_doubles'):
    '''(D, S_total, the two tables on the device, the workspace) of an explicit-duration call,
    checked; `scratch` names the size query of the entry point the workspace is for.'''
    S_total = log_dur.shape[0] if torch.is_tensor(log_dur) and log_dur.dim() == 2 else 0
    D = check_durations(log_dur, S_total, leave_w)
    if len(batch._pdf_ids_h) and int(batch._pdf_ids_h.max()) >= S_total:
        raise ValueError(f'durations: a pdf id of the batch is not below {S_total}')
    if pc_llhs.dtype != batch.dtype or pc_llhs.numel() != batch.n_elems:
        raise ValueError('durations: pc_llhs is the packed buffer of the batch, in its dtype')
    duration_route(batch, D)
    log_dur = _hip.on_device(log_dur)
    leave_w = None if leave_w is None else _hip.on_device(leave_w)
    extra = getattr(_hip.lib(), scratch)(_hip.dtype_code(batch.dtype), batch.ref(), D)
    ws = torch.empty(max(2 * batch.n_elems + 2 * batch.n_frames + extra, 1), dtype=torch.float64,
                     device=batch.device)
    return D, S_total, log_dur, leave_w, ws


def _duration_outputs(batch, S_total, D, want_counts):
    '''(gamma packed, evidence [nutt] fp64, dur_counts [S_total, D], entry_sum [S], gamma0_sum [S])
    of an explicit-duration forward-backward: the counts zero-filled fp64, None unless
    `want_counts`, the last two also None unless the batch shares one graph.'''
    dev = batch.device
    gamma = torch.empty(batch.n_elems, dtype=batch.dtype, device=dev)
    evidence = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
    counts = entry = g0 = None
    if want_counts:
        counts = torch.zeros(S_total, D, dtype=torch.float64, device=dev)
        if batch.shared_graph:
            entry = torch.zeros(batch.n_states[0], dtype=torch.float64, device=dev)
            g0 = torch.zeros(batch.n_states[0], dtype=torch.float64, device=dev)
    return gamma, evidence, counts, entry, g0


def duration_forward_backward(batch, pc_llhs, log_dur, leave_w=None, want_counts=True):
    '''Forward-backward over (state, duration) (`beer_hsmm_forward_backward`): (gamma packed,
    evidence [nutt] fp64, dur_counts [S_total, D] fp64 or None, entry_sum [S] fp64 or None,
    gamma0_sum [S] fp64 or None).  `log_dur` [S_total, D] float64 are the log duration laws by
    pdf id, `leave_w` [S_total] float64 (None: 0) is added to every arc that leaves a state.
    `want_counts`: the duration counts and -- when the batch shares one graph -- the segment
    entries per state from the second frame on and in the first frame.'''
    D, S_total, log_dur, leave_w, ws = _duration_args(batch, pc_llhs, log_dur, leave_w)
    gamma, evidence, counts, entry, g0 = _duration_outputs(batch, S_total, D, want_counts)
    _hip.call('beer_hsmm_forward_backward', _hip.dtype_code(batch.dtype), batch.ref(),
              _hip.ptr(pc_llhs), _hip.ptr(log_dur), _hip.ptr(leave_w), D, S_total, _hip.ptr(ws),
              _hip.ptr(gamma), _hip.ptr(evidence), _hip.ptr(counts), _hip.ptr(entry),
              _hip.ptr(g0))
    return gamma, evidence, counts, entry, g0


def duration_arcs_route(batch, D, n_cat, per_frame=True):
    '''beer_hsmm_arcs_route: the form `duration_arc_posteriors` takes (team, ring and the two bin
    bits `_hip.HSMM_ARCS_FRAME_LDS` / `_hip.HSMM_ARCS_UTT_LDS`); HipInvalid -- naming the limit --
    where it refuses.'''
    args = (int(D), int(n_cat), 1 if per_frame else 0)
    return _route_or_refuse('beer_hsmm_arcs_route', batch, args, lambda: (
        f'explicit durations: {n_cat} arc categories with D = {D} on graphs of up to '
        f'{batch.struct.max_states} states: at least one category, at most '
        f'{_hip.HSMM_MAX_DUR} frames a stay (BEER_HSMM_MAX_DUR) and '
        f'{_hip.HSMM_MAX_STATES} states a graph (BEER_HSMM_MAX_STATES)'))


def duration_arc_posteriors(batch, pc_llhs, log_dur, leave_w, arc_cat, init_cat, n_cat,
                            per_frame=True, per_utt=False, total=False, want_counts=True):
    '''Forward-backward over (state, duration) that also folds the arc every segment is entered
    by into categories (`beer_hsmm_arc_posteriors`): (gamma, evidence, dur_counts, entry_sum,
    gamma0_sum) as `duration_forward_backward` gives them, then (frame_out [n_frames, n_cat] of
    the batch's dtype, utt_out [nutt, n_cat] fp64, total_out [n_cat] fp64), each None unless
    asked for.  Row t >= 1 of an utterance holds per category the posterior that a segment
    begins at t entered by an arc of that category, row 0 the first segment's state by
    `init_cat`: a row sums to the posterior that a segment begins there, not to 1.  Categories
    as for `arc_posteriors` (the full out-CSR; self-loops count nothing).'''
    if not (per_frame or per_utt or total):
        raise ValueError('duration_arc_posteriors: none of per_frame, per_utt and total is '
                         'asked for')
    arcs, inits = check_arc_categories(batch.n_arcs, batch.n_states, arc_cat, init_cat, n_cat,
                                       per_frame, per_utt or total)
    n_cat = int(n_cat)
    D, S_total, log_dur, leave_w, ws = _duration_args(batch, pc_llhs, log_dur, leave_w,
                                                      'beer_hsmm_arcs_scratch_doubles')
    duration_arcs_route(batch, D, n_cat, per_frame)
    dt, dev = batch.dtype, batch.device
    dcode = _hip.dtype_code(dt)
    amap, keep = _arc_map(batch, arcs, inits)               # (`keep` lives until the call)
    gamma, evidence, counts, entry, g0 = _duration_outputs(batch, S_total, D, want_counts)
    frame = torch.empty(batch.n_frames, n_cat, dtype=dt, device=dev) if per_frame else None
    utt = torch.empty(batch.nutt, n_cat, dtype=torch.float64, device=dev) if per_utt else None
    tot = torch.zeros(n_cat, dtype=torch.float64, device=dev) if total else None
    _hip.call('beer_hsmm_arc_posteriors', dcode, batch.ref(), _hip.ptr(pc_llhs),
              _hip.ptr(log_dur), _hip.ptr(leave_w), D, S_total, ctypes.byref(amap), n_cat,
              _hip.ptr(ws), _hip.ptr(gamma), _hip.ptr(evidence), _hip.ptr(counts),
              _hip.ptr(entry), _hip.ptr(g0), _hip.ptr(frame), _hip.ptr(utt), _hip.ptr(tot))
    return gamma, evidence, counts, entry, g0, frame, utt, tot


def duration_viterbi(batch, pc_llhs, log_dur, leave_w=None, map_pdf=False):
    '''(path int64 [n_frames] -- state indices, or pdf ids with `map_pdf` --, score [nutt] fp64):
    the best segmentation under explicit durations (`beer_hsmm_viterbi`).  An utterance without
    a finite path has the score -inf and a path of -1.'''
    D, S_total, log_dur, leave_w, ws = _duration_args(batch, pc_llhs, log_dur, leave_w)
    dev = batch.device
    path = torch.empty(batch.n_frames, dtype=torch.int64, device=dev)
    score = torch.empty(batch.nutt, dtype=torch.float64, device=dev)
    _hip.call('beer_hsmm_viterbi', _hip.dtype_code(batch.dtype), batch.ref(), _hip.ptr(pc_llhs),
              _hip.ptr(log_dur), _hip.ptr(leave_w), D, S_total, _hip.ptr(ws), _hip.ptr(path),
              _hip.ptr(score), 1 if map_pdf else 0)
    return path, score


def path_posteriors(batch, path, want_xi=False):
    '''(gamma one-hot packed, xi_sum [S, S] fp64 or None, gamma0_sum [S] fp64 or None) of a state
    path; xi / gamma0 need a batch sharing one graph.'''
    dt, dev = batch.dtype, batch.device
    path = _hip.on_device(torch.as_tensor(path)).to(torch.int64).contiguous()
    gamma = torch.empty(batch.n_elems, dtype=dt, device=dev)
    xi = g0 = None
    if want_xi:
        if not batch.shared_graph:
            raise ValueError('transition counts of a path need one graph for the whole batch')
        S = batch.n_states[0]
        xi = torch.zeros(S, S, dtype=torch.float64, device=dev)
        g0 = torch.zeros(S, dtype=torch.float64, device=dev)
    _hip.call('beer_hmm_path_posteriors', _hip.dtype_code(dt), batch.ref(), _hip.ptr(path),
              _hip.ptr(gamma), _hip.ptr(xi), _hip.ptr(g0))
    return gamma, xi, g0


def scatter(batch, pc_llhs, gamma, S_total, scale=1., want_resps=True, want_exp_llh=True,
            utt_llh=None):
    '(state_resps [n_frames, S_total] or None, exp_llh [n_frames] or None).'
    dt, dev = batch.dtype, batch.device
    sr = torch.zeros(batch.n_frames, S_total, dtype=dt, device=dev) if want_resps else None
    el = torch.empty(batch.n_frames, dtype=dt, device=dev) if want_exp_llh else None
    _hip.call('beer_hmm_scatter', _hip.dtype_code(dt), batch.ref(), S_total,
              _hip.ptr(pc_llhs), _hip.ptr(gamma), float(scale), _hip.ptr(sr), _hip.ptr(el),
              _hip.ptr(utt_llh))
    return sr, el


def segment_sum(values, frame_off_dev, nutt, out=None):
    'out[u] += sum of values over the frames of utterance u (fp64).'
    values = values.contiguous()
    if out is None:
        out = torch.zeros(nutt, dtype=torch.float64, device=values.device)
    _hip.call('beer_segment_sum', _hip.dtype_code(values.dtype), nutt,
              _hip.ptr(frame_off_dev), _hip.ptr(values), _hip.ptr(out))
    return out


class _Columns:
    'Minimal stand-in for a graph: only n_states / pdf ids matter for gather.'

    def __init__(self, order):
        self.pdf_id_mapping = [int(i) for i in order]
        self.n_states = len(self.pdf_id_mapping)
        self._dg = None

    def device_graph(self, dtype):
        if self._dg is None:
            self._dg = type('DG', (), {})()
            self._dg.n_states, self._dg.n_arcs = self.n_states, 0
            self._dg.n_in_seg = self._dg.n_out_seg = 0
            self._dg.lowdeg = None
            self._dg.struct = _hip.Graph(self.n_states, 0, 0, 0, *([None] * 15))
        return self._dg


def gather_columns(matrix, order):
    'matrix[:, order] on the GPU (modelset.py:140-146).'
    matrix = _hip.on_device(matrix)
    batch = HmmBatch([_Columns(order)], [0], [matrix.shape[0]], matrix.dtype)
    return gather(batch, matrix, 1.).view(matrix.shape[0], len(order))


def scatter_columns(resps, order, n_total):
    'out[:, order[i]] += resps[:, i] (repeated ids add, modelset.py:148-154).'
    resps = _hip.on_device(resps)
    batch = HmmBatch([_Columns(order)], [0], [resps.shape[0]], resps.dtype)
    flat = resps.reshape(-1)
    sr, _ = scatter(batch, flat, flat, n_total, 1., want_exp_llh=False)
    return sr
