'''Segment posteriors (`hk.segment_posteriors`, max_dur 100) beside their two neighbours on the same
batch and per-state log-likelihoods, in one process, float32: the arc posteriors per frame
(`hk.arc_posteriors(per_frame=True)`, beside the trellis kernel) and the unit segment lattice
(`hk.segment_margins`, beam 10, beside the whole call), on tools/bench_segments.py's two batches:

 * BASELINE config 3's phone loop (40 units x 3 states = 120 states), about 1 M frames in
   300-frame utterances;
 * alignment graphs of the reference's recipe shapes, every utterance its own graph, 300 frames
   each.

`min_post` is chosen per batch so that the number of entries is that of the beam: the n-th largest
start posterior, n the entries `segment_margins` keeps (both counts are printed).  The whole call
with the closures built beforehand, and its three parts alone: the trellis kernel, the entry
selection (`torch.nonzero`, which waits for the device, and the offsets), the expand kernel.  ms per
call by HIP events, warm-ups dropped: median (min .. max), with the shader clock under load
(benchlib.timers.ClockProbe), the route, the entries and the kept segments per utterance, and the
expand kernel's picoseconds per entry and step.

    python tools/bench_segment_posteriors.py [--frames 999900] [--steps 10] [--warmup 3]
                                             [--beam 10] [--max-dur 100]
'''

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beer_amd import _hip, hmm_kernels as hk  # noqa: E402
from beer_amd.models.sequence import unit_start_categories  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_arc_posteriors import alignment_graphs, loop_model  # noqa: E402
from tools.bench_sample_paths import event_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=999_900)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--beam', type=float, default=10.)
    ap.add_argument('--max-dur', type=int, default=100)
    args = ap.parse_args()
    n_utts = max(args.frames // 300, 1)
    rng = np.random.RandomState(2)
    loop = loop_model()
    recipe_model, graphs = alignment_graphs(n_utts, rng)
    lens = [300] * n_utts
    loop_cats = unit_start_categories(loop.graph, loop.start_pdf, loop.end_pdf)
    ali_cats = [unit_start_categories(g, recipe_model.start_pdf, recipe_model.end_pdf)
                for g in graphs]
    runs = (('phone loop', hk.HmmBatch([loop.graph], [0] * n_utts, lens, torch.float32),
             [loop_cats[0]], [loop_cats[1]], len(loop.start_pdf)),
            ('alignment graphs', hk.HmmBatch(graphs, list(range(n_utts)), lens, torch.float32),
             [c[0] for c in ali_cats], [c[1] for c in ali_cats], len(recipe_model.start_pdf)))
    gen = torch.Generator(device='cuda').manual_seed(2)
    probe = ClockProbe(torch.device('cuda'))
    name = torch.cuda.get_device_properties(0).name
    dev = torch.device('cuda', torch.cuda.current_device())
    beam, max_dur = args.beam, args.max_dur

    for what, batch, arc_cats, init_cats, n_cat in runs:
        pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
        # the categories on the device once, as a caller that keeps them would
        arcs = torch.from_numpy(np.concatenate(arc_cats)).cuda()
        inits = torch.from_numpy(np.concatenate(init_cats)).cuda()
        smap = hk.segment_map(batch.source_graphs, arc_cats, init_cats, n_cat)
        route = hk.segposts_route(batch, n_cat, smap.max_closure)

        # min_post: as many entries as the beam keeps
        lattice = hk.segment_margins(batch, pc_llhs, arcs, inits, n_cat, beam, max_dur, seg_map=smap)
        beam_entries = len(lattice[2])
        beam_segments = len(hk.segments_within(lattice[2], lattice[3], lattice[4], beam)[0])
        del lattice
        starts = hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat)[0]
        positive = starts[starts > 0]
        min_post = 0. if beam_entries >= len(positive) else \
            float(torch.sort(positive, descending=True)[0][max(beam_entries - 1, 0)])
        del starts, positive
        out = hk.segment_posteriors(batch, pc_llhs, arcs, inits, n_cat, min_post, max_dur, seg_map=smap)
        kept = hk.segments_above(out[2], out[3], out[4], min_post)[0]
        counts = {'entries_per_utterance': round(len(out[2]) / n_utts, 1),
                  'segments_per_utterance': round(len(kept) / n_utts, 1),
                  'seg_megabytes': round(out[4].numel() * out[4].element_size() / 2 ** 20, 1)}
        print(json.dumps({'batch': what, 'device': name, 'max_states': batch.struct.max_states,
                          'max_arcs': batch.struct.max_arcs, 'frames': batch.n_frames,
                          'utterances': n_utts, 'elements': batch.n_elems, 'categories': n_cat,
                          'max_closure': smap.max_closure, 'team': _hip.segposts_team(route),
                          'beam': beam, 'beam_entries': beam_entries,
                          'beam_segments': beam_segments, 'min_post': min_post,
                          'min_post_entries': len(out[2]), 'min_post_segments': len(kept),
                          'max_dur': max_dur}), flush=True)
        del out, kept
        seen = {}

        def report(call, fn, route, beside=None, **more):
            ms = event_ms(fn, args.steps, args.warmup)
            med = ms[len(ms) // 2]
            clock = probe.measure(fn, med)
            if beside is not None:
                more['ratio_to_' + beside.strip().split()[0]] = round(med / seen[beside], 2)
            seen[call] = med
            print(json.dumps({'batch': what, 'call': call, 'route': route,
                              'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
                              'ms_max': round(ms[-1], 3), 'steps': args.steps,
                              'mhz_under_load': round(clock['under_load']['mhz']),
                              'mhz_idle': round(clock['idle']['mhz']), **more}), flush=True)

        report('arc_posteriors per frame', lambda: hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat),
               hex(hk.arcs_route(batch, n_cat, True)))
        report('segment_margins', lambda: hk.segment_margins(batch, pc_llhs, arcs, inits, n_cat, beam,
                                                             max_dur, seg_map=smap),
               hex(hk.segments_route(batch, n_cat, smap.max_closure)))
        report('segment_posteriors', lambda: hk.segment_posteriors(batch, pc_llhs, arcs, inits, n_cat,
                                                                   min_post, max_dur, seg_map=smap),
               hex(route), beside='segment_margins', **counts)

        # the three parts alone, on buffers of their own
        dcode = _hip.dtype_code(batch.dtype)
        state_off = np.concatenate([[0], np.cumsum(batch.n_states)[:-1]]).astype(np.int64)
        arc_off = np.concatenate([[0], np.cumsum(batch.n_arcs)[:-1]]).astype(np.int64)
        up = _hip.upload({'arc_off': torch.from_numpy(arc_off),
                          'state_off': torch.from_numpy(state_off)}, dev)
        amap = _hip.ArcMap(arcs.data_ptr(), inits.data_ptr(), up['arc_off'].data_ptr(),
                           up['state_off'].data_ptr())
        alpha = torch.empty(batch.n_elems, dtype=torch.float64, device=dev)
        y = torch.empty_like(alpha)
        norm = torch.empty(batch.n_frames, dtype=torch.float64, device=dev)
        starts = torch.empty(batch.n_frames, n_cat, dtype=batch.dtype, device=dev)
        evidence = torch.empty(batch.nutt, dtype=torch.float64, device=dev)

        def trellis():
            _hip.call('beer_hmm_segpost_trellis', dcode, batch.ref(), _hip.ptr(pc_llhs),
                      ctypes.byref(amap), n_cat, _hip.ptr(alpha), _hip.ptr(y), _hip.ptr(norm),
                      _hip.ptr(starts), _hip.ptr(evidence))

        def select():
            at = torch.nonzero((starts >= min_post) & (starts > 0))
            frame = at[:, 0].contiguous()
            return frame, at[:, 1].to(torch.int32), \
                torch.searchsorted(frame, batch.bufs['frame_off'])

        report('  trellis kernel', trellis, hex(route), beside='arc_posteriors per frame')
        report('  entry selection (nonzero)', select, None)
        frame, cat, off = select()
        seg = torch.empty(len(frame), max_dur, dtype=batch.dtype, device=dev)
        sm = smap.struct(dev)

        def expand():
            _hip.call('beer_hmm_segment_posteriors', dcode, batch.ref(), _hip.ptr(pc_llhs),
                      ctypes.byref(sm), n_cat, _hip.ptr(alpha), _hip.ptr(y), _hip.ptr(norm),
                      _hip.ptr(evidence), _hip.ptr(frame), _hip.ptr(cat), _hip.ptr(off), len(frame),
                      max_dur, _hip.ptr(seg))

        report('  expand kernel', expand, hex(route), entries=len(frame), steps_per_entry=max_dur)
        print(json.dumps({'batch': what, 'expand_ps_per_entry_and_step':
                          round(seen['  expand kernel'] * 1e9 / max(len(frame) * max_dur, 1), 1)}),
              flush=True)
        del alpha, y, norm, seg, starts, frame, cat


if __name__ == '__main__':
    main()
