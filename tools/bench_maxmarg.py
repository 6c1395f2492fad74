'''Viterbi max-marginals beside `hk.viterbi`, `hk.viterbi_nbest` at k = 4 and the per-frame
`hk.arc_posteriors` on the same batch and per-state log-likelihoods, in one process, float32:

 * BASELINE config 3's phone loop (40 units x 3 states = 120 states), about 1 M frames in
   300-frame utterances;
 * alignment graphs of the reference's recipe shapes (`sil p .. p sil` with 6 .. 11 three-state
   units around a five-state non-speech unit), every utterance its own graph, 300 frames each.

The max-marginals of the states alone, and of the states with the unit-start categories per
frame (what `unit_start_margins_batch` asks for, with the states besides).  ms per call by HIP
events, warm-ups dropped: median (min .. max), with the shader clock under load
(benchlib.timers.ClockProbe), the route each call took, and the ratios to the three neighbours.

    python tools/bench_maxmarg.py [--frames 999900] [--steps 10] [--warmup 3]
'''

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beer_amd import hmm_kernels as hk  # noqa: E402
from beer_amd.models.sequence import unit_start_categories  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_arc_posteriors import alignment_graphs, loop_model  # noqa: E402
from tools.bench_sample_paths import event_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=999_900)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
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

    for what, batch, arc_cats, init_cats, n_cat in runs:
        pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
        # the categories on the device once, as a caller that keeps them would
        arcs = torch.from_numpy(np.concatenate(arc_cats)).cuda()
        inits = torch.from_numpy(np.concatenate(init_cats)).cuda()
        print(json.dumps({'batch': what, 'device': name, 'max_states': batch.struct.max_states,
                          'max_arcs': batch.struct.max_arcs, 'frames': batch.n_frames,
                          'utterances': n_utts, 'elements': batch.n_elems,
                          'categories': n_cat}), flush=True)
        seen = {}

        def report(call, fn, route, rel=False, **more):
            ms = event_ms(fn, args.steps, args.warmup)
            med = ms[len(ms) // 2]
            clock = probe.measure(fn, med)
            if rel:         # against the three neighbours measured first
                more.update({f'ratio_to_{k.split()[0]}': round(med / v, 2)
                             for k, v in list(seen.items())[:3]})
            seen[call] = med
            print(json.dumps({'batch': what, 'call': call, 'route': route,
                              'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
                              'ms_max': round(ms[-1], 3), 'steps': args.steps,
                              'mhz_under_load': round(clock['under_load']['mhz']),
                              'mhz_idle': round(clock['idle']['mhz']), **more}), flush=True)

        report('viterbi', lambda: hk.viterbi(batch, pc_llhs), None)
        report('viterbi_nbest k=4', lambda: hk.viterbi_nbest(batch, pc_llhs, 4),
               hex(hk.nbest_route(batch, 4)))
        report('arc_posteriors per frame',
               lambda: hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat),
               hex(hk.arcs_route(batch, n_cat, True)))
        more = {}
        if what == 'phone loop':
            # (float32 Viterbi sums against float64 ones: its path may lie a rounding below)
            state = hk.max_marginals(batch, pc_llhs)[1]
            cells = torch.arange(batch.n_frames, device='cuda') * batch.struct.max_states + \
                hk.viterbi(batch, pc_llhs)
            more['lowest_margin_on_viterbi_path'] = float(state[cells].min())
        report('max_marginals states', lambda: hk.max_marginals(batch, pc_llhs),
               hex(hk.maxmarg_route(batch)), True, **more)
        report('max_marginals states + unit starts per frame',
               lambda: hk.max_marginals(batch, pc_llhs, arcs, inits, n_cat, per_frame=True),
               hex(hk.maxmarg_route(batch, n_cat, True, True, False)), True)
        report('max_marginals unit starts per frame alone',
               lambda: hk.max_marginals(batch, pc_llhs, arcs, inits, n_cat, states=False,
                                        per_frame=True),
               hex(hk.maxmarg_route(batch, n_cat, False, True, False)), True)


if __name__ == '__main__':
    main()
