'''The forward log-evidence beside the only way the forward-backward kernels yield the same
numbers, `hk.forward_backward(..., want_lognorm=True)`, on the same batch and per-state
log-likelihoods, in one process, float32:

 * BASELINE config 3's phone loop (40 units x 3 states = 120 states), about 1 M frames in
   300-frame utterances;
 * alignment graphs of the reference's recipe shapes (tests/test_gpu_recipe.py: `sil p .. p sil`
   with 6 .. 11 three-state units around a five-state non-speech unit), every utterance its own
   graph, about 300 frames each.

ms per call by HIP events, warm-ups dropped, with the shader clock under load
(benchlib.timers.ClockProbe), the route each call took and the largest difference of the two
results.

    python tools/bench_log_evidence.py [--frames 1000000] [--steps 10] [--warmup 3]
'''

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import beer_amd as beer  # noqa: E402
from beer_amd import _hip, hmm_kernels as hk  # noqa: E402
from benchlib import recipe  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_sample_paths import event_ms, loop_graph  # noqa: E402


def alignment_graphs(n_utts, rng):
    'One alignment graph per utterance, as tests/test_gpu_recipe.py draws its transcriptions.'
    _, units = recipe.phone_loop(40, torch.zeros(2), torch.ones(2), noise_std=1., seed=1)
    speech = [n for n in units if not str(n).startswith('sil')]
    seqs = [['sil'] + [speech[i] for i in rng.randint(0, len(speech), rng.randint(6, 12))] + ['sil']
            for _ in range(n_utts)]
    return list(beer.graph.compile_alignments(seqs, units))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    n_utts = max(args.frames // 300, 1)
    rng = np.random.RandomState(2)
    loop = loop_graph()
    graphs = alignment_graphs(n_utts, rng)
    lens = [300] * n_utts
    batches = (('phone loop', hk.HmmBatch([loop], [0] * n_utts, lens, torch.float32)),
               ('alignment graphs', hk.HmmBatch(graphs, list(range(n_utts)), lens, torch.float32)))
    gen = torch.Generator(device='cuda').manual_seed(2)
    probe = ClockProbe(torch.device('cuda'))
    for what, batch in batches:
        pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
        fb_route = hk._route(torch.float32, batch.struct, 0, 1)
        print(json.dumps({'batch': what, 'device': torch.cuda.get_device_properties(0).name,
                          'max_states': batch.struct.max_states, 'max_arcs': batch.struct.max_arcs,
                          'frames': batch.n_frames, 'utterances': n_utts,
                          'elements': batch.n_elems}), flush=True)
        ours = hk.log_evidence(batch, pc_llhs)[0]
        theirs = hk.forward_backward(batch, pc_llhs, want_lognorm=True)[3].double()
        diff = float(((ours - theirs).abs() / theirs.abs()).max())
        calls = (('log_evidence', lambda: hk.log_evidence(batch, pc_llhs), hk.evidence_route(batch)),
                 ('log_evidence per_frame', lambda: hk.log_evidence(batch, pc_llhs, per_frame=True),
                  hk.evidence_route(batch)),
                 ('forward_backward want_lognorm',
                  lambda: hk.forward_backward(batch, pc_llhs, want_lognorm=True), fb_route))
        for name, fn, route in calls:
            ms = event_ms(fn, args.steps, args.warmup)
            med = ms[len(ms) // 2]
            clock = probe.measure(fn, med)
            print(json.dumps({'batch': what, 'call': name, 'route': hex(route),
                              'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
                              'ms_max': round(ms[-1], 3), 'steps': args.steps,
                              'mhz_under_load': round(clock['under_load']['mhz']),
                              'mhz_idle': round(clock['idle']['mhz']),
                              'largest_relative_difference': diff}), flush=True)


if __name__ == '__main__':
    main()
