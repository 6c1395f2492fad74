'''Explicit state durations (`hk.duration_forward_backward`, `hk.duration_viterbi`) beside the HMM
forward-backward (`hk.forward_backward`) on the same batch and per-state log-likelihoods, and
beside them the arc posteriors under durations (`hk.duration_arc_posteriors`: the unit-start
categories with the per-frame rows, and the P^2 bigram categories with the batch total alone), in
one process, float32: BASELINE config 3's phone loop (40 units x 3 states = 120 states, the pivot
declared as a hub), about 1 M frames in 300-frame utterances, at D = 16, 32 and 64; then one
`accumulate_elbo` iteration of that loop with and without durations.

ms per call by HIP events, warm-ups dropped: median (min .. max), with the shader clock under load
(benchlib.timers.ClockProbe), the route, the ratio to the HMM kernel and the (state, duration,
frame) terms per second of either direction (forward-backward walks every term twice).

    python tools/bench_durations.py [--frames 999900] [--steps 5] [--warmup 2] [--durations 16 32 64]
'''

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import beer_amd as beer  # noqa: E402
from beer_amd import hmm_kernels as hk  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds  # noqa: E402
from beer_amd.models.sequence import unit_start_categories  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_arc_posteriors import N_PHONES, TOPO  # noqa: E402
from tools.bench_sample_paths import event_ms  # noqa: E402


def loop_model(max_duration=0):
    'Config 3\'s loop as a model (one Gaussian a state on 2-d frames), with durations or not.'
    conf = {'g': {'topology': [{'start_id': s, 'end_id': e, 'trans_prob': p} for s, e, p in TOPO],
                  'n_normal_per_state': 1, 'prior_strength': 1., 'noise_std': 1.,
                  'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(N_PHONES)]
    torch.manual_seed(1)
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(2), torch.ones(2))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet',
                               max_duration=max_duration).float().cuda()


def bigram_categories(model):
    '(arc_cat, init_cat): i P + j on the arcs end_i -> start_j of the loop, -1 elsewhere.'
    graph = model.graph
    src, dst = (np.asarray(a, dtype=np.int64) for a in graph.out_arcs())
    ends, starts = list(model.end_pdf.values()), list(model.start_pdf.values())
    P = len(starts)
    end_of = np.full(graph.n_states, -1, dtype=np.int64)
    end_of[ends] = np.arange(P)
    start_of = np.full(graph.n_states, -1, dtype=np.int64)
    start_of[starts] = np.arange(P)
    cat = np.where((end_of[src] >= 0) & (start_of[dst] >= 0) & (src != dst),
                   end_of[src] * P + start_of[dst], -1)
    return cat.astype(np.int32), np.full(graph.n_states, -1, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=999_900)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--durations', type=int, nargs='+', default=[16, 32, 64])
    args = ap.parse_args()
    n_utts = max(args.frames // 300, 1)
    lens = [300] * n_utts
    probe = ClockProbe(torch.device('cuda'))
    name = torch.cuda.get_device_properties(0).name
    gen = torch.Generator(device='cuda').manual_seed(2)
    plain = loop_model()
    batch = hk.HmmBatch([plain.graph], [0] * n_utts, lens, torch.float32)
    S = batch.n_states[0]
    pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
    print(json.dumps({'device': name, 'states': S, 'arcs': batch.struct.max_arcs,
                      'hub_members': batch.struct.max_hub_members, 'frames': batch.n_frames,
                      'utterances': n_utts}), flush=True)
    seen = {}

    def report(call, fn, route=None, beside=None, **more):
        ms = event_ms(fn, args.steps, args.warmup)
        med = ms[len(ms) // 2]
        clock = probe.measure(fn, med)
        if beside is not None:
            more['ratio_to_' + beside.split()[0]] = round(med / seen[beside], 2)
        seen[call] = med
        print(json.dumps({'call': call, 'route': route, 'ms_median': round(med, 3),
                          'ms_min': round(ms[0], 3), 'ms_max': round(ms[-1], 3),
                          'steps': args.steps, 'mhz_under_load': round(clock['under_load']['mhz']),
                          'mhz_idle': round(clock['idle']['mhz']), **more}), flush=True)
        return med

    report('hmm forward_backward', lambda: hk.forward_backward(batch, pc_llhs),
           hex(hk._route(batch.dtype, batch.struct, 0, 1)))
    report('hmm viterbi', lambda: hk.viterbi(batch, pc_llhs))
    for D in args.durations:
        model = loop_model(D)
        log_dur, leave_w = model._duration_tables()
        route = hex(hk.duration_route(batch, D))
        terms = batch.n_frames * S * D
        med = report(f'duration_forward_backward D={D}',
                     lambda: hk.duration_forward_backward(batch, pc_llhs, log_dur, leave_w),
                     route, beside='hmm forward_backward')
        print(json.dumps({'D': D, 'fb_gigaterms_per_s': round(2 * terms / med / 1e6, 2)}), flush=True)
        if hasattr(hk, 'duration_arc_posteriors'):
            # (the categories are uploaded once: the calls below time the launch, not the copies)
            P = len(model.start_pdf)
            for what, (arcs, inits), n_cat, kw in (
                    ('unit starts, frame_out', unit_start_categories(
                        model.graph, model.start_pdf, model.end_pdf), P, dict(per_frame=True)),
                    ('bigram, total_out', bigram_categories(model), P * P,
                     dict(per_frame=False, total=True))):
                arcs, inits = torch.from_numpy(arcs).cuda(), torch.from_numpy(inits).cuda()
                report(f'duration_arc_posteriors D={D} ({what})',
                       lambda: hk.duration_arc_posteriors(batch, pc_llhs, log_dur, leave_w, arcs,
                                                          inits, n_cat, **kw),
                       hex(hk.duration_arcs_route(batch, D, n_cat, kw['per_frame'])),
                       beside=f'duration_forward_backward D={D}', n_cat=n_cat)
        med = report(f'duration_viterbi D={D}',
                     lambda: hk.duration_viterbi(batch, pc_llhs, log_dur, leave_w),
                     route, beside='hmm viterbi')
        print(json.dumps({'D': D, 'viterbi_gigaterms_per_s': round(terms / med / 1e6, 2)}),
              flush=True)
        del model

    # one VB E-step of the shard through the model
    rng = np.random.RandomState(3)
    X = torch.from_numpy(rng.randn(sum(lens), 2).astype(np.float32)).cuda()
    report('accumulate_elbo without durations',
           lambda: beer.accumulate_elbo(plain, (X, lens), datasize=sum(lens)))
    for D in args.durations[:2]:
        model = loop_model(D)
        report(f'accumulate_elbo D={D}',
               lambda: beer.accumulate_elbo(model, (X, lens), datasize=sum(lens)),
               beside='accumulate_elbo without durations')


if __name__ == '__main__':
    main()
