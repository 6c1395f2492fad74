'''Posterior path sampling beside Viterbi at BASELINE config 3's phone loop (40 units x 3 states
= 120 states, float32), on the bench's utterance lengths (U[200, 400], seed 2), in one process:
ms per `hk.sample_paths` launch pair at nsamples = 1 and 8 and per `hk.viterbi` launch on the
same batch and per-state log-likelihoods, by HIP events, warm-ups dropped, with the shader
clock under load (benchlib.timers.ClockProbe).

    python tools/bench_sample_paths.py [--frames 1000000] [--steps 10] [--warmup 3]
'''

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beer_amd import _hip, hmm_kernels as hk  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds  # noqa: E402
from benchlib.shapes import N_PHONES, TOPO  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402


def loop_graph():
    'The compiled graph of config 3\'s loop (its emissions do not matter here: one Gaussian a state).'
    conf = {'g': {'topology': [{'start_id': s, 'end_id': e, 'trans_prob': p} for s, e, p in TOPO],
                  'n_normal_per_state': 1, 'prior_strength': 1., 'noise_std': 1.,
                  'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(N_PHONES)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(2), torch.ones(2))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet').float().cuda().graph


def corpus(total_frames):
    rng = np.random.RandomState(2)
    lengths = []
    while sum(lengths) < total_frames:
        lengths.append(int(rng.randint(200, 401)))
    return lengths


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    evs[0].record()
    for i in range(steps):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    graph = loop_graph()
    lens = corpus(args.frames)
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, torch.float32)
    S = batch.n_states[0]
    gen = torch.Generator(device='cuda').manual_seed(2)
    pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
    print(json.dumps({'device': torch.cuda.get_device_properties(0).name, 'states': S,
                      'arcs': batch.struct.max_arcs, 'frames': batch.n_frames,
                      'utterances': len(lens)}), flush=True)
    # the workspaces are allocated once: the launches alone are timed
    bt = torch.empty(batch.n_elems, dtype=torch.int32, device='cuda')
    vpath = torch.empty(batch.n_frames, dtype=torch.int64, device='cuda')
    alpha = torch.empty(batch.n_elems, dtype=torch.float64, device='cuda')
    code = _hip.dtype_code(torch.float32)

    def viterbi():
        _hip.call('beer_hmm_viterbi', code, batch.ref(), _hip.ptr(pc_llhs), _hip.ptr(bt),
                  _hip.ptr(vpath), 0)

    def sampler(n):
        U = torch.rand(n, batch.n_frames, dtype=torch.float64, device='cuda', generator=gen)
        path = torch.empty(n, batch.n_frames, dtype=torch.int64, device='cuda')

        def run():
            _hip.call('beer_hmm_sample_paths', code, batch.ref(), _hip.ptr(pc_llhs), _hip.ptr(U),
                      n, _hip.ptr(alpha), _hip.ptr(path), 0)
        return run

    probe = ClockProbe(torch.device('cuda'))
    for name, fn, route in (('viterbi', viterbi, None),
                            ('sample_paths nsamples=1', sampler(1), hk.sample_route(batch, 1)),
                            ('sample_paths nsamples=8', sampler(8), hk.sample_route(batch, 8))):
        ms = event_ms(fn, args.steps, args.warmup)
        med = ms[len(ms) // 2]
        clock = probe.measure(fn, med)
        out = {'call': name, 'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
               'ms_max': round(ms[-1], 3), 'steps': args.steps,
               'mhz_under_load': round(clock['under_load']['mhz']),
               'mhz_idle': round(clock['idle']['mhz'])}
        if route is not None:
            out['route'] = hex(route)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
