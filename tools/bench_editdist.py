'''What minimum-Bayes-risk selection adds to a search, in one process: `beer_unit_sequences` and
`beer_edit_distance` beside the `viterbi_nbest` / `sample_paths` call that produced the paths.

BASELINE config 3's phone loop (40 units x 3 states), 3333 utterances of 300 frames, float32,
random per-state log-likelihoods; the 16 best paths and 64 posterior draws of every utterance;
their unit sequences; the N (N - 1) / 2 pairs of every utterance -- 0.4 M and 6.7 M pairs -- with
and without `ops`.  For the distances two figures: the bare launch on the pairs as they come (one
launch, its route from the maxima of all the pairs) and `kernels.edit_distance` (the pairs
ordered and launched by class, results back in the caller's order).  ms by HIP events, the median
of `--steps` runs after `--warmup`, cells (len_a * len_b) per second, and the shader clock under
load (benchlib.timers.ClockProbe).

    python tools/bench_editdist.py [--utts 3333] [--frames 300] [--steps 5] [--warmup 2]
'''

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beer_amd import _hip, hmm_kernels as hk, kernels  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds  # noqa: E402
from beer_amd.scoring import _unit_table  # noqa: E402
from benchlib.shapes import N_PHONES, TOPO  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_sample_paths import event_ms  # noqa: E402


def loop_model():
    conf = {'g': {'topology': [{'start_id': s, 'end_id': e, 'trans_prob': p} for s, e, p in TOPO],
                  'n_normal_per_state': 1, 'prior_strength': 1., 'noise_std': 1.,
                  'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(N_PHONES)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(2), torch.ones(2))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet').float().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=3333)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    dev = torch.device('cuda')
    model = loop_model()
    table = _unit_table(model).to(dev)
    U, T = args.utts, args.frames
    batch = hk.HmmBatch([model.graph], [0] * U, [T] * U, torch.float32)
    gen = torch.Generator(device='cuda').manual_seed(2)
    # smooth log-likelihoods: units that last a few frames, as speech has them
    pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * .7
    probe = ClockProbe(dev)
    print(json.dumps({'device': torch.cuda.get_device_properties(0).name, 'utterances': U,
                      'frames': batch.n_frames, 'states': batch.struct.max_states}), flush=True)

    def report(name, fn, **more):
        ms = event_ms(fn, args.steps, args.warmup)
        med = ms[len(ms) // 2]
        clock = probe.measure(fn, med)
        cells = more.pop('cells', None)
        print(json.dumps({'call': name, 'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
                          'ms_max': round(ms[-1], 3),
                          **({'gcells_per_s': round(cells / med / 1e6, 2)} if cells else {}),
                          'mhz_under_load': round(clock['under_load']['mhz']), **more}), flush=True)
        return med

    searches = (('viterbi_nbest k=16', 16,
                 lambda: hk.viterbi_nbest(batch, pc_llhs, 16, map_pdf=True)[0]),
                ('sample_paths n=64', 64,
                 lambda: hk.sample_paths(batch, pc_llhs, nsamples=64, generator=gen, map_pdf=True)))
    for name, N, search in searches:
        paths = search()                                        # [N, n_frames] pdf ids
        report(name, search)
        sym = paths.reshape(-1)
        start = (torch.arange(N).unsqueeze(1) * batch.n_frames + torch.arange(U) * T).reshape(-1)
        start, lens = start.to(dev), torch.full((N * U,), T, dtype=torch.int32, device=dev)
        units = torch.empty(sym.numel(), dtype=torch.int32, device=dev)
        n_units = torch.empty(N * U, dtype=torch.int32, device=dev)

        def collapse():
            _hip.call('beer_unit_sequences', _hip.ptr(sym), _hip.ptr(start), _hip.ptr(lens), N * U,
                      _hip.ptr(table), table.numel(), _hip.ptr(units), _hip.ptr(n_units), None)
        collapse()
        counts = n_units.clamp(min=0)
        report(f'unit_sequences of {N} paths', collapse, cells=float(sym.numel()),
               units_per_path=round(float(counts.float().mean()), 1))
        i, j = torch.triu_indices(N, N, 1, device=dev)
        seq = torch.arange(U, device=dev).unsqueeze(1)
        pair_a = (i.unsqueeze(0) * U + seq).reshape(-1).to(torch.int32)
        pair_b = (j.unsqueeze(0) * U + seq).reshape(-1).to(torch.int32)
        la, lb = counts[pair_a.long()].long(), counts[pair_b.long()].long()
        cells = float((la * lb).sum())
        short, long_ = int(torch.minimum(la, lb).max()), int(torch.maximum(la, lb).max())
        dist = torch.empty(pair_a.numel(), dtype=torch.int32, device=dev)
        moves = torch.empty(pair_a.numel(), 3, dtype=torch.int32, device=dev)
        for ops in (False, True):
            route = hex(kernels.edit_distance_route(short, long_, ops))
            report(f'edit_distance launch, N={N}' + (' ops' if ops else ''),
                   lambda: kernels.edit_distance_launch(units, start, counts, pair_a, pair_b, short,
                                                        long_, dist, moves if ops else None),
                   cells=cells, pairs=pair_a.numel(), route=route, max_short=short, max_long=long_)
            report(f'kernels.edit_distance, N={N}' + (' ops' if ops else ''),
                   lambda: kernels.edit_distance(units, start, counts, pair_a, pair_b, ops=ops),
                   cells=cells, pairs=pair_a.numel())
        del paths, sym, units, dist, moves


if __name__ == '__main__':
    main()
