'''Learned transition probabilities trained against alignment graphs, at the recipe's monophone
model (recipes/aud/conf/hmm.yml: one 5-state non-speech unit x 10 diagonal Gaussians + 40
three-state units x 4, D = 40, float32): alignment graphs of random transcriptions of 20-60
phones over about 1 M frames, the same `GraphSet` for
  * fixed transitions: the fused forward-backward launch and the E-step (accumulate_elbo) as
    they were -- the yardstick;
  * learned transitions on the bound set: the refresh of the bound image (E[ln a] by category)
    + the fused launch with the counts by category, and the E-step with both.
One JSON line per model, then the overheads and the shader clock under load.

    python tools/bench_transitions_aligned.py [--frames 1000000] [--steps 10] [--warmup 3]
'''

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import beer_amd as beer  # noqa: E402
from beer_amd import hmm_kernels as hk  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds  # noqa: E402
from beer_amd.graph import compile_alignments  # noqa: E402
from beer_amd.inference.batch import ShardStatics  # noqa: E402
from benchlib.recipe import hmm_conf  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402

D = 40


def build(learned, n_speech=40):
    '(the recipe\'s phone loop on the GPU, its units).'
    torch.manual_seed(0)
    groups = {g['group_name']: g for g in hmm_conf()}
    names = {'non-speech-unit': ['sil'], 'speech-unit': [str(i) for i in range(n_speech)]}
    units, ems = hmm_cmds.build_units(groups, names, torch.zeros(D), torch.ones(D))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(list(units)), units)
    model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet', train_transitions=learned)
    return model.float().cuda(), units


def corpus(units, frames, rng):
    '(transcriptions of 20-60 phones between two `sil`, lengths): 4-12 frames a state.'
    speech = [n for n in units if n != 'sil']
    seqs, lens = [], []
    while sum(lens) < frames:
        seq = ['sil'] + [speech[i] for i in rng.randint(len(speech), size=rng.randint(18, 59))] + \
            ['sil']
        states = 3 * (len(seq) - 2) + 10
        seqs.append(seq)
        lens.append(states * int(rng.randint(4, 13)))
    return seqs, lens


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(name, model, graphs, X, lens, steps, warmup):
    learned = model.transitions is not None
    bound = graphs[0]._set if learned else None
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    batch = hk.HmmBatch(graphs, list(range(len(graphs))), lens, pc_all.dtype)
    assert hk.fused_ok(batch)

    def launch():
        if learned:
            # (the refresh as the E-step runs it after an update: the token of the last one dropped)
            for p in model.transitions.parameters_of_groups():
                p.posterior.__dict__['_memo'] = {}
            bound.refresh(pc_all.dtype)
        hk.posteriors_fused(batch, pc_all, 1., want_transitions=learned)

    def recursion():
        hk.posteriors_fused(batch, pc_all, 1., want_transitions=learned)

    statics = ShardStatics()

    def estep():
        beer.accumulate_elbo(model, (X, lens), datasize=len(X), inference_graphs=graphs,
                             statics=statics)

    out = {'transitions': name, 'frames': int(len(X)), 'utterances': len(lens),
           'max_states': max(batch.n_states), 'max_degree': batch.struct.max_degree,
           'ms_fused_launch': round(timed(launch, steps, warmup), 4),
           'ms_fused_recursion_only': round(timed(recursion, steps, warmup), 4),
           'ms_per_estep': round(timed(estep, steps, warmup), 4)}
    out['clock'] = ClockProbe(X.device).measure(estep, out['ms_per_estep'])['under_load']['mhz']
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=['fixed', 'learned'], help='one model only (for a profile)')
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    print(json.dumps({'device': torch.cuda.get_device_properties(0).name}), flush=True)
    results = {}
    for name in ('fixed', 'learned'):
        if args.only and args.only != name:
            continue
        model, units = build(name == 'learned')
        if not results:
            seqs, lens = corpus(units, args.frames, rng)
            X = torch.from_numpy(rng.randn(sum(lens), D).astype(np.float32) * 1.5).cuda()
        gset = compile_alignments(seqs, units)
        graphs = list(model.bind_alignment_graphs(gset)) if name == 'learned' else list(gset)
        results[name] = measure(name, model, graphs, X, lens, args.steps, args.warmup)
    if len(results) == 2:
        print(json.dumps({f'overhead_pct_{k[3:]}': round(
            100 * (results['learned'][k] / results['fixed'][k] - 1), 2)
            for k in ('ms_fused_launch', 'ms_fused_recursion_only', 'ms_per_estep')}), flush=True)


if __name__ == '__main__':
    main()
