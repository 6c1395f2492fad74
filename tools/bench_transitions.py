'''Learned transition probabilities at BASELINE config 3's shape (40 units x 3 states x 16
diagonal Gaussians, D = 40, float32, >= 1 M frames), the same phone loop with fixed and with
learned transitions:
  * ms per E-step (accumulate_elbo), per ROUND of mean-field groups (every group updated once:
    one iteration with fixed transitions, two with learned ones -- the emissions get one update
    per round either way) and per round as captured HIP graphs (CapturedIteration);
  * ms per fused forward-backward launch without and with the transition counts at three
    shapes: config 3 (120 states: two slots a lane, degree 2), the recipe's mix (one 5-state
    non-speech unit beside them: degree 4) and 57 units (175 states: four slots a lane).

    python tools/bench_transitions.py [--frames 1000000] [--steps 6] [--warmup 2]
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
from beer_amd.inference.batch import ShardStatics  # noqa: E402
from beer_amd.inference.captured import CapturedIteration  # noqa: E402

TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}] + \
    [{'start_id': s, 'end_id': e, 'trans_prob': p}
     for s in (1, 2, 3) for e, p in ((s, .75), (s + 1, .25))]
NON_SPEECH = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.0}] + \
    [{'start_id': 1, 'end_id': e, 'trans_prob': .25} for e in (1, 2, 3, 4)] + \
    [{'start_id': s, 'end_id': e, 'trans_prob': .25} for s in (2, 3, 4) for e in (2, 3, 4, 5)] + \
    [{'start_id': 5, 'end_id': 5, 'trans_prob': .75}, {'start_id': 5, 'end_id': 6, 'trans_prob': .25}]


def build(learned, P=40, n_ns=0, D=40, ncomp=16):
    torch.manual_seed(0)
    common = {'n_normal_per_state': ncomp, 'prior_strength': 1., 'noise_std': 1.,
              'cov_type': 'diagonal', 'shared_cov': False}
    conf = {'g': {'topology': TOPO, **common}, 'ns': {'topology': NON_SPEECH, **common}}
    grouped = {'g': [f'u{i}' for i in range(P)], 'ns': [f'n{i}' for i in range(n_ns)]}
    if not n_ns:
        del conf['ns'], grouped['ns']
    units, ems = hmm_cmds.build_units(conf, grouped, torch.zeros(D), torch.ones(D))
    names = [n for g in grouped.values() for n in g]
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet',
                               train_transitions=learned).float().cuda()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure_iteration(name, model, X, lens, steps, warmup):
    utts = (X, lens)
    groups = model.conjugate_bayesian_parameters(keepgroups=True)
    optim = beer.VBConjugateOptimizer(groups, 1.)
    n = len(optim.groups)
    statics = ShardStatics()

    def estep():
        optim.init_step()
        beer.accumulate_elbo(model, utts, datasize=len(X), statics=statics)

    def round_of_groups():
        for _ in range(n):
            optim.init_step()
            elbo = beer.accumulate_elbo(model, utts, datasize=len(X), statics=statics)
            elbo.backward()
            optim.step()

    e_ms = timed(estep, steps, warmup)
    r_ms = timed(round_of_groups, steps, warmup)
    it = CapturedIteration(model, beer.VBConjugateOptimizer(groups, 1.), utts, datasize=len(X))

    def captured_round():
        for _ in range(n):
            it()
    c_ms = timed(captured_round, steps, warmup + 2)
    out = {'transitions': name, 'frames': int(len(X)), 'utterances': len(lens), 'groups': n,
           'ms_per_estep': round(e_ms, 3), 'ms_per_round_of_groups': round(r_ms, 3),
           'ms_per_round_captured': round(c_ms, 3), 'captured_mode': it.mode}
    print(json.dumps(out), flush=True)
    return out


def measure_launch(shape, P, n_ns, X, lens, steps, warmup):
    out = {'shape': shape}
    for learned in (False, True):
        model = build(learned, P, n_ns)
        pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
        batch = hk.HmmBatch([model.graph], [0] * len(lens), lens, pc_all.dtype)
        assert hk.fused_ok(batch)
        out['states'] = batch.n_states[0]
        out['max_degree'] = batch.struct.max_degree
        ms = timed(lambda: hk.posteriors_fused(batch, pc_all, 1., want_counts=True,
                                               want_transitions=learned), steps, warmup)
        out['ms_with_counts' if learned else 'ms_without'] = round(ms, 3)
    out['overhead_pct'] = round(100 * (out['ms_with_counts'] / out['ms_without'] - 1), 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    lens = []
    while sum(lens) < args.frames:
        lens.append(int(rng.randint(100, 600)))
    X = torch.from_numpy(rng.randn(sum(lens), 40).astype(np.float32) * 1.5).cuda()
    print(json.dumps({'device': torch.cuda.get_device_properties(0).name}), flush=True)
    fixed = measure_iteration('fixed', build(False), X, lens, args.steps, args.warmup)
    learned = measure_iteration('learned', build(True), X, lens, args.steps, args.warmup)
    print(json.dumps({k.replace('ms_per', 'overhead_pct'): round(100 * (learned[k] / fixed[k] - 1), 2)
                      for k in ('ms_per_estep', 'ms_per_round_of_groups',
                                'ms_per_round_captured')}), flush=True)
    for shape, P, n_ns in (('config3', 40, 0), ('recipe_mix', 40, 1), ('four_slots', 55, 2)):
        measure_launch(shape, P, n_ns, X, lens, args.steps, args.warmup)


if __name__ == '__main__':
    main()
