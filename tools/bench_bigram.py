'''Bigram phone loop at the recipe's shape (100 units x 3 states x 4 diagonal Gaussians,
D = 39, float32, ~1 M frames): ms per VB iteration (accumulate_elbo + update) and per
forward-backward launch, for the fused bigram kernel, the general log-space path on the same
model (the block not declared), and the unigram PhoneLoop of the same size for context.

    python tools/bench_bigram.py [--frames 1000000] [--steps 5] [--warmup 2]
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
from benchlib.timers import ClockProbe  # noqa: E402

TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}] + \
    [{'start_id': s, 'end_id': e, 'trans_prob': .5}
     for s in (1, 2, 3) for e in (s, s + 1)]


def build(prior, P=100, D=39):
    torch.manual_seed(0)
    conf = {'g': {'topology': TOPO, 'n_normal_per_state': 4, 'prior_strength': 1.,
                  'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(P)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(D), torch.ones(D))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return hmm_cmds.phone_loop(graph, start, end, ems, prior).float().cuda()


def undeclare(model):
    '''The same model on the general path: the graph offers no image of its block, so
    `posteriors_bigram` takes the log-space forward-backward with the summed xi.'''
    model.graph.bigram_image = lambda dtype: None
    return model


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(name, model, X, lens, steps, warmup):
    utts = (X, lens)
    optim = beer.VBConjugateOptimizer(model.conjugate_bayesian_parameters(keepgroups=True), 1.)

    def iteration():
        optim.init_step()
        elbo = beer.accumulate_elbo(model, utts, datasize=len(X))
        elbo.backward()
        optim.step()

    it_ms = timed(iteration, steps, warmup)
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    batch = hk.HmmBatch([model.graph], [0] * len(lens), lens, pc_all.dtype)
    if isinstance(model, beer.BigramPhoneLoop):
        if hk.bigram_ok(batch):
            def fb():
                hk.posteriors_bigram(batch, pc_all, 1.)
        else:
            def fb():
                pc = hk.gather(batch, pc_all, 1.)
                hk.forward_backward(batch, pc, want_xi=True, dense_xi=True)
    elif hk.fused_ok(batch):
        def fb():
            hk.posteriors_fused(batch, pc_all, 1., want_counts=True)
    else:                   # (more states than the one-wave kernel takes: hub flows in log space)
        def fb():
            hk.forward_backward(batch, hk.gather(batch, pc_all, 1.), want_xi=True)
    fb_ms = timed(fb, steps, warmup)
    # the shader clock while the forward-backward launches run (bench.py's probe)
    clock = ClockProbe(X.device).measure(fb, fb_ms)
    print(json.dumps({'path': name, 'frames': int(len(X)), 'utterances': len(lens),
                      'ms_per_iteration': round(it_ms, 3), 'ms_per_fb_launch': round(fb_ms, 3),
                      'clock_mhz_idle': round(clock['idle']['mhz']),
                      'clock_mhz_under_load': round(clock['under_load']['mhz'])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    lens = []
    while sum(lens) < args.frames:
        lens.append(int(rng.randint(100, 600)))
    X = torch.from_numpy(rng.randn(sum(lens), 39).astype(np.float32) * 1.5).cuda()
    print(json.dumps({'device': torch.cuda.get_device_properties(0).name}), flush=True)
    measure('bigram_fused', build('dirichlet2'), X, lens, args.steps, args.warmup)
    measure('bigram_general', undeclare(build('dirichlet2')), X, lens, args.steps, args.warmup)
    measure('unigram_phoneloop', build('dirichlet_process'), X, lens, args.steps, args.warmup)


if __name__ == '__main__':
    main()
