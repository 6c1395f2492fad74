'''A nested mixture against the flat one at BASELINE config 2's shape (D = 40, 1 M float32
frames, full covariances): ms per VB iteration (accumulate_elbo + update) of the flat
K = 256 mixture and of Mixture(MixtureSet(16, NormalSet(256))), 16 mixtures of 16
Gaussians, on the same frames.  Both run the same E-step and accumulation kernels; what
the nested model adds is the leaf log-weights (E ln pi of two levels, summed) and the fold
of the leaf counts into the two levels' weight statistics.

    python tools/bench_nested.py [--frames 1000000] [--steps 10] [--warmup 3]
                                 [--model flat|nested|both]

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_nested.py --model nested` the
kernel list of one model alone.
'''

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import beer_amd as beer  # noqa: E402
from bench import D, K, synth_frames  # noqa: E402

M = 16


def build(nested, device):
    'Config 2\'s initial model (bench.make_gmm), or the same Gaussians under 16 x 16 weights.'
    torch.manual_seed(7)
    X = synth_frames(1 << 17, device, seed=12345)
    ns = beer.NormalSet.create(X.mean(0).cpu(), torch.cov(X.t()).cpu(), size=K,
                               prior_strength=1., noise_std=1., cov_type='full')
    comps = beer.MixtureSet.create(M, ns) if nested else ns
    return beer.Mixture.create(comps, prior_strength=1.).to(device)


def measure(nested, X, lengths, steps, warmup):
    model = build(nested, X.device)
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
    statics = beer.ShardStatics()
    values = []

    def step():
        optim.init_step()
        elbo = beer.accumulate_elbo(model, (X, lengths), datasize=len(X), statics=statics)
        elbo.backward()
        optim.step()
        values.append(elbo.value)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    return {'model': 'nested 16x16' if nested else 'flat 256', 'ms_per_iteration': round(ms, 3),
            'last_elbo_per_frame': float(values[-1]) / len(X)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--chunk', type=int, default=8192, help='frames per "utterance"')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--model', choices=('flat', 'nested', 'both'), default='both')
    args = ap.parse_args()
    device = torch.device('cuda')
    X = synth_frames(args.frames, device, seed=1)
    lengths = [args.chunk] * (args.frames // args.chunk)
    if args.frames % args.chunk:
        lengths.append(args.frames % args.chunk)
    which = {'flat': [False], 'nested': [True], 'both': [False, True]}[args.model]
    out = {'frames': args.frames, 'D': D, 'K': K, 'dtype': 'float32', 'cov_type': 'full',
           'results': [measure(n, X, lengths, args.steps, args.warmup) for n in which]}
    if len(out['results']) == 2:
        flat, nest = (r['ms_per_iteration'] for r in out['results'])
        out['nested_over_flat'] = round(nest / flat, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
