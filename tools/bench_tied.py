'''A tied-mixture phone loop against what it replaces and against its floor, on one GPU: ms and
frames/s per VB iteration (accumulate_elbo + update) of

  tied     the phone loop of BASELINE config 3 (40 phones x 3 states, free loop) whose 120
           states share ONE pool of K = 256 full-covariance Gaussians (`TiedMixtureSet`)
  untied   config 3 with full covariances as bench.py runs it (`config3_full`: 120 states x
           16 Gaussians of their own, 1920 in all) -- another model, for context
  mixture  a plain `Mixture` over the same 256-Gaussian pool and the same frames: the floor
           a tied step cannot beat (it evaluates and accumulates the pool, nothing else)

on config 3's utterance lengths, D = 40, float32, 2 M frames.  The models take turns
(`--rounds` rounds of `--steps` iterations each, HIP events around every turn) so that all
three see the same clock; the clock under load is reported beside the numbers
(benchlib.timers.ClockProbe).  `tied_kernels_share`: the time of `beer_tied_lognorm` +
`beer_tied_accumulate` (HIP events around the calls) over the tied step.

    python tools/bench_tied.py [--frames 2000000] [--steps 5] [--warmup 2] [--rounds 3]
                               [--models tied,untied,mixture] [--pool 256]

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_tied.py --models tied` the
kernel list of the tied step alone.
'''

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import beer_amd as beer  # noqa: E402
from bench import D, N_PHONES, hmm_corpus, make_phone_loop  # noqa: E402
from benchlib.timers import ClockProbe, KernelTimer  # noqa: E402

TIED_CALLS = ('beer_tied_lognorm', 'beer_tied_accumulate')
POOL_CALLS = ('beer_mixtureset_estep', 'beer_normal_accumulate', 'beer_normal_accumulate_packed',
              'beer_pack_resps', 'beer_mixture_estep_packed')


def pool(K):
    torch.manual_seed(5)
    return beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=K, prior_strength=1.,
                                 noise_std=1., cov_type='full')


def build(which, K, device):
    if which == 'untied':
        return make_phone_loop('full', device)
    if which == 'mixture':
        return beer.Mixture.create(pool(K), prior_strength=1.).float().to(device)
    donor = make_phone_loop('full', torch.device('cpu'))       # its graph and phone boundaries
    emissions = beer.JointModelSet([beer.TiedMixtureSet.create(3 * N_PHONES, pool(K))])
    return beer.PhoneLoop.create(donor.graph, donor.start_pdf, donor.end_pdf,
                                 emissions).float().to(device)


class Runner:
    def __init__(self, which, K, X, lengths):
        self.which, self.X, self.lengths = which, X, lengths
        self.model = build(which, K, X.device)
        self.optim = beer.VBConjugateOptimizer(self.model.mean_field_factorization(), 1.)
        self.statics = beer.ShardStatics()
        self.ms, self.value = [], None

    def step(self):
        self.optim.init_step()
        elbo = beer.accumulate_elbo(self.model, (self.X, self.lengths), datasize=len(self.X),
                                    statics=self.statics)
        elbo.backward()
        self.optim.step()
        self.value = elbo.value

    def turn(self, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            self.step()
        b.record()
        torch.cuda.synchronize()
        self.ms.append(a.elapsed_time(b) / steps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=2_000_000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pool', type=int, default=256)
    ap.add_argument('--models', default='tied,untied,mixture')
    args = ap.parse_args()
    device = torch.device('cuda')
    lengths = hmm_corpus(args.frames)
    g = torch.Generator(device=device).manual_seed(2)
    X = torch.randn(sum(lengths), D, generator=g, device=device)
    runners = [Runner(w, args.pool, X, lengths) for w in args.models.split(',')]
    for r in runners:
        for _ in range(args.warmup):
            r.step()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for r in runners:
            r.turn(args.steps)
    out = {'frames': len(X), 'utterances': len(lengths), 'D': D, 'dtype': 'float32',
           'cov_type': 'full', 'pool': args.pool, 'states': 3 * N_PHONES, 'results': {}}
    for r in runners:
        ms = statistics.median(r.ms)
        out['results'][r.which] = {
            'ms_per_iteration': round(ms, 3), 'turns_ms': [round(v, 3) for v in r.ms],
            'frames_per_s': round(len(X) / (ms * 1e-3)),
            'last_elbo_per_frame': float(r.value) / len(X) / len(lengths)}
    tied = next((r for r in runners if r.which == 'tied'), None)
    if tied is not None:
        # the share of the two new calls: HIP events around them, in a run of their own (the
        # events serialise the call with what surrounds it)
        with KernelTimer(TIED_CALLS + POOL_CALLS) as kt:
            for _ in range(args.steps):
                tied.step()
            torch.cuda.synchronize()
        per_step = {n: kt.mean_ms(n)[0] * kt.mean_ms(n)[1] / args.steps
                    for n in TIED_CALLS + POOL_CALLS}
        ms = out['results']['tied']['ms_per_iteration']
        out['tied_calls_ms_per_iteration'] = {n: round(v, 3) for n, v in per_step.items() if v}
        out['tied_kernels_share'] = round(sum(per_step[n] for n in TIED_CALLS) / ms, 4)
        out['clock'] = ClockProbe(device).measure(tied.step, ms)
    res = out['results']
    if 'tied' in res and 'mixture' in res:
        out['tied_over_floor'] = round(res['tied']['ms_per_iteration'] /
                                       res['mixture']['ms_per_iteration'], 3)
    if 'tied' in res and 'untied' in res:
        out['untied_over_tied'] = round(res['untied']['ms_per_iteration'] /
                                        res['tied']['ms_per_iteration'], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
