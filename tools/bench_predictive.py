'''The posterior-predictive (Student-t) emission kernel against the variational E-step on the same
model and frames, on one GPU: ms and frames/s of

  predictive  `kernels.mixtureset_predictive` (csrc/predictive.hip): ln sum_g E[pi_g] St_g(x_t)
  estep       `kernels.mixtureset_estep`, log-normalisers only (what a search runs on today)

at two shapes, float32, D = 40:

  c3diag   BASELINE config 3's emissions: 120 states x 16 diagonal Gaussians, 2 M frames
  c2full   BASELINE config 2's mixture: 256 full-covariance Gaussians, 1 M frames

The two calls take turns (`--rounds` rounds of `--steps` calls each, HIP events around every
turn, after `--warmup` calls of each) so that both see the same clock; the clock under load is
reported beside the numbers (benchlib.timers.ClockProbe).  For the diagonal shape the line also
gives log1p evaluations per second as the kernel issues them (T K D / kFold, kFold = 8 dimensions
folded per logarithm) and per dimension (T K D): the kernel is bound by vector-instruction issue,
the transcendental among them.

    python tools/bench_predictive.py [--shapes c3diag,c2full] [--steps 5] [--warmup 2] [--rounds 3]
                                     [--frames-scale 1.0]
'''

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import beer_amd as beer  # noqa: E402
from beer_amd import kernels  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402

D = 40
FOLD = 8                    # kFold of csrc/predictive.hip
SHAPES = {'c3diag': ('diagonal', 120, 16, 2_000_000), 'c2full': ('full', 1, 256, 1_000_000)}


class Shape:
    def __init__(self, name, scale, device):
        self.name = name
        self.cov, self.S, self.G, frames = SHAPES[name]
        self.T = max(1, int(frames * scale))
        torch.manual_seed(5)
        K = self.S * self.G
        ns = beer.NormalSet.create(torch.zeros(D), torch.ones(D), size=K, prior_strength=1.,
                                   noise_std=1., cov_type=self.cov).float().to(device)
        post = ns.means_precisions.posterior
        self.table = post.predictive_table()
        self.exp_stats = ns.means_precisions.natural_form()
        self.lw = torch.full((self.S, self.G), -float(torch.tensor(float(self.G)).log()),
                             device=device)
        g = torch.Generator(device=device).manual_seed(2)
        self.stats = beer.FrameStats(torch.randn(self.T, D, generator=g, device=device), self.cov)
        self.ms = {'predictive': [], 'estep': []}

    def predictive(self):
        return kernels.mixtureset_predictive(self.stats, self.table, self.lw, self.S, self.G,
                                             self.cov)

    def estep(self):
        return kernels.mixtureset_estep(self.stats, self.exp_stats, self.lw, self.S, self.G,
                                        self.cov, want_resps=False)[0]

    def turn(self, which, steps):
        fn = getattr(self, which)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        self.ms[which].append(a.elapsed_time(b) / steps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--shapes', default='c3diag,c2full')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--frames-scale', type=float, default=1.)
    args = ap.parse_args()
    device = torch.device('cuda')
    out = {'D': D, 'dtype': 'float32', 'fold': FOLD, 'results': {}}
    for name in args.shapes.split(','):
        shape = Shape(name, args.frames_scale, device)
        for which in shape.ms:
            for _ in range(args.warmup):
                getattr(shape, which)()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for which in shape.ms:
                shape.turn(which, args.steps)
        # Jensen, on the whole matrix: the two numbers are of one model and one set of frames
        assert (shape.predictive() >= shape.estep()).all()
        ms = {w: statistics.median(v) for w, v in shape.ms.items()}
        res = {'cov_type': shape.cov, 'states': shape.S, 'components': shape.G, 'frames': shape.T}
        for w, v in ms.items():
            res[w] = {'ms': round(v, 3), 'turns_ms': [round(t, 3) for t in shape.ms[w]],
                      'frames_per_s': round(shape.T / (v * 1e-3))}
        res['predictive_over_estep'] = round(ms['predictive'] / ms['estep'], 3)
        if shape.cov == 'diagonal':
            evals = shape.T * shape.S * shape.G * D
            res['log1p_per_s_issued'] = round(evals / FOLD / (ms['predictive'] * 1e-3))
            res['log1p_per_s_per_dimension'] = round(evals / (ms['predictive'] * 1e-3))
        res['clock'] = ClockProbe(device).measure(
            lambda: [shape.predictive() for _ in range(args.steps)],
            ms['predictive'] * args.steps)
        out['results'][name] = res
        del shape
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
