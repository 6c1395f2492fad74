"""Times of the three CMLLR kernels at D = 40, S G = 1920, 1 M frames, 1 and 64 speakers, and of
the route they are meant to beat: `normal_accumulate(..., 'full')` of the same frames and
responsibilities (full second-order statistics per Gaussian, from which the Gram matrices
G_{s,i} would have to be assembled -- for one speaker; per speaker it would run once each).
Device events around warmed-up calls, the routes alternating; prints, asserts nothing.

    python tools/probes/cmllr_time.py [frames]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from beer_amd import kernels
from beer_amd.stats import FrameStats

DEV = 'cuda'
T = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
D, S, G = 40, 640, 3
K, REPS = S * G, 5


def timed(calls):
    'Median ms of every call of {name: f}, the calls alternating, after one warm-up round.'
    times = {name: [] for name in calls}
    for rep in range(REPS + 1):
        for name, f in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            f()
            stop.record()
            stop.synchronize()
            if rep:
                times[name].append(start.elapsed_time(stop))
    return {name: sorted(v)[len(v) // 2] for name, v in times.items()}


torch.manual_seed(0)
X = torch.randn(T, D, device=DEV)
cr = torch.rand(T, K, device=DEV)
cr /= cr.view(T, S, G).sum(-1, keepdim=True).repeat_interleave(G, dim=-1).view(T, K)
sr = torch.softmax(torch.randn(T, S, device=DEV) * 4., dim=-1)
E = torch.cat([torch.randn(K, D, device=DEV), torch.rand(K, D, device=DEV) + .5,
               torch.randn(K, 2, device=DEV)], dim=1)
W = torch.eye(D, D + 1, dtype=torch.float64, device=DEV).repeat(64, 1, 1)
n_utt = max(T // 512, 1)
lengths = [T // n_utt] * n_utt
lengths[-1] += T - sum(lengths)
params = kernels.cmllr_frame_params(cr, sr, E, S, G, D, 'diagonal')
stats = FrameStats(X, 'full')
for n_spk in (1, 64):
    spk = [u % n_spk for u in range(n_utt)]
    table = kernels.cmllr_table(lengths, spk, n_spk)
    frame_off = kernels._frame_offsets(lengths, X.device)
    out = kernels.cmllr_accumulate(X, params, lengths, spk, n_spk, table=table, frame_off=frame_off)
    ms = timed({
        'frame_params': lambda: kernels.cmllr_frame_params(cr, sr, E, S, G, D, 'diagonal', out=params),
        'accumulate': lambda: kernels.cmllr_accumulate(X, params, lengths, spk, n_spk, *out,
                                                       table=table, frame_off=frame_off),
        'apply': lambda: kernels.cmllr_apply(X, W[:n_spk], lengths, spk),
        'full statistics': lambda: kernels.normal_accumulate(stats, cr, sr, S, G, 'full'),
    })
    fma = {'frame_params': T * K * (2 * D + 1), 'accumulate': T * (D * (D + 1) * (D + 2) // 2 + D * (D + 1)),
           'apply': T * D * (D + 1), 'full statistics': T * K * (D * (D + 1) // 2 + D + 1)}
    print(f'T={T} D={D} S={S} G={G} speakers={n_spk} items={table.n_items}: ' + ', '.join(
        f'{name} {ms[name]:.2f} ms ({2e-9 * fma[name] / ms[name]:.1f} TFLOP/s of its own count)'
        for name in ms) + f'; new path {ms["frame_params"] + ms["accumulate"]:.2f} ms against '
        f'{ms["full statistics"]:.2f} ms')
