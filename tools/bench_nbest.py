'''N-best Viterbi beside `hk.viterbi` on the same batch and per-state log-likelihoods, in one
process, float32:

 * BASELINE config 3's phone loop (40 units x 3 states = 120 states), about 1 M frames in
   300-frame utterances;
 * alignment graphs of the reference's recipe shapes (tests/test_gpu_recipe.py: `sil p .. p sil`
   with 6 .. 11 three-state units around a five-state non-speech unit), every utterance its own
   graph, about 300 frames each.

k = 1, 4 and 16.  ms per call by HIP events, warm-ups dropped, with the shader clock under load
(benchlib.timers.ClockProbe), the route each call took, the ratio to `hk.viterbi`, whether rank 0
is its path, and the largest error of a reported score against the path rescored in float64,
relative to tol * (sum of |terms| + 1) at tol = 1e-5 (a sample of the utterances).

    python tools/bench_nbest.py [--frames 1000000] [--steps 10] [--warmup 3]
'''

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beer_amd import hmm_kernels as hk  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_log_evidence import alignment_graphs  # noqa: E402
from tools.bench_sample_paths import event_ms, loop_graph  # noqa: E402


def score_errors(batch, graphs, pc_llhs, paths, scores, sample):
    '''Largest |reported - rescored| / (1e-5 * (sum |terms| + 1)) over the ranks of `sample`
    utterances, the rescoring in float64 on the host from the dense graph.'''
    off_f, off_e = batch.frame_off_h.numpy(), batch.llh_off_h.numpy()
    paths, scores, flat = paths.cpu().numpy(), scores.cpu().numpy(), pc_llhs.cpu().numpy()
    worst = 0.
    for u in sample:
        g = graphs[batch.graph_ids[u]]
        g = g.to_dense() if hasattr(g, 'to_dense') else g
        init, final, trans = (getattr(g, n).double().cpu().numpy()
                              for n in ('init_log_probs', 'final_log_probs', 'trans_log_probs'))
        T = int(off_f[u + 1] - off_f[u])
        llh = flat[off_e[u]:off_e[u + 1]].reshape(T, -1).astype(np.float64)
        for r in range(paths.shape[0]):
            p = paths[r, off_f[u]:off_f[u + 1]]
            if p[0] < 0:
                continue
            terms = np.concatenate([[init[p[0]]], llh[np.arange(T), p], trans[p[:-1], p[1:]],
                                    [final[p[-1]]]])
            worst = max(worst, abs(terms.sum() - scores[u, r]) / (1e-5 * (np.abs(terms).sum() + 1.)))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    n_utts = max(args.frames // 300, 1)
    rng = np.random.RandomState(2)
    loop = loop_graph()
    graphs = alignment_graphs(n_utts, rng)
    lens = [300] * n_utts
    batches = (('phone loop', [loop], hk.HmmBatch([loop], [0] * n_utts, lens, torch.float32)),
               ('alignment graphs', graphs,
                hk.HmmBatch(graphs, list(range(n_utts)), lens, torch.float32)))
    gen = torch.Generator(device='cuda').manual_seed(2)
    probe = ClockProbe(torch.device('cuda'))
    sample = list(range(0, n_utts, max(n_utts // 8, 1)))[:8]
    for what, distinct, batch in batches:
        pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
        print(json.dumps({'batch': what, 'device': torch.cuda.get_device_properties(0).name,
                          'max_states': batch.struct.max_states, 'max_arcs': batch.struct.max_arcs,
                          'frames': batch.n_frames, 'utterances': n_utts,
                          'elements': batch.n_elems}), flush=True)
        best = hk.viterbi(batch, pc_llhs)

        def report(name, fn, route, base=None, **more):
            ms = event_ms(fn, args.steps, args.warmup)
            med = ms[len(ms) // 2]
            clock = probe.measure(fn, med)
            print(json.dumps({'batch': what, 'call': name, 'route': route,
                              'ms_median': round(med, 3), 'ms_min': round(ms[0], 3),
                              'ms_max': round(ms[-1], 3), 'steps': args.steps,
                              'mhz_under_load': round(clock['under_load']['mhz']),
                              'mhz_idle': round(clock['idle']['mhz']),
                              **({'ratio_to_viterbi': round(med / base, 2)} if base else {}),
                              **more}), flush=True)
            return med

        base = report('viterbi', lambda: hk.viterbi(batch, pc_llhs), None)
        for k in (1, 4, 16):
            paths, scores = hk.viterbi_nbest(batch, pc_llhs, k)
            report(f'viterbi_nbest k={k}', lambda: hk.viterbi_nbest(batch, pc_llhs, k),
                   hex(hk.nbest_route(batch, k)), base,
                   rank0_is_viterbi=bool(torch.equal(paths[0], best)),
                   finite_ranks=int(torch.isfinite(scores).sum()) / max(n_utts, 1),
                   largest_score_error_over_bound=score_errors(batch, distinct, pc_llhs, paths,
                                                               scores, sample))


if __name__ == '__main__':
    main()
