'''The arc posteriors by category with the unit-start categories (`PhoneLoop.unit_starts`), per
frame and per utterance, beside `hk.log_evidence` and `hk.forward_backward(want_lognorm=True)` on
the same batch and per-state log-likelihoods, in one process, float32:

 * BASELINE config 3's phone loop (40 units x 3 states = 120 states), about 1 M frames in
   300-frame utterances;
 * alignment graphs of the reference's recipe shapes (tests/test_gpu_recipe.py: `sil p .. p sil`
   with 6 .. 11 three-state units around a five-state non-speech unit), every utterance its own
   graph, about 300 frames each;

and, on 100 utterances of the loop, the only route to the same per-frame numbers without
`beer_hmm_arc_posteriors`: `forward_backward(dense_xi=True)` on one-utterance batches, the dense
[T - 1, S, S] tensor of `trans_posteriors_dense`, and a fold by category on the device.

ms per call by HIP events, warm-ups dropped, a median with min .. max, with the shader clock under
load (benchlib.timers.ClockProbe) and the route each call took.

    python tools/bench_arc_posteriors.py [--frames 1000000] [--steps 10] [--warmup 3]
'''

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from beer_amd import hmm_kernels as hk  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds  # noqa: E402
from beer_amd.models.sequence import unit_start_categories  # noqa: E402
from benchlib import recipe  # noqa: E402
from benchlib.timers import ClockProbe  # noqa: E402
from tools.bench_sample_paths import N_PHONES, TOPO, event_ms  # noqa: E402
import beer_amd as beer  # noqa: E402


def loop_model():
    'Config 3\'s loop as a model (its emissions do not matter here: one Gaussian a state).'
    conf = {'g': {'topology': [{'start_id': s, 'end_id': e, 'trans_prob': p} for s, e, p in TOPO],
                  'n_normal_per_state': 1, 'prior_strength': 1., 'noise_std': 1.,
                  'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(N_PHONES)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(2), torch.ones(2))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    return hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet').float().cuda()


def alignment_graphs(n_utts, rng):
    '(model of the recipe, one alignment graph per utterance), as tests/test_gpu_recipe.py draws them.'
    model, units = recipe.phone_loop(40, torch.zeros(2), torch.ones(2), noise_std=1., seed=1)
    speech = [n for n in units if not str(n).startswith('sil')]
    seqs = [['sil'] + [speech[i] for i in rng.randint(0, len(speech), rng.randint(6, 12))] + ['sil']
            for _ in range(n_utts)]
    return model, list(beer.graph.compile_alignments(seqs, units))


def parent_route(graph, arc_cat, init_cat, n_cat, lens, pc_llhs):
    '''The per-frame rows without the new entry point: per utterance the dense xi, folded on the
    device.  Returns a closure for the timer; the index tensors are made once, outside it.'''
    S = graph.n_states
    src, dst = graph.out_arcs()
    keep = arc_cat >= 0
    flat = torch.from_numpy((src.astype(np.int64) * S + dst)[keep]).cuda()
    cats = torch.from_numpy(arc_cat[keep].astype(np.int64)).cuda()
    ikeep = torch.from_numpy(np.nonzero(init_cat >= 0)[0]).cuda()
    icats = torch.from_numpy(init_cat[init_cat >= 0].astype(np.int64)).cuda()
    batches = [hk.HmmBatch([graph], [0], [T], torch.float32) for T in lens]
    off = np.concatenate([[0], np.cumsum(lens)]) * S

    def run():
        out = []
        for u, (batch, T) in enumerate(zip(batches, lens)):
            pc = pc_llhs[off[u]:off[u + 1]]
            gamma = hk.forward_backward(batch, pc, dense_xi=True)[0]
            xi = hk.trans_posteriors_dense(batch, pc, gamma, graph.trans_log_probs)
            rows = torch.zeros(T, n_cat, dtype=torch.float32, device='cuda')
            rows[1:].index_add_(1, cats, xi.view(T - 1, S * S)[:, flat])
            rows[0].index_add_(0, icats, gamma.view(T, S)[0, ikeep])
            out.append(rows)
        return torch.cat(out)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1_000_000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    n_utts = max(args.frames // 300, 1)
    rng = np.random.RandomState(2)
    loop = loop_model()
    recipe_model, graphs = alignment_graphs(n_utts, rng)
    lens = [300] * n_utts
    loop_cats = unit_start_categories(loop.graph, loop.start_pdf, loop.end_pdf)
    ali_cats = [unit_start_categories(g, recipe_model.start_pdf, recipe_model.end_pdf)
                for g in graphs]
    runs = (('phone loop', hk.HmmBatch([loop.graph], [0] * n_utts, lens, torch.float32),
             [loop_cats[0]], [loop_cats[1]], len(loop.start_pdf)),
            ('alignment graphs', hk.HmmBatch(graphs, list(range(n_utts)), lens, torch.float32),
             [c[0] for c in ali_cats], [c[1] for c in ali_cats], len(recipe_model.start_pdf)))
    gen = torch.Generator(device='cuda').manual_seed(2)
    probe = ClockProbe(torch.device('cuda'))
    name = torch.cuda.get_device_properties(0).name

    def report(what, call, fn, route, **more):
        ms = event_ms(fn, args.steps, args.warmup)
        med = ms[len(ms) // 2]
        clock = probe.measure(fn, med)
        print(json.dumps({'batch': what, 'call': call, 'route': route, 'ms_median': round(med, 3),
                          'ms_min': round(ms[0], 3), 'ms_max': round(ms[-1], 3),
                          'steps': args.steps,
                          'mhz_under_load': round(clock['under_load']['mhz']),
                          'mhz_idle': round(clock['idle']['mhz']), **more}), flush=True)

    for what, batch, arc_cats, init_cats, n_cat in runs:
        pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
        # the categories on the device once, as a caller that keeps them would
        arcs = torch.from_numpy(np.concatenate(arc_cats)).cuda()
        inits = torch.from_numpy(np.concatenate(init_cats)).cuda()
        print(json.dumps({'batch': what, 'device': name, 'max_states': batch.struct.max_states,
                          'max_arcs': batch.struct.max_arcs, 'frames': batch.n_frames,
                          'utterances': n_utts, 'elements': batch.n_elems,
                          'categories': n_cat}), flush=True)
        report(what, 'arc_posteriors per frame',
               lambda: hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat),
               hex(hk.arcs_route(batch, n_cat, True)))
        report(what, 'arc_posteriors per utterance',
               lambda: hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat, per_frame=False,
                                         per_utt=True), hex(hk.arcs_route(batch, n_cat, False)))
        report(what, 'log_evidence', lambda: hk.log_evidence(batch, pc_llhs),
               hex(hk.evidence_route(batch)))
        report(what, 'forward_backward want_lognorm',
               lambda: hk.forward_backward(batch, pc_llhs, want_lognorm=True),
               hex(hk._route(torch.float32, batch.struct, 0, 1)))

    # 100 utterances of the loop: the new call against the dense route
    n = min(100, n_utts)
    lens = [300] * n
    batch = hk.HmmBatch([loop.graph], [0] * n, lens, torch.float32)
    pc_llhs = torch.randn(batch.n_elems, generator=gen, device='cuda') * 3
    n_cat = len(loop.start_pdf)
    arcs, inits = (torch.from_numpy(c).cuda() for c in loop_cats)
    dense = parent_route(loop.graph, loop_cats[0], loop_cats[1], n_cat, lens, pc_llhs)
    ours = hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat)[0]
    diff = float((ours - dense()).abs().max())
    what = f'{n} utterances of the loop'
    report(what, 'arc_posteriors per frame', lambda: hk.arc_posteriors(batch, pc_llhs, arcs, inits, n_cat),
           hex(hk.arcs_route(batch, n_cat, True)), largest_difference=diff)
    report(what, 'forward_backward + trans_posteriors_dense + fold, per utterance', dense, 'dense',
           largest_difference=diff, dense_bytes_per_frame=4 * loop.graph.n_states ** 2)


if __name__ == '__main__':
    main()
