"""Graphs that sit on the dispatch boundaries of the forward-backward / Viterbi kernels of
csrc/hmm.hip, and the float64 truth of everything those kernels return (no GPU needed).

The graphs are CIRCULANT: state i has an arc to (i + o) mod S for every offset o of a set O
that contains 0, so every state has a self-loop (every utterance length T >= 1 has finite
evidence) and in-degree = out-degree = |O mod S| exactly -- the number that picks the DEG
template argument of the one-wave kernels.  An optional hub (sources E, destinations B,
trans[e, s] = a[e] + c[s], declared with `CompiledGraph.set_hub`) is what a phone loop's
eliminated pivot leaves behind; its arcs do not count towards the degree.

The truth is the repository's own oracle (oracle/beer_oracle.py: `posteriors`, `best_path`)
in float64 on the SAME inputs -- float32 inputs upcast -- and plain numpy for what the kernels
derive from the posteriors."""

import numpy as np

from helpers import orc

LENGTHS = (1, 2, 3, 4, 5, 6, 8, 9)        # utterance lengths of the ragged batches
FLAVOURS = ('perm', 'repeat', 'partial')  # pdf ids: a permutation, with repeats, leaving ids out


def offsets(n, S):
    '''An offset set of n elements (fewer when S has fewer residues) with 0 in it.  The
    utterances are at most 9 frames long and start in the first three states: the strides are
    fractions of S, and the first is -1, so that within a few frames the mass sits on the LAST
    states (the ones a wrong lane mask or states-per-lane count loses) and all over the graph --
    with strides of 1, 2, 3 a graph of 256 states would keep all but its first 30 states at 0.'''
    out = []
    for o in [0, -1, S // 2, 1, S // 4, S // 3, S // 8, S // 5, 2, S // 6, S // 7, 3] + list(range(4, S)):
        if len(out) < n and o % S not in [v % S for v in out]:
            out.append(o)
    return tuple(out)


def circulant_mask(S, O):
    'bool [S, S]: arc i -> (i + o) mod S for every o in O.'
    mask = np.zeros((S, S), dtype=bool)
    idx = np.arange(S)
    for o in O:
        mask[idx, (idx + o) % S] = True
    return mask


def degree(S, O):
    '|O mod S|: the in- and out-degree of every state of the circulant graph.'
    return len({o % S for o in O})


def hub_sets(S, m):
    'm sources (the first states) and m destinations (the last states; they may overlap).'
    return list(range(m)), list(range(S - m, S))


def make_graph(S, O, seed, hub=0, dtype=np.float64, integer=False):
    '''dict(init, final, trans [S, S], hub): log-weights in `dtype`.  `hub` members per side
    (0: none) -> hub = (E, a, B, c).  `integer`: weights in {-3..0}, init / final in {-2..0}
    (Viterbi: every sum is exact in float32); else uniform in (-3, 0), the hub's weights on a
    grid of 1/256 so that a[e] + c[s] is exact in float32 too and the block is rank one in
    either precision.'''
    assert 0 in O
    rng = np.random.RandomState(seed)
    mask = circulant_mask(S, O)
    if integer:
        w = rng.randint(-3, 1, size=(S, S)).astype(np.float64)
        init_w = rng.randint(-2, 1, size=S).astype(np.float64)
        final = rng.randint(-2, 1, size=S).astype(np.float64)
    else:
        w = rng.uniform(-3., 0., size=(S, S))
        init_w = rng.uniform(-2., 0., size=S)
        final = rng.uniform(-2., 0., size=S)
    trans = np.where(mask, w, -np.inf)
    init = np.full(S, -np.inf)
    init[:min(S, 3)] = init_w[:min(S, 3)]
    hub_decl = None
    if hub:
        E, B = hub_sets(S, hub)
        if integer:
            a = rng.randint(-2, 1, size=hub).astype(np.float64)
            c = rng.randint(-1, 1, size=hub).astype(np.float64)
        else:
            a = np.round(rng.uniform(-2., 0., size=hub) * 256) / 256
            c = np.round(rng.uniform(-1., 0., size=hub) * 256) / 256
        trans[np.ix_(E, B)] = a[:, None] + c[None, :]
        hub_decl = (E, a.astype(dtype), B, c.astype(dtype))
    return dict(S=S, init=init.astype(dtype), final=final.astype(dtype),
                trans=trans.astype(dtype), hub=hub_decl)


def pdf_ids(S, flavour, S_total, seed):
    'int pdf id of every state; S_total columns of per-pdf log-likelihoods.'
    rng = np.random.RandomState(seed + 7)
    if flavour == 'perm':
        assert S_total == S
        return rng.permutation(S)
    if flavour == 'repeat':
        ids = rng.randint(0, S_total, size=S)
        if S > 1:
            ids[-1] = ids[0]                       # at least one repeat
        return ids
    assert flavour == 'partial' and S_total > S
    return rng.choice(S_total, size=S, replace=False)


def lengths(nutt, seed):
    '''A ragged batch with lengths from LENGTHS: one utterance walks through them by seed,
    five always hold the shortest and the longest, nine hold every length.'''
    rng = np.random.RandomState(seed + 13)
    if nutt == 1:
        return [LENGTHS[seed % len(LENGTHS)]]
    lens = list(LENGTHS) if nutt >= len(LENGTHS) else [1, 9]
    lens += list(rng.choice(LENGTHS, size=nutt - len(lens)))
    return [int(T) for T in rng.permutation(lens)]


def inputs(graph, lens, ids, S_total, scale, seed, dtype=np.float64):
    '''(pc_all [n_frames, S_total], llhs per utterance [T, S]) in `dtype`: the per-state
    log-likelihoods are scale * pc_all[:, ids] rounded once, as the gather computes them.'''
    rng = np.random.RandomState(seed + 29)
    pc_all = (rng.randn(sum(lens), S_total) * 3).astype(dtype)
    packed = (dtype(scale) * pc_all)[:, ids]
    off = np.concatenate([[0], np.cumsum(lens)])
    return pc_all, [packed[off[u]:off[u + 1]] for u in range(len(lens))]


def lowdeg_arcs(graph):
    '(src, dst) of the low-degree image\'s arcs in its out-CSR order: by source, destinations ascending, hub arcs left out.'
    keep = np.isfinite(graph['trans'])
    if graph['hub'] is not None:
        E, _, B, _ = graph['hub']
        keep[np.ix_(E, B)] = False
    return np.nonzero(keep)


def truth(graph, llhs, ids=None, S_total=None, scale=1., dtype=np.float64, factored_hub=True):
    '''Everything the forward-backward entry points return for the batch `llhs` (a list of
    [T, S] arrays) on `graph`, computed by the oracle in `dtype` (float64: the truth, inputs
    upcast; float32: the reference's own float32 op sequence) and summed in float64.
    `factored_hub`: the hub's transition posteriors are reported as `hub_flow` (per destination,
    summed over the sources) and left out of `xi_sum`, as the factorised kernels do; else they
    stay in the matrix and `hub_flow` is zero (the general kernel).'''
    S = graph['S']
    init, final, trans = (graph[k].astype(dtype) for k in ('init', 'final', 'trans'))
    out = dict(gamma=[], lognorm=[], xi_sum=np.zeros((S, S)), gamma0=np.zeros(S),
               last=np.zeros(S), utt_llh=[], frame_llh=[])
    for l in llhs:
        l = l.astype(dtype)
        with np.errstate(invalid='ignore', divide='ignore'):
            gam, xi, lnm = orc.posteriors(l, init, final, trans, True)
        out['gamma'].append(gam)
        out['lognorm'].append(lnm)
        out['xi_sum'] += xi.astype(np.float64).sum(0)
        out['gamma0'] += gam[0]
        out['last'] += gam[-1]
        per_frame = (gam.astype(np.float64) * l.astype(np.float64)).sum(1)
        out['frame_llh'].append(per_frame)
        out['utt_llh'].append(per_frame.sum())
    out['lognorm'] = np.asarray(out['lognorm'], dtype=np.float64)
    out['utt_llh'] = np.asarray(out['utt_llh'])
    out['frame_llh'] = np.concatenate(out['frame_llh'])
    out['xi_dense'] = out['xi_sum'].copy()
    out['hub_flow'] = np.zeros(S)
    out['src_flow'] = out['last'].copy()
    if graph['hub'] is not None:
        E, _, B, _ = graph['hub']
        block = out['xi_dense'][np.ix_(E, B)]
        out['src_flow'][E] += block.sum(1)
        if factored_hub:
            out['hub_flow'][B] = block.sum(0)
            out['xi_sum'][np.ix_(E, B)] = 0.
    src, dst = lowdeg_arcs(graph)
    out['arc_counts'] = out['xi_dense'][src, dst]
    if ids is not None:
        sr = np.zeros((sum(len(l) for l in llhs), S_total))
        np.add.at(sr.T, np.asarray(ids), np.concatenate(out['gamma']).astype(np.float64).T)
        out['state_resps'] = scale * sr
    return out


def xi_frames(graph, llhs, dtype=np.float64):
    'The oracle\'s per-frame transition posteriors [T - 1, S, S] of ONE utterance.'
    init, final, trans = (graph[k].astype(dtype) for k in ('init', 'final', 'trans'))
    with np.errstate(invalid='ignore', divide='ignore'):
        return orc.posteriors(llhs.astype(dtype), init, final, trans, True)[1]


# --- Viterbi ---------------------------------------------------------------------------------

VITERBI_LENGTHS = (1, 2, 31, 32, 33, 64, 65)    # around the back-pointer chunk of 32 frames


def viterbi_inputs(S, lens, seed, dtype=np.float64):
    'Integer log-likelihoods in {-4..0}: with `make_graph(integer=True)` every sum is exact.'
    rng = np.random.RandomState(seed + 31)
    return [rng.randint(-4, 1, size=(T, S)).astype(dtype) for T in lens]


def best_path(graph, llhs, dtype=np.float64):
    init, final, trans = (graph[k].astype(dtype) for k in ('init', 'final', 'trans'))
    return orc.best_path(llhs.astype(dtype), init, final, trans)


def tie_share(graph, llhs):
    '''(cells whose maximum over the sources is attained by more than one source, reachable
    cells) over frames 1 .. T-1 of the Viterbi recursion (graph.py:329-344).'''
    init, trans = graph['init'].astype(np.float64), graph['trans'].astype(np.float64)
    omega = llhs[0].astype(np.float64) + init
    tied = reach = 0
    for t in range(1, len(llhs)):
        hyp = omega[:, None] + trans                        # [source, destination]
        best = hyp.max(0)
        ok = np.isfinite(best)
        tied += int(((hyp == best[None, :]).sum(0)[ok] > 1).sum())
        reach += int(ok.sum())
        omega = llhs[t].astype(np.float64) + best
    return tied, reach
