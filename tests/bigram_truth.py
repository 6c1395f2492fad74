"""Graphs that sit on the launch boundaries of the bigram forward-backward kernel of
csrc/hmm_bigram.hip, and the float64 truth of what `hk.posteriors_bigram` returns (no GPU needed).

A graph is the CIRCULANT residual graph of tests/fb_truth.py (state i -> (i + o) mod S for every
offset o of a set of d offsets with 0 in it: in-degree = out-degree = d exactly) with a dense
P x P block trans[src_i, dst_j] on top, the one `CompiledGraph.set_bigram_block` declares.  Block
cells that coincide with circulant arcs belong to the block, as in `BigramImage`, and the generator
reports the residual degree it produced by `BigramImage`'s rule: the largest in- or out-degree with
the block removed.  The initial states are the last three block sources (of a block of more than
64 only members from 64 on: the second chunk of the kernel's member loop), and the residual arcs that leave a source are LEAVE nats weaker than the
others -- a source is a phone's last state, what follows it is the block's business -- so that
the first transition of every utterance goes through the block whatever the emissions say.

The truth is the repository's oracle (oracle/beer_oracle.py: `posteriors`) in float64 on the SAME
inputs -- the graph built in the case's dtype and upcast -- and, for the batches of thousands of
utterances, a vectorised float64 log-space restatement of it over utterances of equal length
(`batch_posteriors`), pinned to the oracle in tests/test_bigram_routes_host.py."""

import numpy as np

import fb_truth as ft
from helpers import orc

LENGTHS = ft.LENGTHS
FLAVOURS = ft.FLAVOURS
PLACEMENTS = ('disjoint', 'overlap', 'identical', 'reversed')
DEEP = 120.                 # the dirichlet2 regime: exp(-120) is 0 in float32
LEAVE = 8.                  # how much weaker than the others a source's residual arcs are
NOISE = 2.                  # standard deviation of the per-pdf log-likelihoods, nats


def block_states(S, P, placement):
    '''(src, dst) state lists of the block.  disjoint: the first P and the last P states;
    reversed: the last P and the first P; overlap: dst the last P states, src the same window
    moved down by half of P (at most 32 states; the first P states where the graph is too small
    for that); identical: src == dst, the last P states.'''
    assert 1 <= P <= S
    last = list(range(S - P, S))
    if placement == 'identical':
        return last, list(last)
    if placement == 'overlap':
        lo = S - P - min(P - P // 2, 32)
        return (list(range(lo, lo + P)) if lo >= 0 else list(range(P))), last
    assert 2 * P <= S, 'disjoint block sides need 2 P <= S'
    first = list(range(P))
    return (first, last) if placement == 'disjoint' else (last, first)


def residual_degree(trans, src, dst):
    '`BigramImage.max_degree` restated on host arrays.'
    keep = np.isfinite(trans)
    keep[np.ix_(src, dst)] = False
    return int(max(keep.sum(0).max(), keep.sum(1).max()))


def make_graph(S, P, d, placement='disjoint', seed=0, neg=0., deep=False, dtype=np.float64,
               O=None, init_states=None):
    '''dict(S, P, init, final, trans [S, S], src, dst, block [P, P], max_degree): log-weights in
    `dtype`.  `d` residual arcs a state (0: none, then P = S and every arc is in the block);
    `neg`: the share of -inf block entries (a random permutation of the block stays finite, so
    every row and every column keeps an entry); `deep`: every transition DEEP nats down, the
    block as in the dirichlet2 regime and the residual arcs with it, so that the block keeps its
    share of the mass; `O` / `init_states` override the offsets (fb_truth.offsets) and the
    initial states.'''
    rng = np.random.RandomState(seed)
    O = tuple(O) if O is not None else (ft.offsets(d, S) if d else ())
    assert (0 in O) == bool(O) and ft.degree(S, O) == d
    src, dst = block_states(S, P, placement)
    assert d > 0 or (P == S and placement == 'identical')
    trans = np.where(ft.circulant_mask(S, O), rng.uniform(-3., 0., size=(S, S)), -np.inf)
    block = rng.uniform(-3., 0., size=(P, P))
    trans[src, :] -= LEAVE
    if neg:
        forbid = rng.rand(P, P) < neg
        forbid[np.arange(P), rng.permutation(P)] = False
        block[forbid] = -np.inf
    trans[np.ix_(src, dst)] = block
    if deep:
        trans -= DEEP
    init = np.full(S, -np.inf)
    at = list(src[max(64, P - 3) if P > 64 else -3:] if init_states is None else init_states)
    init[at] = rng.uniform(-2., 0., size=len(at))
    final = rng.uniform(-2., 0., size=S)
    trans = trans.astype(dtype)
    return dict(S=S, P=P, init=init.astype(dtype), final=final.astype(dtype), trans=trans,
                src=src, dst=dst, block=trans[np.ix_(src, dst)],
                max_degree=residual_degree(trans, src, dst))


def pdf_ids(S, flavour, S_total, seed):
    return ft.pdf_ids(S, flavour, S_total, seed)


def lengths(nutt, seed, choice=LENGTHS, zero=False):
    '''A ragged batch with every length of `choice` in it (when it has that many utterances),
    the rest drawn from it; `zero`: one more utterance, without a frame, in the middle.'''
    rng = np.random.RandomState(seed + 13)
    lens = list(choice)[:nutt]
    lens += list(rng.choice(choice, size=nutt - len(lens)))
    lens = [int(T) for T in rng.permutation(lens)]
    if zero:
        lens.insert(len(lens) // 2, 0)
    return lens


def inputs(lens, ids, S_total, scale, seed, dtype=np.float64):
    '''(pc_all [n_frames, S_total], llhs per utterance [T, S]) in `dtype`: Gaussian noise of NOISE
    nats; the per-state log-likelihoods are scale * pc_all[:, ids] rounded once, as the gather
    computes them.'''
    rng = np.random.RandomState(seed + 29)
    pc_all = (rng.randn(sum(lens), S_total) * NOISE).astype(dtype)
    packed = (dtype(scale) * pc_all)[:, ids]
    off = np.concatenate([[0], np.cumsum(lens)])
    return pc_all, [packed[off[u]:off[u + 1]] for u in range(len(lens))]


# --- the truth ---------------------------------------------------------------------------------

def _neighbours(keep, w):
    '(index [S, D], weight [S, D]) of the rows of bool `keep` [S, S], padded with -inf weights.'
    S = len(keep)
    D = max(int(keep.sum(1).max()), 1)
    idx = np.zeros((S, D), dtype=np.int64)
    wt = np.full((S, D), -np.inf)
    for i in range(S):
        j = np.nonzero(keep[i])[0]
        idx[i, :len(j)] = j
        wt[i, :len(j)] = w[i, j]
    return idx, wt


def batch_posteriors(g, L):
    '''Forward-backward of U utterances of one length in float64 log space: L [U, T, S] ->
    (gamma [U, T, S], block counts summed over the utterances [P, P], total block count of every
    utterance [U]).  graph.py:270-326 restated with the graph's structure: the residual arcs as
    padded neighbour lists, the block as a dense [P, P] matrix.'''
    init, final, trans = (np.asarray(g[k], dtype=np.float64) for k in ('init', 'final', 'trans'))
    src, dst = np.asarray(g['src']), np.asarray(g['dst'])
    U, T, S = L.shape
    P = len(src)
    W = trans[np.ix_(src, dst)]
    keep = np.isfinite(trans)
    keep[np.ix_(src, dst)] = False
    in_idx, in_w = _neighbours(keep.T, trans.T)          # sources of every state
    out_idx, out_w = _neighbours(keep, trans)            # destinations of every state
    lse = orc.logsumexp

    def step(vec, idx, w, members, blk_axis, targets):
        res = lse(vec[:, idx] + w[None], 2)
        pair = (vec[:, members][:, :, None] + W[None]) if blk_axis == 1 else \
            (W[None] + vec[:, members][:, None, :])
        through = np.full((U, S), -np.inf)
        through[:, targets] = lse(pair, blk_axis)
        with np.errstate(invalid='ignore'):
            return np.logaddexp(res, through)

    la = np.full((U, T, S), -np.inf)
    lb = np.full((U, T, S), -np.inf)
    with np.errstate(invalid='ignore', divide='ignore'):
        la[:, 0] = L[:, 0] + init
        for t in range(1, T):
            la[:, t] = L[:, t] + step(la[:, t - 1], in_idx, in_w, src, 1, dst)
        lb[:, T - 1] = final
        for t in range(T - 2, -1, -1):
            lb[:, t] = step(L[:, t + 1] + lb[:, t + 1], out_idx, out_w, dst, 2, src)
        lognorm = lse((la + lb).reshape(U * T, S), 1).reshape(U, T)
        gamma = np.exp(la + lb - lognorm[:, :, None])
        counts, per_utt = np.zeros((P, P)), np.zeros(U)
        for t in range(T - 1):
            v = (L[:, t + 1] + lb[:, t + 1])[:, dst]
            xi = np.exp(la[:, t][:, src][:, :, None] + W[None] + v[:, None, :]
                        - lognorm[:, t, None, None])
            counts += xi.sum(0)
            per_utt += xi.sum((1, 2))
    return gamma, counts, per_utt


def truth(g, llhs, ids, S_total, scale, vectorised=False):
    '''What `hk.posteriors_bigram` returns for the batch `llhs` (a list of [T, S] arrays, already
    scale * pc_all[:, ids]) on `g`, from the oracle in float64 (inputs upcast):
    state_resps [n_frames, S_total] = scale * gamma scattered to pdf ids (repeats add),
    counts [P, P] = the transition posteriors of the block summed over frames and utterances,
    utt_llh [nutt] = sum_t sum_s gamma * llh; and gamma per utterance, the total block count of
    every utterance.  `vectorised`: by `batch_posteriors`, utterances of equal length together.'''
    S, P = g['S'], g['P']
    init, final, trans = (g[k].astype(np.float64) for k in ('init', 'final', 'trans'))
    nutt = len(llhs)
    gamma = [np.zeros((0, S))] * nutt
    counts, utt_counts = np.zeros((P, P)), np.zeros(nutt)
    if vectorised:
        by_len = {}
        for u, l in enumerate(llhs):
            by_len.setdefault(len(l), []).append(u)
        for T, us in sorted(by_len.items()):
            if T == 0:
                continue
            for at in range(0, len(us), 256):
                part = us[at:at + 256]
                gam, c, per = batch_posteriors(g, np.stack([llhs[u] for u in part]).astype(np.float64))
                counts += c
                utt_counts[part] = per
                for k, u in enumerate(part):
                    gamma[u] = gam[k]
    else:
        for u, l in enumerate(llhs):
            if len(l) == 0:
                continue
            with np.errstate(invalid='ignore', divide='ignore'):
                gam, xi, _ = orc.posteriors(l.astype(np.float64), init, final, trans, True)
            block = xi.sum(0)[np.ix_(g['src'], g['dst'])]
            gamma[u], utt_counts[u] = gam, block.sum()
            counts += block
    utt_llh = np.asarray([(gam * l.astype(np.float64)).sum() for gam, l in zip(gamma, llhs)])
    sr = np.zeros((sum(len(l) for l in llhs), S_total))
    np.add.at(sr.T, np.asarray(ids), np.concatenate(gamma).T)
    return dict(gamma=gamma, state_resps=scale * sr, counts=counts, utt_llh=utt_llh,
                utt_counts=utt_counts)
