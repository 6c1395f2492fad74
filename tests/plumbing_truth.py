"""The truth, in float64 or wider, of the small kernels every HMM path goes through -- the pdf-id
gather and scatter, the one-hot posteriors of a state path, the last-frame sum (csrc/hmm.hip), the
per-utterance sum and the mixture-weight statistics (csrc/estep.hip) -- and the table of batches
the GPU tests run them on.  Plain numpy; nothing of the package is imported (no GPU needed).

Everything is per utterance: `llh`, `gamma` are [T, S] arrays, a batch is a list of them."""

from collections import namedtuple

import numpy as np

# --- launch constants of the kernels (csrc/hmm.hip, csrc/estep.hip) ------------------------------
WAVE = 64                      # lanes of a wave: scatter_kernel, weights_from_acc_kernel stride by it
BLOCK = 256                    # threads of a workgroup: last_frame_kernel, segment_sum_kernel
GATHER_PASS = 4 * BLOCK        # elements of an utterance one pass of gather_kernel covers
FLAT_PASS = 8 * BLOCK          # ... of scatter_flat_kernel
FRAME_PASS = 8 * (BLOCK // WAVE)   # frames a pass of scatter_kernel covers: a wave per frame
PATH_PASS = 2 * BLOCK          # elements a pass of path_post_kernel's one-hot loop covers
PATH_XI_PASS = BLOCK           # transitions a pass of its count loop covers

U = {np.float32: 2. ** -24, np.float64: 2. ** -53}        # unit roundoff
# The sums are taken in numpy's widest float (64 bits of mantissa where the C long double has
# them, float64 elsewhere), so that against a float64 kernel the truth's own rounding does not eat
# into bounds of a few 2^-53; products of float32 values are exact in either.
HP = np.longdouble


def gamma_n(n, u):
    'n u / (1 - n u): the relative error of n roundings on top of each other.'
    return n * u / (1. - n * u)


# --- the operations ----------------------------------------------------------------------------------

def gather(pc_all, ids, scale, dtype):
    'scale * pc_all[:, ids] in `dtype`: one product, rounded once.  pc_all: the frames of ONE utterance.'
    with np.errstate(invalid='ignore'):
        return dtype(scale) * np.asarray(pc_all, dtype=dtype)[:, np.asarray(ids)]


def scatter(llh, gamma, ids, S_total, scale):
    '''(sr [T, S_total], exp_llh [T], utt_llh) of one utterance: sr[t, ids[s]] +=
    scale * gamma[t, s], exp_llh[t] = sum_s llh[t, s] gamma[t, s], utt_llh = sum_t exp_llh[t].
    (`scale`: the value the kernel multiplies with, rounded to its type by the caller.)'''
    llh, gamma = np.asarray(llh, dtype=HP), np.asarray(gamma, dtype=HP)
    sr = np.zeros((len(gamma), S_total), dtype=HP)
    np.add.at(sr.T, np.asarray(ids, dtype=np.int64), (HP(float(scale)) * gamma).T)
    with np.errstate(invalid='ignore'):
        exp_llh = (llh * gamma).sum(1)
    return sr, exp_llh, exp_llh.sum()


def scatter_once(gamma, ids, S_total, scale, dtype):
    '''sr of one utterance whose pdf ids are DISTINCT, in `dtype`: the one product, rounded once,
    in a zero-filled row (the wider product of `scatter`, rounded again, is not always that).'''
    assert len(set(np.asarray(ids).tolist())) == len(ids)
    sr = np.zeros((len(gamma), S_total), dtype=dtype)
    sr[:, np.asarray(ids, dtype=np.int64)] = dtype(scale) * np.asarray(gamma, dtype=dtype)
    return sr


def scatter_abs(llh, gamma, ids, S_total, scale):
    'The same sums over the absolute values of their terms: what the error bounds are made of.'
    return scatter(np.abs(llh), np.abs(gamma), ids, S_total, abs(float(scale)))


def path_posteriors(paths, S):
    '''(one-hot [T, S] per utterance, xi [S, S], g0 [S], last [S]) of the state paths `paths` (one
    int array per utterance): the transitions (p_t, p_t+1) INSIDE every utterance, its first and
    its last state counted; an utterance of no frames contributes nothing.'''
    xi, g0, last, onehot = np.zeros((S, S)), np.zeros(S), np.zeros(S), []
    for p in paths:
        p = np.asarray(p, dtype=np.int64)
        onehot.append((p[:, None] == np.arange(S)[None, :]).astype(np.float64))
        if len(p):
            np.add.at(xi, (p[:-1], p[1:]), 1.)
            g0[p[0]] += 1.
            last[p[-1]] += 1.
    return onehot, xi, g0, last


def last_frame_sum(gammas, S):
    'sum over the utterances that have frames of the last row of their [T, S] posteriors.'
    out = np.zeros(S, dtype=HP)
    for g in gammas:
        if len(g):
            out += np.asarray(g, dtype=HP)[-1]
    return out


def segment_sum(values, frame_off):
    'out[u] = sum of values[frame_off[u]:frame_off[u + 1]].'
    v = np.asarray(values, dtype=HP)
    return np.array([v[frame_off[u]:frame_off[u + 1]].sum() for u in range(len(frame_off) - 1)],
                    dtype=HP)


def weights_from_acc(acc, S, G):
    'out[s, g] = -2 acc[s G + g, Q - 2] for g < G - 1, the sum of the row in column G - 1.'
    n = -2. * np.asarray(acc, dtype=np.float64)[:, -2].reshape(S, G)
    out = n.copy()
    out[:, G - 1] = n.sum(1)
    return out


# --- pdf ids -----------------------------------------------------------------------------------------

FLAVOURS = ('perm', 'subset', 'repeat', 'identity')


def pdf_ids(S, flavour, seed):
    '''(ids [S], S_total, r): a permutation of 0..S-1; S distinct ids out of S + 7; every pdf shared
    by two or three states (and five pdfs nobody uses); exactly 0..S-1.  r: the most states a pdf
    has.'''
    rng = np.random.RandomState(seed + 101)
    if flavour == 'perm':
        return rng.permutation(S), S, 1
    if flavour == 'subset':
        return rng.choice(S + 7, size=S, replace=False), S + 7, 1
    if flavour == 'identity':
        return np.arange(S), S, 1
    assert flavour == 'repeat' and S >= 2
    group, left, k = [], S, 0
    while left:
        n = left if left <= 3 else 2 if left == 4 else 2 + k % 2    # never a group of one state
        group += [k] * n
        left -= n
        k += 1
    S_total = k + 5
    ids = rng.permutation(S_total)[np.asarray(group)][rng.permutation(S)]
    counts = np.bincount(ids, minlength=S_total)
    assert set(counts[counts > 0]) <= {2, 3}
    return ids, S_total, int(counts.max())


# --- the table of batches ----------------------------------------------------------------------------

SIZES = (1, 3, 64, 65, 256, 257, 300)
LENGTHS = (0, 258, 1, 0, 33, 2, 65, 0)      # an empty utterance first, in the middle and last
MIXED = (3, 65, 300)

# sizes: states of every distinct graph; flavours: its pdf ids; gids / lens: per utterance
Case = namedtuple('Case', 'name sizes flavours gids lens seed')


def _cases():
    out, seed = [], 0
    for S in SIZES:
        for fl in FLAVOURS:
            if fl == 'repeat' and S < 2:
                continue
            out.append(Case(f'S{S}-{fl}', (S,), (fl,), (0,) * len(LENGTHS), LENGTHS, seed))
            seed += 1
    out.append(Case('mixed', MIXED, ('subset', 'repeat', 'subset'), (2, 0, 1, 1, 2, 0, 1, 2),
                    LENGTHS, seed))
    out.append(Case('nutt0', (3,), ('perm',), (), (), seed + 1))
    return out


CASES = _cases()


def case_ids(case):
    '(ids per graph, S_total of the batch, r): the graphs of a batch share the columns of pc_all.'
    got = [pdf_ids(S, fl, case.seed + 3 * i) for i, (S, fl) in enumerate(zip(case.sizes, case.flavours))]
    return [g[0] for g in got], max(g[1] for g in got), max(g[2] for g in got)


def grid(rng, shape, lo, hi, dtype):
    'Multiples of 1/64 in [lo, hi): sums and products of a few hundred of them are exact in float32.'
    return (rng.randint(int(lo * 64), int(hi * 64), size=shape) / 64.).astype(dtype)
