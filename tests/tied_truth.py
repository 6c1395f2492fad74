'''The truth of the tied-mixture tests: a float64 numpy restatement of the model computed the
slow way -- `pc` by `np.logaddexp.reduce` over the pool, the joint responsibilities
j[t,s,k] materialised, then the counts C, the pool responsibilities r and acc = r^T phi(X).
The Gaussians' log-likelihoods come from `oracle.beer_oracle` (the pinned restatement of the
reference), state posteriors from the oracle's / `transitions_truth`'s forward-backward.  The
reference has no tied model; tests/test_tied_host.py ties this file to the oracle's `Mixture`
and `MixtureSet`.'''

import numpy as np

from oracle import beer_oracle as orc

# p[t,s] = sum_k e[t,k] w[s,k] below which an entry is redone in log space
# (beer_amd/csrc/tied.hip: K tiny / delta with K <= 2^12)
THRESHOLD = {'float32': 2. ** -94, 'float64': 2. ** -970}


def suffstats(X, cov_type):
    return orc.SUFFSTATS[cov_type](np.asarray(X, dtype=np.float64))


def pool_llh(X, cov_type, exp_T):
    'l[t,k] of the pool from its expected natural statistics E[T] [K, Q].'
    X = np.asarray(X, dtype=np.float64)
    return orc.normal_llh(suffstats(X, cov_type), np.asarray(exp_T, dtype=np.float64), X.shape[1])


def lognorm(l, lw):
    '(pc [T,S], m [T]): pc[t,s] = logsumexp_k(l[t,k] + lw[s,k]), one state at a time.'
    l, lw = np.asarray(l, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        pc = np.stack([np.logaddexp.reduce(l + lw[s][None, :], axis=1) for s in range(len(lw))],
                      axis=1)
    return pc, l.max(axis=1)


def linear_sum(l, lw):
    'p[t,s] = sum_k exp(l[t,k] - m[t]) exp(lw[s,k]) = exp(pc - m): what the range rule looks at.'
    pc, m = lognorm(l, lw)
    return np.exp(pc - m[:, None])


def statistics(l, lw, pc, g, stats=None, chunk=64):
    '''(C [S,K], r [T,K], acc [K,Q] or None) from the state posteriors g [T,S]:
    j[t,s,k] = g[t,s] exp(l[t,k] + lw[s,k] - pc[t,s]) materialised `chunk` frames at a time.'''
    l, lw, pc, g = (np.asarray(a, dtype=np.float64) for a in (l, lw, pc, g))
    T, K = l.shape
    C, r = np.zeros(lw.shape), np.zeros((T, K))
    for t0 in range(0, T, chunk):
        sl = slice(t0, t0 + chunk)
        with np.errstate(invalid='ignore', over='ignore'):
            j = g[sl, :, None] * np.exp(l[sl, None, :] + lw[None, :, :] - pc[sl, :, None])
        j = np.where(g[sl, :, None] == 0, 0., j)              # q of an entry with g = 0 is 0
        C += j.sum(axis=0)
        r[sl] = j.sum(axis=1)
    acc = None if stats is None else r.T @ np.asarray(stats, dtype=np.float64)
    return C, r, acc


def weight_stats(C):
    'Statistics of the Dirichlet rows from the counts: last column <- row sum.'
    out = np.array(C, dtype=np.float64)
    out[..., -1] = C.sum(axis=-1)
    return out


# ---- a whole HMM step -------------------------------------------------------------------
# A tied emission group is dict(tied=True, cov_type, post, prior, w_post [S,K], w_prior [S,K]);
# anything else is a group of the oracle (`orc.emissions_estep`).

def _group_estep(X, grp):
    if not grp.get('tied'):
        pc, cache = orc.emissions_estep(X, [grp])
        return pc, cache[0]
    exp_T = orc.FAMILIES[grp['cov_type']]['exp'](*grp['post'])
    l = pool_llh(X, grp['cov_type'], exp_T)
    lw = orc.log_weights_set(np.asarray(grp['w_post'], dtype=np.float64))
    pc, _ = lognorm(l, lw)
    return pc, (l, lw, pc)


def _group_kl(grp):
    if not grp.get('tied'):
        return orc.emissions_kl([grp])
    return orc.family_kl(grp['cov_type'], grp['post'], grp['prior']).sum() + \
        orc.dir_kl(np.asarray(grp['w_post'], dtype=np.float64),
                   np.asarray(grp['w_prior'], dtype=np.float64)).sum()


def hmm_step(utts, groups, graphs, datasize=-1, scale=1., viterbi=False, extra_kl=0.):
    '''`accumulate_elbo` of an HMM over `groups`: value = sum_u (N / T_u) sum_t exp_llh - U KL
    and, per group, (Gaussian statistics, weight statistics or None).  `graphs`: one
    dict(init, final, trans, order) for all utterances, or a list with one per utterance.'''
    utts = [np.asarray(u, dtype=np.float64) for u in utts]
    if datasize <= 0:
        datasize = sum(len(u) for u in utts)
    kl = sum(_group_kl(g) for g in groups) + extra_kl
    value, accs = 0., [None] * len(groups)
    resps = []
    for u, X in enumerate(utts):
        graph = graphs[u] if isinstance(graphs, (list, tuple)) else graphs
        steps = [_group_estep(X, g) for g in groups]
        pc_all = np.concatenate([pc for pc, _ in steps], axis=1)
        r = orc.hmm_estep(pc_all, graph['order'], graph['init'], graph['final'], graph['trans'],
                          scale=scale, viterbi=viterbi)
        value += datasize / float(len(X)) * r['exp_llh'].sum() - kl
        by_pdf = orc.scatter_states(scale * r['resps'], graph['order'], pc_all.shape[1])
        resps.append(r['resps'])
        first = 0
        for n, (grp, (pc, cache)) in enumerate(zip(groups, steps)):
            g = by_pdf[:, first:first + pc.shape[1]]
            first += pc.shape[1]
            if grp.get('tied'):
                C, _, acc = statistics(*cache, g, suffstats(X, grp['cov_type']))
                new = (acc, weight_stats(C))
            else:
                new = orc.emissions_accumulate([grp], [cache], g)[0]
            accs[n] = new if accs[n] is None else tuple(
                None if a is None else a + b for a, b in zip(accs[n], new))
    return {'value': value, 'kl': kl, 'acc': accs, 'resps': resps}


# ---- inputs shared by the host and the GPU tests --------------------------------------------

def random_pool(rng, K, D, cov_type, spread=3.):
    'Standard parameters (the oracle\'s order) of K Gaussians with means `spread` apart.'
    mean = spread * rng.standard_normal((K, D))
    scale = np.full((K, 1), 10.)
    if cov_type == 'full':
        dof = np.full((K, 1), D + 10.)
        A = rng.standard_normal((K, D, D)) * .2
        W = (np.eye(D)[None] + A @ A.transpose(0, 2, 1)) / dof[:, :, None]
        return mean, scale, W, dof
    shape = np.full((K, 1), 10.)
    if cov_type == 'diagonal':
        return mean, scale, shape, 10. * rng.uniform(.5, 1.5, (K, D))
    return mean, scale, shape, 10. * rng.uniform(.5, 1.5, (K, 1))


def frames_from_pool(rng, post, T, which=None):
    'T frames, each the mean of a Gaussian of the pool (one of `which`) plus unit noise.'
    mean = post[0]
    which = np.arange(len(mean)) if which is None else np.asarray(which)
    return mean[which[rng.integers(0, len(which), T)]] + rng.standard_normal((T, mean.shape[1]))


def state_posteriors(rng, T, S):
    'Rows on the simplex with exact zeros among them.'
    g = rng.dirichlet(np.full(S, .3), T)
    g[g < 1e-3] = 0.
    return g


def kernel_case(seed, S, K, D, T, cov_type, dtype='float64', conc=(1., 4.)):
    '''Inputs of a kernel-level case, rounded to `dtype` and returned in float64 (the
    log-weights, which the kernels take in fp64, as they are): frames drawn from the pool,
    Dirichlet rows with concentrations uniform in `conc`.'''
    rng = np.random.default_rng(seed)
    post = random_pool(rng, K, D, cov_type)
    X = frames_from_pool(rng, post, T).astype(dtype).astype(np.float64)
    exp_T = orc.FAMILIES[cov_type]['exp'](*post)
    l = pool_llh(X, cov_type, exp_T).astype(dtype).astype(np.float64)
    alpha = rng.uniform(conc[0], conc[1], (S, K))
    lw = orc.log_weights_set(alpha)                       # (fp64 whatever the dtype)
    g = state_posteriors(rng, T, S).astype(dtype).astype(np.float64)
    return {'X': X, 'l': l, 'lw': lw, 'g': g, 'alpha': alpha, 'post': post, 'exp_T': exp_T}


def sparse_rows(rng, S, K, own=8):
    '''Dirichlet rows [S, K]: state s uses the `own` components s * own .. and has
    concentration 1 / K on all others (E[ln pi] about -K there).'''
    alpha = np.full((S, K), 1. / K)
    for s in range(S):
        alpha[s, s * own:(s + 1) * own] = rng.uniform(1., 4., own)
    return alpha


def extreme_case(seed, S=4, K=128, D=8, T=300, cov_type='diagonal', dtype='float32', own=8):
    '''Range case (b): `sparse_rows` and a pool whose means are 30 standard deviations apart,
    every frame next to a component one of the states uses -- for the other states the
    linear-domain sum underflows although their log-normaliser is finite.'''
    rng = np.random.default_rng(seed)
    post = random_pool(rng, K, D, cov_type, spread=30.)
    X = frames_from_pool(rng, post, T, which=np.arange(S * own)).astype(dtype).astype(np.float64)
    exp_T = orc.FAMILIES[cov_type]['exp'](*post)
    l = pool_llh(X, cov_type, exp_T).astype(dtype).astype(np.float64)
    alpha = sparse_rows(rng, S, K, own)
    lw = orc.log_weights_set(alpha)                       # (fp64 whatever the dtype)
    g = state_posteriors(rng, T, S).astype(dtype).astype(np.float64)
    return {'X': X, 'l': l, 'lw': lw, 'g': g, 'alpha': alpha, 'post': post, 'exp_T': exp_T}


KERNEL_SHAPES = [(3, 8, 4, 50), (120, 256, 40, 333), (37, 100, 12, 200), (16, 64, 8, 1),
                 (130, 70, 5, 129), (5, 256, 16, 4200)]
RANGE_SHAPES = [(6, 32, 8, 400), (120, 256, 40, 300)]


def mstep(groups, accs, lrate=1.):
    '''`elbo.backward(); optim.step()` on every emission parameter (the whole data set as
    one batch: statistics unscaled); returns the new groups.'''
    new = []
    for grp, (acc, wstats) in zip(groups, accs):
        if not grp.get('tied'):
            new.append(orc.emissions_mstep([grp], [(acc, wstats)], 1., lrate)[0])
            continue
        f = orc.FAMILIES[grp['cov_type']]
        eta = orc.natural_grad_update(f['nat'](*grp['prior']), f['nat'](*grp['post']), acc, lrate)
        eta_w = orc.natural_grad_update(orc.dir_natural(grp['w_prior']),
                                        orc.dir_natural(grp['w_post']), wstats, lrate)
        new.append(dict(grp, post=f['from_nat'](eta), w_post=orc.dir_from_natural(eta_w)))
    return new
