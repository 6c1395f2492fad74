"""The small kernels every HMM path goes through, each against tests/plumbing_truth.py on the
table of batches of that module: gather_kernel, scatter_kernel, scatter_flat_kernel,
path_post_kernel, last_frame_kernel (csrc/hmm.hip), segment_sum_kernel, weights_from_acc_kernel
(csrc/estep.hip), `hk.gather_columns` / `hk.scatter_columns`.

The C entry points are called into the middle of sentinel-filled buffers: no guard element may
change, an output given as NULL stays unwritten, the inputs keep their bits.  What has one rounding
(the gather, a scatter to distinct pdf ids, one-hot posteriors, counts) must be the truth bit for
bit, and so must everything on inputs on a grid of 1/64, where every sum is exact; on random
inputs a sum stays within the rounding of its own terms, and the largest share of that bound is
printed."""

import functools
import itertools

import numpy as np
import pytest
import torch

import fb_truth as ft
import plumbing_truth as pt

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk, kernels               # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

DEV = 'cuda'
GUARD = 64
SENTINEL = -77.25
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = (torch.float32, torch.float64)
IDS = {torch.float32: 'f32', torch.float64: 'f64'}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64}
TABLE = [pytest.param(c, id=c.name) for c in pt.CASES]
ONE_GRAPH = [pytest.param(c, id=c.name) for c in pt.CASES if len(c.sizes) == 1]
MIXED = next(c for c in pt.CASES if len(c.sizes) > 1)
by_dtype = pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)


# --- buffers with guards -----------------------------------------------------------------------------

class Guarded:
    '''An output of `n` elements in the middle of a sentinel-filled buffer.  `init`: what the
    output holds before the call (None: the sentinel -- an element the kernel skips shows);
    `used=False`: the entry point gets NULL and the whole buffer must stay as it is.'''

    def __init__(self, what, n, dtype, init=None, used=True):
        self.what, self.n, self.used = what, n, used
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        if used and init is not None:
            self.mid[:] = init

    @property
    def mid(self):
        return self.buf[GUARD:GUARD + self.n]

    def ptr(self):
        return _hip.ptr(self.mid) if self.used else None

    def result(self):
        torch.cuda.synchronize()
        if not self.used:
            assert (self.buf == SENTINEL).all(), f'{self.what} = NULL, yet something was written'
            return None
        assert (self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + self.n:] == SENTINEL).all(), \
            f'a guard element of {self.what} was written'
        return npy(self.mid)


class unchanged:
    'The inputs of a call keep their bits.'

    def __init__(self, **tensors):
        self.tensors = tensors
        self.before = {k: t.clone() for k, t in tensors.items()}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        if exc[0] is None:
            for k, t in self.tensors.items():
                assert torch.equal(t.view(BITS[t.dtype]), self.before[k].view(BITS[t.dtype])), \
                    f'the input {k} was changed'


# --- comparisons -------------------------------------------------------------------------------------

def same_bits(got, want, what):
    'Equal bit for bit (so -0. is not 0.); a NaN of the truth is a NaN, whatever its payload.'
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f'{what}: {got.dtype} {got.shape}'
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{what}: NaN in other places than the truth'
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = (got.view(view) != want.view(view)) & ~nan
    assert not bad.any(), f'{what}: {int(bad.sum())} elements differ from the truth, first at ' \
                          f'{np.argwhere(bad)[0]}'


def exactly(got, want, what):
    'The (wider) truth is representable and `got` is it.'
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape}, not {want.shape}'
    bad = ~(got.astype(pt.HP) == want.astype(pt.HP))
    assert not bad.any(), f'{what}: {int(bad.sum())} elements are not the truth, first at ' \
                          f'{np.argwhere(bad)[0] if bad.ndim else ""}'


def share(got, want, tol, what):
    '''|got - want| <= tol with NaN exactly where the truth has it: the largest share of the bound
    that is used (where the bound is 0 the difference must be).'''
    got, want = np.asarray(got).astype(pt.HP), np.asarray(want).astype(pt.HP)
    tol = np.broadcast_to(np.asarray(tol, dtype=pt.HP), want.shape)
    assert got.shape == want.shape, f'{what}: shape {got.shape}, not {want.shape}'
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{what}: NaN in other places than the truth'
    d, tol = np.abs(got - want)[~nan], tol[~nan]
    assert (d[tol == 0] == 0).all(), f'{what}: off where the bound is 0'
    worst = float((d[tol > 0] / tol[tol > 0]).max(initial=0.))
    assert worst <= 1., f'{what}: off by {float(d.max()):.3e}, {worst:.3f} of the bound'
    return worst


# --- batches -----------------------------------------------------------------------------------------

def compiled(g, ids):
    return beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                    [int(i) for i in ids])


@functools.lru_cache(maxsize=None)
def batch_of(case, dtype):
    '(HmmBatch, ids per graph, S_total, states per utterance): built once per case and dtype.'
    ids, S_total, _ = pt.case_ids(case)
    graphs = [compiled(ft.make_graph(S, ft.offsets(2, S), case.seed + i, dtype=NP[dtype]), ids[i])
              for i, S in enumerate(case.sizes)]
    batch = hk.HmmBatch(graphs, list(case.gids), list(case.lens), dtype)
    assert batch.n_frames == sum(case.lens)
    return batch, ids, S_total, [case.sizes[g] for g in case.gids]


@functools.lru_cache(maxsize=None)
def data_of(case, dtype, kind):
    '''Inputs of a case, never changed: pc_all [n_frames, S_total], per utterance llh and gamma
    [T, S] and a state path [T].  kind 'grid': multiples of 1/64, llh in [-4, 0), gamma in [0, 1)
    -- every sum of the kernels is exact in float32; 'random': llh ~ 3 N(0, 1), gamma ~ U(0, 1).'''
    _, _, S_total, sizes = batch_of(case, dtype)
    rng = np.random.RandomState(case.seed + (1000 if kind == 'grid' else 2000))
    n = sum(case.lens)
    if kind == 'grid':
        pc_all = pt.grid(rng, (n, S_total), -4, 0, NP[dtype])
        llh = [pt.grid(rng, (T, S), -4, 0, NP[dtype]) for T, S in zip(case.lens, sizes)]
        gamma = [pt.grid(rng, (T, S), 0, 1, NP[dtype]) for T, S in zip(case.lens, sizes)]
    else:
        pc_all = (3 * rng.randn(n, S_total)).astype(NP[dtype])
        llh = [(3 * rng.randn(T, S)).astype(NP[dtype]) for T, S in zip(case.lens, sizes)]
        gamma = [rng.rand(T, S).astype(NP[dtype]) for T, S in zip(case.lens, sizes)]
    paths = [rng.randint(0, S, size=T) for T, S in zip(case.lens, sizes)]
    return pc_all, llh, gamma, paths


def packed(arrays, dtype):
    flat = np.concatenate([np.asarray(a).reshape(-1) for a in arrays]) if arrays else np.zeros(0)
    return tt(flat.astype(NP.get(dtype, np.int64)))


def frames_of(case):
    return np.concatenate([[0], np.cumsum(case.lens)]).astype(np.int64)


# --- gather ------------------------------------------------------------------------------------------

def c_gather(batch, pc_all, scale):
    out = Guarded('pc_llhs', batch.n_elems, batch.dtype)
    with unchanged(pc_all=pc_all):
        _hip.call('beer_hmm_gather', _hip.dtype_code(batch.dtype), batch.ref(), pc_all.shape[1],
                  _hip.ptr(pc_all), float(scale), out.ptr())
    return out.result()


@by_dtype
@pytest.mark.parametrize('case', TABLE)
def test_gather_is_the_truth_bit_for_bit(case, dtype):
    batch, ids, S_total, _ = batch_of(case, dtype)
    pc_np = data_of(case, dtype, 'random')[0].copy()
    rng = np.random.RandomState(case.seed)
    if pc_np.size:
        # -inf and NaN pass through; so does the sign of a zero
        used = np.unique(np.concatenate(ids))
        for value in (-np.inf, np.nan, -0.):
            pc_np[rng.randint(0, len(pc_np), 40), rng.choice(used, 40)] = value
    pc_all = tt(pc_np).reshape(len(pc_np), S_total)
    off = frames_of(case)
    for scale in (1., .7):
        want = [pt.gather(pc_np[off[u]:off[u + 1]], ids[g], scale, NP[dtype]).reshape(-1)
                for u, g in enumerate(case.gids)]
        want = np.concatenate(want) if want else np.zeros(0, dtype=NP[dtype])
        same_bits(c_gather(batch, pc_all, scale), want, f'gather, scale {scale}')
        same_bits(npy(hk.gather(batch, pc_all, scale)), want, f'hk.gather, scale {scale}')
    if pc_np.size:
        assert np.isnan(want).any() and (want == -np.inf).any()


# --- scatter -----------------------------------------------------------------------------------------

def c_scatter(batch, S_total, pc, gamma, scale, want_resps, want_exp_llh, utt_init):
    '''beer_hmm_scatter: (sr [n_frames, S_total], exp_llh [n_frames], utt_llh [nutt]), None for an
    output that was not asked for.  `utt_init`: what utt_llh holds before the call, or None.'''
    f = batch.n_frames
    sr = Guarded('state_resps', f * S_total, batch.dtype, init=0., used=want_resps)
    el = Guarded('exp_llh', f, batch.dtype, used=want_exp_llh)
    ul = Guarded('utt_llh', batch.nutt, torch.float64, init=utt_init, used=utt_init is not None)
    with unchanged(pc=pc, gamma=gamma):
        _hip.call('beer_hmm_scatter', _hip.dtype_code(batch.dtype), batch.ref(), S_total,
                  _hip.ptr(pc), _hip.ptr(gamma), float(scale), sr.ptr(), el.ptr(), ul.ptr())
    sr = sr.result()
    return None if sr is None else sr.reshape(f, S_total), el.result(), ul.result()


def scatter_truth(case, dtype, llh, gamma, scale):
    '''Per batch: (sr, exp_llh, utt_llh), the same over absolute values, and per column of sr of
    every frame the number of states that share it.'''
    _, ids, S_total, sizes = batch_of(case, dtype)
    parts = [pt.scatter(llh[u], gamma[u], ids[g], S_total, scale) for u, g in enumerate(case.gids)]
    absol = [pt.scatter_abs(llh[u], gamma[u], ids[g], S_total, scale)
             for u, g in enumerate(case.gids)]
    shared = [np.broadcast_to(np.bincount(ids[g], minlength=S_total), (case.lens[u], S_total))
              for u, g in enumerate(case.gids)]

    def cat(parts):
        if not parts:
            return np.zeros((0, S_total), dtype=pt.HP), np.zeros(0, dtype=pt.HP), np.zeros(0, dtype=pt.HP)
        return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                np.array([p[2] for p in parts], dtype=pt.HP))
    return cat(parts), cat(absol), (np.concatenate(shared) if shared else np.zeros((0, S_total)))


def scatter_bounds(case, dtype, absol, shared):
    '''sr: r u sum|terms| (r products and r - 1 adds in any order; one state: the one rounded
    product); exp_llh: gamma_S(u) sum_s |pc gamma|; utt_llh: gamma_S(u) sum|terms| + T S 2^-53
    sum|terms| (the terms in the kernel's type, their sum in float64).'''
    _, _, _, sizes = batch_of(case, dtype)
    u = pt.U[NP[dtype]]
    S_of_frame = np.repeat(np.asarray(sizes, dtype=np.float64), np.asarray(case.lens, dtype=np.int64))
    elems = np.asarray([T * S for T, S in zip(case.lens, sizes)], dtype=np.float64)
    return (shared * u * absol[0], pt.gamma_n(S_of_frame, u) * absol[1],
            (pt.gamma_n(np.asarray(sizes, dtype=np.float64), u) + elems * 2. ** -53) * absol[2])


COMBOS = list(itertools.product((True, False), (True, False), (True, False)))


@by_dtype
@pytest.mark.parametrize('case', TABLE)
def test_scatter_on_a_grid_is_exact(case, dtype):
    'Both kernels, every output on and off; utt_llh and sr are added to what they hold.'
    batch, ids, S_total, _ = batch_of(case, dtype)
    _, llh, gamma, _ = data_of(case, dtype, 'grid')
    pc, g = packed(llh, dtype), packed(gamma, dtype)
    (sr, el, ul), _, _ = scatter_truth(case, dtype, llh, gamma, .5)
    before = .25 + 1.5 * np.arange(batch.nutt)
    for want_exp_llh, want_resps, given in COMBOS:
        what = f'exp_llh {want_exp_llh}, resps {want_resps}, utt_llh {given}'
        got = c_scatter(batch, S_total, pc, g, .5, want_resps, want_exp_llh,
                        tt(before) if given else None)
        if want_resps:
            exactly(got[0], sr, f'{what}: state_resps')
        if want_exp_llh:
            exactly(got[1], el, f'{what}: exp_llh')
        if given:
            exactly(got[2], before + ul, f'{what}: utt_llh')
    # the Python face
    utt = tt(before.copy())
    got_sr, got_el = hk.scatter(batch, pc, g, S_total, .5, utt_llh=utt)
    exactly(npy(got_sr), sr, 'hk.scatter: state_resps')
    exactly(npy(got_el), el, 'hk.scatter: exp_llh')
    exactly(npy(utt), before + ul, 'hk.scatter: utt_llh')
    got_sr, got_el = hk.scatter(batch, pc, g, S_total, .5, want_resps=False, want_exp_llh=False)
    assert got_sr is None and got_el is None


@by_dtype
@pytest.mark.parametrize('case', TABLE)
def test_scatter_of_random_inputs_stays_within_its_rounding(case, dtype):
    batch, ids, S_total, _ = batch_of(case, dtype)
    _, llh, gamma, _ = data_of(case, dtype, 'random')
    pc, g = packed(llh, dtype), packed(gamma, dtype)
    scale = float(NP[dtype](.7))                       # the factor the kernel multiplies with
    (sr, el, ul), absol, shared = scatter_truth(case, dtype, llh, gamma, scale)
    tol_sr, tol_el, tol_ul = scatter_bounds(case, dtype, absol, shared)
    distinct = shared.max(initial=1) <= 1
    worst = {'state_resps': 0., 'exp_llh': 0., 'utt_llh': 0., 'utt_llh (flat)': 0.}
    for want_exp_llh, want_resps, given in COMBOS:
        what = f'exp_llh {want_exp_llh}, resps {want_resps}, utt_llh {given}'
        got = c_scatter(batch, S_total, pc, g, .7, want_resps, want_exp_llh,
                        tt(np.zeros(batch.nutt)) if given else None)
        if want_resps and distinct:
            # one rounded product into a zero-filled row
            once = [pt.scatter_once(gamma[u], ids[i], S_total, .7, NP[dtype])
                    for u, i in enumerate(case.gids)]
            same_bits(got[0], np.concatenate(once) if once else sr.astype(NP[dtype]),
                      f'{what}: state_resps')
        elif want_resps:
            worst['state_resps'] = max(worst['state_resps'],
                                       share(got[0], sr, tol_sr, f'{what}: state_resps'))
        if want_exp_llh:
            worst['exp_llh'] = max(worst['exp_llh'], share(got[1], el, tol_el, f'{what}: exp_llh'))
        if given:
            key = 'utt_llh' if want_exp_llh else 'utt_llh (flat)'
            worst[key] = max(worst[key], share(got[2], ul, tol_ul, f'{what}: {key}'))
    print(f'scatter {case.name} {IDS[dtype]}: ' +
          ', '.join(f'{k} within {v:.3f} of the bound' for k, v in worst.items()))


@by_dtype
def test_scatter_minus_infinity_where_the_posterior_is_zero(dtype):
    '''pc = -inf where gamma = 0: 0 * -inf is NaN in the reference's (pc * gamma).sum() and in the
    kernels -- in exactly that frame and that utterance, in no other and not in state_resps.'''
    S, lens = 65, [3, 0, 5, 2]
    ids, S_total, _ = pt.pdf_ids(S, 'subset', 5)
    graph = compiled(ft.make_graph(S, ft.offsets(2, S), 5, dtype=NP[dtype]), ids)
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    rng = np.random.RandomState(6)
    llh = [(3 * rng.randn(T, S)).astype(NP[dtype]) for T in lens]
    gamma = [rng.rand(T, S).astype(NP[dtype]) for T in lens]
    for u, t, s in ((0, 1, 64), (2, 4, 0), (2, 0, 63)):
        llh[u][t, s], gamma[u][t, s] = -np.inf, 0.
    parts = [pt.scatter(l, g, ids, S_total, 1.) for l, g in zip(llh, gamma)]
    absol = [pt.scatter_abs(np.where(np.isinf(l), 0., l), g, ids, S_total, 1.)
             for l, g in zip(llh, gamma)]
    el, ul = np.concatenate([p[1] for p in parts]), np.array([p[2] for p in parts])
    assert np.isnan(el).sum() == 3 and np.isnan(ul).tolist() == [True, False, True, False]
    u_ = pt.U[NP[dtype]]
    tol_el = pt.gamma_n(S, u_) * np.concatenate([a[1] for a in absol])
    tol_ul = (pt.gamma_n(S, u_) + np.asarray(lens) * S * 2. ** -53) * np.array([a[2] for a in absol])
    pc, g = packed(llh, dtype), packed(gamma, dtype)
    worst = []
    for want_exp_llh in (True, False):
        sr, got_el, got_ul = c_scatter(batch, S_total, pc, g, 1., True, want_exp_llh,
                                       tt(np.zeros(len(lens))))
        same_bits(sr, np.concatenate([pt.scatter_once(g_, ids, S_total, 1., NP[dtype])
                                      for g_ in gamma]), 'state_resps')
        if want_exp_llh:
            worst.append(share(got_el, el, tol_el, 'exp_llh'))
        worst.append(share(got_ul, ul, tol_ul, f'utt_llh, exp_llh {want_exp_llh}'))
    print(f'scatter with -inf {IDS[dtype]}: exp_llh within {worst[0]:.3f} of the bound, utt_llh '
          f'within {worst[1]:.3f}, utt_llh (flat) within {worst[2]:.3f}')


# --- one-hot posteriors of a path --------------------------------------------------------------------

def c_path_posteriors(batch, path, S, want_xi):
    gamma = Guarded('gamma', batch.n_elems, batch.dtype)
    xi = Guarded('xi_sum', S * S, torch.float64, init=0., used=want_xi)
    g0 = Guarded('gamma0_sum', S, torch.float64, init=0., used=want_xi)
    with unchanged(path=path):
        _hip.call('beer_hmm_path_posteriors', _hip.dtype_code(batch.dtype), batch.ref(),
                  _hip.ptr(path), gamma.ptr(), xi.ptr(), g0.ptr())
    xi = xi.result()
    return gamma.result(), None if xi is None else xi.reshape(S, S), g0.result()


@by_dtype
@pytest.mark.parametrize('case', ONE_GRAPH)
def test_path_posteriors_are_one_hot_and_the_counts_exact(case, dtype):
    batch, _, _, _ = batch_of(case, dtype)
    S = case.sizes[0]
    paths = data_of(case, dtype, 'random')[3]
    path = packed(paths, torch.int64)
    onehot, xi, g0, last = pt.path_posteriors(paths, S)
    flat = np.concatenate([o.reshape(-1) for o in onehot]) if onehot else np.zeros(0)
    for want_xi in (True, False):
        got = c_path_posteriors(batch, path, S, want_xi)
        same_bits(got[0], flat.astype(NP[dtype]), f'gamma, xi {want_xi}')
        if want_xi:
            same_bits(got[1], xi, 'xi_sum')
            same_bits(got[2], g0, 'gamma0_sum')
    gamma, got_xi, got_g0 = hk.path_posteriors(batch, path, want_xi=True)
    same_bits(npy(gamma), flat.astype(NP[dtype]), 'hk.path_posteriors: gamma')
    same_bits(npy(got_xi), xi, 'hk.path_posteriors: xi')
    same_bits(npy(got_g0), g0, 'hk.path_posteriors: gamma0')
    assert hk.path_posteriors(batch, path)[1:] == (None, None)
    # how often a state ends an utterance: an utterance of no frames ends in none
    kind, same_xi, got_last = hk.path_counts(batch, path, got_xi)
    assert kind == 'dense' and same_xi is got_xi
    same_bits(npy(got_last), last, 'hk.path_counts: last')
    assert last.sum() == sum(T > 0 for T in case.lens)


def test_path_counts_with_a_leading_and_a_trailing_empty_utterance():
    'The last states by hand: [-, 2, -, 0, 2, -] -> state 0 once, state 2 twice.'
    g = ft.make_graph(3, ft.offsets(2, 3), 0)
    lens = [0, 2, 0, 1, 3, 0]
    batch = hk.HmmBatch([compiled(g, range(3))], [0] * 6, lens, torch.float64)
    path = tt(np.array([1, 2, 0, 1, 1, 2], dtype=np.int64))
    _, xi, g0 = hk.path_posteriors(batch, path, want_xi=True)
    assert npy(hk.path_counts(batch, path, xi)[2]).tolist() == [1., 0., 2.]
    assert npy(g0).tolist() == [1., 2., 0.] and npy(xi).sum() == 3
    only_empty = hk.HmmBatch([compiled(g, range(3))], [0, 0], [0, 0], torch.float64)
    none = tt(np.zeros(0, dtype=np.int64))
    _, xi, g0 = hk.path_posteriors(only_empty, none, want_xi=True)
    assert not npy(hk.path_counts(only_empty, none, xi)[2]).any() and not npy(xi).any()


@by_dtype
def test_path_posteriors_of_a_batch_that_mixes_graphs(dtype):
    'gamma is one-hot with every utterance\'s own S; transition counts are refused.'
    batch, _, _, sizes = batch_of(MIXED, dtype)
    paths = data_of(MIXED, dtype, 'random')[3]
    path = packed(paths, torch.int64)
    flat = np.concatenate([(p[:, None] == np.arange(S)[None, :]).reshape(-1)
                           for p, S in zip(paths, sizes)]).astype(NP[dtype])
    same_bits(c_path_posteriors(batch, path, max(sizes), False)[0], flat, 'gamma')
    same_bits(npy(hk.path_posteriors(batch, path)[0]), flat, 'hk.path_posteriors: gamma')
    with pytest.raises(ValueError):
        hk.path_posteriors(batch, path, want_xi=True)
    with pytest.raises(_hip.HipInvalid):
        c_path_posteriors(batch, path, max(sizes), True)


# --- the posteriors of the last frames ---------------------------------------------------------------

def c_last_frame_sum(batch, gamma, S, init):
    out = Guarded('out', S, torch.float64, init=init)
    with unchanged(gamma=gamma):
        _hip.call('beer_hmm_last_frame_sum', _hip.dtype_code(batch.dtype), batch.ref(),
                  _hip.ptr(gamma), out.ptr())
    return out.result()


@by_dtype
@pytest.mark.parametrize('case', ONE_GRAPH)
def test_last_frame_sum(case, dtype):
    batch, _, _, _ = batch_of(case, dtype)
    S = case.sizes[0]
    # on the grid: exact, and added to what `out` holds
    gamma = data_of(case, dtype, 'grid')[2]
    before = .5 + .25 * np.arange(S)
    want = pt.last_frame_sum(gamma, S)
    g = packed(gamma, dtype)
    exactly(c_last_frame_sum(batch, g, S, tt(before)), before + want, 'out, preloaded')
    exactly(npy(hk.last_frame_sum(batch, g)), want, 'hk.last_frame_sum')
    out = tt(before.copy())
    assert hk.last_frame_sum(batch, g, out=out) is out
    exactly(npy(out), before + want, 'hk.last_frame_sum, out given')
    # random: nutt adds in any order
    gamma = data_of(case, dtype, 'random')[2]
    want = pt.last_frame_sum(gamma, S)
    tol = len(case.lens) * 2. ** -53 * pt.last_frame_sum([np.abs(x) for x in gamma], S)
    worst = share(c_last_frame_sum(batch, packed(gamma, dtype), S, 0.), want, tol, 'out')
    print(f'last_frame_sum {case.name} {IDS[dtype]}: within {worst:.3f} of the bound')
    if case.lens:
        assert (want > 0).all()                     # every state, the strided ones too, got its sum


@by_dtype
def test_last_frame_sum_refuses_a_batch_that_mixes_graphs(dtype):
    batch, _, _, _ = batch_of(MIXED, dtype)
    g = packed(data_of(MIXED, dtype, 'grid')[2], dtype)
    with pytest.raises(ValueError):
        hk.last_frame_sum(batch, g)
    with pytest.raises(_hip.HipInvalid):
        c_last_frame_sum(batch, g, 300, 0.)


# --- per-utterance sums ------------------------------------------------------------------------------

SEG_LENGTHS = (0, 1, 255, 0, 256, 257, 1000, 0)


def c_segment_sum(values, off, nutt, init):
    out = Guarded('out', nutt, torch.float64, init=init)
    with unchanged(values=values, frame_off=off):
        _hip.call('beer_segment_sum', _hip.dtype_code(values.dtype), nutt, _hip.ptr(off),
                  _hip.ptr(values), out.ptr())
    return out.result()


@by_dtype
def test_segment_sum(dtype):
    rng = np.random.RandomState(7)
    off_np = np.concatenate([[0], np.cumsum(SEG_LENGTHS)]).astype(np.int64)
    off, nutt = tt(off_np), len(SEG_LENGTHS)
    # on the grid: exact, and added to what `out` holds
    v = pt.grid(rng, off_np[-1], -4, 4, NP[dtype])
    before = 3. - .5 * np.arange(nutt)
    want = pt.segment_sum(v, off_np)
    exactly(c_segment_sum(tt(v), off, nutt, tt(before)), before + want, 'out, preloaded')
    exactly(npy(hk.segment_sum(tt(v), off, nutt)), want, 'hk.segment_sum')
    out = tt(before.copy())
    assert hk.segment_sum(tt(v), off, nutt, out=out) is out
    exactly(npy(out), before + want, 'hk.segment_sum, out given')
    # random: each utterance's T terms summed in float64, in any order
    v = (3 * rng.randn(off_np[-1])).astype(NP[dtype])
    tol = np.asarray(SEG_LENGTHS) * 2. ** -53 * pt.segment_sum(np.abs(v), off_np)
    worst = share(c_segment_sum(tt(v), off, nutt, 0.), pt.segment_sum(v, off_np), tol, 'out')
    print(f'segment_sum {IDS[dtype]}: within {worst:.3f} of the bound')
    # no utterance: nothing is read or written
    assert c_segment_sum(tt(v), off, 0, None).shape == (0,)
    assert hk.segment_sum(tt(v), off, 0).shape == (0,)


# --- mixture-weight statistics -----------------------------------------------------------------------

@pytest.mark.parametrize('Q', (2, 6))
@pytest.mark.parametrize('G', (1, 2, 64, 65, 130))
@pytest.mark.parametrize('S', (1, 3))
def test_weights_from_acc(S, G, Q):
    rng = np.random.RandomState(S * 1000 + G * 10 + Q)
    acc_np = rng.randint(-64, 65, size=(S * G, Q)) / 8.              # dyadic: every sum is exact
    want = pt.weights_from_acc(acc_np, S, G)
    acc = tt(acc_np)
    with unchanged(acc=acc):
        got = npy(kernels.weights_from_acc(acc, S, G))
    exactly(got, want, 'weights')
    # the last column: the sum of the others plus its own term
    own = -2. * acc_np[:, Q - 2].reshape(S, G)[:, G - 1]
    assert np.array_equal(got[:, G - 1], got[:, :G - 1].sum(1) + own)
    # `out` is added to
    before = .5 * np.arange(S * G).reshape(S, G) - 3.
    out = Guarded('out', S * G, torch.float64, init=tt(before.reshape(-1)))
    _hip.call('beer_weights_from_acc', S, G, Q, _hip.ptr(acc), out.ptr())
    exactly(out.result().reshape(S, G), before + want, 'weights, preloaded')


# --- columns of a matrix -----------------------------------------------------------------------------

@by_dtype
@pytest.mark.parametrize('T', (1, 33))
def test_gather_and_scatter_columns(T, dtype):
    rng = np.random.RandomState(T)
    n_total = 70
    order = rng.randint(0, n_total - 3, size=90)              # repeated columns, and missing ones
    order[:3] = order[-3:]
    assert len(set(order)) < len(order) and len(set(order)) < n_total
    m = (3 * rng.randn(T, n_total)).astype(NP[dtype])
    same_bits(npy(hk.gather_columns(tt(m), order)), m[:, order], 'gather_columns')
    one = rng.permutation(n_total)[:40]
    same_bits(npy(hk.gather_columns(tt(m), one)), m[:, one], 'gather_columns, distinct')
    # scatter: exact on the grid; a column nobody names stays 0
    r = pt.grid(rng, (T, len(order)), 0, 1, NP[dtype])
    want = np.zeros((T, n_total))
    np.add.at(want.T, order, r.astype(np.float64).T)
    got = npy(hk.scatter_columns(tt(r), order, n_total))
    assert got.dtype == NP[dtype]
    exactly(got, want, 'scatter_columns')
    assert not got[:, sorted(set(range(n_total)) - set(order))].any()
    r = rng.rand(T, len(one)).astype(NP[dtype])
    want = np.zeros((T, n_total), dtype=NP[dtype])
    want[:, one] = r
    same_bits(npy(hk.scatter_columns(tt(r), one, n_total)), want, 'scatter_columns, distinct')
