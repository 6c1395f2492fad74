"""The CMLLR kernels (csrc/cmllr.hip) and what is built on them against tests/cmllr_truth.py.

Kernel bound, derived: the inputs are exact in float64 (float32 ones too), a product of three
factors rounds once before the matrix core and once in it, and a running sum of n terms rounds n
times, so every entry obeys  |got - truth| <= (n + 4) 2^-52 sum |terms|  with the truth's own
sum of absolute terms; `cmllr_apply` adds half a unit in the last place of the output's dtype.
Every entry of every case is compared.

Model level: `cmllr_statistics_batch` against the truth's formulas fed with the library's own
dense responsibilities and `HMM.posteriors` of the transformed frames, at the suite's TOL (1e-10
float64, 1e-5 float32) relative to sum |terms|; EM's own guarantee for `adapt`; the CLI."""

import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

import cmllr_truth as ct

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, kernels                                  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402
from beer_amd.stats import FrameStats                               # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
EPS = 2. ** -52


def hold(got, truth, what, extra=0.):
    'Every entry of `got` within (n + 4) 2^-52 sum |terms| (+ extra) of the truth triple.'
    value, mag, n = truth
    got = np.asarray(got, dtype=np.longdouble)
    assert got.shape == value.shape, what
    n = np.asarray(n, dtype=np.longdouble)
    while n.ndim and n.ndim < value.ndim:
        n = n[..., None]
    bound = (n + 4) * EPS * mag + extra
    err = np.abs(got - value)
    with np.errstate(divide='ignore', invalid='ignore'):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.)), initial=0.)
    print(f'{what}: worst entry at {float(worst):.3f} of its bound')
    assert (err <= bound).all(), what


def exact32(rng, *shape, scale=1.):
    'Random values that float32 holds exactly (so both precisions see the same inputs).'
    return (rng.randn(*shape) * scale).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------
# cmllr_frame_params

SG = [(1, 1), (7, 1), (1, 5), (3, 4), (2, 257)]
FP_D, FP_T = [1, 3, 40, 63], [1, 63, 64, 65, 257]


def fp_cases(sg):
    'Every D with both covariance types (T by rotation), and every T at D = 3.'
    n = SG.index(sg)
    cases = [(D, FP_T[(n + i + j) % 5], cov) for i, D in enumerate(FP_D)
             for j, cov in enumerate(('diagonal', 'isotropic'))]
    cases += [(3, T, ('diagonal', 'isotropic')[(n + i) % 2]) for i, T in enumerate(FP_T)]
    return sorted(set(cases))


@functools.lru_cache(maxsize=None)
def fp_data(S, G, D, T, cov):
    rng = np.random.RandomState(S * 1000 + G * 10 + D + T)
    K, P = S * G, D if cov == 'diagonal' else 1
    cr = [None if G == 1 else rng.randint(0, 1025, (T, K)) / 1024. for _ in range(2)]
    sr = [rng.randint(0, 1025, (T, S)) / 1024. for _ in range(2)]
    if S == 1 and G > 1:
        sr[0] = None                                      # a plain mixture: no state posteriors
    E = np.concatenate([exact32(rng, K, D, scale=3.), np.abs(exact32(rng, K, P)) + .5,
                        exact32(rng, K, 2)], axis=1).astype(np.float32).astype(np.float64)
    truths = [ct.frame_params(cr[i], sr[i], E, S, G, D, P) for i in range(2)]
    return cr, sr, E, P, truths


@DTYPES
@pytest.mark.parametrize('sg', SG, ids=[f'{s}x{g}' for s, g in SG])
def test_frame_params(sg, dtype):
    S, G = sg
    assert {c[0] for c in fp_cases(sg)} == set(FP_D) and {c[1] for c in fp_cases(sg)} == set(FP_T)
    for D, T, cov in fp_cases(sg):
        cr, sr, E, P, truths = fp_data(S, G, D, T, cov)
        dev = [None if a is None else tt(a, dtype) for a in cr + sr]
        out = kernels.cmllr_frame_params(dev[0], dev[2], tt(E, dtype), S, G, D, cov)
        assert out.dtype == torch.float64 and out.shape == (T, P + D + 1)
        what = f'frame_params {S}x{G} D={D} T={T} {cov}'
        hold(npy(out), truths[0], what)
        # a second call adds into the first call's output
        again = kernels.cmllr_frame_params(dev[1], dev[3], tt(E, dtype), S, G, D, cov, out=out)
        assert again is out
        both = (truths[0][0] + truths[1][0], truths[0][1] + truths[1][1], 2 * S * G)
        hold(npy(out), both, what + ' (+=)')


# ---------------------------------------------------------------------------
# cmllr_accumulate, cmllr_apply

ACC_D = [1, 3, 15, 16, 17, 40, 63]
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 257]
# utterances interleaved out of speaker order; with 3 and 5 speakers one has no utterance
SPEAKERS = {1: [0] * 8, 3: [2, 0, 2, 0, 0, 2, 0, 2], 5: [4, 0, 3, 1, 0, 4, 1, 3]}
CHUNK = 48                          # a speaker of several hundred frames spans several items
ACC_CASES = [(D, P, (1, 3, 5)[(i + j) % 3]) for i, D in enumerate(ACC_D)
             for j, P in enumerate(sorted({1, D}))]


@functools.lru_cache(maxsize=None)
def acc_data(D, P, n_spk):
    rng = np.random.RandomState(100 * D + 10 * P + n_spk)
    T = sum(LENGTHS)
    X = exact32(rng, T, D, scale=2.)
    prm = [np.concatenate([np.abs(rng.randn(T, P)) + .1, rng.randn(T, D), rng.rand(T, 1)], axis=1)
           for _ in range(2)]
    spk = SPEAKERS[n_spk]
    truths = [ct.statistics(X, p, LENGTHS, spk, n_spk, P) for p in prm]
    return X, prm, spk, truths


def hold_stats(got, truths, what, calls=1):
    G, k, beta = (npy(t) for t in got)
    for name, arr, triples in (('G', G, [t[0] for t in truths]), ('k', k, [t[1] for t in truths]),
                               ('beta', beta, [t[2] for t in truths])):
        value = sum(t[0] for t in triples[:calls])
        mag = sum(t[1] for t in triples[:calls])
        n = triples[0][2] * calls
        if name == 'G':
            value, mag = ct.pack_lower(value), ct.pack_lower(mag)
        hold(arr, (value, mag, n), f'{what} {name}')


def test_the_accumulate_cases_cover_the_list():
    assert {c[0] for c in ACC_CASES} == set(ACC_D) and {c[2] for c in ACC_CASES} == {1, 3, 5}
    assert {c[:2] for c in ACC_CASES} == {(D, P) for D in ACC_D for P in (1, D)}
    for n_spk in (3, 5):
        assert set(range(n_spk)) - set(SPEAKERS[n_spk])          # a speaker with no utterance
    assert max(LENGTHS) > 4 * CHUNK


@DTYPES
@pytest.mark.parametrize('case', ACC_CASES, ids=[f'D{D}-P{P}-{n}spk' for D, P, n in ACC_CASES])
def test_accumulate(case, dtype):
    D, P, n_spk = case
    X, prm, spk, truths = acc_data(D, P, n_spk)
    Xd, p0, p1 = tt(X, dtype), tt(prm[0]), tt(prm[1])
    what = f'accumulate D={D} P={P} {n_spk} speakers'
    table = kernels.cmllr_table(LENGTHS, spk, n_spk, CHUNK)
    assert table.n_items > n_spk                                 # several chunks per speaker
    got = kernels.cmllr_accumulate(Xd, p0, LENGTHS, spk, n_spk, chunk_frames=CHUNK)
    E = D + 1
    assert [tuple(t.shape) for t in got] == [(n_spk, P, E * (E + 1) // 2), (n_spk, D, E), (n_spk,)]
    assert all(t.dtype == torch.float64 for t in got)
    hold_stats(got, truths, what)
    for s in set(range(n_spk)) - set(spk):                       # no utterance: nothing added
        assert all(float(t[s].abs().sum()) == 0. for t in got)
    # two runs give the same bits (and the table may be the caller's)
    rerun = kernels.cmllr_accumulate(Xd, p0, LENGTHS, spk, n_spk, chunk_frames=CHUNK, table=table)
    assert all(torch.equal(a, b) for a, b in zip(got, rerun))
    # a second call adds into the first
    kernels.cmllr_accumulate(Xd, p1, LENGTHS, spk, n_spk, *got, chunk_frames=CHUNK)
    hold_stats(got, truths, what + ' (+=)', calls=2)
    # the default chunk: one item per speaker here, the same sums
    whole = kernels.cmllr_accumulate(Xd, p0, LENGTHS, spk, n_spk)
    hold_stats(whole, truths, what + ' (default chunk)')


def test_accumulate_leaves_out_speaker_minus_one_and_refuses():
    X, prm, _, _ = acc_data(3, 3, 3)
    spk = [0, -1, 2, -1, 0, 2, -1, 2]
    truth = ct.statistics(X, prm[0], LENGTHS, spk, 3, 3)
    got = kernels.cmllr_accumulate(tt(X), tt(prm[0]), LENGTHS, spk, 3, chunk_frames=7)
    hold_stats(got, [truth], 'speaker -1')
    with pytest.raises(_hip.HipInvalid):
        kernels.cmllr_accumulate(tt(X), tt(prm[0]), LENGTHS, [3] + spk[1:], 3)
    with pytest.raises(_hip.HipInvalid):                         # P = 2 is neither 1 nor D
        kernels.cmllr_accumulate(tt(X), tt(prm[0][:, :6]), LENGTHS, spk, 3)
    X64 = torch.zeros(4, 64, dtype=torch.float64, device='cuda')
    with pytest.raises(_hip.HipInvalid):
        kernels.cmllr_accumulate(X64, torch.zeros(4, 129, dtype=torch.float64, device='cuda'),
                                 [4], [0], 1)


@DTYPES
@pytest.mark.parametrize('D', ACC_D)
def test_apply(D, dtype):
    rng = np.random.RandomState(D)
    T = sum(LENGTHS)
    X = exact32(rng, T, D, scale=2.)
    W = np.concatenate([np.eye(D) + .3 * rng.randn(4, D, D), rng.randn(4, D, 1)], axis=2)
    spk = [3, 0, -1, 1, 0, 3, -1, 1]                              # interleaved; 2 unused; -1 copies
    value, mag, n = ct.apply(X, W, LENGTHS, spk)
    Y = kernels.cmllr_apply(tt(X, dtype), tt(W), LENGTHS, spk)
    assert Y.dtype == dtype and Y.shape == (T, D)
    half_ulp = np.spacing(np.abs(np.asarray(value, dtype=np.float64)).astype(NP[dtype])) / 2.
    hold(npy(Y), (value, mag, n), f'apply D={D}', extra=half_ulp.astype(np.float64))
    copied = np.repeat(np.asarray(spk) < 0, LENGTHS)
    assert np.array_equal(npy(Y)[copied], X[copied].astype(NP[dtype]))
    with pytest.raises(_hip.HipInvalid):
        kernels.cmllr_apply(tt(X, dtype), tt(W), LENGTHS, [4] + spk[1:])


# ---------------------------------------------------------------------------
# the model level

_TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
         {'start_id': 1, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 2, 'trans_prob': .5},
         {'start_id': 2, 'end_id': 3, 'trans_prob': .5}, {'start_id': 3, 'end_id': 3, 'trans_prob': .5},
         {'start_id': 3, 'end_id': 4, 'trans_prob': .5}]
D3 = 3
UTT_LENS = [23, 5, 40, 17, 31, 9]
UTT_SPK = [1, 0, 2, 0, 1, 2]


def group_conf(n_normal, cov='diagonal', **more):
    return {'topology': _TOPO, 'n_normal_per_state': n_normal, 'prior_strength': 1.,
            'noise_std': 1., 'cov_type': cov, 'shared_cov': False, **more}


def make_loop(kind, dtype):
    torch.manual_seed(5)
    if kind == 'joint':
        conf = {'g': group_conf(2), 'h': group_conf(3)}
        grouped = {'g': ['u0', 'u1'], 'h': ['u2']}
    else:
        conf = {'g': group_conf(2, **({'cov_type': 'full'} if kind == 'full' else {}))}
        if kind == 'tied':
            del conf['g']['n_normal_per_state']
            conf['g']['shared_normal_pool'] = 5
        grouped = {'g': ['u0', 'u1', 'u2']}
    names = [u for us in grouped.values() for u in us]
    units, ems = hmm_cmds.build_units(conf, grouped, torch.zeros(D3), torch.ones(D3))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet')
    return (model.double() if dtype == torch.float64 else model.float()).to('cuda'), units


def make_mixture(dtype, cov='isotropic'):
    torch.manual_seed(6)
    ns = beer.NormalSet.create(torch.zeros(D3), torch.ones(D3), size=4, prior_strength=1.,
                               noise_std=1., cov_type=cov)
    model = beer.Mixture.create(ns)
    return (model.double() if dtype == torch.float64 else model.float()).to('cuda')


def utterances(dtype, seed=7):
    rng = np.random.RandomState(seed)
    return [tt(rng.randn(T, D3) * 1.5, dtype) for T in UTT_LENS]


def some_transforms(seed=8):
    rng = np.random.RandomState(seed)
    tr = beer.AffineTransforms(['a', 'b', 'c'], D3)
    tr.W = np.concatenate([np.eye(D3) + .2 * rng.randn(3, D3, D3), .5 * rng.randn(3, D3, 1)], axis=2)
    return tr


def model_truth(model, utts, tr, graphs=None):
    '''The truth's statistics from the library's own responsibilities and posteriors of the
    transformed frames, utterance by utterance.'''
    ys = tr.apply(utts, UTT_SPK)
    params = []
    if isinstance(model, beer.Mixture):
        ns = model.normalset
        cov, K = ns.cov_type, len(ns)
        E = ns.means_precisions.natural_form()
        for Y in ys:
            resps = kernels.mixtureset_estep(FrameStats(Y, cov), E, model._log_weights().view(1, K),
                                             1, K, cov)[1]
            params.append(ct.frame_params(npy(resps), None, npy(E), 1, K, D3, 1 if cov == 'isotropic' else D3)[0])
    else:
        from beer_amd.inference.batch import _groups, _normalset
        groups = _groups(model._emissions())
        S_total = sum(S for _, S, _ in groups)
        for u, Y in enumerate(ys):
            graph = model.graph if graphs is None else graphs[u]
            gamma = npy(model.posteriors(Y, inference_graph=None if graphs is None else graph))
            sr = np.zeros((len(Y), S_total), dtype=gamma.dtype)
            for j, pdf in enumerate(graph.pdf_id_mapping):
                sr[:, int(pdf)] += gamma[:, j]
            total, first = 0, 0
            for grp, S, G in groups:
                ns = _normalset(grp)
                E = ns.means_precisions.natural_form()
                resps = kernels.mixtureset_estep(FrameStats(Y, ns.cov_type), E, grp.leaf_log_weights(),
                                                 S, G, ns.cov_type)[1]
                total = total + ct.frame_params(npy(resps), sr[:, first:first + S], npy(E), S, G,
                                                D3, D3)[0]
                first += S
            params.append(total)
    prm = np.concatenate(params)
    X = np.concatenate([npy(u) for u in utts])
    P = prm.shape[1] - D3 - 1
    return X, prm, P, ct.statistics(X, prm, UTT_LENS, UTT_SPK, 3, P)


def hold_model(stats, truth, tol, what):
    X, prm, P, (G, k, beta) = truth
    for name, got, (value, mag, _) in (('G', stats.G, (ct.pack_lower(G[0]), ct.pack_lower(G[1]), 0)),
                                       ('k', stats.k, k), ('beta', stats.beta, beta)):
        err = np.abs(got - np.asarray(value, dtype=np.float64))
        bound = tol * np.asarray(mag, dtype=np.float64)
        print(f'{what} {name}: worst entry at {(err / np.maximum(bound, 1e-300)).max():.3f} of '
              'tol x sum |terms|')
        assert (err <= bound).all(), (what, name)
    # the objective of a random W against the truth's direct sum over the frames
    rng = np.random.RandomState(9)
    W = np.concatenate([np.eye(D3) + .3 * rng.randn(3, D3, D3), rng.randn(3, D3, 1)], axis=2)
    got = stats.objective(W)
    frames = np.repeat(UTT_SPK, UTT_LENS)
    for s in range(3):
        Xs, ps = X[frames == s], prm[frames == s]
        want = float(ct.objective_from_frames(W[s], Xs, ps, P))
        y = np.concatenate([Xs, np.ones((len(Xs), 1))], axis=1) @ W[s].T
        om, nu, c = np.asarray(ps[:, :P], float), np.asarray(ps[:, P:P + D3], float), np.asarray(ps[:, -1], float)
        mag = abs(c.sum() * np.linalg.slogdet(W[s][:, :D3])[1]) + np.abs(nu * y).sum() + .5 * (om * y * y).sum()
        assert abs(got[s] - want) <= tol * mag, (what, s)


@DTYPES
@pytest.mark.parametrize('kind', ['phoneloop', 'joint', 'mixture'])
def test_statistics_batch(kind, dtype):
    utts, tr = utterances(dtype), some_transforms()
    model = make_mixture(dtype) if kind == 'mixture' else make_loop(kind, dtype)[0]
    truth = model_truth(model, utts, tr)
    for max_frames in (1 << 20, 45):                    # one launch; several sub-batches
        stats = beer.cmllr_statistics_batch(model, utts, UTT_SPK, 3, transforms=tr,
                                            max_frames=max_frames, chunk_frames=16)
        assert stats.names == ['0', '1', '2'] and stats.G.shape[1] == (1 if kind == 'mixture' else D3)
        hold_model(stats, truth, TOL[dtype], f'{kind} max_frames={max_frames}')
    packed = beer.cmllr_statistics_batch(model, (torch.cat(utts), UTT_LENS), UTT_SPK, 3, transforms=tr)
    hold_model(packed, truth, TOL[dtype], f'{kind} packed')
    # without transforms: those of the identity
    plain = beer.cmllr_statistics_batch(model, utts, UTT_SPK, 3)
    ident = beer.cmllr_statistics_batch(model, utts, UTT_SPK, 3,
                                        transforms=beer.AffineTransforms('abc', D3))
    assert np.array_equal(plain.G, ident.G) and np.array_equal(plain.k, ident.k)


@DTYPES
def test_statistics_batch_with_alignment_graphs(dtype):
    model, units = make_loop('phoneloop', dtype)
    utts, tr = utterances(dtype), some_transforms()
    seqs = [['u0', 'u1'], ['u2'], ['u1', 'u0', 'u2'], ['u0'], ['u2', 'u1'], ['u1']]
    graphs = list(beer.graph.compile_alignments(seqs, units))
    truth = model_truth(model, utts, tr, graphs)
    for max_frames in (1 << 20, 45):
        stats = beer.cmllr_statistics_batch(model, utts, UTT_SPK, 3, transforms=tr,
                                            inference_graphs=graphs, max_frames=max_frames)
        hold_model(stats, truth, TOL[dtype], f'aligned max_frames={max_frames}')


def test_models_that_are_not_covered():
    utts = utterances(torch.float64)
    for kind in ('full', 'tied'):
        model = make_loop(kind, torch.float64)[0]
        with pytest.raises(NotImplementedError, match='full cov' if kind == 'full' else 'tied'):
            beer.cmllr_statistics_batch(model, utts, UTT_SPK, 3)
    with pytest.raises(NotImplementedError, match='full cov'):
        beer.cmllr_statistics_batch(make_mixture(torch.float64, 'full'), utts, UTT_SPK, 3)


def distorted_utterances(model, dtype, seed=11):
    '''Frames drawn from the loop's own Gaussians along a fixed path (every state held four
    frames, the units in turn), every speaker distorted by a known affine map.'''
    from beer_amd.inference.batch import _groups, _normalset
    grp, S, G = _groups(model._emissions())[0]
    E = npy(_normalset(grp).means_precisions.natural_form()).astype(np.float64)
    mu = E[:, :D3] / E[:, D3:2 * D3]
    rng = np.random.RandomState(seed)
    maps = [(np.eye(D3) * (1. + .3 * s) + .2 * rng.randn(D3, D3), rng.randn(D3)) for s in range(3)]
    out = []
    for T, s in zip(UTT_LENS, UTT_SPK):
        state = (np.arange(T) // 4) % S
        clean = mu[state * G + rng.randint(0, G, T)] + .3 * rng.randn(T, D3)
        out.append(tt(clean @ maps[s][0].T + maps[s][1], dtype))
    return out


@DTYPES
def test_adapt_is_em(dtype):
    model, _ = make_loop('phoneloop', dtype)
    utts = distorted_utterances(model, dtype)
    names = ['a', 'b', 'c']
    spk = [names[s] for s in UTT_SPK]

    def total(tr):
        ys = tr.apply(utts, spk)
        return float(beer.log_evidence_batch(model, ys).sum()) + tr.log_det_terms(UTT_LENS, spk).sum()
    tr = beer.AffineTransforms(names, D3)
    totals, tol = [total(tr)], TOL[dtype]
    for it in range(3):
        # (iteration by iteration, to score each: `adapt(iters=3)` is the same loop)
        tr, gains = beer.adapt(model, utts, spk, names, iters=1, transforms=tr, min_count=0.)
        totals.append(total(tr))
        assert (gains[0] >= 0).all()
    print(f'adapt {dtype}: log-evidence + log-determinants {totals}')
    for before, after in zip(totals, totals[1:]):
        assert after >= before - tol * abs(before)
    assert totals[1] > totals[0]
    whole, gains = beer.adapt(model, utts, spk, names, iters=3, min_count=0.)
    assert len(gains) == 3 and np.array_equal(whole.W, tr.W)


# ---------------------------------------------------------------------------
# the CLI

def cli(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_adapt_and_transform(tmp_path):
    model, _ = make_loop('phoneloop', torch.float32)
    utts = distorted_utterances(model, torch.float32)
    ids = [f'utt{u}' for u in range(len(utts))]
    arch, ds, mdl = str(tmp_path / 'feats.npz'), str(tmp_path / 'ds.pkl'), str(tmp_path / 'model.pkl')
    np.savez(arch, **{i: npy(u) for i, u in zip(ids, utts)})
    hmm_cmds._dump(model.cpu(), mdl)
    cli(['dataset', 'create', str(tmp_path), arch, ds])
    names = ['alice', 'bob', 'carol']
    u2s = str(tmp_path / 'utt2spk')
    with open(u2s, 'w') as f:
        f.writelines(f'{i} {names[s]}\n' for i, s in zip(ids, UTT_SPK))
    # carol's utterances (2 and 5) are not adapted on: she gets no transform
    used = [u for u in range(len(ids)) if UTT_SPK[u] != 2]
    out = str(tmp_path / 'transforms.npz')
    lines = cli(['hmm', 'adapt', '--iters', '2', '--min-count', '0', '-u', '-', mdl, ds, u2s, out],
                stdin=''.join(f'{ids[u]}\n' for u in used)).strip().split('\n')
    model = model.to('cuda')
    # (speakers in order of first appearance: utt0 is bob's -- index 1 -- then alice's utt1)
    remap = {1: 0, 0: 1}
    want, gains = beer.adapt(model, [utts[u] for u in used], [remap[UTT_SPK[u]] for u in used],
                             ['bob', 'alice'], iters=2, min_count=0.)
    got = beer.AffineTransforms.load(out)
    assert got.names == ['bob', 'alice'] and np.array_equal(got.W, want.W)
    frames = {'bob': UTT_LENS[0] + UTT_LENS[4], 'alice': UTT_LENS[1] + UTT_LENS[3]}
    total = np.sum(gains, axis=0)
    assert [l.split() for l in lines] == [[n, str(frames[n]), '%.6f' % g]
                                          for n, g in zip(got.names, total)]
    assert (total > 0).all()
    # --init: the transforms of the file are where the next run starts
    again = str(tmp_path / 'again.npz')
    cli(['hmm', 'adapt', '--iters', '1', '--min-count', '0', '--init', out, '-u', '-', mdl, ds, u2s,
         again], stdin=''.join(f'{ids[u]}\n' for u in used))
    more, _ = beer.adapt(model, [utts[u] for u in used], [remap[UTT_SPK[u]] for u in used],
                         ['bob', 'alice'], iters=1, min_count=0., transforms=want)
    assert np.array_equal(beer.AffineTransforms.load(again).W, more.W)
    # features transform: the archive, the log-determinant terms, carol copied
    new = str(tmp_path / 'adapted.npz')
    cli(['features', 'transform', arch, u2s, out, new])
    assert os.path.exists(new) and os.path.exists(new + '.logdet')
    spk = [names[s] for s in UTT_SPK]
    ys = got.apply(utts, spk)
    with np.load(new) as z:
        assert sorted(z.files) == sorted(ids)
        for i, y, x, s in zip(ids, ys, utts, spk):
            assert z[i].dtype == np.float32 and np.array_equal(z[i], npy(y))
            assert np.array_equal(z[i], npy(x)) == (s == 'carol')
    terms = got.log_det_terms(UTT_LENS, spk)
    with open(new + '.logdet') as f:
        assert [l.split() for l in f] == [[i, '%.6f' % t] for i, t in zip(ids, terms)]
    assert terms[2] == 0. and terms[5] == 0. and (terms[[0, 1, 3, 4]] != 0).all()
    # the transformed archive is an archive: `beer dataset create` takes it
    cli(['dataset', 'create', str(tmp_path), new, str(tmp_path / 'ds2.pkl')])
    assert hmm_cmds._load(str(tmp_path / 'ds2.pkl')).size == sum(UTT_LENS)
    # an utterance without a speaker is named
    with open(u2s, 'w') as f:
        f.writelines(f'{i} x\n' for i in ids[:-1])
    with pytest.raises(SystemExit, match='utt5'):
        cli(['features', 'transform', arch, u2s, out, new])
