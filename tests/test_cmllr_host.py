"""The host side of the speaker-adaptive transforms (beer_amd/adaptation.py, the CLI, the header
and the host-side refusals of csrc/cmllr.hip) against tests/cmllr_truth.py.  No GPU.

Bounds: the truth's two objectives agree to 1e-12 |Q| (longdouble sums of a few thousand terms);
a row step of `estimate` does not lower Q by more than 1e-12 |Q| (a numpy trial of the recursion
saw 1e-15); perturbations and gains as the issue of this feature sets them."""

import ctypes
import os

import numpy as np
import pytest

import cmllr_truth as ct

import beer_amd as beer
from beer_amd import _hip, kernels
from beer_amd.cli import features as fea_cmds, hmm as hmm_cmds, main as cli_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def speaker_data(T, D, iso, seed, K=3):
    '(X, params, P): frames of one distorted speaker and [omega | nu | c] of a small GMM.'
    rng = np.random.RandomState(seed)
    P = 1 if iso else D
    mu = rng.randn(K, D) * 2.
    lam = np.exp(rng.randn(K, P) * .3)
    z = rng.randint(0, K, T)
    A = np.eye(D) + .2 * rng.randn(D, D)
    X = (mu[z] + rng.randn(T, D) / np.sqrt(lam[z] if not iso else lam[z].repeat(D, 1))) @ A.T + \
        rng.randn(D) * .5
    resps = rng.dirichlet(np.ones(K) * .3, T)
    E = np.concatenate([mu * lam, lam, np.zeros((K, 2))], axis=1)
    params = ct.frame_params(resps, None, E, 1, K, D, P)[0]
    return X, np.asarray(params, dtype=np.float64), P


def truth_stats(datas, names=None):
    '`CmllrStats` of speakers [(X, params, P)] from the truth, and the truth\'s own triples.'
    D, P = datas[0][0].shape[1], datas[0][2]
    X = np.concatenate([d[0] for d in datas])
    prm = np.concatenate([d[1] for d in datas])
    lengths = [len(d[0]) for d in datas]
    G, k, beta = ct.statistics(X, prm, lengths, list(range(len(datas))), len(datas), P)
    names = names or [f's{i}' for i in range(len(datas))]
    stats = beer.CmllrStats(np.asarray(ct.pack_lower(G[0]), dtype=np.float64),
                            np.asarray(k[0], dtype=np.float64),
                            np.asarray(beta[0], dtype=np.float64), names)
    return stats, (G[0], k[0], beta[0])


SHAPES = [(1, False), (2, False), (3, False), (3, True), (13, False), (13, True), (40, False),
          (40, True), (1, True)]


@pytest.mark.parametrize('D,iso', SHAPES)
def test_the_truth_agrees_with_itself(D, iso):
    X, prm, P = speaker_data(120 if D < 40 else 200, D, iso, D)
    _, (G, k, beta) = truth_stats([(X, prm, P)])
    rng = np.random.RandomState(1)
    W = np.concatenate([np.eye(D) + .3 * rng.randn(D, D), rng.randn(D, 1)], axis=1)
    a = ct.objective_from_stats(W, G[0], k[0], beta[0])
    b = ct.objective_from_frames(W, X, prm, P)
    assert abs(a - b) <= 1e-12 * abs(b)


def test_objective_equals_the_truth():
    datas = [speaker_data(90, 3, False, 5), speaker_data(70, 3, False, 6)]
    stats, (G, k, beta) = truth_stats(datas)
    rng = np.random.RandomState(2)
    W = np.concatenate([np.eye(3) + .3 * rng.randn(2, 3, 3), rng.randn(2, 3, 1)], axis=2)
    got = stats.objective(W)
    for s in range(2):
        want = float(ct.objective_from_frames(W[s], datas[s][0], datas[s][1], 3))
        assert abs(got[s] - want) <= 1e-12 * abs(want)
    tr = beer.AffineTransforms(stats.names, 3)
    tr.W = W
    assert np.array_equal(stats.objective(tr), got)


@pytest.mark.parametrize('D,iso', SHAPES)
def test_estimate_never_lowers_the_objective(D, iso):
    T = 150 if D < 40 else 260
    datas = [speaker_data(T, D, iso, 10 + D), speaker_data(T + 17, D, iso, 50 + D)]
    stats, (G, k, beta) = truth_stats(datas)
    small = D <= 3
    trace = []

    def on_row(sweep, i, W):
        trace.append([float(ct.objective_from_stats(W[s], G[s], k[s], beta[s])) for s in range(2)])
    Q0 = stats.objective(beer.AffineTransforms(stats.names, D))
    tr, gain = stats.estimate(sweeps=200 if small else 5, min_gain=0. if small else 1e-7,
                              min_count=0., on_row=on_row)
    trace = np.asarray([list(Q0)] + trace)
    drop = trace[:-1] - trace[1:]
    print(f'D={D} iso={iso}: {len(trace) - 1} row steps, largest drop '
          f'{(drop / np.abs(trace[1:])).max():.2e} of |Q|, gains {gain}')
    assert (drop <= 1e-12 * np.abs(trace[1:])).all()
    Q1 = stats.objective(tr)
    assert (Q1 > Q0).all()
    assert np.abs(gain - (Q1 - Q0) / stats.beta).max() <= 1e-12 * np.abs(Q1 / stats.beta).max()
    if small:
        rng = np.random.RandomState(3)
        for _ in range(50):
            Wp = tr.W + 1e-3 * rng.randn(*tr.W.shape)
            assert (stats.objective(Wp) <= Q1).all()


def test_a_sweep_is_the_restated_row_update():
    D = 3
    stats, (G, k, beta) = truth_stats([speaker_data(80, D, False, 4)])
    W = np.eye(D, D + 1)
    for i in range(D):
        W = ct.row_update(W, G[0], k[0], beta[0], i)
    got, _ = stats.estimate(sweeps=1, min_gain=0., min_count=0.)
    assert np.abs(got.W[0] - W).max() <= 1e-9 * np.abs(W).max()


def test_speakers_that_are_not_estimated():
    D = 3
    many, few, lone = speaker_data(200, D, False, 1), speaker_data(30, D, False, 2), \
        speaker_data(2, D, False, 3)
    none = (np.zeros((0, D)), np.zeros((0, 2 * D + 1)), D)
    stats, _ = truth_stats([many, few, none, lone])
    ident = beer.AffineTransforms(stats.names, D).W
    tr, gain = stats.estimate(min_count=100., sweeps=3)
    assert not np.array_equal(tr.W[0], ident[0]) and gain[0] > 0
    assert np.array_equal(tr.W[1:], ident[1:]) and (gain[1:] == 0).all()
    # two frames cannot span the four entries of xi: singular G_i, no error, the identity kept
    tr, gain = stats.estimate(min_count=0., sweeps=3)
    assert np.isfinite(tr.W).all() and np.isfinite(gain).all()
    assert np.array_equal(tr.W[2:], ident[2:]) and (gain[2:] == 0).all()
    assert gain[1] > 0
    # W0's block is what is kept
    W0 = ident.copy()
    W0[3] *= 2.
    tr, _ = stats.estimate(W0=W0, min_count=0., sweeps=1)
    assert np.array_equal(tr.W[3], W0[3])
    assert np.abs(tr.log_abs_det()[2:] - [0., np.log(8.)]).max() <= 1e-15


def test_statistics_add_and_files_round_trip(tmp_path):
    D = 3
    a, b = speaker_data(60, D, True, 7), speaker_data(45, D, True, 8)
    c, d = speaker_data(33, D, True, 9), speaker_data(21, D, True, 10)
    first, _ = truth_stats([a, b])
    second, _ = truth_stats([c, d])
    union, _ = truth_stats([tuple(np.concatenate([x, y]) for x, y in zip(a[:2], c[:2])) + (1,),
                            tuple(np.concatenate([x, y]) for x, y in zip(b[:2], d[:2])) + (1,)])
    both = first + second
    for name in ('G', 'k', 'beta'):
        got, want = getattr(both, name), getattr(union, name)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    with pytest.raises(ValueError):
        first + truth_stats([a, b], names=['x', 'y'])[0]
    tr, _ = both.estimate(min_count=0., sweeps=2)
    path = str(tmp_path / 'transforms.npz')
    tr.save(path)
    assert os.path.exists(path)                                   # (no ".npz" appended)
    back = beer.AffineTransforms.load(path)
    assert back.names == tr.names == ['s0', 's1'] and back.dim == D
    assert back.W.dtype == np.float64 and np.array_equal(back.W, tr.W)
    with np.load(path) as z:
        assert sorted(z.files) == ['W', 'speakers'] and z['speakers'].dtype.kind == 'U'
    terms = tr.log_det_terms([10, 0, 7], ['s1', 's0', 'nobody'])
    ld = tr.log_abs_det()
    assert np.array_equal(terms, [10 * ld[1], 0., 0.])
    assert np.array_equal(tr.indices(['s1', 'zz', 0, -1]), [1, -1, 0, -1])
    with pytest.raises(ValueError):
        tr.indices([2])


def test_utt2spk_and_the_argument_tables(tmp_path):
    path = tmp_path / 'utt2spk'
    path.write_text('u1 alice\n\nu2 bob\nu3 alice\n')
    table = hmm_cmds.read_utt2spk(str(path))
    assert table == {'u1': 'alice', 'u2': 'bob', 'u3': 'alice'}
    assert hmm_cmds.speakers_of(['u2', 'u1', 'u3'], table) == (['bob', 'alice'], [0, 1, 1])
    with pytest.raises(SystemExit, match='u9'):
        hmm_cmds.speakers_of(['u1', 'u9'], table)
    (tmp_path / 'bad').write_text('u1 alice extra\n')
    with pytest.raises(SystemExit, match='bad:1'):
        hmm_cmds.read_utt2spk(str(tmp_path / 'bad'))
    assert hmm_cmds.adapt in hmm_cmds.COMMANDS and fea_cmds.transform in fea_cmds.COMMANDS
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'adapt', 'mdl', 'ds', 'u2s', 'out'])
    assert (args.model, args.dataset, args.utt2spk, args.out) == ('mdl', 'ds', 'u2s', 'out')
    assert (args.alis, args.acoustic_scale, args.iters, args.sweeps, args.min_count, args.init,
            args.utts) == (None, 1., 3, 20, 500., None, None)
    assert args.func is hmm_cmds.adapt.main
    args = parser.parse_args(['hmm', 'adapt', '-a', 'alis', '-s', '.5', '--iters', '2', '--sweeps',
                              '7', '--min-count', '10', '--init', 'old', '-u', '-', 'm', 'd', 'u', 'o'])
    assert (args.alis, args.acoustic_scale, args.iters, args.sweeps, args.min_count, args.init,
            args.utts) == ('alis', .5, 2, 7, 10., 'old', '-')
    args = parser.parse_args(['features', 'transform', 'arch', 'u2s', 'tr', 'out'])
    assert (args.archive, args.utt2spk, args.transforms, args.out_archive) == \
        ('arch', 'u2s', 'tr', 'out')
    assert args.func is fea_cmds.transform.main


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, 'include', 'beer_hip.h')) as f:
        text = f.read()
    for name in ('int beer_cmllr_frame_params(', 'int beer_cmllr_accumulate(',
                 'int beer_cmllr_apply(', 'int beer_cmllr_table(',
                 'size_t beer_cmllr_workspace_bytes(', '#define BEER_CMLLR_MAX_DIM 63'):
        assert text.count(name) == 1, name
    assert _hip.CMLLR_MAX_DIM == 63
    for name in ('beer_cmllr_frame_params', 'beer_cmllr_accumulate', 'beer_cmllr_apply'):
        assert name in _hip.SIGNATURES
    assert 'beer_cmllr_table' in _hip.HOST_SIGNATURES
    assert 'beer_cmllr_workspace_bytes' in _hip.SIZE_QUERIES


def test_the_table_and_the_refusals_need_no_device():
    lib = _hip.lib()
    table = kernels.cmllr_table([5, 0, 3, 4, 2], [1, 1, 0, -1, 1], 3, chunk_frames=4)
    n_items, n_segs, n_spk, nutt = table.host[:4].tolist()
    assert (n_items, n_spk, nutt, table.n_items) == (3, 3, 5, 3)
    rest = table.host[4:]
    spk_ptr, item_spk = rest[:4].tolist(), rest[4:4 + n_items].tolist()
    item_ptr = rest[4 + n_items:5 + 2 * n_items].tolist()
    segs = rest[5 + 2 * n_items:].reshape(-1, 3).tolist()
    assert spk_ptr == [0, 1, 3, 3] and item_spk == [0, 1, 1] and item_ptr == [0, 1, 2, 4]
    # speaker 0: utterance 2; speaker 1: utterance 0 cut after 4 frames, its last with utterance 4
    assert segs == [[2, 0, 3], [0, 0, 4], [0, 4, 1], [4, 0, 2]] and n_segs == 4
    assert lib.beer_cmllr_workspace_bytes(3, 3, 3) == 3 * (3 * 10 + 12 + 1) * 8
    assert lib.beer_cmllr_workspace_bytes(3, 1, 2) == 2 * (10 + 12 + 1) * 8
    # a speaker out of range, before anything else is looked at
    for bad in ([0, 3], [0, -2]):
        with pytest.raises(_hip.HipInvalid):
            kernels.cmllr_table([4, 4], bad, 3)
    # D = 64 and a P that is neither 1 nor D: refused with every pointer NULL
    host = ctypes.c_void_p(table.host.ctypes.data)
    for D, P in ((64, 64), (64, 1), (5, 2), (5, 0)):
        assert lib.beer_cmllr_workspace_bytes(D, P, 1) == 0
        for dtype in (_hip.F32, _hip.F64):
            rc = lib.beer_cmllr_accumulate(dtype, 14, D, P, 5, 3, None, None, None, host, None,
                                           len(table.host), 4, None, None, None, None, 0, None)
            assert rc == _hip.EINVAL, (D, P)
    # a table for other speakers, another chunk or with a speaker out of range
    good = (_hip.F64, 14, 3, 3, 5, 3, None, None, None)
    tail = (None, None, None, None, 0, None)
    assert lib.beer_cmllr_accumulate(*good[:5], 2, *good[6:], host, None, len(table.host), 4,
                                     *tail) == _hip.EINVAL            # n_spk of the call
    assert lib.beer_cmllr_accumulate(*good, host, None, len(table.host), 3, *tail) == \
        _hip.EINVAL                                                    # items of 4 frames, chunk 3
    broken = table.host.copy()
    broken[4 + 4] = 3                                                  # item_spk[0] = n_spk
    assert lib.beer_cmllr_accumulate(*good, ctypes.c_void_p(broken.ctypes.data), None,
                                     len(broken), 4, *tail) == _hip.EINVAL
    broken = table.host.copy()
    broken[5 + 2 * n_items + 4] = 5                                    # seg[0].utterance = nutt
    assert lib.beer_cmllr_accumulate(*good, ctypes.c_void_p(broken.ctypes.data), None,
                                     len(broken), 4, *tail) == _hip.EINVAL
    # the sound table gets past the host checks: refused only for its missing device pointers
    assert lib.beer_cmllr_accumulate(*good, host, None, len(table.host), 4, *tail) == _hip.EINVAL
    empty = kernels.cmllr_table([], [], 2)
    assert lib.beer_cmllr_accumulate(_hip.F64, 0, 3, 3, 0, 2, None, None, None,
                                     ctypes.c_void_p(empty.host.ctypes.data), None,
                                     len(empty.host), 0, *tail) == 0
    # frame_params and apply
    assert lib.beer_cmllr_frame_params(_hip.F64, _hip.FULL, 4, 3, 1, 2, None, None, None, None,
                                       None) == _hip.EINVAL
    assert lib.beer_cmllr_frame_params(_hip.F32, _hip.DIAG, 4, 64, 1, 2, None, None, None, None,
                                       None) == _hip.EINVAL
    assert lib.beer_cmllr_frame_params(_hip.F32, _hip.DIAG, 0, 63, 1, 2, None, None, None, None,
                                       None) == 0
    spk = np.asarray([0, 2], dtype=np.int32)
    assert lib.beer_cmllr_apply(_hip.F64, 8, 3, 2, 2, None, None, None, None,
                                ctypes.c_void_p(spk.ctypes.data), None, None) == _hip.EINVAL
    assert lib.beer_cmllr_apply(_hip.F64, 8, 64, 2, 3, None, None, None, None,
                                ctypes.c_void_p(spk.ctypes.data), None, None) == _hip.EINVAL
    assert lib.beer_cmllr_apply(_hip.F64, 0, 3, 2, 3, None, None, None, None,
                                ctypes.c_void_p(spk.ctypes.data), None, None) == 0
