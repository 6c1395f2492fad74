"""tests/plumbing_truth.py against naive Python loops on tiny inputs, and the table of batches
against the launch constants of the kernels: every stride the GPU tests claim to reach (CPU)."""

import numpy as np
import pytest

import plumbing_truth as pt


def test_gather_is_one_rounded_product():
    rng = np.random.RandomState(0)
    pc = rng.randn(4, 6)
    pc[1, 2], pc[3, 0] = -np.inf, np.nan
    ids = [5, 0, 0, 2]
    for dtype in (np.float32, np.float64):
        got = pt.gather(pc.astype(dtype), ids, .7, dtype)
        assert got.dtype == dtype and got.shape == (4, 4)
        for t in range(4):
            for s in range(4):
                want = dtype(dtype(.7) * dtype(pc[t, ids[s]]))
                assert np.array_equal(got[t, s], want, equal_nan=True)
    assert pt.gather(pc, ids, 1., np.float64)[1, 3] == -np.inf
    assert np.isnan(pt.gather(pc, ids, 1., np.float64)[3, 1:3]).all()
    # float32: the product of the ROUNDED scale, not the rounded float64 product
    x = np.array([[3.]], dtype=np.float32)
    assert pt.gather(x, [0], .7, np.float32)[0, 0] == np.float32(.7) * np.float32(3.)


def test_scatter_against_loops():
    rng = np.random.RandomState(1)
    T, S, S_total, scale = 5, 4, 6, .5
    llh, gamma = rng.randn(T, S), rng.rand(T, S)
    ids = [4, 1, 4, 0]
    sr, exp_llh, utt_llh = pt.scatter(llh, gamma, ids, S_total, scale)
    want_sr, want_e = np.zeros((T, S_total)), np.zeros(T)
    for t in range(T):
        for s in range(S):
            want_sr[t, ids[s]] += scale * gamma[t, s]
            want_e[t] += llh[t, s] * gamma[t, s]
    assert np.allclose(sr, want_sr, rtol=1e-15, atol=0) and (sr[:, [2, 3, 5]] == 0).all()
    assert np.allclose(exp_llh, want_e, rtol=1e-14, atol=1e-15)
    assert abs(utt_llh - want_e.sum()) < 1e-14
    a_sr, a_e, a_u = pt.scatter_abs(llh, gamma, ids, S_total, -scale)
    assert (a_sr >= np.abs(sr)).all() and (a_e >= np.abs(exp_llh)).all() and a_u >= abs(utt_llh)
    # distinct ids: one product in the kernel's type
    for dtype in (np.float32, np.float64):
        once = pt.scatter_once(gamma.astype(dtype), [4, 1, 5, 0], S_total, .7, dtype)
        assert once.dtype == dtype and (once[:, [2, 3]] == 0).all()
        for t in range(T):
            for s, i in enumerate([4, 1, 5, 0]):
                assert once[t, i] == dtype(dtype(.7) * dtype(gamma[t, s]))
    # no frames
    sr, exp_llh, utt_llh = pt.scatter(np.zeros((0, S)), np.zeros((0, S)), ids, S_total, 1.)
    assert sr.shape == (0, S_total) and exp_llh.shape == (0,) and utt_llh == 0.
    # -inf where the posterior is 0: NaN in that frame and in the utterance, nowhere else
    llh[2, 1], gamma[2, 1] = -np.inf, 0.
    sr, exp_llh, utt_llh = pt.scatter(llh, gamma, ids, S_total, 1.)
    assert np.isnan(exp_llh).tolist() == [False, False, True, False, False]
    assert np.isnan(utt_llh) and np.isfinite(sr).all()


def test_path_posteriors_against_loops():
    S = 4
    paths = [[], [1, 1, 3, 0], [2], [], [0, 3]]
    onehot, xi, g0, last = pt.path_posteriors(paths, S)
    want_xi, want_g0, want_last = np.zeros((S, S)), np.zeros(S), np.zeros(S)
    for p, g in zip(paths, onehot):
        assert g.shape == (len(p), S)
        for t, st in enumerate(p):
            assert g[t].tolist() == [1. if s == st else 0. for s in range(S)]
            if t + 1 < len(p):
                want_xi[st, p[t + 1]] += 1
        if p:
            want_g0[p[0]] += 1
            want_last[p[-1]] += 1
    assert np.array_equal(xi, want_xi) and np.array_equal(g0, want_g0)
    assert np.array_equal(last, want_last)
    # nothing crosses an utterance boundary: 3 -> 2 and 2 -> 0 are not transitions
    assert xi.sum() == 4 and xi[3, 2] == 0 and xi[2, 0] == 0 and xi[0, 2] == 0
    assert g0.sum() == last.sum() == 3


def test_the_sums_against_loops():
    rng = np.random.RandomState(2)
    gammas = [rng.rand(T, 3) for T in (2, 0, 1, 0)]
    want = np.zeros(3)
    for g in gammas:
        for s in range(3):
            if len(g):
                want[s] += g[len(g) - 1, s]
    assert np.allclose(pt.last_frame_sum(gammas, 3), want, rtol=1e-15)
    assert np.array_equal(pt.last_frame_sum([], 3), np.zeros(3))
    v = rng.randn(9).astype(np.float32)
    off = [0, 0, 4, 4, 9]
    got = pt.segment_sum(v, off)
    assert got.dtype == pt.HP and got[0] == 0. and got[2] == 0.
    for u in range(4):
        s = 0.
        for t in range(off[u], off[u + 1]):
            s += float(v[t])
        assert abs(got[u] - s) < 1e-14
    assert pt.segment_sum(v, [0]).shape == (0,)


@pytest.mark.parametrize('S,G,Q', [(1, 1, 2), (3, 1, 6), (1, 2, 6), (3, 5, 2), (2, 3, 4)])
def test_weights_from_acc_against_loops(S, G, Q):
    acc = np.random.RandomState(3).randint(-8, 9, size=(S * G, Q)) / 4.
    got = pt.weights_from_acc(acc, S, G)
    for s in range(S):
        tot = 0.
        for g in range(G):
            n = -2. * acc[s * G + g, Q - 2]
            tot += n
            if g < G - 1:
                assert got[s, g] == n
        assert got[s, G - 1] == tot


def test_pdf_id_flavours():
    for S in pt.SIZES:
        for fl in pt.FLAVOURS:
            if fl == 'repeat' and S < 2:
                continue
            ids, S_total, r = pt.pdf_ids(S, fl, S)
            assert len(ids) == S and ids.min() >= 0 and ids.max() < S_total
            counts = np.bincount(ids, minlength=S_total)
            if fl == 'repeat':
                assert set(counts[counts > 0]) <= {2, 3} and r == counts.max()
                assert (counts == 0).sum() == 5
                assert r == 3 or S in (2, 4)
            else:
                assert counts.max() == 1 and r == 1
            if fl == 'perm':
                assert S_total == S and sorted(ids) == list(range(S))
                assert S < 3 or list(ids) != list(range(S))
            if fl == 'subset':
                assert S_total > S and (counts == 0).sum() == 7
            if fl == 'identity':
                assert S_total == S and list(ids) == list(range(S))


def test_the_table_reaches_every_stride_it_claims():
    'Arithmetic on the launch constants of csrc/hmm.hip: which loop runs how many passes.'
    single = [c for c in pt.CASES if len(c.sizes) == 1 and c.lens]
    assert {c.sizes[0] for c in single} == set(pt.SIZES) == {1, 3, 64, 65, 256, 257, 300}
    for S in pt.SIZES:
        assert {c.flavours[0] for c in single if c.sizes[0] == S} == \
            set(pt.FLAVOURS) - ({'repeat'} if S == 1 else set())
    mixed = [c for c in pt.CASES if len(c.sizes) > 1]
    assert len(mixed) == 1 and mixed[0].sizes == (3, 65, 300)
    assert set(mixed[0].gids) == {0, 1, 2} and 'repeat' in mixed[0].flavours
    assert any(len(c.lens) == 0 for c in pt.CASES)
    for c in pt.CASES:
        if not c.lens:
            continue
        assert set(c.lens) == {0, 1, 2, 33, 65, 258}
        assert c.lens[0] == 0 and c.lens[-1] == 0 and 0 in c.lens[1:-1]
        assert len(c.gids) == len(c.lens)
    elems = {c.name: [T * c.sizes[g] for T, g in zip(c.lens, c.gids)] for c in pt.CASES}
    every = [e for c in pt.CASES for e in elems[c.name]]
    # the element loops: a first pass only, and a third pass that ends inside the pass
    assert pt.GATHER_PASS == 1024 and pt.FLAT_PASS == 2048 and pt.PATH_PASS == 512
    for per_pass in (pt.GATHER_PASS, pt.FLAT_PASS, pt.PATH_PASS):
        assert any(0 < e < per_pass for e in every)
        assert any(e > 2 * per_pass and e % per_pass for e in every)
    assert max(every) > 2 * 2048                              # T * S > 2 * 2048
    # and not only with a power of two as the row length (idx / S, idx % S)
    assert any(T * S > 2 * pt.FLAT_PASS for c in single for T in c.lens for S in c.sizes if S % 2)
    # the per-frame scatter: 8 workgroups of 4 waves, a frame per wave
    assert pt.FRAME_PASS == 32
    lens = set(pt.LENGTHS)
    assert any(0 < T < pt.FRAME_PASS for T in lens) and any(pt.FRAME_PASS < T <= 64 for T in lens)
    assert any(T >= 65 for T in lens) and max(lens) > 2 * pt.FRAME_PASS
    # the transition counts of a path: 256 per pass, T - 1 of them
    assert any(0 < T - 1 <= pt.PATH_XI_PASS for T in lens) and max(lens) - 1 > pt.PATH_XI_PASS
    # lanes over the states: one pass, exactly a wave, one more state, 2, 4 full passes, 5
    sizes = set(pt.SIZES)
    assert any(S < pt.WAVE for S in sizes) and pt.WAVE in sizes and pt.WAVE + 1 in sizes
    assert 4 * pt.WAVE in sizes and 4 * pt.WAVE + 1 in sizes
    # threads over the states (last_frame_kernel): a workgroup, one more state
    assert pt.BLOCK in sizes and pt.BLOCK + 1 in sizes and max(sizes) > pt.BLOCK
    # the mixed batch has its largest graph neither first nor last in the launch
    m = mixed[0]
    assert m.sizes[m.gids[1]] == 3 and max(elems['mixed']) > 2 * pt.FLAT_PASS


def test_grid_values_are_exact_in_float32():
    rng = np.random.RandomState(4)
    g = pt.grid(rng, (300,), 0, 1, np.float32).astype(np.float64)
    p = pt.grid(rng, (300,), -4, 0, np.float32).astype(np.float64)
    assert ((g * 64) % 1 == 0).all() and ((p * 64) % 1 == 0).all()
    # 300 products of magnitude < 4 on a grid of 2^-12: below 2^24 units
    assert 300 * 4 * 4096 < 2 ** 24
    acc = np.float32(0)
    for a, b in zip(g, p):
        acc = np.float32(acc + np.float32(np.float32(a) * np.float32(b)))
    assert float(acc) == float((g * p).sum())
