"""Unit sequences and edit distances on the device (csrc/editdist.hip) against the plain-Python
truth of tests/editdist_truth.py: every comparison of kernel output is integer equality.

 * `edit_distance`, both cell types: one static table, each case naming the route
   `beer_edit_distance_route` must report for it with and without `ops`; the table reaches every
   value the route takes.  Lengths 0, 1, 2, both sides of every team size, 63 / 64 / 65,
   128 / 129, 700 x 1500 beside short pairs, the first length whose boundary row leaves LDS for
   either cell; alphabets of 1, 2 and 50 symbols; identical pairs, disjoint alphabets, a sequence
   paired with itself, one pair listed three times, no pair at all.  Guards around `dist`, `ops`
   and the workspace; the inputs unchanged bit for bit.  The truth of every case is computed once.
 * `unit_sequences` against `phones_of_path`, lengths 0 .. 4096, rows of -1 and bad pdfs.
 * The model level: `mbr_decode_batch`, `beer hmm decode --mbr`, `beer hmm evaluate`."""

import io
import os
import sys

import numpy as np
import pytest
import torch

import editdist_truth as et
import scoring_truth as st
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, kernels                                  # noqa: E402
from beer_amd.cli import hmm as hmm_cmds, main as cli_main          # noqa: E402

O, L, W = et.OPS, et.ROW_LDS, et.ROW_WS
GUARD = 0x5A5A5A5A

# (name, route without ops, route with ops, pairs (len_a, len_b, kind))
#   kind: r random, s the same sequence twice, d disjoint alphabets, i the sequence with ITSELF
#   (one index twice), n the second a few edits from the first
CASES = (
    ('team8', 8, 8 | O,
     ((0, 0, 'r'), (0, 1, 'r'), (1, 0, 'r'), (1, 1, 'r'), (1, 1, 's'), (2, 2, 'r'), (1, 2, 'r'),
      (2, 1, 'd'), (7, 8, 'r'), (8, 7, 'r'), (8, 8, 'r'), (8, 8, 's'), (8, 8, 'd'), (8, 3, 'r'),
      (0, 8, 'r'), (8, 100, 'r'), (100, 8, 'r'), (5, 5, 'i'), (6, 9, 'n'), (3, 70, 'd'),
      (8, 64, 'r'), (4, 65, 'n'))),
    ('team16', 16, 16 | O,
     ((9, 9, 'r'), (9, 16, 'r'), (16, 9, 'n'), (16, 16, 'r'), (16, 16, 's'), (16, 40, 'r'),
      (12, 12, 'd'), (3, 5, 'r'), (0, 9, 'r'), (130, 15, 'r'), (10, 10, 'i'), (9, 17, 'n'))),
    ('team32', 32, 32 | O,
     ((17, 17, 'r'), (32, 32, 'r'), (32, 32, 'd'), (17, 60, 'r'), (32, 5, 'r'), (31, 33, 'n'),
      (33, 31, 'r'), (20, 20, 'i'), (0, 0, 'r'), (32, 129, 'r'))),
    ('team64', 64, 64 | O,
     ((33, 33, 'r'), (63, 63, 'r'), (64, 64, 'r'), (64, 64, 's'), (63, 64, 'n'), (64, 65, 'r'),
      (65, 64, 'd'), (64, 200, 'r'), (129, 40, 'r'), (2, 2, 'r'), (50, 50, 'i'), (0, 64, 'r'))),
    ('strips', 64 | L, 64 | O | L,
     ((65, 65, 'r'), (65, 65, 's'), (65, 66, 'n'), (128, 128, 'r'), (129, 129, 'r'),
      (128, 129, 'd'), (129, 128, 'n'), (700, 1500, 'r'), (3, 4, 'r'), (65, 300, 'r'),
      (300, 66, 'r'), (0, 70, 'r'), (130, 130, 'i'), (64, 64, 'r'), (193, 192, 'n'))),
    ('row_leaves_lds_with_ops', 64 | L, 64 | O | W, ((65, 2048, 'r'), (2047, 66, 'n'), (5, 9, 'r'))),
    ('row_leaves_lds', 64 | W, 64 | O | W,
     ((65, 4096, 'n'), (70, 100, 'r'), (4096, 65, 'r'), (1, 1, 'r'), (66, 66, 'i'))),
)
ALPHABETS = (2, 50, 1)


def build(case_no):
    '''(sequences, pair_a, pair_b) of a case: every pair has its own two sequences, but for
    kind i; the first pair is listed three times.'''
    pairs = CASES[case_no][3]
    rng = np.random.RandomState(100 + case_no)
    seqs, pa, pb = [], [], []
    for n, (la, lb, kind) in enumerate(pairs):
        K = ALPHABETS[n % 3]
        a = rng.randint(0, K, la)
        if kind == 's':
            assert la == lb
            b = a.copy()
        elif kind == 'd':
            b = rng.randint(K, 2 * K, lb)
        elif kind == 'n':
            b = np.resize(a, lb) if la else rng.randint(0, K, lb)
            if lb:
                b[rng.randint(0, lb, 3)] = rng.randint(0, K + 1, 3)
        else:
            b = rng.randint(0, K, lb)
        pa.append(len(seqs))
        seqs.append(a)
        if kind == 'i':
            assert la == lb
            pb.append(pa[-1])
        else:
            pb.append(len(seqs))
            seqs.append(b)
    return seqs, pa + [pa[0], pa[0]], pb + [pb[0], pb[0]]


_TRUTH = {}


def truth(case_no):
    'The (cost, sub, del, ins) of the pairs of a case, computed once for all the tests.'
    if case_no not in _TRUTH:
        seqs, pa, pb = build(case_no)
        got = {}
        for a, b in zip(pa, pb):
            if (a, b) not in got:
                got[a, b] = et.edit_ops(seqs[a].tolist(), seqs[b].tolist())
        want = np.asarray([got[a, b] for a, b in zip(pa, pb)], dtype=np.int64)
        want.setflags(write=False)
        _TRUTH[case_no] = want
    return _TRUTH[case_no]


def packed(seqs):
    lens = np.asarray([len(s) for s in seqs], dtype=np.int64)
    sym = np.concatenate(seqs).astype(np.int32) if lens.sum() else np.zeros(0, dtype=np.int32)
    return (torch.from_numpy(sym).cuda(), torch.from_numpy(np.cumsum(lens) - lens).cuda(),
            torch.from_numpy(lens.astype(np.int32)).cuda(), lens)


def guarded(n, dtype=torch.int32, pad=64):
    'A buffer of n elements between two guards: (whole, the view).'
    whole = torch.full((n + 2 * pad,), GUARD if dtype == torch.int32 else 0x5A, dtype=dtype,
                       device='cuda')
    return whole, whole[pad:pad + n]


def guards_hold(whole, n, pad=64):
    fill = GUARD if whole.dtype == torch.int32 else 0x5A
    return bool((whole[:pad] == fill).all()) and bool((whole[pad + n:] == fill).all())


@pytest.mark.parametrize('ops', [False, True], ids=['cost', 'ops'])
@pytest.mark.parametrize('case_no', range(len(CASES)), ids=[c[0] for c in CASES])
def test_edit_distance_is_the_truth_on_every_route(case_no, ops):
    name, route_plain, route_ops, pairs = CASES[case_no]
    seqs, pa, pb = build(case_no)
    want = truth(case_no)
    sym, start, lens, lens_h = packed(seqs)
    short = max(min(lens_h[a], lens_h[b]) for a, b in zip(pa, pb))
    long_ = max(max(lens_h[a], lens_h[b]) for a, b in zip(pa, pb))
    route = kernels.edit_distance_route(short, long_, ops)
    assert route == (route_ops if ops else route_plain), hex(route)
    a_t = torch.tensor(pa, dtype=torch.int32, device='cuda')
    b_t = torch.tensor(pb, dtype=torch.int32, device='cuda')
    inputs = [t.clone() for t in (sym, start, lens, a_t, b_t)]
    n = len(pa)
    dist_all, dist = guarded(n)
    ops_all, ops_v = guarded(3 * n)
    need = _hip.lib().beer_edit_distance_scratch_bytes(n, int(short), int(long_), int(ops))
    assert (need > 0) == bool(route & W)
    ws_all, ws = guarded(need, torch.uint8, 256)
    kernels.edit_distance_launch(sym, start, lens, a_t, b_t, short, long_, dist,
                                 ops_v.view(n, 3) if ops else None, ws if need else None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dist.cpu().numpy(), want[:, 0], err_msg=name)
    if ops:
        np.testing.assert_array_equal(ops_v.view(n, 3).cpu().numpy(), want[:, 1:], err_msg=name)
    else:
        assert bool((ops_v == GUARD).all())
    assert guards_hold(dist_all, n) and guards_hold(ops_all, 3 * n) and guards_hold(ws_all, need, 256)
    for before, after in zip(inputs, (sym, start, lens, a_t, b_t)):
        assert torch.equal(before, after)
    # what the definitions promise, on the kernel's own output
    got = dist.cpu().numpy()
    for p, (la, lb, kind) in enumerate(pairs):
        if kind in 'si':
            assert got[p] == 0
        if kind == 'd':
            assert got[p] == max(la, lb)
    assert got[-1] == got[-2] == got[0]


def test_edit_distance_orders_the_pairs_and_answers_in_the_callers_order():
    'Every case in one call: the 700 x 1500 pair beside the short ones, five launches, one answer.'
    seqs, pa, pb, want = [], [], [], []
    for case_no in range(len(CASES)):
        s, a, b = build(case_no)
        pa += [len(seqs) + i for i in a]
        pb += [len(seqs) + i for i in b]
        seqs += s
        want.append(truth(case_no))
    want = np.concatenate(want)
    perm = np.random.RandomState(7).permutation(len(pa))
    pa, pb, want = np.asarray(pa)[perm], np.asarray(pb)[perm], want[perm]
    sym, start, lens, _ = packed(seqs)
    dist, moves = kernels.edit_distance(sym, start, lens, pa, pb, ops=True)
    assert dist.dtype == moves.dtype == torch.int32 and moves.shape == (len(pa), 3)
    np.testing.assert_array_equal(dist.cpu().numpy(), want[:, 0])
    np.testing.assert_array_equal(moves.cpu().numpy(), want[:, 1:])
    plain = kernels.edit_distance(sym, start, lens, torch.from_numpy(pa), torch.from_numpy(pb))
    assert torch.equal(plain, dist)
    # the arguments swapped: deletions and insertions swap
    back = kernels.edit_distance(sym, start, lens, pb, pa, ops=True)[1]
    assert torch.equal(back[:, [0, 2, 1]], moves)
    # no pair at all; indices outside the sequences are refused on the host
    none = kernels.edit_distance(sym, start, lens, [], [], ops=True)
    assert none[0].shape == (0,) and none[1].shape == (0, 3)
    for bad in ([len(seqs)], [-1]):
        with pytest.raises(ValueError):
            kernels.edit_distance(sym, start, lens, bad, [0])
        with pytest.raises(ValueError):
            kernels.edit_distance(sym, start, lens, [0], bad)


def test_public_error_rates():
    refs = [[1, 2, 3, 4], [5, 5], [], [7, 8, 9]]
    hyps = [[1, 3, 4, 4], np.array([5, 5]), torch.tensor([6]), [8, 9]]
    dist, moves = beer.edit_distances(refs, hyps, ops=True)
    want = [et.edit_ops(list(r), np.asarray(h).tolist()) for r, h in zip(refs, hyps)]
    assert dist.tolist() == [w[0] for w in want] and moves.tolist() == [list(w[1:]) for w in want]
    assert torch.equal(beer.edit_distances(refs, hyps), dist)
    got = beer.token_error_rate(refs, hyps)
    assert tuple(got) == st.token_errors(refs, [np.asarray(h).tolist() for h in hyps])
    assert got.rate == pytest.approx(100. * got.errors / 9)
    lists = [[[1, 2], [1, 2, 3, 5], [1, 2, 3, 4, 4]], [[5], [5, 5]], [[], [1]], [[1], [2]]]
    got = beer.closest_error_rate(refs, lists)
    assert tuple(got) == st.oracle_errors(refs, lists) and got.errors == 1 + 0 + 0 + 3
    assert tuple(beer.token_error_rate([], [])) == (0, 0, 0, 0, 0, 0)


# --- unit sequences ----------------------------------------------------------------------------

START = {'u0': 0, 'u1': 3, 'u2': 6}
TABLE = np.full(9, -1, dtype=np.int32)
TABLE[[0, 3, 6]] = [0, 1, 2]


def unit_paths():
    rng = np.random.RandomState(5)
    paths = []
    for T in (0, 1, 63, 64, 65, 129, 4096):
        paths.append(np.zeros(T, dtype=np.int64) + 3)                       # constant
        paths.append(np.arange(T, dtype=np.int64) % 9)                      # a new pdf every frame
        paths.append(np.resize(np.array([0, 1, 2, 0, 0, 1, 2, 2, 6, 6, 0]), T).astype(np.int64))
        walk = rng.randint(0, 9, T).astype(np.int64)                        # (re-entry above)
        if T:
            walk[0] = rng.choice([0, 3, 6])
        paths.append(walk)
    paths.append(np.full(70, -1, dtype=np.int64))                           # a rank without a path
    bad_first = rng.randint(0, 9, 66).astype(np.int64)
    bad_first[0] = 4
    paths.append(bad_first)
    for at, value in ((100, 9), (64, -1), (1, 1 << 40)):                    # outside the table
        off = np.resize(np.array([0, 1, 3]), 129).astype(np.int64)
        off[at] = value
        paths.append(off)
    paths.append(np.array([6, 7, 8, 3], dtype=np.int64))
    return paths


@pytest.mark.parametrize('per_frame', [False, True], ids=['units', 'per_frame'])
def test_unit_sequences_are_phones_of_path(per_frame):
    paths = unit_paths()
    lens = np.asarray([len(p) for p in paths], dtype=np.int64)
    start = np.cumsum(lens) - lens
    total = int(lens.sum())
    sym = torch.from_numpy(np.concatenate(paths)).cuda()
    before = sym.clone()
    table = torch.from_numpy(TABLE).cuda()
    start_t = torch.from_numpy(start).cuda()
    lens_t = torch.from_numpy(lens.astype(np.int32)).cuda()
    units_all, units = guarded(total)
    count_all, count = guarded(len(paths))
    frame_all, frame = guarded(total)
    _hip.call('beer_unit_sequences', _hip.ptr(sym), _hip.ptr(start_t), _hip.ptr(lens_t), len(paths),
              _hip.ptr(table), len(TABLE), _hip.ptr(units), _hip.ptr(count),
              _hip.ptr(frame) if per_frame else None)
    torch.cuda.synchronize()
    assert guards_hold(units_all, total) and guards_hold(count_all, len(paths))
    assert guards_hold(frame_all, total) and torch.equal(sym, before)
    units, count, frame = units.cpu().numpy(), count.cpu().numpy(), frame.cpu().numpy()
    names = list(START)
    seen = set()
    for q, path in enumerate(paths):
        want_units, want_frames = et.unit_sequence(path, TABLE)
        mine = slice(start[q], start[q] + lens[q])
        if isinstance(want_units, int):
            assert count[q] == want_units, q
            seen.add(want_units)
            if want_units == -1:                                    # nothing is written
                assert (units[mine] == GUARD).all() and (frame[mine] == GUARD).all()
            continue
        assert count[q] == len(want_units), q
        got = units[mine]
        assert [names[u] for u in got[:count[q]]] == hmm_cmds.phones_of_path(path, START) \
            if len(path) else count[q] == 0
        np.testing.assert_array_equal(got[:count[q]], want_units)
        assert (got[count[q]:] == GUARD).all()                      # compact: nothing behind
        if per_frame:
            np.testing.assert_array_equal(frame[mine], want_frames)
            if len(path):
                assert [names[u] for u in frame[mine]] == \
                    hmm_cmds.phones_of_path(path, START, per_frame=True)
    assert seen == {-1, -2}
    if not per_frame:
        assert (frame == GUARD).all()
    # the Python face: the same numbers
    u2, n2, f2 = kernels.unit_sequences(sym, start, lens, TABLE, per_frame=per_frame)
    np.testing.assert_array_equal(n2.cpu().numpy(), count)
    assert (f2 is not None) == per_frame
    ok = np.repeat(count >= 0, lens)
    if per_frame:
        np.testing.assert_array_equal(f2.cpu().numpy()[ok], frame[ok])


# --- model level -----------------------------------------------------------------------------------

_TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
         {'start_id': 1, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 2, 'trans_prob': .5},
         {'start_id': 2, 'end_id': 3, 'trans_prob': .5}, {'start_id': 3, 'end_id': 3, 'trans_prob': .5},
         {'start_id': 3, 'end_id': 4, 'trans_prob': .5}]
D = 4
LENS = (7, 40, 23, 12, 31)


@pytest.fixture(scope='module')
def loop():
    'A three-unit, three-states-per-unit phone loop and 5 utterances of 7 to 40 frames.'
    torch.manual_seed(3)
    conf = {'g': {'topology': _TOPO, 'n_normal_per_state': 2, 'prior_strength': 1.,
                  'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(3)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(D), torch.ones(D))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet').double().to('cuda')
    rng = np.random.RandomState(11)
    utts = [torch.from_numpy(rng.randn(T, D) * 1.5).to('cuda') for T in LENS]
    table = np.full(max(list(start.values()) + list(end.values())) + 1, -1)
    for u, pdf in enumerate(start.values()):
        table[pdf] = u
    return model, utts, table


def hypotheses(stack, table):
    out = []
    for path in stack.cpu().numpy():
        units = et.unit_sequence(path, table)[0]
        assert units != -2
        out.append(None if units == -1 else units)
    return out


def test_unit_sequences_batch(loop):
    model, utts, table = loop
    best = beer.decode_batch(model, utts)
    stacks, _ = beer.decode_nbest_batch(model, utts, 3)
    got = beer.unit_sequences_batch(model, best + stacks)
    names = list(model.start_pdf)
    for path, units in zip(best, got[:len(best)]):
        assert units.dtype == torch.int32 and units.is_cuda
        assert [names[u] for u in units.tolist()] == \
            hmm_cmds.phones_of_path(path.cpu().numpy(), model.start_pdf)
    for stack, rows in zip(stacks, got[len(best):]):
        want = hypotheses(stack, table)
        assert [None if r is None else r.tolist() for r in rows] == want
    frames = beer.unit_sequences_batch(model, best, per_frame=True)
    for path, f in zip(best, frames):
        assert [names[u] for u in f.tolist()] == \
            hmm_cmds.phones_of_path(path.cpu().numpy(), model.start_pdf, per_frame=True)
    with pytest.raises(ValueError, match='a phone loop'):
        beer.unit_sequences_batch(object(), best)
    with pytest.raises(KeyError):
        beer.unit_sequences_batch(model, [torch.tensor([1, 1, 3])])


def test_mbr_over_the_nbest_list(loop):
    model, utts, table = loop
    k, ws = 4, .5
    stacks, scores = beer.decode_nbest_batch(model, utts, k, scale=.9)
    units, index, risk = beer.mbr_decode_batch(model, utts, nbest=k, scale=.9, weight_scale=ws)
    assert risk.shape == (len(utts), k) and risk.dtype == torch.float64 and risk.is_cuda
    assert index.shape == (len(utts),) and index.dtype == torch.int64
    scores, risk, index = scores.cpu().numpy(), risk.cpu().numpy(), index.cpu().tolist()
    for u, stack in enumerate(stacks):
        seqs = hypotheses(stack, table)
        weights = np.exp(ws * (scores[u].astype(np.longdouble) - scores[u, 0]))
        want, lowest = et.mbr(seqs, weights)
        for r in range(k):
            if seqs[r] is None:
                assert np.isposinf(risk[u, r])
            else:
                print(u, r, risk[u, r], float(want[r]))
                assert abs(risk[u, r] - float(want[r])) <= 1e-10 * max(1., abs(float(want[r])))
        assert want[index[u]] <= lowest + 1e-9
        assert units[u].tolist() == seqs[index[u]]


def test_mbr_over_posterior_samples(loop):
    model, utts, table = loop
    N = 8

    def generator():
        g = torch.Generator(device='cuda')
        g.manual_seed(17)
        return g
    stacks = beer.sample_paths_batch(model, utts, nsamples=N, generator=generator())
    units, index, risk = beer.mbr_decode_batch(model, utts, nsamples=N, generator=generator())
    risk, index = risk.cpu().numpy(), index.cpu().tolist()
    for u, stack in enumerate(stacks):
        seqs = hypotheses(stack, table)
        sums = [sum(et.distance(a, b) for b in seqs) for a in seqs]
        # uniform weights 1 / 8: every product and sum is exact in float64
        assert (risk[u] * N).tolist() == sums
        assert index[u] == sums.index(min(sums))
        assert units[u].tolist() == seqs[index[u]]


def test_mbr_of_one_hypothesis_is_decode(loop):
    model, utts, table = loop
    units, index, risk = beer.mbr_decode_batch(model, utts, nbest=1)
    best = beer.unit_sequences_batch(model, beer.decode_batch(model, utts))
    assert index.tolist() == [0] * len(utts) and risk.tolist() == [[0.]] * len(utts)
    assert [u.tolist() for u in units] == [b.tolist() for b in best]
    model.durations = object()
    try:
        with pytest.raises(NotImplementedError):
            beer.mbr_decode_batch(model, utts, nbest=2)
    finally:
        model.durations = None


def run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_decode_mbr(tmp_path):
    feats = os.path.join(GOLDEN, 'ref_feats.npz')
    ds, mdl = str(tmp_path / 'ds.pkl'), os.path.join(GOLDEN, 'ref_phoneloop.pkl')
    run(['dataset', 'create', str(tmp_path), feats, ds])
    model = hmm_cmds._load(mdl).to('cuda')
    dataset = hmm_cmds._load(ds)
    ids = ['utt0', 'utt1', 'utt2']
    utts = [dataset[u].features for u in ids]
    names = list(model.start_pdf)
    units, index, risk = beer.mbr_decode_batch(model, utts, nbest=8, weight_scale=.25)
    index, risk = index.tolist(), risk.cpu().numpy()
    rk = tmp_path / 'risks'
    out = run(['hmm', 'decode', '--mbr', '--nbest', '8', '--mbr-scale', '0.25', '--risks', str(rk),
               mdl, ds])
    assert out == ''.join(f'{u} ' + ' '.join(names[i] for i in units[n].tolist()) + '\n'
                          for n, u in enumerate(ids))
    assert rk.read_text() == ''.join(f'{u} {index[n] + 1} {risk[n, index[n]]:.6f} {risk[n, 0]:.6f}\n'
                                     for n, u in enumerate(ids))
    # samples: the command seeds its own generator
    g = torch.Generator(device='cuda')
    g.manual_seed(5)
    units, index, _ = beer.mbr_decode_batch(model, utts, nsamples=6, generator=g)
    out = run(['hmm', 'decode', '--mbr', '--nsamples', '6', '--seed', '5', mdl, ds])
    assert out == ''.join(f'{u} ' + ' '.join(names[i] for i in units[n].tolist()) + '\n'
                          for n, u in enumerate(ids))
    per_frame = run(['hmm', 'decode', '--mbr', '--nsamples', '6', '--seed', '5', '--per-frame',
                     mdl, ds]).strip().split('\n')
    assert [len(l.split()) - 1 for l in per_frame] == [35, 50, 41]
    for line, u in zip(per_frame, units):
        assert st.merged(line.split()[1:]) == st.merged([names[i] for i in u.tolist()])
    # one hypothesis: what plain decode prints
    assert run(['hmm', 'decode', '--mbr', '--nbest', '1', mdl, ds]) == run(['hmm', 'decode', mdl, ds])
    with pytest.raises(SystemExit):
        run(['hmm', 'decode', '--mbr', mdl, ds])


def alignments(seed, n_utts=6):
    rng = np.random.RandomState(seed)
    phones = ['aa', 'b', 'iy', 'k', 'sil']
    ref = {}
    for n in range(n_utts):
        frames = []
        while len(frames) < 30 + 10 * n:
            frames += [phones[rng.randint(len(phones))]] * rng.randint(2, 9)
        ref[f'utt{n}'] = frames
    return ref


def write_ali(path, alis):
    path.write_text(''.join(f'{u} ' + ' '.join(frames) + '\n' for u, frames in alis.items()))


def test_cli_evaluate(tmp_path):
    ref = alignments(0)
    relabel = {'aa': 'au3', 'b': 'au1', 'iy': 'au7', 'k': 'au2', 'sil': 'au5'}
    copy = {u: [relabel[l] for l in frames] for u, frames in ref.items()}
    rng = np.random.RandomState(1)
    noisy = {}
    for u, frames in copy.items():
        frames = list(frames)
        for t in rng.choice(len(frames), len(frames) // 3, replace=False):
            frames[t] = f'au{rng.randint(1, 8)}'
        noisy[u] = frames
    write_ali(tmp_path / 'ref', ref)
    utts = list(ref)
    R = [ref[u] for u in utts]
    for name, hyp in (('copy', copy), ('noisy', noisy)):
        write_ali(tmp_path / name, hyp)
        for delta in (2, 0):
            out = run(['hmm', 'evaluate', '--delta', str(delta), '--mapping', str(tmp_path / 'map'),
                       str(tmp_path / 'ref'), str(tmp_path / name)])
            lines, _, amap = st.evaluate_lines(R, [[hyp[u]] for u in utts], delta)
            assert out.strip().split('\n') == lines, (name, delta)
            assert [l.split()[0] for l in lines] == list(hmm_cmds.evaluate.KEYS)
            got_map = dict(l.split() for l in (tmp_path / 'map').read_text().strip().split('\n'))
            assert got_map == amap
    assert out.split('\n')[0] != 'PER 0.00'
    out = run(['hmm', 'evaluate', str(tmp_path / 'ref'), str(tmp_path / 'copy')]).split('\n')
    assert out[0] == 'PER 0.00' and out[4] == 'NMI 100.00' and out[9] == 'fscore 100.00'
    # lists: the noisy hypothesis first, the copy second -- the oracle finds the copy; an utterance
    # only one side has is skipped, a length mismatch is named
    lists = {}
    for u in utts[:-1]:
        lists[f'{u}-1'], lists[f'{u}-2'] = noisy[u], copy[u]
    lists['other-1'] = ['au1']
    write_ali(tmp_path / 'lists', lists)
    out = run(['hmm', 'evaluate', '--lists', str(tmp_path / 'ref'), str(tmp_path / 'lists')])
    lines, oracle, _ = st.evaluate_lines(R[:-1], [[noisy[u], copy[u]] for u in utts[:-1]])
    assert out.strip().split('\n') == lines + [oracle] and oracle == 'closest_PER 0.00'
    assert lines[0] != 'PER 0.00'
    short = dict(copy)
    short['utt3'] = short['utt3'][:-1]
    write_ali(tmp_path / 'short', short)
    with pytest.raises(SystemExit, match='utt3'):
        run(['hmm', 'evaluate', str(tmp_path / 'ref'), str(tmp_path / 'short')])
