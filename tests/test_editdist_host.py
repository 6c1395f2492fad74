"""CPU checks of the edit-distance feature: the C symbols and the header's constants,
`beer_edit_distance_route` against a restatement of the header's formula on both sides of every
boundary, the refusals made before any device work, the truth of tests/editdist_truth.py against
the enumeration of every alignment, tests/scoring_truth.py and beer_amd.scoring's host functions
on hand-computed cases, and the command line's options."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import editdist_truth as et
import scoring_truth as st
from helpers import ROOT

import beer_amd as beer
from beer_amd import _hip, kernels, scoring
from beer_amd.cli import hmm as hmm_cmds, main as cli_main

HAS_GPU = torch.cuda.is_available()


def route(max_short, max_long, ops):
    return _hip.lib().beer_edit_distance_route(max_short, max_long, int(ops))


def test_symbols_are_declared_exported_and_in_the_ctypes_table():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('beer_unit_sequences', 'beer_edit_distance', 'beer_edit_distance_route'):
        assert re.search(r'^int %s\(' % name, text, flags=re.M), f'{name} is not declared'
        assert hasattr(lib, name), f'{name} is not exported'
        assert name in _hip.SIGNATURES
    assert re.search(r'^size_t beer_edit_distance_scratch_bytes\(', text, flags=re.M)
    assert hasattr(lib, 'beer_edit_distance_scratch_bytes')
    assert 'beer_edit_distance_scratch_bytes' in _hip.SIZE_QUERIES
    assert _hip.SIGNATURES['beer_edit_distance_route'] == [ctypes.c_int32, ctypes.c_int32, _hip.c_i]
    assert len(_hip.SIGNATURES['beer_unit_sequences']) == 10            # (with the stream)
    assert len(_hip.SIGNATURES['beer_edit_distance']) == 14
    for macro, value in (('BEER_EDIT_OPS', _hip.EDIT_OPS), ('BEER_EDIT_ROW_LDS', _hip.EDIT_ROW_LDS),
                         ('BEER_EDIT_ROW_WS', _hip.EDIT_ROW_WS)):
        assert int(re.search(r'#define\s+%s\s+(0x[0-9A-Fa-f]+)' % macro, text).group(1), 16) == value
    assert (_hip.EDIT_OPS, _hip.EDIT_ROW_LDS, _hip.EDIT_ROW_WS) == (et.OPS, et.ROW_LDS, et.ROW_WS)
    assert re.search(r'#define\s+BEER_EDIT_MAX_LEN\s+\(1 << 30\)', text)
    assert re.search(r'#define\s+BEER_EDIT_MAX_LEN_OPS\s+\(\(1 << 21\) - 1\)', text)
    assert (_hip.EDIT_MAX_LEN, _hip.EDIT_MAX_LEN_OPS) == (et.MAX_LEN, et.MAX_LEN_OPS) \
        == (1 << 30, 2097151)
    assert _hip.edit_team(0x1140) == 64
    for name in ('unit_sequences', 'edit_distance', 'edit_distance_route'):
        assert name in kernels.__all__ and callable(getattr(kernels, name))
    for name in ('unit_sequences_batch', 'edit_distances', 'token_error_rate', 'closest_error_rate',
                 'mbr_decode_batch', 'contingency', 'maxoverlap_mapping',
                 'normalized_mutual_information', 'entropy_rate', 'boundary_scores'):
        assert name in scoring.__all__ and getattr(beer, name) is getattr(scoring, name)


SHORTS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 2047, 2048, 4095, 4096)
LONGS = (0, 1, 8, 9, 64, 65, 2046, 2047, 2048, 4094, 4095, 4096, 4097, 100000,
         et.MAX_LEN_OPS - 1, et.MAX_LEN_OPS, et.MAX_LEN_OPS + 1, et.MAX_LEN - 1, et.MAX_LEN,
         et.MAX_LEN + 1)


def test_route_is_the_headers_formula():
    seen = set()
    for s, l, ops in itertools.product(SHORTS + (-1,), LONGS + (-1,), (False, True)):
        want = et.route_formula(s, l, ops)
        assert route(s, l, ops) == want, (s, l, ops)
        seen.add(want)
    teams = {8, 16, 32, 64}
    assert seen == {_hip.EINVAL} | teams | {t | et.OPS for t in teams} | \
        {64 | r | o for r in (et.ROW_LDS, et.ROW_WS) for o in (0, et.OPS)}


def test_route_thresholds_sit_where_the_header_says():
    O, L, W = et.OPS, et.ROW_LDS, et.ROW_WS
    for s, team in ((0, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)):
        assert route(s, 5000, False) == team and route(s, 5000, True) == team | O
        assert _hip.edit_team(route(s, 64, True)) == team
    # strips: the boundary row of max_long + 1 cells in a wave's 16 KiB of LDS, or the workspace
    assert route(65, 4095, False) == 64 | L and route(65, 4096, False) == 64 | W
    assert route(65, 2047, True) == 64 | O | L and route(65, 2048, True) == 64 | O | W
    assert route(65, 65, False) == 64 | L and route(700, 1500, True) == 64 | O | L
    # the length limits, and orders that make no sense
    assert route(65, et.MAX_LEN_OPS, True) == 64 | O | W
    assert route(65, et.MAX_LEN_OPS + 1, True) == _hip.EINVAL
    assert route(3, et.MAX_LEN_OPS + 1, True) == _hip.EINVAL
    assert route(3, et.MAX_LEN_OPS + 1, False) == 8
    assert route(65, et.MAX_LEN, False) == 64 | W and route(65, et.MAX_LEN + 1, False) == _hip.EINVAL
    assert route(9, 8, False) == _hip.EINVAL and route(-1, 8, False) == _hip.EINVAL
    with pytest.raises(_hip.HipInvalid):
        kernels.edit_distance_route(4, et.MAX_LEN_OPS + 1, ops=True)
    assert kernels.edit_distance_route(4, 9, ops=True) == 8 | O


def test_scratch_query_and_refusals_with_no_device_work():
    'NULL pointers everywhere: the launcher returns before it looks at one.'
    lib = _hip.lib()
    size = lib.beer_edit_distance_scratch_bytes
    assert size(10, 64, 100000, 0) == 0 and size(10, 65, 4095, 0) == 0 and size(0, 65, 5000, 0) == 0
    # one row per wave of the grid (four waves a workgroup, a pair a wave)
    assert size(10, 65, 4096, 0) == 12 * 4097 * 4
    assert size(4, 65, 2048, 1) == 4 * 2049 * 8
    assert size(10, 65, et.MAX_LEN_OPS + 1, 1) == 0
    fn = lib.beer_edit_distance
    for s, l, with_ops in ((9, 8, False), (-1, 8, False), (65, et.MAX_LEN + 1, False)):
        assert fn(None, None, None, 3, None, None, 5, s, l, None, None, None, 0, None) == _hip.EINVAL
    assert fn(None, None, None, -1, None, None, 5, 3, 4, None, None, None, 0, None) == _hip.EINVAL
    assert fn(None, None, None, 3, None, None, -1, 3, 4, None, None, None, 0, None) == _hip.EINVAL
    assert fn(None, None, None, 3, None, None, 5, 3, 4, None, None, None, 0, None) == _hip.EINVAL
    assert fn(None, None, None, 3, None, None, 0, 3, 4, None, None, None, 0, None) == 0
    units = lib.beer_unit_sequences
    assert units(None, None, None, -1, None, 4, None, None, None, None) == _hip.EINVAL
    assert units(None, None, None, 2, None, 0, None, None, None, None) == _hip.EINVAL
    assert units(None, None, None, 2, None, 4, None, None, None, None) == _hip.EINVAL
    assert units(None, None, None, 0, None, 4, None, None, None, None) == 0


# --- the truth itself ---------------------------------------------------------------------------

def random_pairs(n, max_len, alphabet, seed):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, alphabet, rng.randint(0, max_len + 1)).tolist(),
             rng.randint(0, alphabet, rng.randint(0, max_len + 1)).tolist()) for _ in range(n)]


def test_truth_is_the_enumeration_of_every_alignment():
    ties = 0
    for a, b in random_pairs(3000, 5, 3, 0):
        got = et.edit_ops(a, b)
        assert got == et.enumerated(a, b), (a, b)
        assert got[0] == sum(got[1:]) and got[2] - got[3] == len(a) - len(b)
        # deletions and insertions swap with the arguments
        back = et.edit_ops(b, a)
        assert back == (got[0], got[1], got[3], got[2]), (a, b)
        ties += got[2] > 0 and got[3] > 0
    # the order on (sub, del, ins) decides often: ab -> ba is a deletion and an insertion, not
    # two substitutions
    assert ties > 100 and et.edit_ops([0, 1], [1, 0]) == (2, 0, 1, 1)


def test_truth_is_a_metric():
    rng = np.random.RandomState(1)
    for _ in range(300):
        a, b, c = (rng.randint(0, 3, rng.randint(0, 9)).tolist() for _ in range(3))
        assert et.distance(a, a) == 0 and et.edit_ops(a, a) == (0, 0, 0, 0)
        assert et.distance(a, b) == et.distance(b, a)
        assert et.distance(a, c) <= et.distance(a, b) + et.distance(b, c)
        assert abs(len(a) - len(b)) <= et.distance(a, b) <= max(len(a), len(b))
    assert et.edit_ops('kitten', 'sitting') == (3, 2, 0, 1)
    assert et.edit_ops([], [1, 2]) == (2, 0, 0, 2) and et.edit_ops([1, 2], []) == (2, 0, 2, 0)
    # of the two cheapest alignments of ab -> b the truth names the deletion, not sub + ...
    assert et.edit_ops([0, 1], [1]) == (1, 0, 1, 0)


def test_truth_unit_sequences_are_phones_of_path():
    start = {'a': 0, 'b': 3, 'c': 6}
    table = np.full(9, -1)
    table[[0, 3, 6]] = [0, 1, 2]
    names = list(start)
    rng = np.random.RandomState(2)
    for _ in range(50):
        path = np.concatenate([[rng.choice([0, 3, 6])], rng.randint(0, 9, rng.randint(0, 30))])
        units, frames = et.unit_sequence(path, table)
        assert [names[u] for u in units] == hmm_cmds.phones_of_path(path, start)
        assert [names[u] for u in frames] == hmm_cmds.phones_of_path(path, start, per_frame=True)
    assert et.unit_sequence([], table) == ([], [])
    assert et.unit_sequence([-1, -1], table) == (-1, -1)
    assert et.unit_sequence([1, 3], table) == (-2, -2) and et.unit_sequence([0, 9], table) == (-2, -2)
    # re-entry into the same unit through its first pdf
    assert et.unit_sequence([0, 1, 2, 0, 0, 1], table)[0] == [0, 0]


# --- the scores of acoustic unit discovery ---------------------------------------------------

def as_ids(utts):
    names = sorted({l for u in utts for l in u})
    return [np.asarray([names.index(l) for l in u]) for u in utts]


def test_a_perfect_relabelling_scores_perfectly():
    ref = [list('aaabbbccaa'), list('ccccab')]
    relabel = {'a': 'z', 'b': 'x', 'c': 'y'}
    hyp = [[relabel[l] for l in u] for u in ref]
    counts = st.frame_counts(ref, hyp)
    assert st.nmi(counts) == pytest.approx(100.)
    amap = st.mapping(counts, sorted(relabel))
    assert amap == {v: k for k, v in relabel.items()}
    mapped = [st.merged([amap[l] for l in u]) for u in hyp]
    assert st.token_errors([st.merged(u) for u in ref], mapped) == (0, 0, 0, 0, 7, 2)
    assert st.boundary_scores(ref, hyp)[0] == (100., 100., 100.)
    lines, oracle, _ = st.evaluate_lines(ref, [[h] for h in hyp])
    assert lines[0] == 'PER 0.00' and lines[4] == 'NMI 100.00' and lines[9] == 'fscore 100.00'
    assert lines[10] == 'n_units 3' and oracle == 'closest_PER 0.00'
    # ... and the library's host functions agree
    R, H = as_ids(ref), as_ids(hyp)
    table = beer.contingency(R, H)
    assert table.dtype == np.int64 and table.shape == (3, 3) and table.sum() == 16
    assert beer.normalized_mutual_information(table) == pytest.approx(100.)
    np.testing.assert_array_equal(beer.maxoverlap_mapping(table), [1, 2, 0])    # x y z -> b c a
    assert tuple(beer.boundary_scores(R, H)) == (100., 100., 100., 5, 5, 5)


def test_nmi_entropy_and_mapping_by_hand():
    # one constant label on both sides: no entropy at all
    assert st.nmi(st.frame_counts([list('aaaa')], [list('zzzz')])) == 0.
    assert beer.normalized_mutual_information(np.array([[4]])) == 0.
    # independent labels: no mutual information; a 2 x 2 table worked by hand
    assert beer.normalized_mutual_information(np.array([[2, 2], [2, 2]])) == pytest.approx(0.)
    table = np.array([[3, 1], [0, 4]])
    h_x = 1.
    h_y = -(3 / 8 * np.log2(3 / 8) + 5 / 8 * np.log2(5 / 8))
    h_xy = -(3 / 8 * np.log2(3 / 8) + 1 / 8 * np.log2(1 / 8) + .5 * np.log2(.5))
    want = 200 * (h_y - (h_xy - h_x)) / (h_x + h_y)
    assert beer.normalized_mutual_information(table) == pytest.approx(want, abs=1e-12)
    assert st.nmi({'x': {'a': 3, 'b': 1}, 'y': {'b': 4}}) == pytest.approx(want, abs=1e-12)
    # the first maximum wins
    np.testing.assert_array_equal(beer.maxoverlap_mapping(np.array([[2, 2, 1], [0, 5, 5]])), [0, 1])
    assert st.mapping({'x': {'b': 2, 'a': 2}}, ['a', 'b']) == {'x': 'a'}
    # entropy rate: repeats merged, then unigrams -- a a b | b a -> a b b a: one bit
    assert beer.entropy_rate([[0, 0, 1], [1, 0]]) == pytest.approx((1., 2.))
    assert st.entropy_rate([list('aab'), list('ba')]) == pytest.approx((1., 2.))
    assert beer.entropy_rate([[5, 5, 5]]) == (0., 1.) and beer.entropy_rate([]) == (0., 1.)


def test_boundaries_by_hand():
    ref = [0] * 10 + [1] * 10                                  # one boundary, at frame 10

    def hyp(at):
        return [0] * at + [1] * (20 - at)
    for delta in (0, 1, 2, 3):
        for off in (delta, delta + 1):
            for at in (10 - off, 10 + off):
                want_hit = off <= delta
                got = beer.boundary_scores([ref], [hyp(at)], delta=delta)
                assert (got.hits, got.n_ref, got.n_hyp) == (int(want_hit), 1, 1), (delta, at)
                assert got.fscore == (100. if want_hit else 0.)
                assert st.boundary_scores([ref], [hyp(at)], delta)[1] == (int(want_hit), 1, 1)
    # two hypothesis boundaries (9 and 11) compete for the one at 10: the first takes it
    two = [0] * 9 + [1] * 2 + [0] * 9
    got = beer.boundary_scores([ref], [two])
    assert (got.hits, got.n_ref, got.n_hyp) == (1, 1, 2)
    assert (got.recall, got.precision) == (100., 50.) and got.fscore == pytest.approx(200 / 3)
    assert st.boundary_scores([ref], [two])[1] == (1, 1, 2)
    # the nearest FREE one: reference at 5 and 8, hypothesis at 6 and 7 -> 6 takes 5, 7 takes 8
    r2 = [0] * 5 + [1] * 3 + [2] * 4
    h2 = [0] * 6 + [1] + [2] * 5
    assert beer.boundary_scores([r2], [h2], delta=1).hits == 2 == st.boundary_scores([r2], [h2], 1)[1][0]
    # equally near: the first; no reference boundary: no hits
    r3 = [0] * 4 + [1] * 4 + [2] * 4                           # 4 and 8
    h3 = [0] * 6 + [1] * 6                                     # 6
    assert beer.boundary_scores([r3], [h3]).hits == 1
    got = beer.boundary_scores([[0] * 8], [h3[:8]])
    assert tuple(got) == (0., 0., 0., 0, 0, 1)
    assert st.boundary_scores([[0] * 8], [h3[:8]]) == ((0., 0., 0.), (0, 0, 1))


def test_token_errors_tuple():
    got = scoring.TokenErrors(3, 1, 1, 1, 12, 2)
    assert got.rate == 25. and got.dele == 1 and scoring.TokenErrors(0, 0, 0, 0, 0, 0).rate == 0.
    assert st.token_errors([[1, 2, 3]], [[1, 3]]) == (1, 0, 1, 0, 3, 1)
    assert st.oracle_errors([[1, 2, 3]], [[[1], [1, 2, 4], [1, 2, 3, 3]]]) == (1, 1, 0, 0, 3, 1)


# --- errors raised on the host, the command line --------------------------------------------

def test_index_and_argument_errors_come_before_any_device_work():
    with pytest.raises(ValueError):
        beer.edit_distances([[1]], [[1], [2]])
    with pytest.raises(ValueError):
        beer.closest_error_rate([[1]], [[]])
    with pytest.raises(ValueError):
        beer.mbr_decode_batch(None, [], nbest=2, nsamples=3)
    with pytest.raises(ValueError):
        beer.mbr_decode_batch(None, [])
    with pytest.raises(ValueError):
        beer.contingency([0, 1], [0])
    with pytest.raises(ValueError):
        beer.boundary_scores([[0]], [])


@pytest.mark.skipif(HAS_GPU, reason='checks behaviour on a GPU-less host')
def test_fails_loudly_without_gpu():
    with pytest.raises(_hip.HipUnavailable):
        beer.edit_distances([[1, 2]], [[1]])
    with pytest.raises(_hip.HipUnavailable):
        kernels.unit_sequences(torch.zeros(3, dtype=torch.int64), [0], [3], [0, -1])


def test_decode_takes_the_mbr_options_and_refuses_bad_ones():
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'decode', '--mbr', '--nbest', '4', '--risks', 'r',
                              '--mbr-scale', '0.5', '--per-frame', 'mdl', 'ds'])
    assert (args.mbr, args.nbest, args.risks, args.mbr_scale) == (True, 4, 'r', .5)
    hmm_cmds.decode.check(args)
    hmm_cmds.decode.check(parser.parse_args(['hmm', 'decode', '--mbr', '--nsamples', '8', 'm', 'd']))
    args = parser.parse_args(['hmm', 'decode', 'mdl', 'ds'])
    assert (args.mbr, args.risks, args.mbr_scale) == (False, None, 1.)
    hmm_cmds.decode.check(args)
    # refused before the model (a file that does not exist) is read
    for argv in (['--mbr'], ['--mbr', '--predictive'], ['--mbr', '--nbest', '3', '--predictive'],
                 ['--mbr', '--nbest', '3', '--scores', 'sc'], ['--mbr', '--nbest', '3', '--distinct'],
                 ['--mbr', '--nbest', '3', '--nsamples', '3'], ['--mbr', '--nbest', '17'],
                 ['--mbr', '--nsamples', '0'], ['--risks', 'r'], ['--nbest', '3', '--risks', 'r']):
        args = parser.parse_args(['hmm', 'decode'] + argv + ['no-such-model', 'no-such-dataset'])
        with pytest.raises(SystemExit):
            args.func(args, None)


def test_evaluate_is_a_command_and_parses(tmp_path):
    parser = cli_main.build_parser()
    args = parser.parse_args(['hmm', 'evaluate', 'ref', 'hyp'])
    assert (args.delta, args.mapping, args.lists, args.ref_ali, args.hyp_ali) == \
        (2, None, False, 'ref', 'hyp')
    args = parser.parse_args(['hmm', 'evaluate', '--delta', '3', '--mapping', 'm', '--lists', 'r', 'h'])
    assert (args.delta, args.mapping, args.lists) == (3, 'm', True)
    assert hmm_cmds.COMMANDS.count(hmm_cmds.evaluate) == 1
    assert hmm_cmds.COMMANDS[-1] is hmm_cmds.boundaries
    # reading and pairing the two files: no device work
    (tmp_path / 'ref').write_text('u1 a a b\nu2 b b\n\nu3 a\n')
    (tmp_path / 'hyp').write_text('u2 x y\nu1 x x y\nu4 x\n')
    ref = hmm_cmds.read_alignments(str(tmp_path / 'ref'))
    hyp = hmm_cmds.read_alignments(str(tmp_path / 'hyp'))
    assert list(ref) == ['u1', 'u2', 'u3'] and ref['u1'] == ['a', 'a', 'b']
    uttids, R, H, skipped = hmm_cmds.evaluate.collect(ref, hyp, False)
    assert uttids == ['u1', 'u2'] and skipped == 2
    assert R == [['a', 'a', 'b'], ['b', 'b']] and H == [[['x', 'x', 'y']], [['x', 'y']]]
    lists = {'u1-2': ['y', 'y', 'y'], 'u1-1': ['x', 'x', 'y'], 'u2-1': ['x', 'y']}
    uttids, R, H, skipped = hmm_cmds.evaluate.collect(ref, lists, True)
    assert uttids == ['u1', 'u2'] and skipped == 1
    assert H == [[['x', 'x', 'y'], ['y', 'y', 'y']], [['x', 'y']]]
    # a length mismatch names the utterance; a label that is no "<uttid>-<r>" is refused
    with pytest.raises(SystemExit, match='u2'):
        hmm_cmds.evaluate.collect(ref, {'u1': ['x'] * 3, 'u2': ['x'] * 3}, False)
    with pytest.raises(SystemExit, match='u9'):
        hmm_cmds.evaluate.collect(ref, {'u9': ['x']}, True)
