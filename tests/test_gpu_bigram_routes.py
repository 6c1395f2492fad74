"""Every launch form of the bigram forward-backward kernel (csrc/hmm_bigram.hip:
`fb_bigram_kernel<T, WT, SPL, DEG>` behind `beer_hmm_posteriors_bigram`) against the oracle, on
graphs that sit on the launcher's boundaries (tests/bigram_truth.py).

One static table: each case names the form the launcher must pick for it -- SPL states per lane,
DEG residual arcs unrolled, waves per workgroup (`beer_hmm_bigram_route`) -- and each test first
holds the C layer's answer for the live device against the table, then sees through a spy on
`_hip.call` that the kernel ran exactly once and the log-space path not at all, then compares
`state_resps`, `counts` and `utt_llh` with the float64 oracle: float64 to a relative 1e-9,
float32 to a flat 1e-5 (`state_resps` absolute).  FORMS: all 15 SPL x DEG forms at the smallest and
the largest size of every SPL band, P from 1 to 128 around the two member chunks of 64, ragged
batches of 1 to 9 frames with one utterance without a frame, every pdf-id flavour, -inf block
entries, and the block 120 nats down (below float32's exp).  WAVES: 2, 3, 7 and 8 waves per
workgroup with every utterance different, and utterances run alone (one wave) equal to their rows
of the batch bit for bit.  Then the range fallback on both sides of the kernel's 2^-800, and the
refusals (9 residual arcs, 129 phones) on the general path.

Worst errors observed on an MI355X over the whole file: float64 1.0e-13 (state_resps), 5.3e-14
(counts), 3.2e-14 (utt_llh); float32 7.7e-8 (state_resps, absolute), 7.9e-8 (counts), 9.8e-8
(utt_llh)."""

from collections import namedtuple
import ctypes

import numpy as np
import pytest
import torch

import bigram_truth as bt
from helpers import assert_close, rel_err

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import _hip, hmm_kernels as hk                        # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
DTYPES = dict(argvalues=[torch.float64, torch.float32], ids=['f64', 'f32'])

# nutt = per_cu * (compute units of the device) + extra; `waves`: what the launcher then picks
Case = namedtuple('Case', 'S P d placement neg deep flavour scale S_total per_cu extra lens '
                          'spl deg waves seed')
VARIANTS = [('perm', 1., 0), ('repeat', .8, 0), ('partial', 1., 5), ('perm', .8, 0),
            ('repeat', 1., 3), ('partial', .8, 1)]
SPL_BANDS = [(64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 5), (320, 5), (321, 8), (512, 8)]
# residual arcs a state on both sides of 2|3 and 4|5, and at 8: the lower one at the smallest
# size of a band, the upper one at its largest
DEGREES = {2: (1, 2), 4: (3, 4), 8: (5, 8)}
BLOCK_SIZES = (1, 2, 63, 64, 65, 127, 128)
FORMS, WAVES = [], []


def add(table, S, P, d, placement, spl, deg, waves=1, per_cu=0, extra=8, lens=bt.LENGTHS,
        neg=None, deep=None):
    i = len(FORMS) + len(WAVES)
    flavour, scale, wider = VARIANTS[i % len(VARIANTS)]
    table.append(Case(S, P, d, placement, (.3 if i % 3 == 1 else 0.) if neg is None else neg,
                      (i % 4 == 2) if deep is None else deep, flavour, scale, S + wider,
                      per_cu, extra, tuple(lens), spl, deg, waves, 500 + i))


# 1. every SPL x DEG form at both ends of its band of sizes; the block sizes walk through
#    BLOCK_SIZES (P < S: with P = S no arc is left outside the block, see 2.)
for k_, (S_, spl_) in enumerate(SPL_BANDS):
    for deg_ in (2, 4, 8):
        n_ = len(FORMS)
        fit_ = [p for p in BLOCK_SIZES if p < S_]
        P_ = fit_[(2 * n_ + n_ // 7) % len(fit_)]
        place_ = ('disjoint', 'overlap', 'identical')[n_ % 3]
        # (a block of one or two arcs that leads back into its own sources loses a long utterance
        #  to the many paths of the residual graph: those keep their sides apart)
        place_ = 'disjoint' if P_ <= 2 else ('overlap' if 2 * P_ > S_ and place_ == 'disjoint' else place_)
        add(FORMS, S_, P_, DEGREES[deg_][k_ % 2], place_, spl_, deg_)
# 2. no residual arc at all (one-state phones): every arc in the block, src == dst
for S_, spl_ in [(1, 1), (64, 1), (65, 2), (128, 2)]:
    add(FORMS, S_, S_, 0, 'identical', spl_, 2)
# 3. the member chunks of 64 on the smallest graphs that hold them, block sides apart
for P_, S_, spl_ in [(1, 2, 1), (63, 126, 2), (64, 128, 2), (65, 130, 4), (127, 254, 4), (128, 256, 4)]:
    add(FORMS, S_, P_, 2, 'disjoint', spl_, 2)

# 4. more than one wave per workgroup: every utterance different, the last workgroup not full
add(WAVES, 40, 7, 2, 'overlap', 1, 2, waves=2, per_cu=1, extra=1, neg=0., deep=False)
add(WAVES, 64, 31, 3, 'disjoint', 1, 4, waves=8, per_cu=7, extra=1, neg=.3, deep=False)
add(WAVES, 15, 5, 2, 'disjoint', 1, 2, waves=8, per_cu=8, extra=3, neg=0., deep=True)
#    the LDS behind W = exp(block) (P = 128: 129 KiB of 160) holds 7 waves' columns of 128
#    states, 3 waves' of 512
add(WAVES, 128, 128, 0, 'identical', 2, 2, waves=7, per_cu=6, extra=1, lens=(1, 2, 3, 4), neg=.3,
    deep=False)
add(WAVES, 512, 128, 2, 'reversed', 8, 2, waves=3, per_cu=2, extra=1, lens=(1, 2, 3), neg=0.,
    deep=False)


def case_id(c):
    return (f'{c.seed}-S{c.S}-P{c.P}-d{c.d}-{c.placement}-{c.flavour}'
            f'{"-neg" if c.neg else ""}{"-deep" if c.deep else ""}-spl{c.spl}-deg{c.deg}-w{c.waves}')


def case_nutt(c, n_cu):
    return c.per_cu * n_cu + c.extra


def case_graph(c, dtype=np.float64):
    return bt.make_graph(c.S, c.P, c.d, c.placement, c.seed, c.neg, c.deep, dtype)


def case_inputs(c, n_cu, dtype=np.float64):
    '(graph arrays, pdf ids, lengths, pc_all, llhs) of a case on a device of `n_cu` compute units.'
    g = case_graph(c, dtype)
    ids = bt.pdf_ids(c.S, c.flavour, c.S_total, c.seed)
    lens = bt.lengths(case_nutt(c, n_cu), c.seed, c.lens, zero=not c.per_cu)
    pc_all, llhs = bt.inputs(lens, ids, c.S_total, c.scale, c.seed, dtype)
    return g, ids, lens, pc_all, llhs


def route_value(spl, deg, waves):
    return spl | deg << 8 | waves << 16


class Spy:
    'Records the names of the entry points called through _hip.call.'

    def __init__(self, monkeypatch):
        self.names = []
        real = _hip.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(_hip, 'call', call)

    def count(self, name):
        return self.names.count(name)


def compiled(g, ids):
    graph = beer.graph.CompiledGraph(tt(g['init']), tt(g['final']), tt(g['trans']),
                                     [int(i) for i in ids])
    graph.set_bigram_block(g['src'], torch.zeros(g['P'], dtype=graph.trans_log_probs.dtype),
                           g['dst'], tt(g['block']))
    return graph


def route_of(img, dtype, nutt, n_cu=0):
    return _hip.lib().beer_hmm_bigram_route(_hip.dtype_code(dtype), ctypes.byref(img.struct), nutt,
                                            n_cu)


def n_cu_of_device():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def run(graph, lens, pc_all, scale, dtype):
    batch = hk.HmmBatch([graph], [0] * len(lens), lens, dtype)
    utt = torch.zeros(len(lens), dtype=torch.float64, device=batch.device)
    sr, counts = hk.posteriors_bigram(batch, tt(pc_all), scale, utt_llh=utt)
    return batch, npy(sr), npy(counts), npy(utt)


def check(dtype, got, want, what):
    'float64: relative 1e-9; float32: 1e-5 flat, state_resps absolute.  Prints what it saw.'
    sr, counts, utt = got
    assert sr.dtype == NP[dtype] and counts.dtype == np.float64
    f32 = dtype == torch.float32
    errs = (np.abs(sr - want['state_resps']).max() if f32 else rel_err(sr, want['state_resps']),
            rel_err(counts, want['counts']), rel_err(utt, want['utt_llh']))
    print(f'{what} {"f32" if f32 else "f64"}: state_resps {errs[0]:.3e} '
          f'counts {errs[1]:.3e} utt_llh {errs[2]:.3e}')
    assert sr.shape == want['state_resps'].shape
    if f32:
        np.testing.assert_allclose(sr, want['state_resps'], rtol=0, atol=1e-5,
                                   err_msg=f'{what} state_resps')
    else:
        assert_close(sr, want['state_resps'], 1e-9, f'{what} state_resps')
    tol = 1e-5 if f32 else 1e-9
    assert_close(counts, want['counts'], tol, f'{what} counts')
    assert_close(utt, want['utt_llh'], tol, f'{what} utt_llh')


def run_case(c, dtype, monkeypatch):
    n_cu = n_cu_of_device()
    g, ids, lens, pc_all, llhs = case_inputs(c, n_cu, NP[dtype])
    graph = compiled(g, ids)
    img = graph.bigram_image(dtype)
    assert img is not None and img.max_degree == g['max_degree'] == c.d
    want_route = route_value(c.spl, c.deg, c.waves)
    for cus in (0, n_cu):
        assert route_of(img, dtype, len(lens), cus) == want_route
    spy = Spy(monkeypatch)
    batch, sr, counts, utt = run(graph, lens, pc_all, c.scale, dtype)
    assert hk.bigram_ok(batch)
    assert spy.count('beer_hmm_posteriors_bigram') == 1
    assert spy.count('beer_hmm_forward_backward') == 0 and spy.count('beer_hmm_gather') == 0
    repeats, covers = batch.pdf_ids_profile(c.S_total)
    assert (repeats, covers) == (c.flavour == 'repeat' and c.S > 1, c.flavour == 'perm')
    want = bt.truth(g, llhs, ids, c.S_total, c.scale, vectorised=len(lens) > 16)
    check(dtype, (sr, counts, utt), want, case_id(c))
    if c.deep:
        assert want['counts'].sum() > 0 and counts.sum() > 0
        assert float(np.exp(np.float32(g['block'][np.isfinite(g['block'])].max()))) == 0.
    return g, ids, lens, pc_all, graph, (sr, utt)


@pytest.mark.parametrize('dtype', **DTYPES)
@pytest.mark.parametrize('c', FORMS, ids=case_id)
def test_every_form_against_the_oracle(c, dtype, monkeypatch):
    g, ids, lens, pc_all, graph, (sr, utt) = run_case(c, dtype, monkeypatch)
    off = np.concatenate([[0], np.cumsum(lens)])
    u = lens.index(0)
    assert off[u] == off[u + 1] and utt[u] == 0.
    # ids left out of a wider S_total stay zero
    left_out = np.setdiff1d(np.arange(c.S_total), ids)
    assert not sr[:, left_out].any()


@pytest.mark.parametrize('dtype', **DTYPES)
@pytest.mark.parametrize('c', WAVES, ids=case_id)
def test_waves_of_a_workgroup_do_not_see_each_other(c, dtype, monkeypatch):
    '''Several waves share W and the workgroup's LDS.  An utterance run alone is a workgroup of
    one wave running the same program on the same data: its rows of the batch result must be the
    same bit for bit (where the posteriors are stored, not added atomically).'''
    g, ids, lens, pc_all, graph, (sr, utt) = run_case(c, dtype, monkeypatch)
    assert len(lens) > n_cu_of_device() and 0 not in lens
    off = np.concatenate([[0], np.cumsum(lens)])
    order = np.argsort(-np.asarray(lens), kind='stable')       # the order waves take utterances
    # the first and the last workgroup, and one in the middle on either side of a workgroup's edge
    sample = {int(order[k]) for k in (0, 1, c.waves - 1, c.waves, len(lens) // 2, len(lens) - 2,
                                      len(lens) - 1)}
    img = graph.bigram_image(dtype)
    for u in sorted(sample):
        assert route_of(img, dtype, 1) == route_value(c.spl, c.deg, 1)
        _, sr1, _, utt1 = run(graph, [lens[u]], pc_all[off[u]:off[u + 1]], c.scale, dtype)
        np.testing.assert_array_equal(utt[u], utt1[0], err_msg=f'utterance {u}')
        if c.flavour != 'repeat':       # (repeated ids are added atomically, in any order)
            np.testing.assert_array_equal(sr[off[u]:off[u + 1]], sr1, err_msg=f'utterance {u}')


# --- the range fallback ------------------------------------------------------------------------
# The kernel gives an utterance up when a column's largest entry, or a frame's normaliser, falls
# below 2^-800 = e^-554.5 (hmm_bigram.hip: `rescale`, `norm`).  Residual arcs i -> i, i + 1; the
# block from the last P states to the first P; init on states 0..2: at frame 1 of a 3-frame
# utterance the reachable states are 0..3, and their log-likelihoods sit `gap` nats below the
# other states' -- the column's largest entry is e^-gap times a predecessor sum between e^-4 and 2
# (weights in (-3, 0), the previous column in [1/2, 1)).  So gap = 500 stays inside by 50 nats and
# gap = 700 is outside by 140.

FALLBACK_S, FALLBACK_P = 6, 2


def fallback_batch(gap, dtype):
    g = bt.make_graph(FALLBACK_S, FALLBACK_P, 2, 'reversed', 77, dtype=dtype, O=(0, 1),
                      init_states=(0, 1, 2))
    ids = bt.pdf_ids(FALLBACK_S, 'perm', FALLBACK_S, 77)
    lens = [5, 2, 3, 9, 1]                     # (the third one is the twin)
    pc_all, llhs = bt.inputs(lens, ids, FALLBACK_S, 1., 77, dtype)
    pc_all[7 + 1, ids[:4]] -= dtype(gap)
    llhs[2][1, :4] -= dtype(gap)
    return g, ids, lens, pc_all, llhs


@pytest.mark.parametrize('dtype', **DTYPES)
@pytest.mark.parametrize('gap,flagged', [(500., False), (700., True)], ids=['gap500', 'gap700'])
def test_range_fallback_on_both_sides_of_the_kernels_limit(gap, flagged, dtype, monkeypatch):
    '''Inside the range the kernel serves the batch alone; outside it flags the utterance and the
    whole sub-batch -- ordinary utterances included -- is redone in log space, with the same
    results.'''
    g, ids, lens, pc_all, llhs = fallback_batch(gap, NP[dtype])
    np.testing.assert_array_equal(llhs[2], pc_all[7:10][:, ids])
    graph = compiled(g, ids)
    assert graph.bigram_image(dtype).max_degree == 2
    spy = Spy(monkeypatch)
    batch, sr, counts, utt = run(graph, lens, pc_all, 1., dtype)
    assert hk.bigram_ok(batch)
    assert spy.count('beer_hmm_posteriors_bigram') == 1
    assert spy.count('beer_hmm_forward_backward') == int(flagged)
    assert spy.count('beer_hmm_gather') == int(flagged)
    want = bt.truth(g, llhs, ids, FALLBACK_S, 1.)
    assert want['counts'].sum() > .05 and want['utt_counts'][2] == 0.
    check(dtype, (sr, counts, utt), want, f'gap {gap:g}')


@pytest.mark.parametrize('dtype', **DTYPES)
@pytest.mark.parametrize('S,P,d', [(64, 5, 9), (300, 129, 2)], ids=['9arcs', '129phones'])
def test_graphs_the_kernel_refuses_take_the_general_path(S, P, d, dtype, monkeypatch):
    g = bt.make_graph(S, P, d, 'disjoint', 91, dtype=NP[dtype])
    assert g['max_degree'] == d
    ids = bt.pdf_ids(S, 'perm', S, 91)
    lens = bt.lengths(5, 91)
    pc_all, llhs = bt.inputs(lens, ids, S, .8, 91, NP[dtype])
    graph = compiled(g, ids)
    assert graph.bigram_image(dtype) is None
    desc = _hip.Bigram(S, P, d, 0, *([None] * 14))
    assert _hip.lib().beer_hmm_bigram_route(_hip.dtype_code(dtype), ctypes.byref(desc), 5, 0) == \
        _hip.EINVAL
    spy = Spy(monkeypatch)
    batch, sr, counts, utt = run(graph, lens, pc_all, .8, dtype)
    assert not hk.bigram_ok(batch)
    assert spy.count('beer_hmm_posteriors_bigram') == 0
    assert spy.count('beer_hmm_forward_backward') == 1
    check(dtype, (sr, counts, utt), bt.truth(g, llhs, ids, S, .8), f'refused S{S} P{P} d{d}')
