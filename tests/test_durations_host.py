"""CPU checks of the explicit-duration (hidden semi-Markov) layer: the truth of
tests/hsmm_truth.py itself, pinned three ways (the geometric equivalence and the count-down HMM
against the repository's HMM oracle, and enumeration of every segmentation), the route and the
workspace size against restatements of the header's text, the argument errors raised before any
device work, `StateDurations`, pickles and the refused combinations of the model and the command
line."""

import ctypes
import io
import pickle
import sys

import numpy as np
import pytest
import torch

import evidence_truth as et
import fb_truth as ft
import hsmm_truth as ht
from helpers import rel_err
from transitions_truth import decode_graph, loop_topology

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import hmm as hmm_cmds, main as cli_main
from beer_amd.models.durations import StateDurations

PIN = 1e-12            # the two float64 computations differ by rounding only (1.2e-14 observed)
GRAPHS = ((1, 0), (3, 0), (8, 0), (12, 4))


def desc(max_states, nutt=3, all_lowdeg=0, max_degree=0, max_hubs=0):
    'A beer_batch with only its scalar fields filled: all the queries may read.'
    return _hip.Batch(nutt, max_states, 1, 1, all_lowdeg, 1, None, None, None, None, None, None,
                      max_degree, max_hubs, 0, 0, None)


# --- the truth, pinned -------------------------------------------------------------------------

@pytest.mark.parametrize('S,hub', GRAPHS)
def test_geometric_duration_laws_are_the_hmm(S, hub):
    g = ft.make_graph(S, ft.offsets(3, S), 5, hub)
    for T in ft.LENGTHS:
        l = np.random.RandomState(T).randn(T, S) * 3
        p = ht.posteriors(g, ht.geometric_log_dur(g, T), None, l)
        t = ft.truth(g, [l], factored_hub=False)
        _, Z = et.evidence(g, l)
        xi = t['xi_dense'].copy()
        np.fill_diagonal(xi, 0.)
        assert rel_err(p['gamma'], t['gamma'][0]) <= PIN
        assert abs(p['Z'] - Z) <= PIN * (abs(Z) + 1)
        assert rel_err(p['entry_sum'], xi.sum(0)) <= PIN
        assert rel_err(p['gamma0_sum'], t['gamma0']) <= PIN


@pytest.mark.parametrize('S,hub', GRAPHS)
@pytest.mark.parametrize('D', [1, 3, 4])
def test_the_count_down_hmm_computes_the_same(S, hub, D):
    g = ft.make_graph(S, ft.offsets(3, S), 6, hub)
    rng = np.random.RandomState(S * D)
    ld, lw = rng.uniform(-3, 0, size=(S, D)), rng.uniform(0, 1, size=S)
    infeasible = 0
    for T in ft.LENGTHS:
        l = rng.randn(T, S) * 3
        p = ht.posteriors(g, ld, lw, l)
        eg = ht.expanded(g, ld, lw)
        le = np.repeat(l, D, axis=1)
        _, Z = et.evidence(eg, le)
        if not np.isfinite(Z):
            # (S = 1: no arc is left once the self-loop is the law's, and T > D cannot be covered)
            assert S == 1 and T > D and p['Z'] == -np.inf and not p['gamma'].any()
            assert not p['dur_counts'].any() and not p['entry_sum'].any()
            infeasible += 1
            continue
        t = ft.truth(eg, [le], factored_hub=False)
        n = S * D
        into = t['gamma0'] + t['xi_dense'].sum(0)
        # (what enters (j, r) from (j, r + 1) is the count-down, not a new segment)
        down = np.zeros(n)
        k = np.arange(n - 1)
        down[:-1] = np.where(k % D < D - 1, t['xi_dense'][k + 1, k], 0.)
        assert rel_err(p['gamma'], t['gamma'][0].reshape(T, S, D).sum(2)) <= PIN
        assert abs(p['Z'] - Z) <= PIN * (abs(Z) + 1)
        assert rel_err(p['dur_state'], (into - down).reshape(S, D)) <= PIN
    assert infeasible == (sum(T > D for T in ft.LENGTHS) if S == 1 else 0)


@pytest.mark.parametrize('S,D,T', [(2, 2, 4), (3, 3, 5), (3, 2, 3), (1, 3, 2), (2, 1, 3), (3, 5, 1),
                                   (1, 2, 5)])
@pytest.mark.parametrize('integer', [False, True])
def test_enumeration_of_every_segmentation(S, D, T, integer):
    g = ft.make_graph(S, ft.offsets(3, S), 7, 0, integer=integer)
    rng = np.random.RandomState(S * D + T)
    if integer:
        ld = rng.randint(-2, 1, size=(S + 2, D)).astype(np.float64)
        lw = rng.randint(0, 2, size=S + 2).astype(np.float64)
        l = rng.randint(-4, 1, size=(T, S)).astype(np.float64)
    else:
        ld, lw, l = rng.uniform(-3, 0, size=(S + 2, D)), rng.uniform(0, 1, size=S + 2), \
            rng.randn(T, S) * 3
    ld[0, 0] = -np.inf
    ids = rng.choice(S + 2, size=S, replace=False)
    p, b = ht.posteriors(g, ld, lw, l, ids), ht.brute_force(g, ld, lw, l, ids)
    path, score = ht.best_path(g, ld, lw, l, ids)
    if not np.isfinite(b['Z']):
        assert p['Z'] == -np.inf and score == -np.inf and (path == -1).all()
        return
    assert abs(p['Z'] - b['Z']) <= PIN * (abs(b['Z']) + 1)
    for k in ('gamma', 'dur_counts', 'entry_sum', 'gamma0_sum'):
        assert np.abs(p[k] - b[k]).max() <= PIN, k
    assert np.abs(p['gamma'].sum(1) - 1).max() <= PIN
    assert abs(score - b['best']) <= PIN * (abs(score) + 1)
    assert abs(ht.path_score(g, ld, lw, l, path, ids) - score) <= PIN * (abs(score) + 1)
    if integer:
        assert score == b['best']


def test_ties_go_to_the_shorter_duration_then_the_smaller_state():
    'All weights 0: every segmentation scores 0; the rule picks one.'
    S, T, D = 3, 5, 3
    g = dict(S=S, init=np.zeros(S), final=np.zeros(S), trans=np.zeros((S, S)), hub=None)
    path, score = ht.best_path(g, np.zeros((S, D)), None, np.zeros((T, S)))
    assert score == 0.
    # the last segment is of the smallest final state and as short as can be; before it the
    # smallest other state, again for one frame, and so on
    assert path.tolist() == [0, 1, 0, 1, 0]


# --- route and workspace -----------------------------------------------------------------------

def test_route_is_the_header_formula():
    lib = _hip.lib()
    seen = set()
    for S in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 120, 128, 129, 256, 257, 1024, 2048):
        for D in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128):
            for code, size in ((_hip.F32, 4), (_hip.F64, 8)):
                for ld in ((0, 0, 0), (1, 0, 0), (1, 2, 0), (1, 8, 4), (1, 8, 5)):
                    b = desc(S, 3, *ld)
                    got = lib.beer_hsmm_route(code, ctypes.byref(b), D)
                    assert got == ht.route_formula(S, D, size, *ld), (S, D, size, ld)
                    seen.add(got)
                    for nutt in (0, 3, 513):
                        b = desc(S, nutt, *ld)
                        assert lib.beer_hsmm_scratch_doubles(code, ctypes.byref(b), D) == \
                            ht.scratch_formula(S, D, size, nutt)
    assert {r & 0xF for r in seen} == set(range(7))
    assert {r & 0x300 for r in seen} == {0, ht.RING_LDS, ht.LOWDEG, ht.RING_LDS | ht.LOWDEG}
    assert all(r & 0xF000 == ht.BLOCK for r in seen)


def test_route_refusals():
    lib = _hip.lib()
    good = desc(8)
    assert lib.beer_hsmm_route(_hip.F64, ctypes.byref(good), 4) == ht.route_formula(8, 4, 8)
    for code, b, D in ((_hip.F64, good, 0), (_hip.F64, good, _hip.HSMM_MAX_DUR + 1),
                       (_hip.F64, good, -1), (2, good, 4), (_hip.F64, desc(0), 4),
                       (_hip.F64, desc(_hip.HSMM_MAX_STATES + 1), 4), (_hip.F64, desc(8, nutt=-1), 4)):
        assert lib.beer_hsmm_route(code, ctypes.byref(b), D) == _hip.EINVAL
        assert lib.beer_hsmm_scratch_doubles(code, ctypes.byref(b), D) == 0
    assert lib.beer_hsmm_route(_hip.F64, None, 4) == _hip.EINVAL
    assert ht.route_formula(8, 0, 8) == ht.EINVAL and ht.route_formula(2049, 4, 8) == ht.EINVAL
    # the entry points refuse before they launch (no device is touched)
    for name, tail in (('beer_hsmm_forward_backward', [None] * 6), ('beer_hsmm_viterbi', [None, None, None, 0])):
        fn = getattr(lib, name)
        assert fn(_hip.F64, ctypes.byref(good), None, None, None, 0, 8, *tail, None) == _hip.EINVAL
        assert fn(_hip.F64, ctypes.byref(good), None, None, None, 4, 8, *tail, None) == _hip.EINVAL
    assert _hip.HSMM_MAX_DUR >= 128 and _hip.HSMM_MAX_STATES >= 1024


def test_check_durations():
    ok = torch.zeros(5, 4, dtype=torch.float64)
    assert hk.check_durations(ok, 5) == 4
    low = ok.clone()
    low[:, 0] = -float('inf')
    assert hk.check_durations(low, 5, torch.zeros(5, dtype=torch.float64)) == 4
    nan, inf = ok.clone(), ok.clone()
    nan[1, 1], inf[2, 2] = float('nan'), float('inf')
    for bad, S_total, leave in ((ok.float(), 5, None), (ok[0], 5, None), (ok, 6, None),
                                (np.zeros((5, 4)), 5, None), (nan, 5, None), (inf, 5, None),
                                (torch.zeros(5, 0, dtype=torch.float64), 5, None),
                                (torch.zeros(5, _hip.HSMM_MAX_DUR + 1, dtype=torch.float64), 5, None),
                                (ok, 5, torch.zeros(4, dtype=torch.float64)),
                                (ok, 5, torch.zeros(5)),
                                (ok, 5, torch.full((5,), float('inf'), dtype=torch.float64))):
        with pytest.raises(ValueError, match='durations'):
            hk.check_durations(bad, S_total, leave)


# --- the model ---------------------------------------------------------------------------------
# (a PhoneLoop's constructor runs the Dirichlet kernel of its phone weights: models that need one
#  are in tests/test_gpu_durations.py; an HMM and the durations themselves are made on the host)

def _graph(loop=.6, n_units=4, n_states=3):
    graph, start, end, ems = decode_graph(n_units, 0, 2, 'diagonal', 1,
                                          loop_topology(loop, n_states), 3)
    return graph.compile(), start, end, ems


def _hmm(max_duration=6, **kw):
    cg, _, _, ems = _graph()
    return beer.HMM.create(cg, ems, max_duration=max_duration, **kw)


def test_state_durations_start_from_the_geometric_law():
    model = _hmm(6, durations_prior_strength=5.)
    dur = model.durations
    assert isinstance(dur, StateDurations) and dur.max_duration == 6 and len(dur) == 12
    law = .6 ** np.arange(6) * .4
    for dist in (dur.weights.prior, dur.weights.posterior):
        conc = dist.params.concentrations.double().numpy()
        assert conc.shape == (12, 6)
        np.testing.assert_allclose(conc, np.tile(5. * law / law.sum(), (12, 1)), rtol=1e-6)
    probs, means = dur.expected_durations()
    assert probs.dtype == torch.float64 and probs.shape == (12, 6)
    np.testing.assert_allclose(probs.numpy().sum(1), 1., rtol=1e-12)
    np.testing.assert_allclose(means.numpy(), ((law / law.sum()) * np.arange(1, 7)).sum(), rtol=1e-6)
    np.testing.assert_allclose(dur.self_loops.numpy(), .6, rtol=1e-6)
    # its own mean-field group, the model's last
    groups = model.mean_field_factorization()
    assert groups[-1] == [dur.weights] and all(dur.weights not in grp for grp in groups[:-1])
    assert model.transitions is None
    # 0 means what exists today
    plain = _hmm(0)
    assert plain.durations is None and len(plain.mean_field_factorization()) == len(groups) - 1


def test_state_durations_refuse_what_they_cannot_start_from():
    cg, _, _, _ = _graph(n_units=2)
    with pytest.raises(ValueError, match='BEER_HSMM_MAX_DUR'):
        StateDurations.create(cg, _hip.HSMM_MAX_DUR + 1)
    with pytest.raises(ValueError, match='BEER_HSMM_MAX_DUR'):
        StateDurations.create(cg, -1)
    # two states with different self-loops on one pdf id
    cg.trans_log_probs[1, 1] = np.log(.5)
    cg.pdf_id_mapping = [0, 1, 2, 3, 4, 1]
    with pytest.raises(ValueError, match='share pdf id 1'):
        StateDurations.create(cg, 4)
    # ... with the same self-loop they share one row
    cg.trans_log_probs[1, 1] = cg.trans_log_probs[5, 5]
    assert len(StateDurations.create(cg, 4)) == 5


def test_pickles():
    model = _hmm(5)
    again = pickle.loads(pickle.dumps(model))
    assert again.durations.max_duration == 5
    np.testing.assert_array_equal(again.durations.weights.posterior.params.concentrations.numpy(),
                                  model.durations.weights.posterior.params.concentrations.numpy())
    np.testing.assert_array_equal(again.durations.self_loops.numpy(),
                                  model.durations.self_loops.numpy())
    # a model pickled before durations existed has no such attribute
    old = _hmm(0)
    old.__dict__.pop('durations', None)
    old._modules.pop('durations', None)
    assert 'durations' not in old.__dict__ and 'durations' not in old._modules
    loaded = pickle.loads(pickle.dumps(old))
    assert loaded.durations is None and loaded.transitions is None
    assert len(loaded.mean_field_factorization()) == len(_hmm(0).mean_field_factorization())


def test_the_model_refuses_what_the_kernels_do_not_cover():
    model = _hmm(4)
    X = torch.zeros(5, 2)
    NIE = NotImplementedError
    cg, start, end, ems = _graph(n_units=3)
    with pytest.raises(NIE, match='train_transitions'):
        beer.PhoneLoop.create(cg, start, end, ems, max_duration=4, train_transitions=True)
    with pytest.raises(NIE, match='train_transitions'):
        beer.HMM.create(cg, ems, max_duration=4, train_transitions=True)
    with pytest.raises(NIE, match='BigramPhoneLoop'):
        beer.BigramPhoneLoop.create(cg, start, end, ems, max_duration=4)
    cg1, s1, e1, ems1 = _graph(n_units=3, n_states=1)
    with pytest.raises(NIE, match='start state is their end state'):
        beer.PhoneLoop.create(cg1, s1, e1, ems1, max_duration=4)
    stats = torch.zeros(5, 6)            # (refused before the statistics are looked at)
    for kw in (dict(viterbi=True), dict(state_path=torch.zeros(5, dtype=torch.int64)),
               dict(sample=True)):
        with pytest.raises(NIE, match='viterbi=, state_path= or sample='):
            model.expected_log_likelihood(stats, **kw)
    none = np.zeros(0, dtype=np.int32)
    for what, call in (('decode_nbest', lambda: model.decode_nbest(X, 2)),
                       ('sample_path', lambda: model.sample_path(X)),
                       ('arc_posteriors', lambda: model.arc_posteriors(X, none, none, 1)),
                       ('max_marginals', lambda: model.max_marginals(X)),
                       ('max_marginals', lambda: model.arc_max_marginals(X, none, none, 1)),
                       ('decode_nbest_batch', lambda: beer.decode_nbest_batch(model, [X], 2)),
                       ('sample_paths_batch', lambda: beer.sample_paths_batch(model, [X])),
                       ('unit_starts_batch', lambda: beer.unit_starts_batch(model, [X])),
                       ('unit_segments_batch', lambda: beer.unit_segments_batch(model, [X])),
                       ('unit_durations', lambda: beer.unit_durations_batch(model, [X], 4)),
                       ('VAE prior', lambda: beer.VAE(model, None, None)),
                       ('adapt', lambda: beer.adaptation.adapt(model, [X], [0], ['a']))):
        with pytest.raises(NIE, match='explicit durations') as err:
            call()
        assert what in str(err.value), (what, str(err.value))
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
    with pytest.raises(NIE, match='CapturedIteration'):
        beer.CapturedIteration(model, optim, X)


def _run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_the_command_line_refuses_with_the_message(tmp_path):
    t = str(tmp_path)
    graph, start, end, ems = decode_graph(3, 0, 2, 'diagonal', 1, loop_topology(.6), 3)
    with open(f'{t}/dg.pkl', 'wb') as f:
        pickle.dump((graph, start, end), f)
    with open(f'{t}/hmms.mdl', 'wb') as f:
        pickle.dump(({}, ems), f)
    args = cli_main.build_parser().parse_args(
        ['hmm', 'mkphoneloop', '--max-duration', '7', '--durations-prior-strength', '2', 'a', 'b', 'c'])
    assert args.max_duration == 7 and args.durations_prior_strength == 2.
    args = cli_main.build_parser().parse_args(['hmm', 'mkphoneloop', 'a', 'b', 'c'])
    assert args.max_duration == 0 and args.durations_prior_strength == 1.
    # the refused combinations: the message, not a traceback
    for argv, what in ((['hmm', 'mkphoneloop', '--weights-prior', 'dirichlet2', '--max-duration',
                         '5', f'{t}/dg.pkl', f'{t}/hmms.mdl', f'{t}/x.mdl'], 'BigramPhoneLoop'),
                       (['hmm', 'mkphoneloop', '--weights-prior', 'dirichlet', '--max-duration',
                         '5', '--train-transitions', f'{t}/dg.pkl', f'{t}/hmms.mdl', f'{t}/x.mdl'],
                        'train_transitions')):
        with pytest.raises(SystemExit) as err:
            _run(argv)
        assert 'explicit durations' in str(err.value) and what in str(err.value)
    with open(f'{t}/plain.mdl', 'wb') as f:
        pickle.dump(_hmm(0), f)
    with pytest.raises(SystemExit, match='no explicit durations'):
        _run(['hmm', 'durations', f'{t}/plain.mdl'])
