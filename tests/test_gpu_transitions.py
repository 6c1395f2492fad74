'''Learned HMM transition probabilities on the GPU: the count kernels against a float64
numpy forward-backward, the unchanged outputs beside them, one VB step, recovery of known
self-loops, the captured iteration, the refused combinations and the command line.'''

import io
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from transitions_truth import (NON_SPEECH, SPEECH, category_counts, decode_graph,
                               forward_backward, loop_topology)

import beer_amd as beer
from beer_amd import _hip, hmm_kernels as hk
from beer_amd.cli import main as cli_main
from beer_amd.inference.batch import accumulate_elbo

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _model(dtype, cov='diagonal', seed=0, speech=SPEECH, n_speech=3, n_nonspeech=1, D=4,
           ncomp=2, learned=True, strength=1.):
    graph, start, end, ems = decode_graph(n_speech, n_nonspeech, D, cov, ncomp, speech, seed)
    model = beer.PhoneLoop.create(graph.compile(), start, end, ems, train_transitions=learned,
                                  transitions_prior_strength=strength)
    model = model.double() if dtype == torch.float64 else model.float()
    return model.to(DEV)


def _utterances(n, D, seed, dtype, lo=20, hi=300):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, hi, size=n).tolist()
    X = torch.from_numpy(rng.randn(sum(lens), D) * 1.5).to(DEV, dtype)
    return X, lens


def _truth(model, pc_all, lens, scale):
    'float64 numpy counts of every category from the per-pdf log-likelihoods.'
    g = model.graph
    ids = np.asarray(g.pdf_id_mapping)
    pc = pc_all.double().cpu().numpy()[:, ids] * scale
    off = np.concatenate([[0], np.cumsum(lens)])
    llhs = [pc[off[u]:off[u + 1]] for u in range(len(lens))]
    return category_counts(model.transitions, g.init_log_probs.double().cpu().numpy(),
                           g.final_log_probs.double().cpu().numpy(),
                           g.trans_log_probs.double().cpu().numpy(), llhs)


def _counts(model, tc, dtype):
    return model.transition_counts(model.graph.device_graph(dtype), tc).cpu().numpy()


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('cov', ['diagonal', 'isotropic', 'full'])
def test_counts_match_numpy_on_every_path(dtype, cov):
    model = _model(dtype, cov, seed=1)
    X, lens = _utterances(7, 4, 2, dtype)
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    scale = .8
    want = _truth(model, pc_all, lens, scale)
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    batch = hk.HmmBatch([model.graph], [0] * len(lens), lens, dtype)
    assert hk.fused_ok(batch)
    # fused
    _, _, _, tc = hk.posteriors_fused(batch, pc_all, scale, want_counts=True, want_transitions=True)
    got = _counts(model, tc, dtype)
    assert _rel(got, want) < tol, ('fused', _rel(got, want))
    # general (packed per-state arrays)
    pc = hk.gather(batch, pc_all, scale)
    tc = hk.forward_backward_counts(batch, pc)[4]
    assert tc[0] == 'arcs'
    assert _rel(_counts(model, tc, dtype), want) < tol
    # the log-space twin alone
    old = _hip.set_option('fb_log', 1)
    try:
        with hk.counting_log_space() as c:
            tc = hk.posteriors_fused(batch, pc_all, scale, want_counts=True,
                                     want_transitions=True)[3]
            tl = hk.forward_backward_counts(batch, pc)[4]
        assert int(c.count) == 2 * len(lens)
    finally:
        _hip.set_option('fb_log', old)
    assert _rel(_counts(model, tc, dtype), want) < tol
    assert _rel(_counts(model, tl, dtype), want) < tol
    _check_viterbi(model, batch, pc, lens, dtype)


def _check_viterbi(model, batch, pc, lens, dtype):
    'Viterbi: the hard counts of the decoded path.'
    path = hk.viterbi(batch, pc)
    _, xi, _ = hk.path_posteriors(batch, path, want_xi=True)
    tc = hk.path_counts(batch, path, xi)
    p = path.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(lens)])
    tr = model.transitions
    hard = np.zeros(len(tr.cat_src))
    pairs = {(i, j): c for c, (i, j) in enumerate(zip(tr.cat_src, tr.cat_dst)) if j >= 0}
    exits = tr.exits()
    for u in range(len(lens)):
        seg = p[off[u]:off[u + 1]]
        for a, b in zip(seg[:-1], seg[1:]):
            if (a, b) in pairs:
                hard[pairs[(a, b)]] += 1
            elif a in exits:
                hard[exits[a]] += 1
        if seg[-1] in exits:
            hard[exits[seg[-1]]] += 1
    np.testing.assert_array_equal(_counts(model, tc, dtype), hard)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('units', [(40, 1), (55, 2), (90, 1)])
def test_counts_on_larger_graphs(dtype, units):
    '''Two slots a lane (125 states), four (175 states, a hub of 57 phones) and the general
    path beyond the one-wave kernels (275 states, a hub of 91 phones): against numpy, the
    counts of the forward-backward calls, of Viterbi and of the batched E-step.'''
    model = _model(dtype, seed=21, n_speech=units[0], n_nonspeech=units[1], ncomp=1)
    X, lens = _utterances(6, 4, 22, dtype, lo=20, hi=120)
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    want = _truth(model, pc_all, lens, 1.)
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    batch = hk.HmmBatch([model.graph], [0] * len(lens), lens, dtype)
    wave = hk.fused_ok(batch)
    assert wave == (units[0] < 64)
    if wave:
        tc = hk.posteriors_fused(batch, pc_all, 1., want_counts=True, want_transitions=True)[3]
        assert _rel(_counts(model, tc, dtype), want) < tol
    pc = hk.gather(batch, pc_all, 1.)
    tc = hk.forward_backward_counts(batch, pc)[4]
    assert tc[0] == ('arcs' if wave else 'dense')
    assert _rel(_counts(model, tc, dtype), want) < tol
    _check_viterbi(model, batch, pc, lens, dtype)
    elbo = accumulate_elbo(model, (X, lens))
    stats = torch.cat([elbo._acc_stats[p].reshape(-1).cpu()
                       for p in model.transitions.parameters_of_groups()]).numpy()
    tr, first, want_stats = model.transitions, 0, want.copy()
    for n, states in zip(tr.arities, tr.group_states):
        block = want_stats[first:first + n * len(states)].reshape(len(states), n)
        block[:, -1] = block.sum(axis=1)
        first += n * len(states)
    assert _rel(stats, want_stats) < tol


def test_counts_leave_every_other_output_unchanged():
    for dtype in (torch.float64, torch.float32):
        model = _model(dtype, seed=3)
        X, lens = _utterances(9, 4, 4, dtype)
        pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
        batch = hk.HmmBatch([model.graph], [0] * len(lens), lens, dtype)
        llh_a = torch.zeros(len(lens), dtype=torch.float64, device=DEV)
        llh_b = torch.zeros_like(llh_a)
        sr_a, g0_a, flow_a = hk.posteriors_fused(batch, pc_all, .7, True, utt_llh=llh_a)
        sr_b, g0_b, flow_b, _ = hk.posteriors_fused(batch, pc_all, .7, True, utt_llh=llh_b,
                                                    want_transitions=True)
        # (posteriors: plain stores, bit for bit; the sums over utterances are fp64 atomics,
        #  whose order is not fixed from one launch to the next)
        assert torch.equal(sr_a, sr_b) and torch.equal(llh_a, llh_b)
        for a, b in ((g0_a, g0_b), (flow_a, flow_b)):
            torch.testing.assert_close(a, b, rtol=1e-14, atol=0)
        pc = hk.gather(batch, pc_all, .7)
        gamma_a, _, g0_a, _, flow_a = hk.forward_backward(batch, pc, want_xi=True)
        gamma_b, g0_b, flow_b, _, _ = hk.forward_backward_counts(batch, pc)
        assert torch.equal(gamma_a, gamma_b)
        for a, b in ((g0_a, g0_b), (flow_a, flow_b)):
            torch.testing.assert_close(a, b, rtol=1e-14, atol=0)
    # the E-step of a model with learned transitions: the same statistics and value terms
    # for everything else as the same model without them
    a, b = _model(torch.float64, seed=5), _model(torch.float64, seed=5, learned=False)
    b.graph.trans_log_probs.copy_(a.graph.trans_log_probs)
    b.graph.weights_rewritten()
    X, lens = _utterances(6, 4, 6, torch.float64)
    ea, eb = accumulate_elbo(a, (X, lens)), accumulate_elbo(b, (X, lens))
    # (the statistics are fp64 atomic sums: equal to their last bits, not bit for bit)
    for pa, pb in zip(list(a.bayesian_parameters())[:-2], b.bayesian_parameters()):
        torch.testing.assert_close(ea._acc_stats[pa], eb._acc_stats[pb], rtol=1e-12, atol=1e-12)
    kl_t = sum(float(p.kl_div_posterior_prior().sum()) for p in a.transitions.parameters_of_groups())
    assert float(ea.value) + len(lens) * kl_t == pytest.approx(float(eb.value), rel=1e-12)


def _np_dirichlet_kl(q, p):
    q, p = torch.as_tensor(q, dtype=torch.float64), torch.as_tensor(p, dtype=torch.float64)
    q0 = q.sum(-1, keepdim=True)
    return (torch.lgamma(q0.squeeze(-1)) - torch.lgamma(q).sum(-1) - torch.lgamma(p.sum(-1)) +
            torch.lgamma(p).sum(-1) + ((q - p) * (torch.digamma(q) - torch.digamma(q0))).sum(-1))


def test_one_vb_step_against_numpy():
    model = _model(torch.float64, seed=7, strength=2.)
    X, lens = _utterances(8, 4, 8, torch.float64)
    tr = model.transitions
    groups = model.mean_field_factorization()
    assert groups[-1] == tr.parameters_of_groups()
    optim = beer.VBConjugateOptimizer(groups, lrate=1.)
    # the groups are updated in turn: the emissions and phone weights first
    for _ in range(len(groups) - 1):
        optim.init_step()
        elbo = accumulate_elbo(model, (X, lens))
        elbo.backward()
        optim.step()
    pc_all = model._emissions().expected_log_likelihood(model.sufficient_statistics(X))
    want = _truth(model, pc_all, lens, 1.)
    prior = torch.cat([p.prior.params.concentrations.reshape(-1).cpu()
                       for p in tr.parameters_of_groups()]).numpy()
    optim.init_step()
    elbo = accumulate_elbo(model, (X, lens))
    # (the Dirichlet rows' statistics: the counts with the last column replaced by the row
    # sum, dirichlet.py:18-21)
    stats = torch.cat([elbo._acc_stats[p].reshape(-1).cpu()
                       for p in tr.parameters_of_groups()]).numpy()
    want_stats, first = want.copy(), 0
    for n, states in zip(tr.arities, tr.group_states):
        block = want_stats[first:first + n * len(states)].reshape(len(states), n)
        block[:, -1] = block.sum(axis=1)
        first += n * len(states)
    assert _rel(stats, want_stats) < 1e-10
    elbo.backward()
    optim.step()
    post = torch.cat([p.posterior.params.concentrations.reshape(-1).cpu()
                      for p in tr.parameters_of_groups()]).numpy()
    assert _rel(post, prior + want) < 1e-10
    # the graph now holds E[ln a] of the new posterior
    logp = tr.log_probs().cpu()
    cats, src, dst = tr.intra()
    np.testing.assert_array_equal(model.graph.trans_log_probs[src, dst].cpu().numpy(),
                                  logp[cats].numpy())
    # the ELBO includes the transitions' KL
    kl_np = sum(float(_np_dirichlet_kl(p.posterior.params.concentrations.cpu(),
                                       p.prior.params.concentrations.cpu()).sum())
                for p in tr.parameters_of_groups())
    assert kl_np > 0
    others = sum(float(p.kl_div_posterior_prior().sum()) for p in model.bayesian_parameters()
                 if p not in tr.parameters_of_groups())
    total = float(model.kl_div_posterior_prior())
    assert abs(total - (others + kl_np)) <= 1e-9 * abs(total)


def _sample(trans, init, means, lens, rng):
    S = trans.shape[0]
    P = np.exp(trans)
    P = P / P.sum(1, keepdims=True)
    p0 = np.exp(init) / np.exp(init).sum()
    out = []
    for T in lens:
        s = rng.choice(S, p=p0)
        states = [s]
        for _ in range(T - 1):
            s = rng.choice(S, p=P[s])
            states.append(s)
        out.append(means[np.asarray(states)] + rng.randn(T, means.shape[1]))
    return np.concatenate(out)


@pytest.mark.parametrize('learned', [True, False])
def test_recovery_of_known_self_loops(learned):
    D, P = 6, 4
    rng = np.random.RandomState(11)
    true_g, _, _, _ = decode_graph(P, 0, D, 'diagonal', 1, loop_topology(.9), seed=0)
    tg = true_g.compile()
    model = _model(torch.float64, 'diagonal', seed=0, speech=loop_topology(.5), n_speech=P,
                   n_nonspeech=0, D=D, ncomp=1, learned=learned)
    S = model.graph.n_states
    ids = np.asarray(model.graph.pdf_id_mapping)
    means = rng.randn(S, D) * 4
    lens = rng.randint(150, 400, size=24).tolist()
    Xn = _sample(tg.trans_log_probs.double().numpy(), tg.init_log_probs.double().numpy(),
                 means, lens, rng)
    X = torch.from_numpy(Xn).to(DEV)
    # emissions started at the truth (state s emits pdf ids[s])
    ns = model._emissions().modelsets[0].normalset
    mean = ns.means_precisions.posterior.params.mean
    pdf_means = np.zeros_like(means)
    pdf_means[ids] = means
    mean.copy_(torch.from_numpy(pdf_means).to(mean))
    before = model.graph.trans_log_probs.clone()
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
    for _ in range(10):
        optim.init_step()
        elbo = accumulate_elbo(model, (X, lens))
        elbo.backward()
        optim.step()
    loops = torch.diagonal(model.graph.trans_log_probs).exp().cpu().numpy()
    if not learned:
        # fixed transitions: the units' arcs are exactly what they were
        inner = torch.isfinite(before) & ~torch.zeros_like(before, dtype=torch.bool)
        ends = list(model.end_pdf.values())
        keep = inner.clone()
        keep[torch.as_tensor(ends)[:, None], torch.as_tensor(list(model.start_pdf.values()))[None, :]] = False
        assert torch.equal(model.graph.trans_log_probs[keep], before[keep])
        np.testing.assert_allclose(loops, .5, rtol=1e-6)
        return
    probs, exits = model.expected_transition_probs()
    loop = torch.diagonal(probs).numpy()
    assert np.abs(loop - .9).max() < .03, loop
    ends = list(model.end_pdf.values())
    assert np.abs(exits[ends].numpy() - .1).max() < .03


def test_captured_iteration_replays_the_eager_one():
    from beer_amd.inference.captured import CapturedIteration
    X, lens = _utterances(10, 4, 12, torch.float64)
    values = []
    for captured in (False, True):
        model = _model(torch.float64, seed=13)
        optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), lrate=1.)
        if captured:
            it = CapturedIteration(model, optim, (X, lens))
            run = [float(it()) for _ in range(8)]
            assert it.mode == 'replayed'
        else:
            run = []
            for _ in range(8):
                optim.init_step()
                elbo = accumulate_elbo(model, (X, lens))
                run.append(float(elbo.value))
                elbo.backward()
                optim.step()
        conc = torch.cat([p.posterior.params.concentrations.reshape(-1)
                          for p in model.transitions.parameters_of_groups()])
        values.append((np.asarray(run), conc.cpu().numpy(),
                       model.graph.trans_log_probs.cpu().numpy()))
    (ve, ce, te), (vc, cc, tc) = values
    assert np.abs(vc - ve).max() <= 1e-12 * np.abs(ve).max()
    assert np.abs(cc - ce).max() <= 1e-12 * np.abs(ce).max()
    fin = np.isfinite(te)
    np.testing.assert_array_equal(fin, np.isfinite(tc))
    assert np.abs(tc[fin] - te[fin]).max() <= 1e-12 * np.abs(te[fin]).max()


def test_out_of_scope_combinations_raise():
    model = _model(torch.float64, seed=14)
    X, lens = _utterances(2, 4, 15, torch.float64)
    with pytest.raises(ValueError):
        accumulate_elbo(model, (X, lens), inference_graphs=[model.graph, model.graph])
    with pytest.raises(ValueError):
        beer.evidence_lower_bound(model, X[:lens[0]], inference_graph=model.graph)
    from beer_amd.cli import hmm as hmm_cmds
    with pytest.raises(ValueError):
        hmm_cmds.bigram_loop(model, 'dirichlet2')
    # the per-utterance path counts as the batched one does
    elbo = beer.evidence_lower_bound(model, X[:lens[0]], datasize=100)
    batched = accumulate_elbo(model, (X[:lens[0]], lens[:1]), datasize=100)
    for p in model.transitions.parameters_of_groups():
        np.testing.assert_allclose(elbo._acc_stats[p].cpu().numpy(),
                                   batched._acc_stats[p].cpu().numpy(), rtol=1e-10, atol=1e-12)


HMM_CONF = """
- group_name: sil
  n_normal_per_state: 3
  prior_strength: 1.
  noise_std: 0.5
  cov_type: diagonal
  shared_cov: no
  topology:
  - {start_id: 0, end_id: 1, trans_prob: 1.0}
  - {start_id: 1, end_id: 1, trans_prob: 0.5}
  - {start_id: 1, end_id: 2, trans_prob: 0.5}
  - {start_id: 2, end_id: 2, trans_prob: 0.5}
  - {start_id: 2, end_id: 1, trans_prob: 0.25}
  - {start_id: 2, end_id: 3, trans_prob: 0.25}
- group_name: speech
  n_normal_per_state: 4
  prior_strength: 1.
  noise_std: 0.5
  cov_type: diagonal
  shared_cov: no
  topology:
  - {start_id: 0, end_id: 1, trans_prob: 1.0}
  - {start_id: 1, end_id: 1, trans_prob: 0.75}
  - {start_id: 1, end_id: 2, trans_prob: 0.25}
  - {start_id: 2, end_id: 2, trans_prob: 0.75}
  - {start_id: 2, end_id: 3, trans_prob: 0.25}
  - {start_id: 3, end_id: 3, trans_prob: 0.75}
  - {start_id: 3, end_id: 4, trans_prob: 0.25}
"""


def _run(argv, stdin=''):
    old_in, old_out = sys.stdin, sys.stdout
    sys.stdin, sys.stdout = io.StringIO(stdin), io.StringIO()
    try:
        cli_main.main(argv)
        return sys.stdout.getvalue()
    finally:
        sys.stdin, sys.stdout = old_in, old_out


def test_cli_train_transitions_on_the_reference_corpus(tmp_path):
    t = str(tmp_path)
    (tmp_path / 'hmm.yml').write_text(HMM_CONF)
    (tmp_path / 'units').write_text('sil sil\na speech\nb speech\nc speech\nd speech\n')
    _run(['dataset', 'create', t, os.path.join(GOLDEN, 'ref_feats.npz'), f'{t}/ds.pkl'])
    _run(['-s', '1', 'hmm', 'mkphones', '-d', f'{t}/ds.pkl', f'{t}/hmm.yml', f'{t}/units',
          f'{t}/hmms.mdl'])
    _run(['hmm', 'mkphoneloopgraph', '--start-end-group', 'sil', f'{t}/units', f'{t}/g.pkl'])
    _run(['hmm', 'mkdecodegraph', f'{t}/g.pkl', f'{t}/hmms.mdl', f'{t}/dg.pkl'])
    _run(['hmm', 'mkphoneloop', '--train-transitions', '--transitions-prior-strength', '2',
          '--weights-prior', 'dirichlet', f'{t}/dg.pkl', f'{t}/hmms.mdl', f'{t}/0.mdl'])
    _run(['hmm', 'accumulate', f'{t}/0.mdl', f'{t}/ds.pkl', f'{t}/e.pkl'], stdin='utt0\nutt1\nutt2\n')
    # two updates: the transitions are the model's last mean-field group
    _run(['hmm', 'update', '-o', f'{t}/optim.pth', f'{t}/0.mdl', f'{t}/1.mdl'], stdin=f'{t}/e.pkl\n')
    _run(['hmm', 'accumulate', f'{t}/1.mdl', f'{t}/ds.pkl', f'{t}/e1.pkl'], stdin='utt0\nutt1\nutt2\n')
    _run(['hmm', 'update', '-o', f'{t}/optim.pth', f'{t}/1.mdl', f'{t}/2.mdl'], stdin=f'{t}/e1.pkl\n')
    m0 = pickle.load(open(f'{t}/0.mdl', 'rb'))
    m2 = pickle.load(open(f'{t}/2.mdl', 'rb'))
    assert m0.transitions is not None and m2.transitions is not None
    moved = 0.
    for a, b in zip(m0.transitions.parameters_of_groups(), m2.transitions.parameters_of_groups()):
        np.testing.assert_array_equal(a.prior.params.concentrations.numpy(),
                                      b.prior.params.concentrations.numpy())
        moved += float((b.posterior.params.concentrations - a.posterior.params.concentrations)
                       .abs().sum())
    assert moved > 1.
    out = _run(['hmm', 'decode', f'{t}/2.mdl', f'{t}/ds.pkl'])
    assert sorted(l.split()[0] for l in out.strip().split('\n')) == ['utt0', 'utt1', 'utt2']
