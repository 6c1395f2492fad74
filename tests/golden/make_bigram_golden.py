'''Golden fixtures of the BIGRAM phone loop, produced by running the reference
implementation on the CPU (fp64):

  g20_bigram_{dirichlet2,hierarchical_dirichlet_process}{,_p24}.npz   (P = 5 and P = 24)
      the initial model as the reference pickles it (`model`), the data, the first
      E-step (exp_llh, gamma, the time-summed xi of the end -> start block), then 3 VB
      iterations: every parameter's accumulated statistics (mean-field order), the
      posteriors' parameters and trans_log_probs after each, the ELBOs, decode.
  g20_bigram_pickles.npz
      reference pickles written by `mkphoneloop --weights-prior dirichlet2 |
      hierarchical_dirichlet_process` and `mkphoneloopbigram` (both priors), in process.

Run from the repository root: python tests/golden/make_bigram_golden.py
'''

import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference on the path)
import beer  # noqa: E402
from beer.cli.subcommands.hmm import mkphoneloop, mkphoneloopbigram  # noqa: E402

PRIORS = ('dirichlet2', 'hierarchical_dirichlet_process')


def npy(t):
    return t.detach().cpu().numpy().copy()          # (a snapshot: .numpy() shares memory)


def dumps(obj):
    return np.frombuffer(pickle.dumps(obj), dtype=np.uint8)


def unigram(D, seed, P=5):
    'A unigram loop of P phones with stick-breaking weights (the HDP root).'
    units = mg.UNITS
    if P != len(units):              # (make_golden's five phones, or sil + P - 1 speech units)
        mg.UNITS = [('sil', 'sil')] + [(f'p{i}', 'speech') for i in range(1, P)]
    try:
        ploop, _, start_pdf, end_pdf = mg.build_phoneloop('dirichlet_process', D, 'diagonal',
                                                          seed, torch.float64)
    finally:
        mg.UNITS = units
    return ploop, start_pdf, end_pdf


def bigram(prior, ploop):
    size = len(ploop.start_pdf)
    cset = mkphoneloopbigram.priors[prior](size, ploop.categorical)
    return beer.BigramPhoneLoop.create(ploop.graph, ploop.start_pdf, ploop.end_pdf,
                                       ploop.modelset, cset)


def posteriors(model):
    return [npy(p.posterior.natural_parameters())
            for group in model.mean_field_factorization() for p in group]


def g20(P=5, suffix=''):
    D = 4
    rng = np.random.RandomState(20)
    Xn = mg.ploop_data(rng, 150, D)
    X = torch.from_numpy(Xn)
    for prior in PRIORS:
        uni, _, _ = unigram(D, 60, P)
        model = bigram(prior, uni)
        out = {'X': Xn, 'prior_kind': np.array(prior), 'model': dumps(model),
               'start_idxs': np.asarray(list(model.start_pdf.values())),
               'end_idxs': np.asarray(list(model.end_pdf.values()))}
        ends, starts = out['end_idxs'], out['start_idxs']
        stats = model.sufficient_statistics(X)
        out['exp_llh'] = npy(model.expected_log_likelihood(stats))
        out['gamma'] = npy(model.cache['resps'])
        out['xi_block'] = npy(model.cache['trans_resps'].sum(0))[ends][:, starts]
        model.clear_cache()
        params = [p for group in model.mean_field_factorization() for p in group]
        optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
        elbos = []
        for it in range(3):
            optim.init_step()
            elbo = beer.evidence_lower_bound(model, X, datasize=len(X))
            for k, p in enumerate(params):
                out[f'acc{it}.{k}'] = npy(elbo._acc_stats[p])
            elbo.backward()
            optim.step()
            elbos.append(float(elbo))
            for k, post in enumerate(posteriors(model)):
                out[f'it{it}.post{k}'] = post
            out[f'it{it}.trans'] = npy(model.graph.trans_log_probs)
        out['elbos'] = np.asarray(elbos)
        out['decode'] = npy(model.decode(X))
        mg.save(f'g20_bigram_{prior}{suffix}', out)


def g20_pickles():
    'What the command line writes: mkphoneloop with the bigram priors, mkphoneloopbigram.'
    uni, start_pdf, end_pdf = unigram(3, 61)
    out = {}
    size = len(start_pdf)
    for prior in PRIORS:
        cat = mkphoneloop.priors[prior](size, size / 2)
        model = beer.BigramPhoneLoop.create(uni.graph, start_pdf, end_pdf, uni.modelset, cat)
        out[f'mkphoneloop.{prior}'] = dumps(model)
        out[f'mkphoneloopbigram.{prior}'] = dumps(bigram(prior, uni))
    out['unigram'] = dumps(uni)
    mg.save('g20_bigram_pickles', out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    g20()
    g20(24, '_p24')
    g20_pickles()
