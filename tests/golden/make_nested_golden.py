'''Golden fixtures of NESTED mixtures (a mixture whose components are mixtures), produced
by running the reference implementation on the CPU (fp64):

  g21_nested_{full,diagonal,isotropic}.npz
      the model of examples/Nested Mixture Model.ipynb, Mixture(MixtureSet(4, NormalSet(12)))
      on 2-D data stored in the fixture: the initial model as the reference pickles it
      (`model`), 5 VB iterations -- every parameter's accumulated statistics (mean-field
      order), the posteriors' natural parameters after each, the ELBOs -- and the ELBO with
      `labels=` (outer components) of the initial model with its statistics.
  g21_nested_hmm.npz
      an HMM (3 states) whose emissions are MixtureSet(3, MixtureSet(6, NormalSet(18))),
      diagonal: the same records, plus `decode` after the iterations.
  g21_nested_vae.npz
      the nested mixture as the prior of a VAE, statistics in: the value of
      `expected_log_likelihood(stats)` for statistics that require a gradient, and whether
      the value has one (it does not: the inner log-normaliser is detached).
  g21_nested_pickles.npz
      a depth-3 nesting and a MixtureSet of MixtureSets as the reference pickles them.

Run from the repository root: python tests/golden/make_nested_golden.py
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

NITER = 5


def npy(t):
    return t.detach().cpu().numpy().copy()


def dumps(obj):
    return np.frombuffer(pickle.dumps(obj), dtype=np.uint8)


def notebook_data(seed=21):
    'The two clusters of the notebook (400 frames, D = 2).'
    rng = np.random.RandomState(seed)
    data1 = rng.multivariate_normal([-5, 5], .5 * np.array([[.75, .5], [.5, 2.]]), size=200)
    data2 = rng.multivariate_normal([5, 5], 2 * np.array([[2, -.5], [-.5, .75]]), size=200)
    data = np.vstack([data1, data2])
    rng.shuffle(data)
    return data


def notebook_model(data, cov_type, seed):
    torch.manual_seed(seed)
    mean = torch.from_numpy(data.mean(axis=0)).float()
    var = torch.from_numpy(np.var(data, axis=0)).float()
    ns = beer.NormalSet.create(mean, var, size=12, prior_strength=1., noise_std=1.,
                               cov_type=cov_type)
    return beer.Mixture.create(beer.MixtureSet.create(4, ns)).double()


def train(out, model, X, niter=NITER):
    params = [p for group in model.mean_field_factorization() for p in group]
    out['n_groups'] = np.asarray(len(model.mean_field_factorization()))
    out['group_sizes'] = np.asarray([len(g) for g in model.mean_field_factorization()])
    out['param_shapes'] = np.asarray([tuple(p.posterior.natural_parameters().shape) + (0,) *
                                      (2 - p.posterior.natural_parameters().dim())
                                      for p in params])
    optim = beer.VBConjugateOptimizer(model.mean_field_factorization(), 1.)
    elbos = []
    for it in range(niter):
        optim.init_step()
        elbo = beer.evidence_lower_bound(model, X, datasize=len(X))
        for k, p in enumerate(params):
            out[f'acc{it}.{k}'] = npy(elbo._acc_stats[p])
        elbo.backward()
        optim.step()
        elbos.append(float(elbo))
        for k, p in enumerate(params):
            out[f'it{it}.post{k}'] = npy(p.posterior.natural_parameters())
    out['elbos'] = np.asarray(elbos)


def g21_notebook():
    data = notebook_data()
    X = torch.from_numpy(data)
    labels = (data[:, 0] > 0).astype(np.int64) + 2 * (data[:, 1] > 5).astype(np.int64)
    for k, cov_type in enumerate(('full', 'diagonal', 'isotropic')):
        model = notebook_model(data, cov_type, 210 + k)
        out = {'X': data, 'cov_type': np.array(cov_type), 'model': dumps(model),
               'labels': labels}
        stats = model.sufficient_statistics(X)
        out['exp_llh'] = npy(model.expected_log_likelihood(stats))
        model.clear_cache()
        elbo = beer.evidence_lower_bound(model, X, datasize=len(X),
                                         labels=torch.from_numpy(labels))
        out['labels_elbo'] = np.asarray(float(elbo))
        params = [p for group in model.mean_field_factorization() for p in group]
        for j, p in enumerate(params):
            out[f'labels_acc.{j}'] = npy(elbo._acc_stats[p])
        model.clear_cache()
        train(out, model, X)
        mg.save(f'g21_nested_{cov_type}', out)


def g21_hmm():
    rng = np.random.RandomState(22)
    data, _ = mg.hmm_data(rng)
    X = torch.from_numpy(data)
    torch.manual_seed(220)
    ns = beer.NormalSet.create(torch.from_numpy(data.mean(0)).float(),
                               torch.from_numpy(np.var(data, axis=0)).float(),
                               size=3 * 2 * 3, prior_strength=1., noise_std=.5,
                               cov_type='diagonal')
    emissions = beer.MixtureSet.create(3, beer.MixtureSet.create(3 * 2, ns))
    model = beer.HMM.create(mg.notebook_graph(), emissions).double()
    out = {'X': data, 'model': dumps(model)}
    stats = model.sufficient_statistics(X)
    out['exp_llh'] = npy(model.expected_log_likelihood(stats))
    model.clear_cache()
    train(out, model, X)
    out['decode'] = npy(model.decode(X))
    mg.save('g21_nested_hmm', out)


def g21_vae():
    rng = np.random.RandomState(23)
    T, Dz = 60, 3
    torch.manual_seed(230)
    ns = beer.NormalSet.create(torch.zeros(Dz), torch.ones(Dz) * 2., size=6,
                               prior_strength=1., noise_std=1., cov_type='full')
    prior = beer.Mixture.create(beer.MixtureSet.create(2, ns)).double()
    z = torch.from_numpy(rng.randn(T, 2, Dz) * 1.5).requires_grad_(True)
    stats = prior.sufficient_statistics(z.view(-1, Dz)).reshape(T, 2, -1).mean(dim=1)
    exp_llh = prior.expected_log_likelihood(stats)
    out = {'z': npy(z), 'stats': npy(stats), 'model': dumps(prior),
           'exp_llh': npy(exp_llh), 'requires_grad': np.asarray(exp_llh.requires_grad)}
    params = [p for group in prior.mean_field_factorization() for p in group]
    acc = prior.accumulate(stats.detach())
    for k, p in enumerate(params):
        out[f'acc.{k}'] = npy(acc[p])
    mg.save('g21_nested_vae', out)


def g21_pickles():
    torch.manual_seed(240)
    ns = beer.NormalSet.create(torch.zeros(2), torch.ones(2), size=2 * 3 * 2,
                               prior_strength=1., noise_std=1., cov_type='diagonal')
    deep = beer.Mixture.create(beer.MixtureSet.create(2, beer.MixtureSet.create(6, ns)))
    sets = beer.MixtureSet.create(2, beer.MixtureSet.create(4, beer.NormalSet.create(
        torch.zeros(2), torch.ones(2), size=8, prior_strength=1., noise_std=1.,
        cov_type='full')))
    mg.save('g21_nested_pickles', {'depth3': dumps(deep.double()),
                                   'mixtureset2': dumps(sets.double())})


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    g21_notebook()
    g21_hmm()
    g21_vae()
    g21_pickles()
