"""The posterior-predictive (Student-t) kernels (csrc/predictive.hip, the `beer_*_predictive_table`
kernels of csrc/expfam.hip) and the model layers on top, entry by entry against the longdouble
truth of tests/predictive_truth.py.

Tolerances, `tol` = 1e-10 (float64) / 1e-5 (float32), the TOL of tests/test_gpu_log_evidence.py:
 * component entries: |got - truth| <= tol (1 + |c_k| + |truth_tk - c_k|), the magnitudes of the
   two terms whose difference the value is (the construction of evidence_truth.total_bound);
 * state entries: the same with the largest such magnitude among the state's components whose
   term lies within 40 nats of the state's largest.
Every entry of every case is compared.

The kernels have ONE form (no route function); the table below walks the shapes at which its
loops change: D in {1, 3, 40, 65} (diagonal, isotropic: whole and partial groups of folded
dimensions) and {1, 3, 13, 40} (full: partial and whole blocks of rows), T in {1, 63, 64, 65, 257}
(partial, whole and several frame tiles), (S, G) in {(1, 1), (7, 1), (1, 5), (3, 4), (2, 257)}
(several states per workgroup, a partial chunk, many chunks per state), the posterior regimes
near the prior (a = 1, kappa = .1, nu = D + .5), trained (5e3, 1e6) and mixed, weight rows that are
uniform, that span concentrations 1e-3 .. 1e7, and no weights.  Every value of every axis occurs
for every covariance type and dtype; the axes are crossed by the table, not by a full product.

Frames: drawn from the components; frame 0 sits exactly on the mean of component 0 (its value is
bit-equal to the table's c_0); frames 1 and 2 are outliers at 1e3 sigma in one / in all
dimensions."""

import functools
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import expfam_truth as et
import predictive_truth as pt

pytestmark = pytest.mark.gpu

import beer_amd as beer                                             # noqa: E402
from beer_amd import hmm_kernels as hk, kernels                     # noqa: E402
from beer_amd.cli import hmm as hmm_cmds                            # noqa: E402
from beer_amd.inference.batch import _groups                        # noqa: E402
from gpu_helpers import npy, tt                                     # noqa: E402

NP = {torch.float64: np.float64, torch.float32: np.float32}
TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
FAMILY = {'full': 'NormalWishart', 'diagonal': 'NormalGamma', 'isotropic': 'IsotropicNormalGamma'}

Case = namedtuple('Case', 'D T S G regime weights')
# (the last dimension of each row: diagonal / isotropic, full)
_ROWS = [((1, 1), 1, 1, 1, 'prior', None),
         ((3, 3), 63, 7, 1, 'trained5e3', 'uniform'),
         ((40, 13), 64, 1, 5, 'trained1e6', 'wide'),
         ((65, 40), 65, 3, 4, 'mixed', 'wide'),
         ((40, 13), 257, 2, 257, 'mixed', 'wide'),
         ((65, 40), 257, 3, 4, 'prior', 'uniform'),
         ((3, 3), 65, 2, 257, 'trained1e6', None)]
CASES = [(cov, Case(dims[cov == 'full'], *rest)) for cov in pt.COV_TYPES for dims, *rest in _ROWS]
STRENGTH = {'prior': [None], 'trained5e3': [5e3], 'trained1e6': [1e6], 'mixed': [None, 5e3, 1e6]}


def case_id(v):
    if isinstance(v, tuple) and not isinstance(v, Case):
        cov, c = v
        return f'{cov}-D{c.D}-T{c.T}-S{c.S}-G{c.G}-{c.regime}-{c.weights}'
    return None


def test_the_table_reaches_every_value_of_every_axis():
    for cov in pt.COV_TYPES:
        mine = [c for v, c in CASES if v == cov]
        assert {c.D for c in mine} == ({1, 3, 13, 40} if cov == 'full' else {1, 3, 40, 65})
        assert {c.T for c in mine} == {1, 63, 64, 65, 257}
        assert {(c.S, c.G) for c in mine} == {(1, 1), (7, 1), (1, 5), (3, 4), (2, 257)}
        assert {c.regime for c in mine} == set(STRENGTH)
        assert {c.weights for c in mine} == {None, 'uniform', 'wide'}


def make_params(cov, K, D, regime, rng, np_dtype):
    '''Standard parameters of K pdfs rounded to `np_dtype`, and the standard deviations [K, D] /
    covariance factors [K, D, D] the frames are drawn with.  Near the prior: a = 1, kappa = .1,
    nu = D + .5; trained: a = kappa = nu = 5e3 or 1e6, rates and scale matrices scaled so that the
    variance stays of order one.'''
    cycle = STRENGTH[regime]
    s = [cycle[k % len(cycle)] for k in range(K)]
    col = lambda near, far: np.array([[near if v is None else far(v)] for v in s])   # noqa: E731
    kappa = col(.1, float)
    mean = 3 * rng.standard_normal((K, D))
    if cov == 'full':
        dof = col(D + .5, float)
        sigma = et.generic_matrices(rng, D, .5, K)
        W = np.linalg.inv(sigma) / dof[:, :, None]
        p = (mean, kappa, .5 * (W + W.transpose(0, 2, 1)), dof)
        draw = np.linalg.cholesky(sigma)
    else:
        a = col(1., float)
        var = rng.uniform(.5, 2, (K, 1 if cov == 'isotropic' else D))
        p = (mean, kappa, a, a * var)
        draw = np.sqrt(np.broadcast_to(var, (K, D)))
    return tuple(np.ascontiguousarray(t.astype(np_dtype)) for t in p), draw


def make_frames(p, draw, T, rng, np_dtype):
    mean = p[0].astype(np.float64)
    K, D = mean.shape
    ks = rng.integers(0, K, T)
    noise = rng.standard_normal((T, D))
    if draw.ndim == 3:
        X = mean[ks] + np.einsum('tij,tj->ti', draw[ks], noise)
        sd = np.sqrt(np.einsum('kij,kij->ki', draw, draw))
    else:
        X, sd = mean[ks] + draw[ks] * noise, draw
    X[0] = mean[0]                                       # exactly on a mean
    if T >= 3:
        X[1] = mean[ks[1]]
        X[1, 0] += 1e3 * sd[ks[1], 0]                    # an outlier in one dimension ...
        X[2] = mean[ks[2]] + 1e3 * sd[ks[2]]             # ... and in all of them
    return np.ascontiguousarray(X.astype(np_dtype))


def make_weights(kind, S, G, rng, np_dtype):
    'ln E[pi] [S, G] rounded to `np_dtype` (what the kernel is given), or None.'
    if kind is None:
        return None
    if kind == 'uniform':
        conc = np.ones((S, G))
    else:
        conc = np.stack([rng.permutation(np.logspace(-3, 7, G)) for _ in range(S)])
    return np.asarray(pt.log_mean_weights(conc), dtype=np.float64).astype(np_dtype)


@functools.lru_cache(maxsize=None)
def built(cov, case, dtype):
    'Parameters, frames, weights (in `dtype`) and their longdouble truth, once per case.'
    np_dtype = NP[dtype]
    rng = np.random.default_rng(zlib.crc32(repr((cov, tuple(case), str(dtype))).encode()))
    K = case.S * case.G
    p, draw = make_params(cov, K, case.D, case.regime, rng, np_dtype)
    X = make_frames(p, draw, case.T, rng, np_dtype)
    lmw = make_weights(case.weights, case.S, case.G, rng, np_dtype)
    l, c = pt.predictive(cov, X, p)
    return dict(p=p, X=X, lmw=lmw, l=l, c=c, state=pt.mixture(l, lmw, case.S, case.G))


def table_of(cov, p):
    dist = getattr(beer.dists, FAMILY[cov]).from_std_parameters(*[tt(a) for a in p])
    return dist, dist.predictive_table()


def hold(got, truth, bound, what):
    got = et.ld(npy(got))
    assert got.shape == truth.shape, what
    assert not np.isnan(np.asarray(got, dtype=np.float64)).any(), f'{what}: NaN'
    ratio = float((np.abs(got - truth) / bound).max())
    print(f'{what}: largest error / bound = {ratio:.3e}')
    assert ratio <= 1., f'{what}: error {ratio:.3e} x its bound'


@DTYPES
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_kernels_against_the_truth(case, dtype):
    cov, c = case
    b = built(cov, c, dtype)
    tol = TOL[dtype]
    _, table = table_of(cov, b['p'])
    assert table.dtype == dtype and tuple(table.shape) == (c.S * c.G, beer.FrameStats(
        tt(b['X']), cov).shape[1])
    # the table's own constants
    tab = et.ld(npy(table))
    assert (np.abs(tab[:, -2] - b['c']) <= tol * (1 + np.abs(b['c']))).all(), 'c_k'
    X = tt(b['X'])
    l = kernels.predictive_llh(X, table, cov)
    assert l.dtype == dtype and tuple(l.shape) == (c.T, c.S * c.G)
    hold(l, b['l'], pt.component_bound(b['l'], b['c'], tol), f'{cov} {tuple(c)} components')
    # a frame equal to a mean: the table's c_k, bit for bit
    assert l[0, 0].item() == table[0, -2].item()
    stats = beer.FrameStats(X, cov)
    lmw = None if b['lmw'] is None else tt(b['lmw'])
    ln = kernels.mixtureset_predictive(stats, table, lmw, c.S, c.G, cov)
    assert ln.dtype == dtype and tuple(ln.shape) == (c.T, c.S)
    hold(ln, b['state'], pt.state_bound(b['l'], b['c'], b['lmw'], c.S, c.G, tol),
         f'{cov} {tuple(c)} states')
    # the lazy statistics and the raw frames are the same call
    assert torch.equal(kernels.predictive_llh(stats, table, cov), l)


@DTYPES
def test_a_group_of_dimensions_that_overflows_is_redone_one_by_one(dtype):
    '''An outlier at 1e6 (float32) / 1e40 (float64) sigma in all dimensions near the prior: the
    product of a group of (1 + u_d) exceeds the format, every u_d alone does not (D = 9: a whole
    group and a group of one).'''
    rng = np.random.default_rng(5)
    p, draw = make_params('diagonal', 3, 9, 'prior', rng, NP[dtype])
    far = 1e6 if dtype == torch.float32 else 1e40
    X = np.stack([p[0][1].astype(np.float64) + far * draw[1], p[0][2].astype(np.float64)])
    X = X.astype(NP[dtype])
    l, c = pt.predictive('diagonal', X, p)
    _, table = table_of('diagonal', p)
    got = kernels.predictive_llh(tt(X), table, 'diagonal')
    assert torch.isfinite(got).all()
    hold(got, l, pt.component_bound(l, c, TOL[dtype]), 'overflowing group')


def test_the_table_is_memoised_per_parameter_version():
    b = built('diagonal', Case(3, 63, 7, 1, 'trained5e3', 'uniform'), torch.float64)
    dist, table = table_of('diagonal', b['p'])
    assert dist.predictive_table() is table
    dist.params.shape.mul_(2.)
    again = dist.predictive_table()
    assert again is not table and not torch.equal(again[:, -1], table[:, -1])


def test_what_the_library_refuses():
    table = torch.zeros(2, 2 * 3 + 2, dtype=torch.float64, device='cuda')
    X = torch.zeros(4, 3, dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError):
        kernels.mixtureset_predictive(beer.FrameStats(X, 'diagonal'), table, None, 3, 1, 'diagonal')
    with pytest.raises(NotImplementedError):
        kernels.predictive_llh(beer.FrameStats(X, 'diagonal') * .5, table, 'diagonal')
    empty = kernels.predictive_llh(X[:0], table, 'diagonal')
    assert tuple(empty.shape) == (0, 2)
    # a frame tile that cannot fit a CU's LDS
    big = torch.zeros(2, 2 * 1000 + 2, dtype=torch.float64, device='cuda')
    with pytest.raises(beer._hip.HipInvalid):
        kernels.predictive_llh(torch.zeros(4, 1000, dtype=torch.float64, device='cuda'), big,
                               'diagonal')


# ---- the model level -------------------------------------------------------------------------------

def dirichlet(conc):
    return beer.ConjugateBayesianParameter(
        beer.dists.Dirichlet.from_std_parameters(tt(np.ones_like(conc))),
        beer.dists.Dirichlet.from_std_parameters(tt(conc)))


def normalset(cov, p):
    family = getattr(beer.dists, FAMILY[cov])
    make = lambda: family.from_std_parameters(*[tt(a) for a in p])       # noqa: E731
    return beer.NormalSet(beer.ConjugateBayesianParameter(make(), make()))


def std_params(ns):
    post = ns.means_precisions.posterior
    return tuple(npy(getattr(post.params, n)) for n in post._std_params_def)


def group_truth(grp, X):
    '(state values [T, S], their bound at tol = 1) of one emission group, from its own parameters.'
    S, G = _groups(grp)[0][1:]
    ns = grp.normalset if isinstance(grp, beer.MixtureSet) else grp
    l, c = pt.predictive(ns.cov_type, X, std_params(ns))
    lmw, level = None, grp
    while isinstance(level, beer.MixtureSet):               # ln E[pi] summed down to the leaves
        own = pt.log_mean_weights(npy(level.categoricalset.weights.posterior.params.concentrations))
        lmw = own if lmw is None else (lmw[:, :, None] + own.reshape(lmw.shape + (-1,))).reshape(
            lmw.shape[0], -1)
        level = level.modelset
    return pt.mixture(l, lmw, S, G), pt.state_bound(l, c, lmw, S, G, 1.)


def emissions_truth(emissions, X):
    parts = [group_truth(grp, X) for grp, _, _ in _groups(emissions)]
    return np.concatenate([v for v, _ in parts], -1), np.concatenate([b for _, b in parts], -1)


@pytest.mark.parametrize('cov', pt.COV_TYPES)
def test_models_predictive_log_likelihood(cov):
    tol, rng = TOL[torch.float64], np.random.default_rng(11)
    D, T = 5, 70
    p, draw = make_params(cov, 12, D, 'mixed', rng, np.float64)
    X = make_frames(p, draw, T, rng, np.float64)
    ns = normalset(cov, p)
    l, c = pt.predictive(cov, X, p)
    hold(ns.predictive_log_likelihood(tt(X)), l, pt.component_bound(l, c, tol), 'NormalSet')
    one = ns[3].predictive_log_likelihood(tt(X))
    assert tuple(one.shape) == (T,)
    hold(one, l[:, 3], pt.component_bound(l, c, tol)[:, 3], 'Normal')
    conc = rng.uniform(.2, 30, 12)
    mix = beer.Mixture(beer.Categorical(dirichlet(conc)), ns)
    lmw = pt.log_mean_weights(conc[None])
    hold(mix.predictive_log_likelihood(tt(X)), pt.mixture(l, lmw, 1, 12)[:, 0],
         pt.state_bound(l, c, lmw, 1, 12, tol)[:, 0], 'Mixture')
    mset = beer.MixtureSet(beer.CategoricalSet(dirichlet(rng.uniform(.2, 30, (4, 3)))), ns)
    want, bound = group_truth(mset, X)
    got = mset.predictive_log_likelihood(mset.sufficient_statistics(tt(X)))
    hold(got, want, tol * bound, 'MixtureSet')
    # two levels: 2 mixtures of 2 mixtures of 3 Gaussians
    nested = beer.MixtureSet(beer.CategoricalSet(dirichlet(rng.uniform(.2, 30, (2, 2)))), mset)
    want, bound = group_truth(nested, X)
    assert want.shape == (T, 2)
    hold(nested.predictive_log_likelihood(tt(X)), want, tol * bound, 'nested MixtureSet')
    # Jensen ties the new kernels to the existing ones
    assert (mset.predictive_log_likelihood(tt(X)) >=
            mset.expected_log_likelihood(mset.sufficient_statistics(tt(X)))).all()


def test_joint_model_set_concatenates_and_the_ordered_view_gathers():
    tol, rng = TOL[torch.float64], np.random.default_rng(12)
    pa, draw = make_params('diagonal', 6, 4, 'mixed', rng, np.float64)
    pb, _ = make_params('diagonal', 3, 4, 'prior', rng, np.float64)
    X = make_frames(pa, draw, 40, rng, np.float64)
    first = beer.MixtureSet(beer.CategoricalSet(dirichlet(rng.uniform(.2, 30, (2, 3)))),
                            normalset('diagonal', pa))
    joint = beer.JointModelSet([first, normalset('diagonal', pb)])
    want, bound = emissions_truth(joint, X)
    assert want.shape == (40, 5)
    got = joint.predictive_log_likelihood(tt(X))
    hold(got, want, tol * bound, 'JointModelSet')
    order = [4, 0, 0, 2]
    view = beer.DynamicallyOrderedModelSet(joint)
    assert torch.equal(view.predictive_log_likelihood(tt(X), order), got[:, order])


_TOPO = [{'start_id': 0, 'end_id': 1, 'trans_prob': 1.}, {'start_id': 1, 'end_id': 1, 'trans_prob': .5},
         {'start_id': 1, 'end_id': 2, 'trans_prob': .5}, {'start_id': 2, 'end_id': 2, 'trans_prob': .5},
         {'start_id': 2, 'end_id': 3, 'trans_prob': .5}]
D_LOOP = 4


@functools.lru_cache(maxsize=None)
def phone_loop():
    'A loop of 3 units, 2 states each, 2 diagonal Gaussians a state, float64.'
    torch.manual_seed(3)
    conf = {'g': {'topology': _TOPO, 'n_normal_per_state': 2, 'prior_strength': 1.,
                  'noise_std': 1., 'cov_type': 'diagonal', 'shared_cov': False}}
    names = [f'u{i}' for i in range(3)]
    units, ems = hmm_cmds.build_units(conf, {'g': names}, torch.zeros(D_LOOP), torch.ones(D_LOOP))
    graph, start, end = hmm_cmds.decode_graph(hmm_cmds.loop_graph(names), units)
    model = hmm_cmds.phone_loop(graph, start, end, ems, 'dirichlet')
    assert type(model) is beer.PhoneLoop and len(model.start_pdf) == 3
    return model.double().to('cuda')


def utterances(lens, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randn(T, D_LOOP) * 1.5).to('cuda') for T in lens]


def search_truth(model, X):
    '''(log-evidence, Viterbi pdf path, slack) of the EXISTING search kernels fed the truth's
    per-pdf matrix.  The log-evidence is 1-Lipschitz in the largest error of each frame's row:
    the slack is the sum over the frames of the rows' largest entry bounds.'''
    want, bound = emissions_truth(model._emissions(), npy(X))
    batch = model._batch_of_one(model.graph, len(X), torch.float64)
    pc = hk.gather(batch, tt(np.asarray(want, dtype=np.float64)), 1.)
    utt, _ = hk.log_evidence(batch, pc)
    slack = float((TOL[torch.float64] * bound).max(-1).sum())
    return float(utt[0]), hk.viterbi(batch, pc, map_pdf=True).cpu(), slack


def test_searches_on_a_phone_loop_run_on_the_predictive_densities():
    model = phone_loop()
    lens = [57, 23, 40, 9]
    utts = utterances(lens, 1)
    truths = [search_truth(model, X) for X in utts]
    for X, (total, path, slack) in zip(utts, truths):
        value = model.log_evidence(X, predictive=True)
        assert value.dim() == 0 and value.dtype == torch.float64
        assert abs(float(value) - total) <= slack + 1e-10 * (1 + abs(total))
        assert torch.equal(model.decode(X, predictive=True), path)
        # a density integrates the posterior's spread in: never below the variational value
        assert float(value) >= float(model.log_evidence(X))
    # the ragged batch, in one launch and in sub-batches
    for max_frames in (1 << 20, 45):
        got = beer.log_evidence_batch(model, utts, predictive=True, max_frames=max_frames)
        paths = beer.decode_batch(model, utts, predictive=True, max_frames=max_frames)
        for u, (total, path, slack) in enumerate(truths):
            assert abs(float(got[u]) - total) <= slack + 1e-10 * (1 + abs(total)), (max_frames, u)
            assert torch.equal(paths[u].cpu(), path), (max_frames, u)
    assert (beer.log_evidence_batch(model, utts, predictive=True) >=
            beer.log_evidence_batch(model, utts)).all()


def test_predictive_false_is_the_call_without_the_keyword():
    model = phone_loop()
    utts = utterances([31, 12], 2)
    for X in utts:
        assert torch.equal(model.log_evidence(X, predictive=False), model.log_evidence(X))
        assert torch.equal(model.decode(X, predictive=False), model.decode(X))
        assert not torch.equal(model.log_evidence(X, predictive=True), model.log_evidence(X))
    assert torch.equal(beer.log_evidence_batch(model, utts, predictive=False),
                       beer.log_evidence_batch(model, utts))
    for a, b in zip(beer.decode_batch(model, utts, predictive=False), beer.decode_batch(model, utts)):
        assert torch.equal(a, b)
