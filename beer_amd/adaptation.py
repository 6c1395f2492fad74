"""Speaker-adaptive affine feature transforms (constrained MLLR / fMLLR).

A transform `y = A_s x + b_s` per speaker, `W_s = [A_s | b_s]`, is estimated by maximum
likelihood under the current model: the frame term of the ELBO, E_q[ln p(y | theta)] of a
diagonal (or isotropic) Gaussian, sees a frame through E[lambda mu] and E[lambda] only, so
with the responsibilities r_tk of the transformed frames and xi = [x; 1]

    Q_s(W) = beta ln|det A| + sum_i (w_i . k_i - 1/2 w_i G_i w_i^T)
    G_i = sum_t omega_ti xi_t xi_t^T,   k_i = sum_t nu_ti xi_t,   beta = sum_t c_t
    omega_ti = sum_k r_tk E[lambda]_ki, nu_ti = sum_k r_tk E[lambda mu]_ki, c_t = sum_k r_tk

is what the transform of speaker s maximises (the Jacobian ln|det A| makes the transformed
density a density of x).  The statistics come from the HIP kernels of csrc/cmllr.hip
(`cmllr_statistics_batch`); the maximisation is the row-by-row closed form of Gales (1998)
on the host in float64 (`CmllrStats.estimate`).  The transforms are point estimates outside
the mean-field machinery: no model class changes, a transformed data set runs through every
subcommand as it is.  DESIGN.md section 28.
"""

import numpy as np
import torch

from . import _hip, hmm_kernels as hk, kernels
from .inference.batch import _groups, _normalset, _sub_batches, pack_utterances
from .models.mixtures import Mixture, MixtureSet, TiedMixtureSet
from .models.sequence import HMM
from .models.vae import VAE
from .stats import FrameStats

__all__ = ['AffineTransforms', 'CmllrStats', 'cmllr_statistics_batch', 'adapt']


def _is_packed(utterances):
    return isinstance(utterances, tuple) and len(utterances) == 2 and \
        isinstance(utterances[0], torch.Tensor)


class AffineTransforms:
    '''One affine transform of the features per speaker: `W` float64 [n, D, D + 1] = [A | b]
    (numpy, on the host), `names` the speakers.  Starts as the identity.'''

    def __init__(self, names, dim):
        self.names = [str(n) for n in names]
        if len(set(self.names)) != len(self.names):
            raise ValueError('AffineTransforms: a speaker is named twice')
        self.dim = int(dim)
        self.W = np.zeros((len(self.names), self.dim, self.dim + 1), dtype=np.float64)
        self.W[:, np.arange(self.dim), np.arange(self.dim)] = 1.

    def __len__(self):
        return len(self.names)

    def indices(self, speakers):
        '''int64 indices of `speakers`: names (a name without a transform: -1) or indices
        (-1: none) as they are.'''
        where = {n: i for i, n in enumerate(self.names)}
        out = np.asarray([where.get(s, -1) if isinstance(s, str) else int(s) for s in speakers],
                         dtype=np.int64).reshape(-1)
        if len(out) and (out.min() < -1 or out.max() >= len(self)):
            raise ValueError(f'AffineTransforms: speaker index outside -1 .. {len(self) - 1}')
        return out

    def apply(self, utterances, speakers):
        '''The transformed utterances, `speakers[u]` naming the transform of utterance u (a name,
        an index, -1 or an unknown name: copied).  A list of [T_u, D] tensors gives a list, a
        packed `(X, lengths)` pair a pair; the tensors are on the device, in the frames' dtype.'''
        packed = _is_packed(utterances)
        X, lengths = pack_utterances(utterances)
        if X.shape[1] != self.dim:
            raise ValueError(f'AffineTransforms of dimension {self.dim} on frames of {X.shape[1]}')
        Y = kernels.cmllr_apply(X, torch.from_numpy(self.W), lengths, self.indices(speakers))
        return (Y, lengths) if packed else list(torch.split(Y, lengths))

    def log_abs_det(self):
        'ln|det A_s| of every transform, float64 [n].'
        return np.linalg.slogdet(self.W[:, :, :self.dim])[1] if len(self) else np.zeros(0)

    def log_det_terms(self, lengths, speakers):
        '''T_u ln|det A_s| per utterance (0 where the utterance has no transform): what the
        score of the transformed utterance lacks to be a log-density of the original one.'''
        idx = self.indices(speakers)
        if len(idx) != len(lengths):
            raise ValueError(f'{len(idx)} speakers for {len(lengths)} utterances')
        logdet = np.concatenate([self.log_abs_det(), [0.]])         # (index -1: the last entry)
        return np.asarray(lengths, dtype=np.float64) * logdet[idx]

    def save(self, path):
        'An `.npz` with `speakers` (strings) and `W`.'
        with open(path, 'wb') as f:
            np.savez(f, speakers=np.asarray(self.names, dtype=str), W=self.W)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            names, W = [str(n) for n in z['speakers']], np.asarray(z['W'], dtype=np.float64)
        if W.ndim != 3 or W.shape[0] != len(names) or W.shape[2] != W.shape[1] + 1:
            raise ValueError(f'{path}: W of shape {W.shape} for {len(names)} speakers')
        out = cls(names, W.shape[1])
        out.W = W.copy()
        return out


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) \
        else np.asarray(t, dtype=np.float64)


class CmllrStats:
    '''The statistics of the transforms of n speakers, float64 on the host: `G` [n, P, E (E+1)/2]
    (the packed lower triangles of G_i; P = D, or 1 for isotropic models, whose one matrix serves
    every row), `k` [n, D, E], `beta` [n]; E = D + 1.'''

    def __init__(self, G, k, beta, names):
        self.G, self.k, self.beta = _host(G), _host(k), _host(beta)
        self.names = [str(n) for n in names]
        n, D, E = self.k.shape
        if E != D + 1 or self.G.shape not in ((n, D, E * (E + 1) // 2), (n, 1, E * (E + 1) // 2)) \
                or self.beta.shape != (n,) or len(self.names) != n:
            raise ValueError(f'CmllrStats: G {self.G.shape}, k {self.k.shape}, beta '
                             f'{self.beta.shape} for {len(self.names)} speakers')

    @property
    def dim(self):
        return self.k.shape[1]

    def __add__(self, other):
        if self.names != other.names or self.G.shape != other.G.shape:
            raise ValueError('CmllrStats: statistics of other speakers or another model')
        return CmllrStats(self.G + other.G, self.k + other.k, self.beta + other.beta, self.names)

    def full_G(self):
        'G as symmetric matrices [n, P, E, E].'
        n, D, E = self.k.shape
        a, b = np.tril_indices(E)
        out = np.zeros(self.G.shape[:2] + (E, E))
        out[:, :, a, b] = self.G
        out[:, :, b, a] = self.G
        return out

    def _objective(self, W, Gf):
        D = self.dim
        Gi = Gf if Gf.shape[1] == D else np.broadcast_to(Gf, (len(Gf), D) + Gf.shape[2:])
        quad = np.einsum('sie,sief,sif->s', W, Gi, W)
        sign, logdet = np.linalg.slogdet(W[:, :, :D])
        with np.errstate(invalid='ignore'):
            jac = np.where(self.beta > 0, self.beta * logdet, 0.)
        return jac + np.einsum('sie,sie->s', W, self.k) - .5 * quad

    def objective(self, W):
        'Q_s(W) of every speaker, float64 [n]; `W` [n, D, D + 1] or `AffineTransforms`.'
        W = W.W if isinstance(W, AffineTransforms) else np.asarray(W, dtype=np.float64)
        return self._objective(W, self.full_G())

    def estimate(self, W0=None, sweeps=20, min_gain=1e-6, min_count=500., on_row=None):
        '''(AffineTransforms, gain per frame [n]): `sweeps` sweeps of the row update over the
        rows 0 .. D-1, from `W0` (default: the identity), vectorised over the speakers.  With
        p = [row i of A^-T, 0] (the cofactors up to their common factor det A, which the update
        does not see), a = p G_i^-1 p^T, b = p G_i^-1 k_i, alpha the root of
        a alpha^2 + b alpha - beta = 0 with the larger beta ln|alpha a + b| - alpha^2 a / 2:
        w_i = (alpha p + k_i) G_i^-1.  A speaker with beta < min_count or a singular G_i keeps
        W0's block (gain 0); a sweep that gains less than `min_gain` per frame is the
        speaker's last.  The gain is (Q(W) - Q(W0)) / beta.  `on_row(sweep, i, W)`: called
        after every row step (tests, traces).'''
        n, D, E = self.k.shape
        if W0 is None:
            W = AffineTransforms(self.names, D).W
        else:
            W = np.array(W0.W if isinstance(W0, AffineTransforms) else W0, dtype=np.float64)
            if W.shape != (n, D, E):
                raise ValueError(f'W0 of shape {W.shape}, expected {(n, D, E)}')
        Gf = self.full_G()
        P = Gf.shape[1]
        eig = np.linalg.eigvalsh(Gf)                              # [n, P, E] ascending
        sound = np.isfinite(eig).all(axis=(1, 2)) & \
            (eig[:, :, 0] > E * np.finfo(np.float64).eps * np.abs(eig[:, :, -1])).all(axis=1)
        with np.errstate(invalid='ignore'):
            active = sound & (self.beta >= min_count) & (self.beta > 0) & \
                (np.abs(np.linalg.slogdet(W[:, :, :D])[0]) > 0)
        estimated = active.copy()
        Ginv = np.zeros_like(Gf)
        Ginv[active] = np.linalg.inv(Gf[active])
        Q0 = self._objective(W, Gf)
        Q = Q0.copy()
        for sweep in range(int(sweeps)):
            if not active.any():
                break
            act = np.nonzero(active)[0]
            beta = self.beta[act]
            for i in range(D):
                p = np.zeros((len(act), E))
                p[:, :D] = np.linalg.inv(W[act][:, :, :D])[:, :, i]
                Gi = Ginv[act, i if P > 1 else 0]
                ki = self.k[act, i]
                pG = np.einsum('me,mef->mf', p, Gi)
                a, b = np.einsum('me,me->m', pG, p), np.einsum('me,me->m', pG, ki)
                disc = np.sqrt(b * b + 4. * a * beta)
                roots = np.stack([(-b + disc) / (2. * a), (-b - disc) / (2. * a)])
                with np.errstate(divide='ignore'):
                    value = beta * np.log(np.abs(roots * a + b)) - .5 * roots * roots * a
                alpha = np.where(value[0] >= value[1], roots[0], roots[1])
                W[act, i] = np.einsum('me,mef->mf', alpha[:, None] * p + ki, Gi)
                if on_row is not None:
                    on_row(sweep, i, W)
            new = self._objective(W, Gf)
            with np.errstate(invalid='ignore', divide='ignore'):
                slow = (new - Q) / self.beta < min_gain
            Q = np.where(active, new, Q)
            active &= ~slow
        with np.errstate(invalid='ignore', divide='ignore'):
            gain = np.where(estimated, (Q - Q0) / self.beta, 0.)
        out = AffineTransforms(self.names, D)
        out.W = W
        return out, gain


def _emission_groups(model):
    '(groups, is_mixture) of a model `cmllr_statistics_batch` covers; else NotImplementedError.'
    if isinstance(model, VAE):
        raise NotImplementedError('CMLLR statistics: not for a VAE (the transform would have to '
                                  'go through the encoder)')
    if isinstance(model, Mixture):
        ns = model.normalset
        groups = [(model, 1, len(ns))]
    elif isinstance(model, HMM):
        groups = _groups(model._emissions())
    else:
        raise NotImplementedError(f'CMLLR statistics: no support for {type(model).__name__}')
    covs = set()
    for grp, _, _ in groups:
        if isinstance(grp, TiedMixtureSet):
            raise NotImplementedError('CMLLR statistics: tied-mixture emissions are not supported')
        covs.add(_normalset(grp).cov_type if not isinstance(grp, Mixture) else grp.normalset.cov_type)
    if 'full' in covs:
        raise NotImplementedError('CMLLR statistics: full covariances are not supported (their '
                                  'statistics couple the rows of the transform; diagonal or '
                                  'isotropic only)')
    if len(covs) != 1:
        raise NotImplementedError('CMLLR statistics: diagonal and isotropic emission groups in '
                                  'one model are not supported')
    return groups, isinstance(model, Mixture), covs.pop()


def cmllr_statistics_batch(model, utterances, speakers, n_speakers, transforms=None,
                           inference_graphs=None, scale=1., max_frames=1 << 20, chunk_frames=0,
                           names=None):
    '''`CmllrStats` of a shard: `speakers[u]` in 0 .. n_speakers - 1 is the speaker of utterance u
    (-1: left out).  The posteriors are those of the frames transformed by `transforms` (an
    `AffineTransforms` of n_speakers speakers; default: none), the statistics are of the
    original frames.  `model`: an HMM / PhoneLoop / BigramPhoneLoop (free loop, or one alignment
    graph per utterance in `inference_graphs`; `scale` the acoustic scale) or a plain Mixture,
    with diagonal or isotropic Gaussians (NormalSet, MixtureSet -- nested ones as their leaves --
    or a JointModelSet of them).  Per sub-batch of at most `max_frames` frames: transform,
    E-step with dense responsibilities, forward-backward, `cmllr_frame_params` per emission
    group, `cmllr_accumulate` (work items of `chunk_frames` frames; 0: the library's default).'''
    if getattr(model, 'durations', None) is not None:
        model._refuse_durations('speaker adaptation (adapt, cmllr_statistics_batch)')
    groups, is_mixture, cov = _emission_groups(model)
    X, lengths = pack_utterances(utterances)
    D, n_speakers = X.shape[1], int(n_speakers)
    spk = np.asarray([int(s) for s in speakers], dtype=np.int64).reshape(-1)
    if len(spk) != len(lengths):
        raise ValueError(f'cmllr_statistics_batch: {len(spk)} speakers for {len(lengths)} utterances')
    if inference_graphs is not None and (is_mixture or len(inference_graphs) != len(lengths)):
        raise ValueError('cmllr_statistics_batch: one inference graph per utterance of an HMM')
    if transforms is not None and (len(transforms) != n_speakers or transforms.dim != D):
        raise ValueError(f'cmllr_statistics_batch: transforms of {len(transforms)} speakers and '
                         f'dimension {transforms.dim} for {n_speakers} speakers and frames of {D}')
    P = D if cov == 'diagonal' else 1
    E = D + 1
    dev = X.device
    Gs = torch.zeros(n_speakers, P, E * (E + 1) // 2, dtype=torch.float64, device=dev)
    ks = torch.zeros(n_speakers, D, E, dtype=torch.float64, device=dev)
    beta = torch.zeros(n_speakers, dtype=torch.float64, device=dev)
    S_total = sum(S for _, S, _ in groups)
    K_total = sum(S * G for _, S, G in groups)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    max_S = 1
    if not is_mixture:
        max_S = model.graph.n_states if inference_graphs is None \
            else max(g.n_states for g in inference_graphs)
        if inference_graphs is not None and len(inference_graphs) and \
                getattr(getattr(inference_graphs[0], '_set', None), 'is_bound', False):
            model._bound_set(inference_graphs).refresh(X.dtype)
    # scratch per frame: the transformed frame, responsibilities, per-state likelihoods and
    # posteriors, the trellis, the float64 parameters
    bpf = (D + K_total + 2 * S_total + 3 * max_S) * X.element_size() + 8 * max_S + 8 * (P + D + 1)
    for run in _sub_batches(lengths, bpf, max_frames):
        f0, f1 = int(off[run[0]]), int(off[run[-1] + 1])
        run_lengths = [lengths[u] for u in run]
        run_spk = spk[run[0]:run[-1] + 1]
        Xr = X[f0:f1]
        Y = Xr if transforms is None else transforms.apply((Xr, run_lengths), run_spk)[0]
        stats = FrameStats(Y, cov)
        params = torch.zeros(f1 - f0, P + D + 1, dtype=torch.float64, device=dev)
        if is_mixture:
            ns = model.normalset
            K = len(ns)
            exp_T = ns.means_precisions.natural_form()
            _, resps = kernels.mixtureset_estep(stats, exp_T, model._log_weights().view(1, K), 1, K,
                                                cov, want_resps=True)
            kernels.cmllr_frame_params(resps, None, exp_T, 1, K, D, cov, out=params)
        else:
            cols, comps = [], []
            for grp, S, G in groups:
                ns = _normalset(grp)
                lw = grp.leaf_log_weights() if isinstance(grp, MixtureSet) else None
                log_norm, resps = kernels.mixtureset_estep(
                    stats, ns.means_precisions.natural_form(), lw, S, G, cov, want_resps=G > 1)
                cols.append(log_norm)
                comps.append(resps)
            pc_all = cols[0] if len(cols) == 1 else torch.cat(cols, dim=-1)
            if inference_graphs is None:
                batch = hk.HmmBatch([model.graph], [0] * len(run), run_lengths, X.dtype)
            else:
                uniq, ids, seen = [], [], {}
                for u in run:
                    g = inference_graphs[u]
                    if id(g) not in seen:
                        seen[id(g)] = len(uniq)
                        uniq.append(g)
                    ids.append(seen[id(g)])
                batch = hk.HmmBatch(uniq, ids, run_lengths, X.dtype)
            pc_llhs = hk.gather(batch, pc_all, scale)
            gamma = hk.forward_backward(batch, pc_llhs)[0]
            sr, _ = hk.scatter(batch, pc_llhs, gamma, S_total, scale, want_exp_llh=False)
            first = 0
            for (grp, S, G), resps in zip(groups, comps):
                ns = _normalset(grp)
                sr_g = sr if len(groups) == 1 else sr[:, first:first + S].contiguous()
                first += S
                kernels.cmllr_frame_params(resps, sr_g, ns.means_precisions.natural_form(), S, G,
                                           D, cov, out=params)
        kernels.cmllr_accumulate(Xr, params, run_lengths, run_spk, n_speakers, G=Gs, k=ks,
                                 beta=beta, chunk_frames=chunk_frames)
    if hasattr(model, 'clear_cache'):
        model.clear_cache()
    names = [str(i) for i in range(n_speakers)] if names is None else names
    return CmllrStats(Gs, ks, beta, names)


_ESTIMATE_ARGS = ('sweeps', 'min_gain', 'min_count')


def adapt(model, utterances, speakers, names, iters=3, transforms=None, **kw):
    '''(AffineTransforms, [gain per frame per speaker of every iteration]): `iters` rounds of
    statistics under the current transforms (`cmllr_statistics_batch`) and `estimate` from
    them.  `speakers[u]`: a name of `names` or its index; `transforms`: where to start
    (default: the identity).  `sweeps`, `min_gain`, `min_count` go to `estimate`, every other
    keyword to `cmllr_statistics_batch`.'''
    if getattr(model, 'durations', None) is not None:
        model._refuse_durations('speaker adaptation (adapt, cmllr_statistics_batch)')
    names = [str(n) for n in names]
    est = {k: kw.pop(k) for k in _ESTIMATE_ARGS if k in kw}
    X, lengths = pack_utterances(utterances)
    if transforms is None:
        transforms = AffineTransforms(names, X.shape[1])
    elif transforms.names != names:
        raise ValueError('adapt: the initial transforms are of other speakers')
    idx = transforms.indices(speakers)
    gains = []
    for _ in range(int(iters)):
        stats = cmllr_statistics_batch(model, (X, lengths), idx, len(names),
                                       transforms=transforms, names=names, **kw)
        transforms, gain = stats.estimate(W0=transforms, **est)
        gains.append(gain)
    return transforms, gains
