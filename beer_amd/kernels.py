"""Python faces of the E-step entry points of include/beer_hip.h.

Shapes and argument checks only: the arithmetic is in beer_amd/csrc.  All
returned tensors live on the GPU.
"""

import ctypes
import functools
import os

import numpy as np
import torch

from . import _hip
from .stats import FrameStats

__all__ = ['normal_llh', 'mixtureset_estep', 'normal_accumulate', 'weights_from_acc',
           'tied_lognorm', 'tied_accumulate', 'predictive_llh', 'mixtureset_predictive',
           'is_dense', 'dense_llh', 'dense_softmax', 'dense_accumulate', 'rowdot',
           'attach_stats_grad', 'differentiable_stats', 'sample_stats', 'attach_frame_grad',
           'frames_llh_backward', 'normal_llh_autograd', 'cmllr_frame_params', 'cmllr_table',
           'cmllr_accumulate', 'cmllr_apply', 'CmllrTable', 'unit_sequences', 'edit_distance',
           'edit_distance_route', 'edit_distance_launch']

LOG_2PI = 1.8378770664093453


def is_dense(stats):
    'True for dense [T, Q] statistics (the VAE "stats-in" path).'
    return isinstance(stats, torch.Tensor)


def _exact(X):
    '''Whether this call multiplies float32 frames on the exact fp32 MFMA: small
    inputs, or the caller asked for it (`_hip.f32_fast_ok`).'''
    return X.dtype == torch.float32 and not _hip.f32_fast_ok(X)


def _frames(stats):
    if not isinstance(stats, FrameStats):
        raise TypeError('expected the lazy statistics returned by '
                        'model.sufficient_statistics(X)')
    return stats


def normal_llh(stats, exp_stats, cov_type):
    'l[t,k] = scale * phi(x_t) . E[T]_k - D/2 ln 2pi -> [T, K].'
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    E = _hip.on_device(exp_stats, X.dtype)
    K = E.shape[0]
    if st.scale == 1.0:
        # K mixtures of one component: the log-normalisers ARE the log-likelihoods, and that
        # form of the call runs on the matrix cores (the per-component output does not)
        return mixtureset_estep(st, E, None, K, 1, cov_type, want_resps=False)[0]
    out = torch.empty(T, K, dtype=X.dtype, device=X.device)
    _hip.call('beer_mixtureset_estep', _hip.dtype_code(X.dtype), _hip.COV_CODE[cov_type],
              T, D, K, 1, _hip.ptr(X), _hip.ptr(E), None, None, st.scale,
              _hip.ptr(out), None, None, None, None, 0)
    return out


@functools.lru_cache(maxsize=4096)
def estep_buffers(dtype_code, cov, D, S, G, args, ws_bytes):
    '''(need_resps, image_ok) of the `beer_mixtureset_estep` call with the `_hip.ARG_*` mask
    `args` and a workspace of `ws_bytes`, as the library's own `beer_estep_route` answers (host
    only, integers only): whether the call must be given a responsibilities buffer -- the
    caller wants one, or the library refuses the call without one and takes it with one (the
    generic kernels normalise in it) -- and whether `beer_mixtureset_lognorm_image` takes the
    same call with a frame image.  A call refused either way raises `HipInvalid`.

    Cached: the refusals behind the query (`estep_plan`, `llhx_form`) read the shape, the mask
    and the workspace size only, never the option table.  The form does: it is not kept.'''
    def refused(entry, mask):
        return _hip.estep_route(entry, dtype_code, cov, D, S, G, mask, ws_bytes) == _hip.EINVAL
    need_resps = bool(args & _hip.ARG_RESPS)
    if not need_resps and refused(_hip.ESTEP_PLAIN, args):
        need_resps = True
    if need_resps and refused(_hip.ESTEP_PLAIN, args | _hip.ARG_RESPS):
        raise _hip.HipInvalid('beer_mixtureset_estep failed: invalid argument')
    return need_resps, not refused(_hip.ESTEP_IMAGE, args)


def mixtureset_estep(stats, exp_stats, log_weights, S, G, cov_type, labels=None,
                     want_resps=True, llh_sum=None):
    '''(log_norm [T,S], comp_resps [T,S*G] or None).  `log_weights` [S,G] or
    None.  `llh_sum`: optional fp64 device scalar, += sum log_norm.'''
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    E = _hip.on_device(exp_stats, X.dtype)
    lw = None if log_weights is None else _hip.on_device(log_weights, X.dtype)
    K = S * G
    if E.shape[0] != K:
        raise ValueError(f'{E.shape[0]} Gaussians for {S} x {G} mixture components')
    code, cov = _hip.dtype_code(X.dtype, _exact(X)), _hip.COV_CODE[cov_type]
    ws, ws_bytes = _hip.workspace('beer_estep_workspace_bytes', X.dtype, cov, D, S, G, X.device)
    args = _hip.ARG_LOG_NORM | (_hip.ARG_RESPS if want_resps else 0) | \
        (0 if llh_sum is None else _hip.ARG_LLH_SUM) | (0 if lw is None else _hip.ARG_LOG_WEIGHTS) | \
        (0 if labels is None else _hip.ARG_LABELS) | (_hip.ARG_SCALED if st.scale != 1.0 else 0)
    need_resps, image_ok = estep_buffers(code, cov, D, S, G, args, ws_bytes)
    log_norm = torch.empty(T, S, dtype=X.dtype, device=X.device)
    # log-normalisers only, on the bf16x3 path: the logits' A fragments from the frame
    # fragment image where the frames have one (the fused accumulation uses the same)
    img = st.frame_image(cov_type) if image_ok else None
    if img is not None:
        _hip.call('beer_mixtureset_lognorm_image', cov, T, D, S, G, _hip.ptr(X), _hip.ptr(E),
                  _hip.ptr(lw), _hip.ptr(img), _hip.ptr(log_norm), _hip.ptr(llh_sum),
                  _hip.ptr(ws), ws_bytes)
        return log_norm, None
    # (the generic kernels normalise in the responsibilities buffer: wanted or not)
    resps = torch.empty(T, K, dtype=X.dtype, device=X.device) if need_resps else None
    lab = None
    if labels is not None:
        lab = _hip.on_device(torch.as_tensor(labels)).to(torch.int64).contiguous()
    _hip.call('beer_mixtureset_estep', code, cov, T, D, S, G, _hip.ptr(X), _hip.ptr(E),
              _hip.ptr(lw), _hip.ptr(lab), st.scale, None, _hip.ptr(log_norm), _hip.ptr(resps),
              _hip.ptr(llh_sum), _hip.ptr(ws), ws_bytes)
    return log_norm, resps if want_resps else None


class PackedResps:
    '''Responsibilities [T, K] of one mixture in the form the bf16x3 accumulation
    kernel multiplies with (include/beer_hip.h: beer_mixture_estep_packed):
    `words` int32, the three-plane tiles of 64 frames x 128 components that kernel
    copies to LDS.  `unpack()` gives the float32 matrix (exactly).'''

    def __init__(self, words, nframes, ncomp):
        self.words, self.shape = words, (nframes, ncomp)

    def unpack(self):
        T, K = self.shape
        out = torch.empty(T, K, dtype=torch.float32, device=self.words.device)
        _hip.call('beer_unpack_resps', T, K, _hip.ptr(self.words), _hip.ptr(out))
        return out


def packed_path_ok(stats, K, cov_type):
    '''True when the E-step of a K-component mixture over `stats` can hand its
    responsibilities to the accumulation in packed form: float32 frames on the
    bf16x3 path, unscaled, shapes with a matrix-core kernel on both sides.'''
    st = _frames(stats)
    X = st.data
    if st.scale != 1.0 or not _hip.f32_fast_ok(X):
        return False
    code, D = _hip.COV_CODE[cov_type], X.shape[1]
    lib, dt = _hip.lib(), _hip.dtype_code(X.dtype)
    # (the packed kernels' own queries: they take D <= 128, the exact ones D <= 96)
    return lib.beer_estep_workspace_bytes(dt, code, D, 1, K) > 0 and \
        lib.beer_accumulate_packed_workspace_bytes(code, X.shape[0], D, K) > 0


def mixture_estep_packed(stats, exp_stats, log_weights, K, cov_type, llh_sum=None):
    '''(log_norm [T,1], PackedResps) of one mixture: `mixtureset_estep` with
    S = 1 whose responsibilities go straight to `normal_accumulate`.  Only where
    `packed_path_ok`.'''
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    E = _hip.on_device(exp_stats, X.dtype)
    lw = _hip.on_device(log_weights, X.dtype)
    if E.shape[0] != K or lw.numel() != K:
        raise ValueError(f'{E.shape[0]} Gaussians, {lw.numel()} weights for {K} components')
    log_norm = torch.empty(T, 1, dtype=X.dtype, device=X.device)
    words = torch.empty(_hip.lib().beer_packed_resps_bytes(T, D, K) // 4, dtype=torch.int32,
                        device=X.device)
    ws, ws_bytes = _hip.workspace('beer_estep_workspace_bytes', X.dtype,
                                  _hip.COV_CODE[cov_type], D, 1, K, X.device)
    _hip.call('beer_mixture_estep_packed', _hip.COV_CODE[cov_type], T, D, K, _hip.ptr(X),
              _hip.ptr(E), _hip.ptr(lw), _hip.ptr(log_norm), _hip.ptr(words), _hip.ptr(llh_sum),
              _hip.ptr(ws), ws_bytes)
    return log_norm, PackedResps(words, T, K)


def packed_sets_ok(stats, S, G, cov_type):
    '''True when a mixture SET can hand the responsibilities within its states'
    mixtures to the accumulation as packed tiles, the state posteriors being
    multiplied in by the accumulation kernel (include/beer_hip.h:
    beer_mixtureset_estep_packed): float32 frames on the bf16x3 path, full
    covariance, G a power of two in 8..128.'''
    st = _frames(stats)
    X = st.data
    if st.scale != 1.0 or X.dtype != torch.float32 or not _hip.f32_fast_ok(X):
        return False
    return bool(_hip.lib().beer_mixtureset_packed_supported(_hip.COV_CODE[cov_type], X.shape[1],
                                                            S, G))


def mixtureset_estep_packed(stats, exp_stats, log_weights, S, G, cov_type, llh_sum=None):
    '''(log_norm [T,S], PackedResps [T, S*G]) of a mixture set: `mixtureset_estep`
    whose responsibilities go to `normal_accumulate(..., state_resps)` in packed
    form.  Only where `packed_sets_ok`.'''
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    K = S * G
    E = _hip.on_device(exp_stats, X.dtype)
    lw = None if log_weights is None else _hip.on_device(log_weights, X.dtype)
    if E.shape[0] != K or (lw is not None and lw.numel() != K):
        raise ValueError(f'{E.shape[0]} Gaussians for {S} x {G} components')
    log_norm = torch.empty(T, S, dtype=X.dtype, device=X.device)
    words = torch.empty(_hip.lib().beer_packed_resps_bytes(T, D, K) // 4, dtype=torch.int32,
                        device=X.device)
    ws, ws_bytes = _hip.workspace('beer_estep_workspace_bytes', X.dtype,
                                  _hip.COV_CODE[cov_type], D, S, G, X.device)
    _hip.call('beer_mixtureset_estep_packed', _hip.COV_CODE[cov_type], T, D, S, G, _hip.ptr(X),
              _hip.ptr(E), _hip.ptr(lw), _hip.ptr(log_norm), _hip.ptr(words), _hip.ptr(llh_sum),
              _hip.ptr(ws), ws_bytes)
    return log_norm, PackedResps(words, T, K)


# ---- one mixture with more than 256 components ---------------------------------------------

class WideResps:
    '''Responsibilities [T, K] of ONE mixture with more than 256 components, in the
    factored form the matrix-core kernels of a mixture set work with: the
    components are cut into S2 blocks of G2; `block_lse` [T, S2] are the blocks'
    log-sum-exps, `block_resps` [T, S2] = exp(block_lse - log_norm) the blocks' shares,
    and within a block r = exp(l - block_lse) is recomputed from the frames
    (diagonal / isotropic) or held as packed tiles (full covariance).  The softmax
    over K components is the two-level softmax of these.  When K is not S2 * G2 the
    last block is filled up with phantom components of weight exp(-1e30) = 0
    (`exp_stats` / `log_weights` are the padded arrays, `K` the real count).
    `dense()` gives the [T, K] matrix.'''

    def __init__(self, stats, exp_stats, log_weights, split, cov_type, block_lse, block_resps,
                 packed, K=None):
        self.stats, self.exp_stats, self.log_weights = stats, exp_stats, log_weights
        self.split, self.cov_type = split, cov_type
        self.block_lse, self.block_resps, self.packed = block_lse, block_resps, packed
        self.K = split[0] * split[1] if K is None else K

    def dense(self):
        S2, G2 = self.split
        within = self.packed.unpack() if self.packed is not None else mixtureset_estep(
            self.stats, self.exp_stats, self.log_weights, S2, G2, self.cov_type)[1]
        return (within * self.block_resps.repeat_interleave(G2, dim=1))[:, :self.K]


def wide_mixture_split(stats, K, cov_type):
    '''(S2, G2), S2 * G2 >= K, when a mixture of K > 256 components over `stats` runs on
    the matrix-core kernels as S2 blocks of G2 components (two-level softmax); None
    otherwise (small inputs, exact mode: the generic kernels take it).  An exact
    factorisation is preferred; any other K gets its last block padded.'''
    st = _frames(stats)
    X = st.data
    if K <= 256 or st.scale != 1.0 or X.dtype != torch.float32 or not _hip.f32_fast_ok(X):
        return None
    ok = (lambda S2, G2: packed_sets_ok(st, S2, G2, cov_type)) if cov_type == 'full' else \
        (lambda S2, G2: fused_accumulate_ok(st, S2, G2, cov_type))
    first = -(-K // 256)
    for S2 in range(first, min(K // 8, first + 64) + 1):
        if K % S2 == 0 and ok(S2, K // S2):
            return S2, K // S2
    for G2 in ((128, 64) if cov_type == 'full' else (256, 128)):
        S2 = -(-K // G2)
        if ok(S2, G2):
            return S2, G2
    return None


def wide_mixture_estep(stats, exp_stats, log_weights, K, cov_type, split):
    '''(log_norm [T, 1], WideResps) of one mixture over `split` = wide_mixture_split(...):
    Mixture.expected_log_likelihood (beer/models/mixture.py:70-93) for K > 256.'''
    S2, G2 = split
    st = _frames(stats)
    E = _hip.on_device(exp_stats, st.data.dtype)
    lw = _hip.on_device(log_weights, st.data.dtype).reshape(-1)
    pad = S2 * G2 - K
    if pad:
        # phantom components: any finite parameters, log-weight -1e30 (exp underflows to an
        # exact 0: their responsibilities and statistics are zeros; not -inf, which the
        # multi-piece products would turn into 0 * inf)
        E = torch.cat([E, E[:1].expand(pad, -1)]).contiguous()
        lw = torch.cat([lw, torch.full((pad,), -1.0e30, dtype=lw.dtype, device=lw.device)])
    lw = lw.reshape(S2, G2)
    packed = None
    if cov_type == 'full':
        lse, packed = mixtureset_estep_packed(st, E, lw, S2, G2, cov_type)
    else:
        lse, _ = mixtureset_estep(st, E, lw, S2, G2, cov_type, want_resps=False)
    log_norm, share = dense_softmax(lse, None, 1, S2)
    return log_norm, WideResps(st, E, lw, split, cov_type, lse, share, packed, K=K)


def pack_resps(stats, comp_resps, state_resps, S, G):
    '''PackedResps of float32 responsibilities [T, S*G] (times `state_resps`
    [T, S] broadcast over each state's G components).'''
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    K = S * G
    cr = _hip.on_device(comp_resps, X.dtype)
    sr = None if state_resps is None else _hip.on_device(state_resps, X.dtype)
    words = torch.empty(_hip.lib().beer_packed_resps_bytes(T, D, K) // 4, dtype=torch.int32,
                        device=X.device)
    _hip.call('beer_pack_resps', T, D, S, G, _hip.ptr(X), _hip.ptr(cr), _hip.ptr(sr),
              _hip.ptr(words))
    return PackedResps(words, T, K)


def _repack_pays(stats, K, cov_type):
    '''Accumulating float32 responsibilities: with more than 32 statistic tiles
    (full covariance, D >= 22) the float32 kernel re-reads them four times at a
    fifth of the MFMA rate; packing them first (one read, one write) and running
    the packed kernel is faster (K = 1920, D = 40: 11.8 -> 6 ms per 500 k frames).'''
    X = stats.data
    if cov_type != 'full' or stats.shape[1] <= 512 or K % 4 or stats.scale != 1.0 or \
            not _hip.f32_fast_ok(X):
        return False
    return _hip.lib().beer_accumulate_packed_workspace_bytes(
        _hip.COV_CODE[cov_type], X.shape[0], X.shape[1], K) > 0


def normal_accumulate(stats, comp_resps, state_resps, S, G, cov_type, acc=None):
    '''acc[k,:] += sum_t comp_resps[t,k] * state_resps[t, k // G] * phi(x_t),
    fp64 [S*G, Q].  `comp_resps` may be the `PackedResps` of
    `mixture_estep_packed` (no state responsibilities then).'''
    st = _frames(stats)
    if st.scale != 1.0:
        raise ValueError('scaled statistics cannot be accumulated')
    X = st.data
    T, D = X.shape
    K = S * G
    Q = st.shape[1]
    if acc is None:
        acc = torch.zeros(K, Q, dtype=torch.float64, device=X.device)
    if isinstance(comp_resps, WideResps):
        # one mixture, K > 256: the blocks' shares play the state posteriors' part
        wr = comp_resps
        S2, G2 = wr.split
        if state_resps is not None or wr.K != K or wr.stats.data.data_ptr() != X.data_ptr():
            raise ValueError('factored responsibilities: one mixture, the frames they came from')
        # (a padded last block: the phantom components' rows are zeros, dropped here)
        full = acc if S2 * G2 == K else torch.zeros(S2 * G2, Q, dtype=torch.float64, device=X.device)
        if wr.packed is not None:
            normal_accumulate(st, wr.packed, wr.block_resps, S2, G2, cov_type, acc=full)
        else:
            mixtureset_accumulate_fused(st, wr.exp_stats, wr.log_weights, wr.block_lse,
                                        wr.block_resps, S2, G2, cov_type, acc=full)
        if full is not acc:
            acc += full[:K]
        return acc
    if isinstance(comp_resps, PackedResps) and state_resps is not None:
        # mixture set: the state posteriors are multiplied in by the kernel
        if tuple(comp_resps.shape) != (T, K) or not packed_sets_ok(st, S, G, cov_type):
            raise ValueError('packed responsibilities of a mixture set: same frames and '
                             'components, a shape with `packed_sets_ok`')
        sr = _hip.on_device(state_resps, X.dtype)
        if tuple(sr.shape) != (T, S):
            raise ValueError(f'state responsibilities {tuple(sr.shape)}, expected {(T, S)}')
        code = _hip.COV_CODE[cov_type]
        ws, ws_bytes = _hip.packed_workspace(code, T, D, K, X.device, sets=(S, G))
        _hip.call('beer_mixtureset_accumulate_packed', code, T, D, S, G, _hip.ptr(X),
                  _hip.ptr(comp_resps.words), _hip.ptr(sr), _hip.ptr(acc), _hip.ptr(ws), ws_bytes)
        return acc
    if isinstance(comp_resps, PackedResps):
        if tuple(comp_resps.shape) != (T, K):
            raise ValueError('packed responsibilities: same frames and components')
        ws, ws_bytes = _hip.packed_workspace(_hip.COV_CODE[cov_type], T, D, K, X.device)
        _hip.call('beer_normal_accumulate_packed', _hip.COV_CODE[cov_type], T, D, K,
                  _hip.ptr(X), _hip.ptr(comp_resps.words), _hip.ptr(acc), _hip.ptr(ws), ws_bytes)
        return acc
    if comp_resps is not None and X.dtype == torch.float32 and _repack_pays(st, K, cov_type):
        return normal_accumulate(st, pack_resps(st, comp_resps, state_resps, S, G), None, S, G,
                                 cov_type, acc=acc)
    cr = None if comp_resps is None else _hip.on_device(comp_resps, X.dtype)
    sr = None if state_resps is None else _hip.on_device(state_resps, X.dtype)
    ws, ws_bytes = _hip.frames_workspace(X.dtype, _exact(X), _hip.COV_CODE[cov_type], T, D, S, G,
                                         X.device)
    _hip.call('beer_normal_accumulate', _hip.dtype_code(X.dtype, _exact(X)),
              _hip.COV_CODE[cov_type], T, D, S, G, _hip.ptr(X), _hip.ptr(cr), _hip.ptr(sr),
              _hip.ptr(acc), _hip.ptr(ws), ws_bytes)
    return acc


def fused_accumulate_ok(stats, S, G, cov_type):
    '''True when `mixtureset_accumulate_fused` takes the call: float32 frames on the
    bf16x3 path, unscaled, diagonal / isotropic Gaussians (few statistics per
    Gaussian) -- the E-step then needs to leave no responsibilities behind.'''
    st = _frames(stats)
    X = st.data
    if st.scale != 1.0 or not _hip.f32_fast_ok(X):
        return False
    # the E-step that leaves the log-normalisers must be the matrix-core one: the
    # recomputed logits then carry the same roundings as the normalisers (against the
    # generic kernels' logits a 1e-5 mismatch does not cancel)
    code = _hip.COV_CODE[cov_type]
    return _hip.lib().beer_accumulate_fused_workspace_bytes(code, X.shape[1], S, G) > 0 and \
        _hip.lib().beer_estep_workspace_bytes(_hip.F32, code, X.shape[1], S, G) > 0


def mixtureset_accumulate_fused(stats, exp_stats, log_weights, log_norm, state_resps, S, G,
                                cov_type, acc=None):
    '''acc[k,:] += sum_t exp(l[t,k] - log_norm[t, k // G]) * state_resps[t, k // G] *
    phi(x_t), the component logits l recomputed from the frames (no [T, K] matrix).'''
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    K = S * G
    E = _hip.on_device(exp_stats, X.dtype)
    lw = None if log_weights is None else _hip.on_device(log_weights, X.dtype)
    ln = _hip.on_device(log_norm, X.dtype)
    sr = None if state_resps is None else _hip.on_device(state_resps, X.dtype)
    if tuple(ln.shape) != (T, S) or (sr is not None and tuple(sr.shape) != (T, S)):
        raise ValueError(f'log_norm / state_resps must be [{T}, {S}]')
    if acc is None:
        acc = torch.zeros(K, st.shape[1], dtype=torch.float64, device=X.device)
    code = _hip.COV_CODE[cov_type]
    ws, nbytes = _hip.scratch(('accf', code, D, S, G),
                              _hip.lib().beer_accumulate_fused_workspace_bytes(code, D, S, G),
                              X.device)
    img = st.frame_image(cov_type)
    _hip.call('beer_mixtureset_accumulate_fused', code, T, D, S, G, _hip.ptr(X), _hip.ptr(E),
              _hip.ptr(lw), _hip.ptr(ln), _hip.ptr(sr), _hip.ptr(img), _hip.ptr(acc), _hip.ptr(ws),
              nbytes)
    return acc


def weights_from_acc(acc, S, G):
    'Mixture-weight statistics [S, G] (fp64) from accumulated Gaussian stats.'
    out = torch.zeros(S, G, dtype=torch.float64, device=acc.device)
    _hip.call('beer_weights_from_acc', S, G, acc.shape[1], _hip.ptr(acc), _hip.ptr(out))
    return out


# ---- tied mixtures: S sets of weights over one pool of K Gaussians --------------

_tied_counters = {}


def tied_log_counter(device):
    '''The int64 device scalar the models' `tied_lognorm` calls count their log-space entries
    in (one per device, for the life of the process; `tied_log_entries` reads it).'''
    device = torch.device(device)
    if device not in _tied_counters:
        _tied_counters[device] = torch.zeros((), dtype=torch.int64, device=device)
    return _tied_counters[device]


def tied_log_entries(device=None):
    '''How many (frame, state) entries of tied mixtures were redone in log space on `device`
    so far (a host read-back: for tests and diagnostics, not for the training loop).'''
    device = _hip.require_device() if device is None else torch.device(device)
    return int(tied_log_counter(device))


def tied_lognorm(pool_llh, log_weights, log_count=None):
    '''(pc [T,S], m [T]): pc[t,s] = logsumexp_k(pool_llh[t,k] + log_weights[s,k]) and the row
    maxima of `pool_llh` (`beer_tied_lognorm`).  The log-weights go to the kernels in fp64
    whatever the dtype of `pool_llh` (`Dirichlet.log_weights64`).  `log_count`: optional int64 device scalar,
    += the entries that were redone in log space (include/beer_hip.h).'''
    l = _hip.on_device(pool_llh)
    lw = _hip.on_device(log_weights, torch.float64)
    T, K = l.shape
    S = lw.shape[0]
    if lw.dim() != 2 or lw.shape[1] != K:
        raise ValueError(f'log-weights {tuple(lw.shape)} over a pool of {K} Gaussians')
    if log_count is not None and (log_count.dtype != torch.int64 or not log_count.is_cuda):
        raise TypeError('log_count: an int64 tensor on the GPU')
    pc = torch.empty(T, S, dtype=l.dtype, device=l.device)
    m = torch.empty(T, dtype=l.dtype, device=l.device)
    _hip.call('beer_tied_lognorm', _hip.dtype_code(l.dtype), T, K, S, _hip.ptr(l), _hip.ptr(lw),
              _hip.ptr(pc), _hip.ptr(m), _hip.ptr(log_count))
    return pc, m


def tied_accumulate(pool_llh, m, pc, log_weights, state_resps, counts=None):
    '''(r [T,K], counts [S,K] fp64): with j[t,s,k] = state_resps[t,s] * exp(pool_llh[t,k] +
    log_weights[s,k] - pc[t,s]), r = sum_s j (the pool's responsibilities) and
    counts += sum_t j (`beer_tied_accumulate`); `m`, `pc` as `tied_lognorm` returned them.'''
    l = _hip.on_device(pool_llh)
    lw = _hip.on_device(log_weights, torch.float64)
    T, K = l.shape
    S = lw.shape[0]
    mm, norm = _hip.on_device(m, l.dtype), _hip.on_device(pc, l.dtype)
    g = _hip.on_device(state_resps, l.dtype)
    if tuple(lw.shape) != (S, K) or tuple(mm.shape) != (T,) or tuple(norm.shape) != (T, S) or \
            tuple(g.shape) != (T, S):
        raise ValueError(f'tied accumulation over {T} frames, {S} states, {K} Gaussians: got '
                         f'lw {tuple(lw.shape)}, m {tuple(mm.shape)}, pc {tuple(norm.shape)}, '
                         f'state_resps {tuple(g.shape)}')
    if counts is None:
        counts = torch.zeros(S, K, dtype=torch.float64, device=l.device)
    elif counts.dtype != torch.float64 or tuple(counts.shape) != (S, K) or \
            not counts.is_contiguous():
        raise ValueError(f'counts: contiguous fp64 [{S}, {K}]')
    r = torch.empty(T, K, dtype=l.dtype, device=l.device)
    _hip.call('beer_tied_accumulate', _hip.dtype_code(l.dtype), T, K, S, _hip.ptr(l),
              _hip.ptr(mm), _hip.ptr(norm), _hip.ptr(lw), _hip.ptr(g), _hip.ptr(r),
              _hip.ptr(counts))
    return r, counts


# ---- posterior-predictive (Student-t) densities ------------------------------------------------
# ln of the integral of p(x | theta) q(theta) from the frames and the family's
# `predictive_table()` (include/beer_hip.h, "Posterior-predictive densities").

def _table_dim(table, cov_type):
    'D of a predictive table [K, Q] (Q = the family\'s statistics dimension).'
    Q = table.shape[-1]
    if cov_type == 'diagonal':
        return (Q - 2) // 2
    if cov_type == 'isotropic':
        return Q - 3
    D = int(round((-1 + (1 + 4 * (Q - 2)) ** .5) / 2))
    if D * D + D + 2 != Q:
        raise ValueError(f'a full-covariance predictive table has D^2 + D + 2 columns, not {Q}')
    return D


def predictive_frames(data_or_stats, dim, cov_type):
    '''The `FrameStats` a predictive density is evaluated on: raw frames [T, dim] or the lazy
    statistics of such frames.  Dense [T, Q] statistics (sample averages handed to the prior
    of a VAE), scaled statistics and frames that carry an autograd graph raise
    `NotImplementedError`: the predictive density of averaged or scaled statistics is not
    defined, and it has no gradient kernel.  Checked before any device work.'''
    if isinstance(data_or_stats, FrameStats):
        st = data_or_stats
        if has_source(st):
            raise NotImplementedError('predictive densities are not differentiable w.r.t. the '
                                      'frames: detach them')
        if st.scale != 1.0:
            raise NotImplementedError('predictive densities of scaled statistics are not defined')
        if st.data.shape[1] != dim:
            raise ValueError(f'frames of dimension {st.data.shape[1]} for a model of dimension {dim}')
        return st.as_cov(cov_type)
    X = data_or_stats
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise TypeError('expected frames [T, D] or the statistics returned by '
                        'model.sufficient_statistics(X)')
    if torch.is_grad_enabled() and X.requires_grad:
        raise NotImplementedError('predictive densities are not differentiable w.r.t. the '
                                  'frames: detach them')
    if X.shape[1] != dim:
        raise NotImplementedError(
            f'a [T, {X.shape[1]}] tensor is not frames of dimension {dim}: the predictive density '
            'of dense (sample-averaged) statistics is not defined')
    return FrameStats(X, cov_type)


def predictive_llh(X_or_stats, table, cov_type):
    '''l[t,k] = ln p(x_t | posterior of component k) -> [T, K] (`beer_predictive_llh`);
    `table` [K, Q] from the family's `predictive_table()`.'''
    table = table.view(1, -1) if table.dim() == 1 else table
    st = predictive_frames(X_or_stats, _table_dim(table, cov_type), cov_type)
    X = st.data
    T, D = X.shape
    tab = _hip.on_device(table, X.dtype)
    out = torch.empty(T, tab.shape[0], dtype=X.dtype, device=X.device)
    _hip.call('beer_predictive_llh', _hip.dtype_code(X.dtype), _hip.COV_CODE[cov_type], T, D,
              tab.shape[0], _hip.ptr(X), _hip.ptr(tab), _hip.ptr(out))
    return out


def mixtureset_predictive(stats, table, log_mean_weights, S, G, cov_type):
    '''log_norm [T, S]: ln sum_g exp(log_mean_weights[s,g] + l[t, s G + g]), the predictive
    density of S mixtures of G components (`beer_mixtureset_predictive`; the [T, S G] matrix is
    not formed).  `log_mean_weights` [S, G] = ln E[pi] or None (= 0).'''
    if not isinstance(stats, FrameStats):
        raise NotImplementedError('predictive densities take the lazy statistics of frames '
                                  '(model.sufficient_statistics(X)): the predictive density of '
                                  'dense (sample-averaged) statistics is not defined')
    table = table.view(1, -1) if table.dim() == 1 else table
    if table.shape[0] != S * G:
        raise ValueError(f'{table.shape[0]} table rows for {S} x {G} mixture components')
    st = predictive_frames(stats, _table_dim(table, cov_type), cov_type)
    X = st.data
    T, D = X.shape
    tab = _hip.on_device(table, X.dtype)
    lw = None if log_mean_weights is None else _hip.on_device(log_mean_weights, X.dtype)
    if lw is not None and lw.numel() != S * G:
        raise ValueError(f'{lw.numel()} weights for {S} x {G} mixture components')
    log_norm = torch.empty(T, S, dtype=X.dtype, device=X.device)
    _hip.call('beer_mixtureset_predictive', _hip.dtype_code(X.dtype), _hip.COV_CODE[cov_type], T,
              D, S, G, _hip.ptr(X), _hip.ptr(tab), _hip.ptr(lw), _hip.ptr(log_norm))
    return log_norm


# ---- dense ("stats-in") statistics: the prior of a VAE ------------------------
# beer/models/vae.py:63-89 hands the prior sample-averaged statistics [T, Q]
# and differentiates its expected log-likelihood w.r.t. them.

def cmllr_frame_params(comp_resps, state_resps, exp_stats, S, G, dim, cov_type, out=None):
    '''out [T, P + D + 1] float64 += [omega | nu | c], the posterior-averaged parameters of
    every frame (`beer_cmllr_frame_params`): r[t, k] = comp_resps[t, k] * state_resps[t, k // G]
    as in `normal_accumulate`, `exp_stats` [S*G, Q] the Gaussians' `natural_form()`; P = D
    for diagonal, 1 for isotropic covariances.'''
    given = comp_resps if comp_resps is not None else state_resps
    if given is None:
        raise ValueError('cmllr_frame_params: component or state responsibilities')
    dtype, T, D = given.dtype, given.shape[0], int(dim)
    cr = None if comp_resps is None else _hip.on_device(comp_resps, dtype)
    sr = None if state_resps is None else _hip.on_device(state_resps, dtype)
    E = _hip.on_device(exp_stats, dtype)
    cov = _hip.COV_CODE[cov_type]
    P = D if cov == _hip.DIAG else 1
    if E.shape[0] != S * G or (cr is not None and tuple(cr.shape) != (T, S * G)) or \
            (sr is not None and tuple(sr.shape) != (T, S)):
        raise ValueError(f'cmllr_frame_params: {E.shape[0]} Gaussians, responsibilities '
                         f'{None if cr is None else tuple(cr.shape)} / '
                         f'{None if sr is None else tuple(sr.shape)} for {S} x {G} components')
    if out is None:
        out = torch.zeros(T, P + D + 1, dtype=torch.float64, device=E.device)
    _hip.call('beer_cmllr_frame_params', _hip.dtype_code(dtype), cov, T, D, S, G, _hip.ptr(cr),
              _hip.ptr(sr), _hip.ptr(E), _hip.ptr(out))
    return out


class CmllrTable:
    '''The host-built table of `beer_cmllr_accumulate` (`beer_cmllr_table`): `host` int32
    numpy, `n_items` work items of at most `chunk_frames` frames (0: the library's default),
    `device()` its copy on the GPU.'''

    def __init__(self, host, nutt, n_speakers, chunk_frames):
        self.host, self.nutt, self.n_speakers, self.chunk_frames = host, nutt, n_speakers, chunk_frames
        self.n_items = int(host[0])
        self._dev = None

    def device(self):
        if self._dev is None:
            self._dev = _hip.to_device(torch.from_numpy(self.host))
        return self._dev


def cmllr_table(lengths, speakers, n_speakers, chunk_frames=0):
    '''`CmllrTable` of a ragged batch: `speakers[u]` in -1 .. n_speakers - 1 (-1: the utterance
    is left out).  Host only; a speaker out of range raises `HipInvalid`.'''
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    spk = np.ascontiguousarray(np.asarray(speakers, dtype=np.int64).reshape(-1))
    if len(lens) != len(spk):
        raise ValueError(f'cmllr_table: {len(spk)} speakers for {len(lens)} utterances')
    if len(spk) and (spk.min() < -(1 << 31) or spk.max() >= 1 << 31):
        raise _hip.HipInvalid('beer_cmllr_table failed: invalid argument')
    spk = spk.astype(np.int32)
    n = ctypes.c_size_t(0)
    args = (len(lens), int(n_speakers), ctypes.c_void_p(lens.ctypes.data),
            ctypes.c_void_p(spk.ctypes.data), int(chunk_frames))
    _hip.call_host('beer_cmllr_table', *args, None, ctypes.byref(n))
    host = np.zeros(n.value, dtype=np.int32)
    _hip.call_host('beer_cmllr_table', *args, ctypes.c_void_p(host.ctypes.data), ctypes.byref(n))
    return CmllrTable(host, len(lens), int(n_speakers), int(chunk_frames))


def _frame_offsets(lengths, device):
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)
    return _hip.to_device(off, device)


def cmllr_accumulate(X, params, lengths, speakers, n_speakers, G=None, k=None, beta=None,
                     chunk_frames=0, table=None, frame_off=None):
    '''(G [n, P, E(E+1)/2], k [n, D, E], beta [n]) float64 += the CMLLR statistics of the
    frames X [T, D] of a ragged batch (`beer_cmllr_accumulate`; E = D + 1, the lower triangle
    of G_i packed row by row) with `params` [T, P + D + 1] of `cmllr_frame_params`.
    `chunk_frames`: the frames of a work item (0: the library's default); `table`: the
    `cmllr_table` of the same lengths, speakers and chunk, `frame_off`: the offsets on the
    device, for callers that keep them.'''
    X = _hip.on_device(X)
    T, D = X.shape
    prm = _hip.on_device(params, torch.float64)
    P = prm.shape[1] - D - 1
    if prm.shape[0] != T or sum(lengths) != T:
        raise ValueError(f'cmllr_accumulate: {T} frames, parameters of {prm.shape[0]}, '
                         f'utterances of {sum(lengths)}')
    if table is None:
        table = cmllr_table(lengths, speakers, n_speakers, chunk_frames)
    n, E = int(n_speakers), D + 1
    if P in (1, D):
        shapes = ((n, P, E * (E + 1) // 2), (n, D, E), (n,))
        G, k, beta = (torch.zeros(s, dtype=torch.float64, device=X.device) if t is None else t
                      for s, t in zip(shapes, (G, k, beta)))
        if any(tuple(t.shape) != s or t.dtype != torch.float64 or not t.is_contiguous()
               for s, t in zip(shapes, (G, k, beta))):
            raise ValueError(f'cmllr_accumulate: float64 statistics of shapes {shapes}')
    ws, ws_bytes = _hip.scratch(('cmllr', D, P), _hip.lib().beer_cmllr_workspace_bytes(
        D, P, table.n_items), X.device)
    if frame_off is None:
        frame_off = _frame_offsets(lengths, X.device)
    _hip.call('beer_cmllr_accumulate', _hip.dtype_code(X.dtype), T, D, P, table.nutt, n,
              _hip.ptr(X), _hip.ptr(prm), _hip.ptr(frame_off),
              ctypes.c_void_p(table.host.ctypes.data), _hip.ptr(table.device()), len(table.host),
              table.chunk_frames, _hip.ptr(G), _hip.ptr(k), _hip.ptr(beta), _hip.ptr(ws), ws_bytes)
    return G, k, beta


def cmllr_apply(X, W, lengths, speakers):
    '''Y[t] = A_s x_t + b_s over a ragged batch (`beer_cmllr_apply`): W [n, D, D + 1] float64,
    `speakers[u]` the transform of utterance u, -1 to copy its frames.  Computed in float64,
    returned in the frames' dtype.'''
    X = _hip.on_device(X)
    T, D = X.shape
    W = _hip.on_device(W, torch.float64)
    if W.dim() != 3 or tuple(W.shape[1:]) != (D, D + 1):
        raise ValueError(f'cmllr_apply: transforms {tuple(W.shape)} for frames of dimension {D}')
    spk = np.ascontiguousarray(np.asarray(speakers, dtype=np.int64).reshape(-1))
    if len(spk) != len(lengths) or sum(lengths) != T:
        raise ValueError(f'cmllr_apply: {len(spk)} speakers, {len(lengths)} utterances of '
                         f'{sum(lengths)} frames for {T} frames')
    if len(spk) and (spk.min() < -1 or spk.max() >= W.shape[0]):
        raise _hip.HipInvalid('beer_cmllr_apply failed: invalid argument')
    spk = spk.astype(np.int32)
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)
    up = _hip.upload({'off': off, 'spk': torch.from_numpy(spk)}, X.device)
    Y = torch.empty_like(X)
    _hip.call('beer_cmllr_apply', _hip.dtype_code(X.dtype), T, D, len(lengths), W.shape[0],
              _hip.ptr(X), _hip.ptr(W), _hip.ptr(up['off']), _hip.ptr(up['spk']),
              ctypes.c_void_p(spk.ctypes.data), _hip.ptr(Y))
    return Y


def _dense(stats, dtype=None):
    return _hip.on_device(stats.detach(), dtype)


def dense_llh(stats, exp_stats, dim):
    'stats @ E[T]^T - dim/2 ln 2pi -> [T, K] (no autograd graph).'
    st = _dense(stats)
    E = _hip.on_device(exp_stats, st.dtype)
    T, Q = st.shape
    if E.shape[1] != Q:
        raise ValueError(f'statistics of dimension {Q} for parameters of dimension {E.shape[1]}')
    out = torch.empty(T, E.shape[0], dtype=st.dtype, device=st.device)
    _hip.call('beer_dense_llh', _hip.dtype_code(st.dtype), T, Q, E.shape[0], _hip.ptr(st),
              _hip.ptr(E), -.5 * dim * LOG_2PI, _hip.ptr(out))
    return out


def dense_softmax(pc_llh, log_weights, S, G, want_resps=True):
    '(log_norm [T,S], resps [T,S*G]) of pc_llh [T,S*G] + log_weights [S,G].'
    pc = _hip.on_device(pc_llh)
    T = pc.shape[0]
    lw = None if log_weights is None else _hip.on_device(log_weights, pc.dtype)
    log_norm = torch.empty(T, S, dtype=pc.dtype, device=pc.device)
    resps = torch.empty(T, S * G, dtype=pc.dtype, device=pc.device) if want_resps else None
    _hip.call('beer_softmax_groups', _hip.dtype_code(pc.dtype), T, S, G, _hip.ptr(pc),
              _hip.ptr(lw), _hip.ptr(log_norm), _hip.ptr(resps))
    return log_norm, resps


def rowdot(a, b):
    'sum_k a[t,k] b[t,k] -> [T].'
    a = _hip.on_device(a)
    b = _hip.on_device(b, a.dtype)
    out = torch.empty(a.shape[0], dtype=a.dtype, device=a.device)
    _hip.call('beer_rowdot', _hip.dtype_code(a.dtype), a.shape[0], a.shape[1], _hip.ptr(a),
              _hip.ptr(b), _hip.ptr(out))
    return out


def dense_accumulate(stats, comp_resps, state_resps, S, G, acc=None):
    'acc[k,:] += sum_t comp_resps[t,k] state_resps[t,k//G] stats[t,:], fp64 [S*G, Q].'
    st = _dense(stats)
    T, Q = st.shape
    K = S * G
    if acc is None:
        acc = torch.zeros(K, Q, dtype=torch.float64, device=st.device)
    if comp_resps is None:
        comp_resps, state_resps, G = state_resps, None, 1
    if comp_resps is None:
        comp_resps = torch.ones(T, K, dtype=st.dtype, device=st.device)
    # the library reads K columns of the weights and K / G of the state posteriors
    if tuple(comp_resps.shape) != (T, K) or \
            (state_resps is not None and tuple(state_resps.shape) != (T, K // G)):
        raise ValueError(f'weights {tuple(comp_resps.shape)} / state posteriors '
                         f'{None if state_resps is None else tuple(state_resps.shape)} for '
                         f'{T} frames, {S} x {G} components')
    if tuple(acc.shape) != (K, Q):
        raise ValueError(f'accumulator {tuple(acc.shape)} for {K} components of {Q} statistics')
    cr = _hip.on_device(comp_resps.detach(), st.dtype)
    sr = None if state_resps is None else _hip.on_device(state_resps.detach(), st.dtype)
    _hip.call('beer_dense_accumulate', _hip.dtype_code(st.dtype), T, K, Q, G, _hip.ptr(cr),
              _hip.ptr(sr), _hip.ptr(st), _hip.ptr(acc))
    return acc


def _llh_backward(weights, grad, exp_stats):
    w = _hip.on_device(weights)
    E = _hip.on_device(exp_stats, w.dtype)
    g = None if grad is None else _hip.on_device(grad, w.dtype)
    out = torch.empty(w.shape[0], E.shape[1], dtype=w.dtype, device=w.device)
    _hip.call('beer_dense_llh_backward', _hip.dtype_code(w.dtype), w.shape[0], w.shape[1],
              E.shape[1], _hip.ptr(w), _hip.ptr(g), _hip.ptr(E), _hip.ptr(out))
    return out


class _StatsGrad(torch.autograd.Function):
    """value[t] = sum_k weights[t,k] llh[t,k] (+ terms without gradient), with
    d value[t] / d stats[t] = sum_k weights[t,k] E[T]_k: what the reference's
    autograd derives for `(pc_llhs * resps).sum(-1)` with detached resps
    (mixture.py:79,92; hmm.py:81-87)."""

    @staticmethod
    def forward(ctx, stats, value, weights, exp_stats):
        ctx.save_for_backward(weights, exp_stats)
        ctx.home = (stats.device, stats.dtype)
        return value.clone()

    @staticmethod
    def backward(ctx, grad):
        weights, exp_stats = ctx.saved_tensors
        out = _llh_backward(weights, grad.contiguous(), exp_stats)
        return out.to(device=ctx.home[0], dtype=ctx.home[1]), None, None, None


def attach_stats_grad(stats, value, weights, exp_stats):
    'Give `value` [T] its gradient w.r.t. dense `stats` (no-op without grad).'
    if not (torch.is_grad_enabled() and stats.requires_grad):
        return value
    return _StatsGrad.apply(stats, value, weights.detach(), exp_stats.detach())


class _DenseLlh(torch.autograd.Function):
    'Differentiable stats @ E[T]^T + base -> [T, K].'

    @staticmethod
    def forward(ctx, stats, exp_stats, dim):
        ctx.save_for_backward(exp_stats)
        ctx.home = (stats.device, stats.dtype)
        return dense_llh(stats, exp_stats, dim)

    @staticmethod
    def backward(ctx, grad):
        exp_stats, = ctx.saved_tensors
        out = _llh_backward(grad.contiguous(), None, exp_stats)
        return out.to(device=ctx.home[0], dtype=ctx.home[1]), None, None


def dense_llh_autograd(stats, exp_stats, dim):
    if torch.is_grad_enabled() and stats.requires_grad:
        return _DenseLlh.apply(stats, exp_stats.detach(), dim)
    return dense_llh(stats, exp_stats, dim)


class _SuffStats(torch.autograd.Function):
    '''Mean over `ns` consecutive rows of phi(X) as a dense [T, Q] tensor,
    differentiable w.r.t. the frames [T * ns, D].'''

    @staticmethod
    def forward(ctx, data, cov_type, ns):
        X = _hip.on_device(data.detach())
        ctx.save_for_backward(X)
        ctx.cov_type, ctx.ns = cov_type, ns
        ctx.home = (data.device, data.dtype)
        T, D = X.shape[0] // ns, X.shape[1]
        Q = FrameStats(X[:1], cov_type).shape[1]
        out = torch.empty(T, Q, dtype=X.dtype, device=X.device)
        _hip.call('beer_suffstats_mean', _hip.dtype_code(X.dtype), _hip.COV_CODE[cov_type],
                  T, ns, D, _hip.ptr(X), _hip.ptr(out))
        return out

    @staticmethod
    def backward(ctx, grad):
        X, = ctx.saved_tensors
        g = _hip.on_device(grad, X.dtype)
        out = torch.empty_like(X)
        _hip.call('beer_suffstats_backward', _hip.dtype_code(X.dtype),
                  _hip.COV_CODE[ctx.cov_type], X.shape[0] // ctx.ns, ctx.ns, X.shape[1],
                  _hip.ptr(X), _hip.ptr(g), _hip.ptr(out))
        return out.to(device=ctx.home[0], dtype=ctx.home[1]), None, None


def differentiable_stats(data, cov_type, nsamples=1):
    '''Dense statistics carrying the autograd graph of `data` [T * nsamples,
    D]: phi(X) for nsamples = 1, else the mean of phi over each run of
    `nsamples` rows -> [T, Q] (vae.py:73-74 without the [T*ns, Q] tensor).'''
    if data.dim() != 2 or data.shape[0] % nsamples:
        raise ValueError('expected [n_frames * nsamples, dim] samples')
    return _SuffStats.apply(data, cov_type, int(nsamples))


# ---- one sample per frame: the prior of a VAE on the frame kernels --------------
# With nsamples = 1 the statistics a VAE hands its prior (vae.py:73-74) are phi(z_t) of the
# samples themselves: the prior runs its frame kernels on them -- no [T, Q] tensor -- and the
# gradient w.r.t. the samples is one product (csrc/sample_grad.hip).

def sample_stats(data, cov_type):
    """Lazy statistics of frames that carry an autograd graph: a `FrameStats` of their
    values whose `source` is the differentiable tensor.  Models that find a `source` give
    their expected log-likelihood its gradient w.r.t. it (`attach_frame_grad`)."""
    if data.dim() != 2:
        raise ValueError('expected [n_frames, dim] samples')
    st = FrameStats(data.detach(), cov_type)
    if torch.is_grad_enabled() and data.requires_grad:
        st.source = data
    return st


def has_source(stats):
    return isinstance(stats, FrameStats) and stats.source is not None and \
        torch.is_grad_enabled() and stats.source.requires_grad


def frames_llh_backward(stats, weights, grad, exp_stats):
    """grad[t] * sum_k weights[t,k] * d l_k(x_t) / d x_t -> [T, D]
    (`beer_frames_llh_backward`; `grad` None = 1)."""
    st = _frames(stats)
    X = st.data
    T, D = X.shape
    w = _hip.on_device(weights, X.dtype)
    E = _hip.on_device(exp_stats, X.dtype)
    g = None if grad is None else _hip.on_device(grad, X.dtype)
    K = E.shape[0]
    if tuple(w.shape) != (T, K) or E.shape[1] != st.shape[1]:
        raise ValueError(f'weights {tuple(w.shape)} / parameters {tuple(E.shape)} for '
                         f'{T} frames of dimension {D}')
    out = torch.empty_like(X)
    code, cov = _hip.dtype_code(X.dtype), _hip.COV_CODE[st.cov_type]
    nbytes = _hip.lib().beer_frames_llh_backward_workspace_bytes(code, cov, T, D, K)
    if X.dtype == torch.float32 and _hip.get_f32_mode() == 'exact':
        # the matrix-core kernels of this call are bf16x3; without a workspace the library
        # runs its thread-per-output kernel (float64 accumulation): exact, and slow
        nbytes = 0
    ws, nbytes = _hip.scratch(('sgrad', cov, D, K), nbytes, X.device)
    _hip.call('beer_frames_llh_backward', code, cov, T, D, K, _hip.ptr(X), _hip.ptr(w),
              _hip.ptr(g), _hip.ptr(E), _hip.ptr(out), _hip.ptr(ws), nbytes)
    if st.scale != 1.0:
        out *= st.scale
    return out


class _FrameGrad(torch.autograd.Function):
    """`_StatsGrad` for statistics that are phi(x_t) of differentiable frames: value[t] =
    sum_k weights[t,k] llh[t,k] (+ terms without gradient) differentiated w.r.t. the
    frames, the chain statistics -> frames included."""

    @staticmethod
    def forward(ctx, source, value, weights, exp_stats, stats):
        ctx.save_for_backward(weights, exp_stats)
        ctx.stats = stats
        ctx.home = (source.device, source.dtype)
        return value.clone()

    @staticmethod
    def backward(ctx, grad):
        weights, exp_stats = ctx.saved_tensors
        out = frames_llh_backward(ctx.stats, weights, grad.contiguous(), exp_stats)
        return out.to(device=ctx.home[0], dtype=ctx.home[1]), None, None, None, None


def attach_frame_grad(stats, value, weights, exp_stats):
    'Give `value` [T] its gradient w.r.t. the source of `stats` (no-op without one).'
    if not has_source(stats):
        return value
    return _FrameGrad.apply(stats.source, value, weights.detach(), exp_stats.detach(),
                            stats.detach())


class _FrameLlh(torch.autograd.Function):
    'Differentiable l[t,k] = phi(x_t) . E[T]_k + base -> [T, K] w.r.t. the frames.'

    @staticmethod
    def forward(ctx, source, exp_stats, stats):
        ctx.save_for_backward(exp_stats)
        ctx.stats = stats
        ctx.home = (source.device, source.dtype)
        return normal_llh(stats, exp_stats, stats.cov_type)

    @staticmethod
    def backward(ctx, grad):
        exp_stats, = ctx.saved_tensors
        out = frames_llh_backward(ctx.stats, grad.contiguous(), None, exp_stats)
        return out.to(device=ctx.home[0], dtype=ctx.home[1]), None, None


def normal_llh_autograd(stats, exp_stats, cov_type):
    '`normal_llh`, differentiable w.r.t. the source of `stats` when it has one.'
    if has_source(stats):
        return _FrameLlh.apply(stats.source, exp_stats.detach(), stats.detach())
    return normal_llh(stats, exp_stats, cov_type)


# ---------------------------------------------------------------------------
# token sequences (csrc/editdist.hip)

def _ragged(what, start, lens, n_sym):
    """`start` / `lens` of a packed batch of sequences as (int64, int32) device tensors, checked
    on the host against the `n_sym` packed symbols; and the lengths on the host."""
    lens_h = torch.as_tensor(lens).detach().cpu().to(torch.int64).reshape(-1)
    start_h = torch.as_tensor(start).detach().cpu().to(torch.int64).reshape(-1)
    if lens_h.numel() != start_h.numel():
        raise ValueError(f'{what}: {start_h.numel()} starts for {lens_h.numel()} lengths')
    if lens_h.numel() and (int(lens_h.min()) < 0 or int(start_h.min()) < 0 or
                           int((start_h + lens_h).max()) > n_sym):
        raise ValueError(f'{what}: a sequence lies outside the {n_sym} packed symbols')
    dev = _hip.require_device()
    return start_h.to(dev), lens_h.to(torch.int32).to(dev), lens_h


def unit_sequences(paths, start, lens, unit_of_pdf, per_frame=False):
    """Packed pdf-id paths as unit sequences (`beer_unit_sequences`): (units int32 as long as
    `paths` -- the units of sequence q compactly at units[start[q]:start[q] + n_units[q]] --,
    n_units int32 [n_seq], frame_unit int32 as long as `paths` or None).  `paths`: int64, packed;
    `unit_of_pdf`: int32 [n_pdf], a unit's index at its first pdf and -1 elsewhere.
    n_units: 0 for an empty sequence, -1 for one that begins with a negative symbol (an n-best
    rank without a path), -2 for one with a pdf outside the table or a first pdf inside a unit."""
    paths = _hip.on_device(torch.as_tensor(paths), torch.int64).reshape(-1)
    table = _hip.on_device(torch.as_tensor(unit_of_pdf), torch.int32).reshape(-1)
    if table.numel() < 1:
        raise ValueError('unit_sequences: an empty pdf table')
    start, lens, _ = _ragged('unit_sequences', start, lens, paths.numel())
    dev = paths.device
    units = torch.empty(paths.numel(), dtype=torch.int32, device=dev)
    n_units = torch.empty(lens.numel(), dtype=torch.int32, device=dev)
    frames = torch.empty(paths.numel(), dtype=torch.int32, device=dev) if per_frame else None
    _hip.call('beer_unit_sequences', _hip.ptr(paths), _hip.ptr(start), _hip.ptr(lens),
              lens.numel(), _hip.ptr(table), table.numel(), _hip.ptr(units), _hip.ptr(n_units),
              _hip.ptr(frames))
    return units, n_units, frames


def edit_distance_route(max_short, max_long, ops=False):
    """beer_edit_distance_route: the form `beer_edit_distance` takes for pairs whose shorter side
    has up to `max_short` symbols and whose longer side up to `max_long` (team size, cell type,
    where a strip's boundary row waits).  HipInvalid where C refuses."""
    route = _hip.lib().beer_edit_distance_route(int(max_short), int(max_long), int(bool(ops)))
    if route == _hip.EINVAL:
        raise _hip.HipInvalid(
            f'edit_distance: sequences of {int(max_short)} x {int(max_long)} symbols: at most '
            f'{_hip.EDIT_MAX_LEN_OPS if ops else _hip.EDIT_MAX_LEN}' + (' with ops' if ops else ''))
    return route


def edit_distance_launch(sym, start, lens, pair_a, pair_b, max_short, max_long, dist, ops=None,
                         workspace=None):
    """One `beer_edit_distance` call on tensors that are already int32 / int64 on the device
    (`dist` [n_pair], `ops` [n_pair, 3] or None are written); `workspace`: a uint8 tensor of at
    least `beer_edit_distance_scratch_bytes`, by default the call's kept scratch."""
    n_pair = pair_a.numel()
    edit_distance_route(max_short, max_long, ops is not None)
    need = _hip.lib().beer_edit_distance_scratch_bytes(n_pair, int(max_short), int(max_long),
                                                       int(ops is not None))
    if workspace is None:
        workspace, _ = _hip.scratch('beer_edit_distance', need, sym.device)
    _hip.call('beer_edit_distance', _hip.ptr(sym), _hip.ptr(start), _hip.ptr(lens), lens.numel(),
              _hip.ptr(pair_a), _hip.ptr(pair_b), n_pair, int(max_short), int(max_long),
              _hip.ptr(dist), _hip.ptr(ops), _hip.ptr(workspace),
              0 if workspace is None else workspace.numel())


# the shorter side's length classes: a team of 8 / 16 / 32 / 64 lanes in one strip, then strips
_EDIT_CLASSES = (8, 16, 32, 64)


def edit_distance(sym, start, lens, pair_a, pair_b, ops=False):
    """Levenshtein distances of pairs of packed int32 sequences (`beer_edit_distance`): int32
    [n_pair] on the device, with `ops` also int32 [n_pair, 3], the (substitutions, deletions,
    insertions) of the cheapest alignment with the smallest such triple; a deletion consumes a
    symbol of sequence `pair_a[p]` alone.
    The pairs are launched by the form their shorter side asks for (a team of 8 / 16 / 32 / 64
    lanes; strips beyond 64 symbols), each class ordered by
    len_a * len_b, largest first, so that the teams of a wave finish together; the results come
    back in the caller's order.  ValueError: a pair index outside the sequences (checked on the
    host, before any device work)."""
    sym = _hip.on_device(torch.as_tensor(sym), torch.int32).reshape(-1)
    start, lens, lens_h = _ragged('edit_distance', start, lens, sym.numel())
    dev = sym.device
    pairs = []
    for what, idx in (('pair_a', pair_a), ('pair_b', pair_b)):
        idx = torch.as_tensor(idx).reshape(-1)
        if idx.numel() == 0:
            idx = idx.to(torch.int32)
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise ValueError(f'edit_distance: {what} must be integers, not {idx.dtype}')
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= lens.numel()):
            raise ValueError(f'edit_distance: {what} outside [0, {lens.numel()}): '
                             f'{int(idx.min())} .. {int(idx.max())}')
        pairs.append(_hip.on_device(idx, torch.int32))
    pair_a, pair_b = pairs
    if pair_a.numel() != pair_b.numel():
        raise ValueError(f'edit_distance: {pair_a.numel()} and {pair_b.numel()} pair indices')
    n_pair = pair_a.numel()
    dist = torch.empty(n_pair, dtype=torch.int32, device=dev)
    moves = torch.empty(n_pair, 3, dtype=torch.int32, device=dev) if ops else None
    if n_pair == 0:
        return (dist, moves) if ops else dist
    wide = lens.to(torch.int64)
    la, lb = wide[pair_a.long()], wide[pair_b.long()]
    short, long_ = torch.minimum(la, lb), torch.maximum(la, lb)
    team = torch.bucketize(short, torch.tensor(_EDIT_CLASSES, device=dev))
    # by class, then by the size of the table, largest first (stable: equal pairs keep their order)
    order = torch.argsort(short * long_, descending=True, stable=True)
    order = order[torch.argsort(team[order], stable=True)]
    counts = torch.bincount(team, minlength=len(_EDIT_CLASSES) + 1)
    tops = torch.stack([torch.stack([torch.where(team == c, v, torch.zeros_like(v)).max()
                                     for v in (short, long_)]) for c in range(len(_EDIT_CLASSES) + 1)])
    counts, tops = counts.tolist(), tops.tolist()
    a_sorted, b_sorted = pair_a[order].contiguous(), pair_b[order].contiguous()
    d_sorted = torch.empty_like(dist)
    m_sorted = torch.empty_like(moves) if ops else None
    lo = 0
    for c, n in enumerate(counts):
        if n:
            edit_distance_launch(sym, start, lens, a_sorted[lo:lo + n], b_sorted[lo:lo + n],
                                 tops[c][0], tops[c][1], d_sorted[lo:lo + n],
                                 m_sorted[lo:lo + n] if ops else None)
        lo += n
    dist[order] = d_sorted
    if ops:
        moves[order] = m_sorted
    return (dist, moves) if ops else dist
