"""Every launch form of the kernels behind a VAE's prior (csrc/dense.hip: `beer_dense_llh`,
`beer_dense_llh_backward`, `beer_dense_accumulate`, `beer_rowdot`, `beer_softmax_groups`,
`beer_suffstats_mean`, `beer_suffstats_backward`; csrc/sample_grad.hip: `beer_frames_llh_backward`)
against the float64 oracle at the smallest shapes that reach it (tests/vae_prior_truth.py).

Static tables: each row names the form the launchers must pick for it (`beer_dense_route`,
`beer_frames_llh_backward_route`), and its test first holds the C layer's answer against the table,
then calls the C entry point itself through `_hip.call` with exactly the advertised workspace.
Outputs are pre-filled with NaN; two guard rows behind every output and 256 guard bytes behind the
workspace must keep their bits; every case is also called with T = 0 (the gradient with the
workspace of its longest call), which returns OK and writes nothing; `beer_dense_accumulate`
starts from a non-zero accumulator and must add to it.

Bounds, per element, with s the error scale of tests/vae_prior_truth.py (the expression in
absolute values) and n its inner length; the whole-output bound of tests/test_gpu_vae.py (float64
1e-12, float32 2e-6 of max |truth|) stays as a ceiling:

* float64 forms: |err| <= (n + 2) 2^-53 s, a dot product in any order;
* float32 on `gemm_kernel`, `sgrad_generic_kernel`, the statistics kernels, `rowdot_kernel`
  (float64 accumulation, one rounding): |err| <= 2^-24 |truth| + (n + 2) 2^-53 s;
* the accumulation adds to an accumulator of eighths (at most 7/8) with up to T / 16 + 2 atomics
  per element, each rounding the accumulator: + (T / 16 + 2) 2^-53 (7/8 + |truth|);
* the chunked gradient in float32 stores the [frames, Q] gradient of the statistics in float32
  between its two steps: + 2^-24 s; where a chunk reaches `gemm3_kernel`: + C['g3bwd'] s;
* `softmax_groups_kernel` (float64 inside): log-normalisers and responsibilities within
  (G + 16) 2^-53 max(1, max |logit|) -- the rounding of logit - max at the size of the logits, G
  exponentials of a few ulp each, one logarithm -- + 2^-24 |truth| in float32;
* the bf16x3 forms (`gemm3_kernel`, `sgrad_kernel`, `sgrad_diag_kernel`): the accumulator of the
  matrix core truncates and how often that bites depends on the data, so no bound follows from
  the code.  Each case meets 2e-6 max |truth|, and per element |err| <= c s with c per family at
  twice the worst ratio observed on an MI355X (the factor two: the order of the atomics, seeds).

Worst errors observed on an MI355X as a fraction of the bound (the module prints them at its end,
`pytest -s`): float64 0.42 on `gemm_kernel`, 0.66 on the statistics kernels, 0.26 chunked, 0.19
generic, 0.07 softmax, 0.03 `rowdot`; float32 on the float64-accumulating kernels 1.00 (a result
rounded to nearest sits half an ulp off: the bound is met with equality) and 0.96 chunked.  The
bf16x3 families, |err| / s: `gemm3_kernel` llh 2.98e-7, backward 3.84e-7, accumulate 2.46e-8 (the
split search gives these shapes chains of 32 to 64 frames), the long chain (4096 frames) 1.62e-6;
`sgrad_kernel<1>` 2.65e-7, `<2>` 4.19e-7; `sgrad_diag_kernel` 3.78e-7.  The c chosen from them: `C`
below: the worst case of a family sits at half its bound by construction, the long chain at 0.81
(see there).
"""

from collections import namedtuple

import numpy as np
import pytest
import torch

import estep_truth as et
import vae_prior_truth as vt

pytestmark = pytest.mark.gpu

from beer_amd import _hip                                            # noqa: E402
from gpu_helpers import DEV, npy, tt                                 # noqa: E402

NP_OF = {'f64': np.float64, 'f32': np.float32}
TORCH_OF = {'f64': torch.float64, 'f32': torch.float32}
CODE_OF = {'f64': _hip.F64, 'f32': _hip.F32}
CEILING = {'f64': 1e-12, 'f32': 2e-6}
GUARD = 256
GUARD_VALUE = 7.25
BASE = -7.25
LLH, BWD, ACC = _hip.DENSE_LLH, _hip.DENSE_BACKWARD, _hip.DENSE_ACCUMULATE
OP_NAME = {LLH: 'llh', BWD: 'bwd', ACC: 'acc'}

# c of |err| <= c s for the bf16x3 families: twice the worst |err| / s observed on an MI355X (in
# the comment, with its case).  The float32 sums of a workgroup do not depend on the order of the
# fp64 atomics, which moves a result by 1e-16 of it only.
C = {
    'g3llh': 6.0e-7,     # 2.98e-7  llh Q = 515, K = 129, T = 8192
    'g3bwd': 7.7e-7,     # 3.84e-7  backward Q = 513, K = 65, T = 8192, signed weights and factor
    'g3acc': 5.0e-8,     # 2.46e-8  accumulate Q = 513, 65 x 1 with state posteriors, T = 8193 (chains of 32 .. 64)
    'sg1': 5.3e-7,       # 2.65e-7  full D = 32, K = 1, T = 4096
    'sg2': 8.4e-7,       # 4.19e-7  full D = 64, K = 1, T = 4096
    'sd': 7.6e-7,        # 3.78e-7  diagonal D = 128, K = 65, T = 4096, factor
    # the long chain, on its own: 1.62e-6 observed, so twice that would be 3.2e-6 -- above the
    # project's 2e-6, which is therefore kept as it is: the case passes at 0.81 of it, not at half.
    # Not the drift dense.hip warns of (the mean relative error is -8.9e-8, extremes -1.62e-6 and
    # +1.38e-6 over 2 M sums): a chain of 4096 frames is 768 accumulations into a float32
    # accumulator, which reads as a random walk of about 3e-7 whose largest of 2 M draws lands
    # there -- an explanation from this one shape, not a bound; only the extremes are asserted.
    # The data and the chain sums are deterministic: the figure does not move from run to run.
    'g3long': 2e-6,
}

WORST, RAW = {}, {}


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    for fam, (frac, cid) in sorted(WORST.items()):
        print(f'\nworst error / bound, {fam}: {frac:.3f} ({cid})', end='')
    for fam, (ratio, cid) in sorted(RAW.items()):
        print(f'\nworst |err| / s, {fam}: {ratio:.3e} ({cid})', end='')
    print()


# --- buffers and the check -----------------------------------------------------------------------

def guarded(nbytes):
    'A buffer of `nbytes` of NaN (all bits set) with a guard behind it.'
    buf = torch.full((nbytes + GUARD,), 0xff, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = torch.arange(GUARD, dtype=torch.uint8, device=DEV)
    return buf


def guard_kept(buf, nbytes):
    return bool((buf[nbytes:] == torch.arange(GUARD, dtype=torch.uint8, device=DEV)).all())


def output(rows, cols, arith):
    'An output [rows, cols] of NaN with two guard rows behind it.'
    out = torch.full((rows + 2, cols), float('nan'), dtype=TORCH_OF[arith], device=DEV)
    out[rows:] = GUARD_VALUE
    return out


def taken(out, rows, T, what):
    'The rows of an output after the call: guard rows kept, nothing written at T = 0.'
    torch.cuda.synchronize()
    assert bool((out[rows:] == GUARD_VALUE).all()), f'{what}: guard rows'
    if T == 0:
        assert bool(torch.isnan(out[:rows]).all()), f'{what}: T = 0 wrote'
        return None
    return npy(out[:rows]).astype(np.float64)


def hold(fam, what, got, truth, s, n, arith, bf16x3=False, extra=0.):
    '''The per-element bound of the module docstring and the whole-output ceiling; `extra` is
    added to the bound (array or scalar).  Records the worst fraction per family.'''
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert np.isfinite(got).all(), f'{what}: not finite'
    err = np.abs(got - truth)
    if bf16x3:
        bound = C[fam] * s + extra
        with np.errstate(divide='ignore', invalid='ignore'):
            raw = float(np.where(s > 0, err / s, 0.).max())
        if raw > RAW.get(fam, (0., ''))[0]:
            RAW[fam] = (raw, what)
    else:
        bound = (n + 2) * 2. ** -53 * s + extra
        if arith == 'f32':
            bound = bound + 2. ** -24 * np.abs(truth)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.))
    worst = float(frac.max()) if frac.size else 0.
    if worst > WORST.get(fam, (0., ''))[0]:
        WORST[fam] = (worst, what)
    i = np.unravel_index(np.argmax(frac), frac.shape) if frac.size else ()
    assert worst <= 1., f'{what}: |err| = {err[i]:.3e} at {i} is {worst:.3f} x its bound {np.broadcast_to(bound, err.shape)[i]:.3e}'
    top = np.abs(truth).max() if truth.size else 0.
    assert err.max() <= CEILING[arith] * top, f'{what}: max |err| {err.max():.3e} > {CEILING[arith]:.0e} x {top:.3e}'


# =================================================================================================
# The dense products
# =================================================================================================

def dense_value(spec):
    '''`beer_dense_route` of a form written 'p' (gemm_kernel) or '3:MxN[.ak][.bk]' (gemm3_kernel
    with its tile and contiguity flags), the chain length left out.'''
    if spec == 'p':
        return _hip.DENSE_PLAIN
    tile, *flags = spec[2:].split('.')
    r = _hip.DENSE_GEMM3 | {'64x128': _hip.DENSE_T64x128, '128x64': _hip.DENSE_T128x64,
                            '128x128': _hip.DENSE_T128x128}[tile]
    return r | (_hip.DENSE_AK if 'ak' in flags else 0) | (_hip.DENSE_BK if 'bk' in flags else 0)


def dense_route(c, T):
    'The query with the chain length masked off.'
    r = _hip.dense_route(c.op, CODE_OF[c.arith], T, c.Q, c.S * c.G)
    return r if r < 0 else r & ~0xFF00


# op, arithmetic, the frame counts, Q, S, G (K = S G components), state posteriors given, form
D = namedtuple('D', 'op arith ts Q S G sr form')
PLAIN_TS = (0, 1, 15, 16, 17, 63, 64, 65, 300)
PLAIN_ACC_TS = (0, 1, 17, 64, 65, 255, 256, 257, 300, 1000)
PLAIN_QK = ((1, 130), (3, 65), (15, 64), (16, 63), (17, 17), (63, 16), (64, 15), (65, 3), (130, 1))
PLAIN_ACC_SETS = ((17, 16, 4), (65, 4, 16), (130, 3, 1), (3, 1, 16), (64, 5, 4), (1, 65, 1))    # Q, S, G
G3_TS = (8192, 8193, 8192 + 127)
G3_ACC_TS = (8192, 8193, 8192 + 33)
G3_ACC_SETS = ((1, 1), (64, 1), (16, 4), (65, 1), (24, 4), (7, 16))

DENSE_CASES = (
    [D(op, a, PLAIN_TS, Q, K, 1, False, 'p') for op in (LLH, BWD, ACC) for a in ('f64', 'f32')
     for Q, K in PLAIN_QK] +
    [D(ACC, a, PLAIN_ACC_TS, Q, S, G, sr, 'p') for a in ('f64', 'f32') for Q, S, G in PLAIN_ACC_SETS
     for sr in (True, False)] +
    # just under each threshold: the plain kernel (and float64 above both: the plain kernel)
    [D(op, 'f32', (T,), Q, 17, 1, False, 'p') for op in (LLH, BWD, ACC) for T, Q in ((8191, 512), (8192, 511))] +
    [D(op, 'f64', (8192,), 512, 17, 1, False, 'p') for op in (LLH, BWD, ACC)] +
    [D(LLH, 'f32', G3_TS, Q, K, 1, False, '3:128x64.ak.bk' if K <= 64 else '3:128x128.ak.bk')
     for Q in (512, 513, 515, 543) for K in (1, 17, 64, 65, 129)] +
    [D(BWD, 'f32', G3_TS, Q, K, 1, False, '3:128x128.ak') for Q in (512, 513, 514, 515, 641)
     for K in (1, 31, 32, 33, 65)] +
    [D(ACC, 'f32', G3_ACC_TS, Q, S, G, sr, '3:64x128' if S * G <= 64 else '3:128x128')
     for Q in (512, 513, 543) for S, G in G3_ACC_SETS for sr in (True, False)])


def dense_id(c):
    return f"{OP_NAME[c.op]}-{c.arith}-Q{c.Q}-{c.S}x{c.G}{'-sr' if c.sr else ''}-T{c.ts[-1]}-{c.form}"


def dense_seed(c):
    return 2000 + 7 * c.Q + 131 * c.S + c.G + 3 * c.op


def dense_family(c):
    if c.form == 'p':
        return 'gemm' + c.arith[1:]
    return 'g3' + OP_NAME[c.op]


def run_dense(c, inp, T):
    'The case on its first T frames: list of (what, got, truth, s, n, extra).'
    K, n, code = c.S * c.G, max(T, 1), CODE_OF[c.arith]
    assert dense_route(c, T) == dense_value(c.form if T else 'p'), (dense_id(c), T, hex(dense_route(c, T)))
    st, E = tt(inp['st'][:n]), tt(inp['E'])
    if c.op == LLH:
        out = output(n, K, c.arith)
        _hip.call('beer_dense_llh', code, T, c.Q, K, _hip.ptr(st), _hip.ptr(E), BASE, _hip.ptr(out))
        got = taken(out, n, T, dense_id(c))
        return [] if T == 0 else [('llh', got) + vt.llh(inp['st'][:T], inp['E'], BASE) + (0.,)]
    if c.op == BWD:
        res = []
        for name, w, g in (('signed weights, factor', inp['ws'], inp['g']), ('signed weights', inp['ws'], None),
                           ('posteriors, factor', inp['w'], inp['g']), ('posteriors', inp['w'], None)):
            out, wd, gd = output(n, c.Q, c.arith), tt(w[:n]), None if g is None else tt(g[:n])
            _hip.call('beer_dense_llh_backward', code, T, K, c.Q, _hip.ptr(wd), _hip.ptr(gd), _hip.ptr(E),
                      _hip.ptr(out))
            got = taken(out, n, T, dense_id(c))
            if T:
                res.append((name, got) + vt.llh_backward(w[:T], None if g is None else g[:T], inp['E']) + (0.,))
        return res
    # acc starts from eighths and has two guard rows
    acc0 = ((torch.arange((K + 2) * c.Q, device=DEV) % 7 + 1).double() / 8.).reshape(K + 2, c.Q)
    acc = acc0.clone()
    sr, wd = tt(inp['sr'][:n]) if c.sr else None, tt(inp['w'][:n])
    _hip.call('beer_dense_accumulate', code, T, K, c.Q, c.G, _hip.ptr(wd), _hip.ptr(sr),
              _hip.ptr(st), _hip.ptr(acc))
    torch.cuda.synchronize()
    assert torch.equal(acc[K:], acc0[K:]), 'guard rows behind acc'
    if T == 0:
        assert torch.equal(acc, acc0)
        return []
    truth, s, ninner = vt.accumulate(inp['st'][:T], inp['w'][:T], inp['sr'][:T] if c.sr else None, c.S, c.G)
    return [('acc', npy(acc[:K] - acc0[:K]), truth, s, ninner, (T // 16 + 2) * 2. ** -53 * (.875 + np.abs(truth)))]


@pytest.mark.parametrize('c', DENSE_CASES, ids=dense_id)
def test_dense_form_vs_oracle(c):
    # (one-signed statistics only where the bound needs them: vae_prior_truth.py)
    inp = vt.dense_inputs(max(c.ts), c.Q, c.S * c.G, c.S, dense_seed(c), NP_OF[c.arith],
                          one_signed=c.op == ACC and c.sr and c.arith == 'f32' and c.form == 'p')
    for T in sorted({0, *c.ts}):
        for name, got, truth, s, n, extra in run_dense(c, inp, T):
            # (the accumulator is float64 whatever the operands are: without state posteriors
            #  gemm_kernel is held to the float64 bound; with them the float32 term of the bound
            #  stands for the rounding of the joint posterior, vae_prior_truth.py)
            hold(dense_family(c), f'{dense_id(c)} T={T} {name}', got, truth, s, n,
                 'f64' if c.op == ACC and not c.sr and c.form == 'p' else c.arith, bf16x3=c.form != 'p',
                 extra=extra)


# The long chain.  The split search of `g3_chain` (dense.hip) takes z = min_z = ceil(T / 4096)
# workgroups along the frames when gx gy min_z fills the 512 workgroup slots exactly: K = 512
# (gx = 4 tiles of 128), Q = 4096 (gy = 32), T = 16384 (min_z = 4): 4 x 32 x 4 = 512, one round of
# 4096 frames, cost 4096; z = 5 .. 7 need two rounds of more than 2048 frames, z = 8 two of 2048,
# the same cost, and the search keeps the first.  T Q = 6.7e7 elements.
LONG = D(ACC, 'f32', (16384,), 4096, 512, 1, False, '3:128x128')


def test_long_chain_accumulation_on_one_signed_data():
    '''Chains of 4096 frames (what config 4 runs near: T = 1 M, Q = 4162 gives 2048), on one-signed
    data: non-negative posteriors and the quadratic columns -1/2 x_i x_j of real statistics of
    frames away from the origin -- every product has the same sign, so the truncation of the
    matrix core's accumulator adds up instead of averaging out.  Truth: torch.float64 on the
    device.  Observed on an MI355X: relative error mean -8.9e-8, min -1.62e-6, max +1.38e-6;
    worst |err| / s 1.62e-6, 0.81 of the 2e-6 it is held to (`C['g3long']`).'''
    c, T, K, Dd = LONG, LONG.ts[0], LONG.S, 64
    r = _hip.dense_route(ACC, _hip.F32, T, c.Q, K)
    assert r & ~0xFF00 == dense_value(c.form) and _hip.dense_chain(r) == 4096, hex(r)
    rng = np.random.default_rng(77)
    X = (1.5 + .5 * np.clip(rng.standard_normal((T, Dd)), -2.5, 2.5)).astype(np.float32)
    st = torch.from_numpy(vt.orc.SUFFSTATS['full'](X)[:, Dd:Dd + Dd * Dd].copy()).to(DEV)
    assert st.dtype == torch.float32 and tuple(st.shape) == (T, c.Q) and bool((st < 0).all())
    w = tt(vt.posteriors(rng, T, 1, K).astype(np.float32))
    acc0 = ((torch.arange((K + 2) * c.Q, device=DEV) % 7 + 1).double() / 8.).reshape(K + 2, c.Q)
    acc = acc0.clone()
    _hip.call('beer_dense_accumulate', _hip.F32, 0, K, c.Q, 1, _hip.ptr(w), None, _hip.ptr(st), _hip.ptr(acc))
    torch.cuda.synchronize()
    assert torch.equal(acc, acc0)
    _hip.call('beer_dense_accumulate', _hip.F32, T, K, c.Q, 1, _hip.ptr(w), None, _hip.ptr(st), _hip.ptr(acc))
    torch.cuda.synchronize()
    assert torch.equal(acc[K:], acc0[K:])
    truth = npy(w.double().t() @ st.double())
    got = npy(acc[:K] - acc0[:K])
    del st, w, acc, acc0
    torch.cuda.empty_cache()
    rel = (got - truth) / np.abs(truth)
    print(f'\nlong chain: relative error mean {rel.mean():.3e}, min {rel.min():.3e}, max {rel.max():.3e}')
    hold('g3long', 'long chain', got, truth, np.abs(truth), 2 * T, 'f32', bf16x3=True,
         extra=(T // 16 + 2) * 2. ** -53 * (.875 + np.abs(truth)))


# =================================================================================================
# Statistics of samples and their gradient
# =================================================================================================

S = namedtuple('S', 'arith cov D ns ts')
STAT_TS = (0, 1, 3, 4, 5, 301)
STAT_CASES = (
    [S(a, 'full', Dd, ns, STAT_TS) for a in ('f64', 'f32') for Dd in (7, 8, 9, 33, 63, 64, 65) for ns in (1, 2, 3)] +
    [S(a, cov, Dd, ns, STAT_TS) for a in ('f64', 'f32') for cov in ('diagonal', 'isotropic')
     for Dd in (1, 13, 65) for ns in (1, 2, 3)])
# one case per kernel whose grid-stride loop (65536 workgroups of 256 threads, of 4 frames in the
# wave-per-frame kernel) runs twice: T Q > 2^24 outputs of `suffstats_mean_kernel` (isotropic,
# D = 1: Q = 4), T ns D > 2^24 of `suffstats_backward_kernel` (isotropic, D = 1, ns = 3),
# T > 2^18 frames of `suffstats_backward_full_kernel` (D = 8)
STRIDE_CASES = [('mean', S('f32', 'isotropic', 1, 1, ((1 << 22) + 5,))),
                ('backward', S('f32', 'isotropic', 1, 3, (5592406,))),
                ('backward', S('f32', 'full', 8, 1, ((1 << 18) + 5,)))]


def stat_id(c):
    return f'{c.arith}-{c.cov[:4]}-D{c.D}-ns{c.ns}-T{c.ts[-1]}'


def run_stats(c, inp, T, which=('mean', 'backward')):
    code, cov, n, Q = CODE_OF[c.arith], _hip.COV_CODE[c.cov], max(T, 1), vt.stats_dim(c.cov, c.D)
    X = tt(inp['X'][:n * c.ns])
    fam = 'stats' + c.arith[1:]
    if 'mean' in which:
        out = output(n, Q, c.arith)
        _hip.call('beer_suffstats_mean', code, cov, T, c.ns, c.D, _hip.ptr(X), _hip.ptr(out))
        got = taken(out, n, T, stat_id(c))
        del out
        if T:
            hold(fam, f'mean {stat_id(c)} T={T}', got, *vt.suffstats_mean(c.cov, inp['X'][:T * c.ns], c.ns), c.arith)
    if 'backward' in which:
        gx = output(n * c.ns, c.D, c.arith)
        gs = tt(inp['gs'][:n])
        _hip.call('beer_suffstats_backward', code, cov, T, c.ns, c.D, _hip.ptr(X), _hip.ptr(gs), _hip.ptr(gx))
        got = taken(gx, n * c.ns, T, stat_id(c))
        del gx, gs
        if T:
            hold(fam, f'backward {stat_id(c)} T={T}', got,
                 *vt.suffstats_backward(c.cov, inp['X'][:T * c.ns], inp['gs'][:T], c.ns), c.arith)


@pytest.mark.parametrize('c', STAT_CASES, ids=stat_id)
def test_statistics_and_their_gradient_vs_oracle(c):
    inp = vt.frame_inputs(c.cov, c.D, 1, max(c.ts), 3000 + c.D, NP_OF[c.arith], ns=c.ns)
    for T in sorted({0, *c.ts}):
        run_stats(c, inp, T)


@pytest.mark.parametrize('which,c', STRIDE_CASES, ids=[f'{w}-{stat_id(c)}' for w, c in STRIDE_CASES])
def test_statistics_grid_stride_loops_run_twice(which, c):
    inp = vt.frame_inputs(c.cov, c.D, 1, c.ts[0], 3100 + c.D, NP_OF[c.arith], ns=c.ns)
    for T in (0, c.ts[0]):
        run_stats(c, inp, T, which=(which,))
    torch.cuda.empty_cache()


# =================================================================================================
# Softmax over groups, row dot products
# =================================================================================================

SOFTMAX_CASES = [(a, Sx, G, lw, outs) for a in ('f64', 'f32') for Sx, G in ((1, 1), (1, 17), (5, 4), (300, 1))
                 for lw in (True, False) for outs in ('ln', 'r', 'both')]


@pytest.mark.parametrize('arith,Sx,G,with_lw,outs', SOFTMAX_CASES,
                         ids=[f"{a}-{s}x{g}{'-lw' if lw else ''}-{o}" for a, s, g, lw, o in SOFTMAX_CASES])
def test_softmax_groups_vs_oracle(arith, Sx, G, with_lw, outs):
    rng = np.random.default_rng(4000 + 17 * Sx + G)
    K, dt = Sx * G, NP_OF[arith]
    pc = (-40. * vt.scales(257, 1)[:, None] + 3. * rng.standard_normal((257, K)) * vt.scales(K, 2)[None, :])
    lw = et.log_weights(Sx, G, 5, phantom=G >= 3) if with_lw else None
    if G >= 3:
        pc[1, 2], pc[3 % 257, K - 1] = et.PHANTOM, -np.inf          # in otherwise finite rows
    pc = np.ascontiguousarray(pc.astype(dt))
    lw = None if lw is None else np.ascontiguousarray(lw.astype(dt))
    for T in (0, 1, 257):
        n = max(T, 1)
        ln = output(n, Sx, arith) if outs != 'r' else None
        r = output(n, K, arith) if outs != 'ln' else None
        pcd, lwd = tt(pc[:n]), None if lw is None else tt(lw)
        _hip.call('beer_softmax_groups', CODE_OF[arith], T, Sx, G, _hip.ptr(pcd), _hip.ptr(lwd), _hip.ptr(ln),
                  _hip.ptr(r))
        got_ln = None if ln is None else taken(ln, n, T, 'log_norm')
        got_r = None if r is None else taken(r, n, T, 'resps')
        if T == 0:
            continue
        want_ln, want_r = vt.softmax_groups(pc[:T], lw, Sx, G)
        logits = np.abs(pc[:T].astype(np.float64).reshape(T, Sx, G) + (0. if lw is None else lw.astype(np.float64)[None]))
        tol = (G + 16) * 2. ** -53 * max(1., logits[logits < 1e29].max())
        assert np.isfinite(want_ln).all() and (want_r >= 0).all()
        what = f'softmax {arith} {Sx}x{G} T={T}'
        if got_ln is not None:
            hold('softmax' + arith[1:], what + ' log_norm', got_ln, want_ln, np.zeros_like(want_ln), 0, arith, extra=tol)
        if got_r is not None:
            if G >= 3 and T > 3:
                assert got_r[1, 2] == 0. and got_r[3, K - 1] == 0.
            hold('softmax' + arith[1:], what + ' resps', got_r, want_r, np.zeros_like(want_r), 0, arith, extra=tol)


@pytest.mark.parametrize('arith', ('f64', 'f32'))
@pytest.mark.parametrize('K', (1, 63, 64, 65, 200))
def test_rowdot_vs_oracle(arith, K):
    rng = np.random.default_rng(4100 + K)
    a = np.ascontiguousarray((rng.standard_normal((1001, K)) * vt.scales(1001, 1)[:, None]).astype(NP_OF[arith]))
    b = np.ascontiguousarray((rng.standard_normal((1001, K)) * vt.scales(K, 2)[None, :]).astype(NP_OF[arith]))
    for T in (0, 1, 3, 4, 5, 1001):
        n = max(T, 1)
        out = output(n, 1, arith)
        ad, bd = tt(a[:n]), tt(b[:n])
        _hip.call('beer_rowdot', CODE_OF[arith], T, K, _hip.ptr(ad), _hip.ptr(bd), _hip.ptr(out))
        got = taken(out, n, T, 'rowdot')
        if T:
            truth, s, ninner = vt.rowdot(a[:T], b[:T])
            hold('rowdot' + arith[1:], f'rowdot {arith} K={K} T={T}', got[:, 0], truth, s, ninner, arith)


# =================================================================================================
# The gradient w.r.t. the frames
# =================================================================================================

def frames_value(spec, T=None):
    '''`beer_frames_llh_backward_route` of a form written 'gen' (sgrad_generic_kernel), 'sg:NKB'
    (sgrad_kernel), 'sd:NJ2' (sgrad_diag_kernel) or 'ch' (chunked; the chunk length masked off).'''
    if spec == 'gen':
        return _hip.SGRAD_GENERIC
    if spec == 'ch':
        return _hip.SGRAD_CHUNKED
    kind, _, n = spec.partition(':')
    return {'sg': _hip.SGRAD_FULL, 'sd': _hip.SGRAD_DIAG}[kind] | int(n)


# arithmetic, covariance type, D, K, the frame counts, workspace ('' advertised, 'nows' none,
# 'short' one byte less), form
F = namedtuple('F', 'arith cov D K ts ws form')
FAST_TS = (0, 4096, 4097, 4096 + 511, 4608 + 17)
SD_DIMS = {2: (1, 4, 5, 32), 3: (33, 48), 4: (49, 64), 8: (65, 100, 127, 128)}
FRAME_CASES = (
    [F('f32', 'full', Dd, K, FAST_TS, '', 'sg:1') for Dd in (8, 9, 16, 17, 31, 32) for K in (1, 2, 3, 4, 5, 9)] +
    [F('f32', 'full', Dd, K, FAST_TS, '', 'sg:2') for Dd in (33, 47, 48, 63, 64) for K in (1, 2, 3, 4, 5, 9)] +
    [F('f32', cov, Dd, K, FAST_TS, '', f'sd:{nj2}') for cov in ('diagonal', 'isotropic')
     for nj2, dims in SD_DIMS.items() for Dd in dims for K in (1, 31, 32, 33, 65)] +
    # the chunked route in one chunk
    [F('f64', 'full', 9, 3, (4100,), '', 'ch'), F('f64', 'diagonal', 13, 3, (4100,), '', 'ch'),
     F('f64', 'isotropic', 5, 3, (4100,), '', 'ch'), F('f32', 'full', 5, 3, (4100,), '', 'ch'),
     F('f32', 'full', 72, 3, (4100,), '', 'ch'), F('f32', 'diagonal', 130, 3, (4100,), '', 'ch')] +
    # the generic kernel: few frames, and many without the workspace that the other routes need
    [F(a, cov, Dd, 3, (0, 1, 300), '', 'gen') for a in ('f64', 'f32')
     for cov, Dd in (('full', 9), ('diagonal', 13), ('isotropic', 5))] +
    [F(a, cov, Dd, 3, (4100,), ws, 'gen') for a in ('f64', 'f32')
     for cov, Dd in (('full', 9), ('diagonal', 13), ('isotropic', 5)) for ws in ('nows', 'short')])
# two chunks with a ragged second one: T = chunk + extra, the chunk length read from the query.
# float32, D = 72: the first chunk (12763 frames, Q = 5258) reaches gemm3_kernel, the second not.
TWO_CHUNK_CASES = [(F('f64', 'full', 64, 3, (), '', 'ch'), 5), (F('f32', 'full', 72, 3, (), '', 'ch'), 3)]
# sgrad_generic_kernel's grid-stride loop twice: T D > 2^24 outputs, no workspace
GENERIC_STRIDE = F('f32', 'isotropic', 4, 2, ((1 << 22) + 5,), 'nows', 'gen')


def frame_id(c):
    return f"{c.arith}-{c.cov[:4]}-D{c.D}-K{c.K}{'-' + c.ws if c.ws else ''}-T{c.ts[-1] if c.ts else 'chunk'}-{c.form}"


def frame_ws_bytes(c, T):
    'The advertised workspace of the case; none, or one byte less, by `c.ws`.'
    full = _hip.lib().beer_frames_llh_backward_workspace_bytes(CODE_OF[c.arith], _hip.COV_CODE[c.cov], T, c.D, c.K)
    return {'': full, 'nows': 0, 'short': max(full - 1, 0)}[c.ws]


def frame_route(c, T):
    'The query with the chunk length masked off.'
    r = _hip.frames_llh_backward_route(CODE_OF[c.arith], _hip.COV_CODE[c.cov], T, c.D, c.K, frame_ws_bytes(c, T))
    return _hip.SGRAD_CHUNKED if r > 0 and _hip.sgrad_family(r) == _hip.SGRAD_CHUNKED else r


def frame_family(c):
    return {'sg:1': 'sg1', 'sg:2': 'sg2', 'ch': 'chunked' + c.arith[1:], 'gen': 'generic' + c.arith[1:]}.get(c.form, 'sd')


def run_frames(c, inp, T, w, g, truth3, extra_scale=0.):
    'One call on the first T frames with weights `w` and factor `g` (None: 1), held to `truth3`.'
    code, cov, n = CODE_OF[c.arith], _hip.COV_CODE[c.cov], max(T, 1)
    nws = frame_ws_bytes(c, T or max(c.ts))        # (T = 0: the workspace of the case's longest call)
    ws = guarded(nws) if nws else None
    assert frame_route(c, T) == frames_value(c.form if T else 'gen'), (frame_id(c), T, hex(frame_route(c, T)))
    out = output(n, c.D, c.arith)
    Xd, wd, gd, Ed = tt(inp['X'][:n]), tt(w[:n]), None if g is None else tt(g[:n]), tt(inp['E'])
    _hip.call('beer_frames_llh_backward', code, cov, T, c.D, c.K, _hip.ptr(Xd), _hip.ptr(wd), _hip.ptr(gd), _hip.ptr(Ed),
              _hip.ptr(out), _hip.ptr(ws), nws)
    got = taken(out, n, T, frame_id(c))
    assert ws is None or guard_kept(ws, nws), 'workspace guard'
    if T == 0:
        assert ws is None or bool((ws[:nws] == 0xff).all()), 'T = 0 wrote to the workspace'
        return
    truth, s, ninner = truth3
    hold(frame_family(c), f"{frame_id(c)} T={T}{'' if g is None else ' factor'}", got, truth[:T], s[:T], ninner,
         c.arith, bf16x3=c.form[:2] in ('sg', 'sd'), extra=extra_scale * s[:T])


def frame_variants(c, inp):
    'Posterior and signed weights, with and without the per-frame factor: (w, g, truth, s, n).'
    for w in (inp['w'], inp['ws']):
        for g in (inp['g'], None):
            yield w, g, vt.frames_gradient(c.cov, inp['X'], w, inp['E'], g)


@pytest.mark.parametrize('c', FRAME_CASES, ids=frame_id)
def test_frames_gradient_form_vs_oracle(c):
    inp = vt.frame_inputs(c.cov, c.D, c.K, max(c.ts), 5000 + 31 * c.D + c.K, NP_OF[c.arith])
    # the chunked route in float32 rounds the gradient of the statistics to float32 in between
    extra = 2. ** -24 if c.form == 'ch' and c.arith == 'f32' else 0.
    for w, g, truth3 in frame_variants(c, inp):
        for T in sorted({0, *c.ts}):
            run_frames(c, inp, T, w, g, truth3, extra)


@pytest.mark.parametrize('c,more', TWO_CHUNK_CASES, ids=[frame_id(c) for c, _ in TWO_CHUNK_CASES])
def test_frames_gradient_over_two_chunks(c, more):
    code, cov = CODE_OF[c.arith], _hip.COV_CODE[c.cov]
    probe = 1 << 20
    r = _hip.frames_llh_backward_route(code, cov, probe, c.D, c.K,
                                       _hip.lib().beer_frames_llh_backward_workspace_bytes(code, cov, probe, c.D, c.K))
    assert _hip.sgrad_family(r) == _hip.SGRAD_CHUNKED
    chunk = _hip.sgrad_form(r)
    T = chunk + more
    c = c._replace(ts=(T,))
    assert _hip.sgrad_form(_hip.frames_llh_backward_route(code, cov, T, c.D, c.K, frame_ws_bytes(c, T))) == chunk
    Q = vt.stats_dim(c.cov, c.D)
    first = _hip.dense_route(BWD, code, chunk, Q, c.K), _hip.dense_route(BWD, code, more, Q, c.K)
    on_cores = c.arith == 'f32'
    assert (_hip.dense_family(first[0]) == _hip.DENSE_GEMM3) == on_cores and first[1] == _hip.DENSE_PLAIN
    inp = vt.frame_inputs(c.cov, c.D, c.K, T, 5100 + c.D, NP_OF[c.arith])
    extra = (2. ** -24 + C['g3bwd']) if on_cores else 0.
    truth3 = vt.frames_gradient(c.cov, inp['X'], inp['ws'], inp['E'], inp['g'])
    for n in (0, T):
        run_frames(c, inp, n, inp['ws'], inp['g'], truth3, extra)
    torch.cuda.empty_cache()


def test_generic_gradient_grid_stride_loop_runs_twice():
    c = GENERIC_STRIDE
    inp = vt.frame_inputs(c.cov, c.D, c.K, c.ts[0], 5200, NP_OF[c.arith])
    truth3 = vt.frames_gradient(c.cov, inp['X'], inp['ws'], inp['E'], inp['g'])
    for T in (0, c.ts[0]):
        run_frames(c, inp, T, inp['ws'], inp['g'], truth3)
    torch.cuda.empty_cache()
