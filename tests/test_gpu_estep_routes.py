"""Every launch form of the E-step forward (csrc/estep.hip, estep_mfma.hip, estep_bf16.hip behind
`beer_mixtureset_estep`, `beer_mixture_estep_packed`, `beer_mixtureset_estep_packed` and
`beer_mixtureset_lognorm_image`) against the float64 oracle at small shapes (tests/estep_truth.py).

One static table: each row names the form the launchers must pick for it (`beer_estep_route`), and
each test first holds the C layer's answer against the table, then calls the C entry point itself
through `_hip.call` -- not through `kernels.*`, whose `f32_fast_ok` keeps the bf16x3 kernels for
16384 frames and more -- at T = 1, 129 and 300 (three 128-frame blocks, two 256-frame `lnfi`
workgroups with a ragged tail, a one-block grid under two or three component chunks), and compares
log-normalisers, responsibilities (packed ones through `beer_unpack_resps`) and `llh_sum` (which
starts from a non-zero value) with the oracle.  Outputs are pre-filled with NaN; two guard rows
behind `log_norm` and the responsibilities, and 256 guard bytes behind the workspace (sized exactly
as `beer_estep_workspace_bytes` says), the packed buffer and the frame image must keep their bits;
T = 0 returns OK and writes nothing.

Bounds (the project's own): float64 1e-9 absolute on log-normalisers and responsibilities; float32
(both arithmetics) 1e-5 max |ln| of the case (its 300 frames) on log-normalisers (`_check` of
test_gpu_band_layout.py), twice that on responsibilities (|dr| <= 2 max |dlogit| to first order);
`llh_sum` T S times the log-normaliser bound.

D walks through 1, 4, 5, 13, 37, 40, 44, 48 (the slab-count edges: one, two, three and four
k-steps of diagonal statistics, Dp % 8 == 0 and == 4 of the band layout), plus 53, 72 and 128 where
the form allows; K includes 17, 65, 129 and 200 (no whole tiles) and sets of two and three chunks
(33 x 16, 3 x 128, 300 x 1).

Worst errors observed on an MI355X over the file, as a fraction of the bound (the module prints
them at its end, `pytest -s`): float64 0.004 at most (1e-12 .. 4e-12); generic kernels in float32
0.06; exact fp32 MFMA 0.25 (log_norm, full covariance); `llhx_kernel` 0.49 (log_norm, full
covariance, padded groups), 0.09 on responsibilities; `lnfi_kernel` 0.26.  The full-covariance
float32 forms are close to the bound by construction: tests/estep_truth.py sizes the terms of a
logit so that float32's own rounding reaches half of it."""

from collections import namedtuple

import numpy as np
import pytest
import torch

import estep_truth as et
from helpers import orc

pytestmark = pytest.mark.gpu

from beer_amd import _hip                                            # noqa: E402
from gpu_helpers import DEV, npy, tt                                 # noqa: E402

DSET = (1, 4, 5, 13, 37, 40, 44, 48)
TS = (1, 129, 300)
RAGGED = (31, 32, 33, 63, 64, 65, 127, 128, 257)
TMAX = 300
SUM0 = 1234.5
PLAIN, PACKED, IMAGE = _hip.ESTEP_PLAIN, _hip.ESTEP_PACKED, _hip.ESTEP_IMAGE
ALL, FULL, DIAGS = et.COVS, ('full',), ('diagonal', 'isotropic')
NP_OF = {'f64': np.float64, 'exact': np.float32, 'x': np.float32}
CODE_OF = {'f64': _hip.F64, 'exact': _hip.F32 | _hip.EXACT, 'x': _hip.F32}
X_FLAGS = {'P': _hip.ESTEP_X_PACKED, 'L': _hip.ESTEP_X_LNO, 'I': _hip.ESTEP_X_IMG,
           'B': _hip.ESTEP_X_BL, 'N': _hip.ESTEP_X_NARROW, 'M': _hip.ESTEP_X_LANE_MAJOR,
           'D': _hip.ESTEP_X_PADDED, 'T': _hip.ESTEP_X_XT}


def route_value(spec, arith='x'):
    '''The `beer_estep_route` value of a form written as
    'g:FORM' (generic: 1 pass 1 only, 2 fused, 3 + normalise_kernel, 4 labels),
    'e:NT.GQ.jw[*chunks]' (exact MFMA, float32 or float64 by `arith`),
    'x:NT.GQ.FLAGS[*chunks]' (llhx_kernel; P packed, L LNO, I IMG, B BL, N narrow, M lane-major,
    D padded groups, T X^T left behind) or 'i:NKU.G.NT[*chunks]' (lnfi_kernel).'''
    kind, rest = spec.split(':')
    rest, _, chunks = rest.partition('*')
    chunks = int(chunks or 1) << 16
    f = rest.split('.')
    if kind == 'g':
        return _hip.ESTEP_GENERIC | int(f[0])
    if kind == 'e':
        fam = _hip.ESTEP_EXACT_F64 if arith == 'f64' else _hip.ESTEP_EXACT_F32
        return fam | int(f[0]) | int(f[1]) << 5 | int(f[2]) << 8 | chunks
    if kind == 'x':
        flags = 0
        for ch in f[2]:
            flags |= X_FLAGS[ch]
        return _hip.ESTEP_LLHX | int(f[0]) | int(f[1]) << 5 | flags | chunks
    assert kind == 'i'
    return _hip.ESTEP_LNFI | int(f[2]) | int(f[0]) << 5 | int(f[1]) << 8 | chunks


# entry, arithmetics, covariance types, the D values the row draws from, S, G, responsibilities
# wanted (plain entry), the form, options: BEER_OPT_* by name, 'ws': 0 = no workspace,
# 'ragged': also the ragged-tail T values
Row = namedtuple('Row', 'entry ariths covs Ds S G resps form opts')
Case = namedtuple('Case', 'entry arith cov D S G resps form opts seed')
ROWS = []


def row(entry, ariths, covs, Ds, S, G, resps, form, **opts):
    ROWS.append(Row(entry, tuple(ariths.split()), covs, Ds, S, G, resps, form, tuple(sorted(opts.items()))))


MFMA = 'f64 exact'
# --- the exact MFMA kernels, llh_kernel<T, NT, MT, GQ> (float64 up to D = 64, float32 up to 96) ---
row(PLAIN, MFMA, ALL, DSET, 1, 17, True, 'e:4.1.4', ragged=1)
row(PLAIN, MFMA, ALL, DSET, 1, 64, False, 'e:4.1.4')
row(PLAIN, MFMA, ALL, DSET, 1, 65, False, 'e:8.2.4')
row(PLAIN, MFMA, ALL, DSET, 1, 128, True, 'e:8.2.4')
row(PLAIN, MFMA, ALL, DSET, 1, 129, True, 'e:16.4.4')
row(PLAIN, MFMA, ALL, DSET, 1, 200, False, 'e:16.4.4')
row(PLAIN, MFMA, ALL, DSET, 1, 256, True, 'e:16.4.4')
row(PLAIN, MFMA, ALL, DSET, 17, 1, False, 'e:16.1.1')
row(PLAIN, MFMA, ALL, DSET, 300, 1, True, 'e:16.1.1*2')
row(PLAIN, MFMA, ALL, DSET, 9, 2, True, 'e:16.1.2')
row(PLAIN, MFMA, ALL, DSET, 150, 2, False, 'e:16.1.2*2')
row(PLAIN, MFMA, ALL, DSET, 5, 4, True, 'e:16.1.4')
row(PLAIN, MFMA, ALL, DSET, 3, 8, False, 'e:16.1.4')
row(PLAIN, MFMA, ALL, DSET, 33, 16, False, 'e:16.1.4*3')
row(PLAIN, MFMA, ALL, DSET, 5, 64, True, 'e:16.1.4*2')
row(PLAIN, MFMA, ALL, DSET, 2, 128, True, 'e:16.2.4')
row(PLAIN, MFMA, ALL, DSET, 3, 128, False, 'e:16.2.4*2')
row(PLAIN, MFMA, ALL, DSET, 2, 256, True, 'e:16.4.4*2')
row(PLAIN, 'f64', ALL, (53, 64), 1, 65, True, 'e:8.2.4')
row(PLAIN, 'exact', ALL, (53, 72, 96), 5, 16, True, 'e:16.1.4')
# --- llhx_kernel, plain entry: one mixture ---
row(PLAIN, 'x', ALL, DSET, 1, 17, True, 'x:4.1.', ragged=1)
row(PLAIN, 'x', ALL, DSET, 1, 64, False, 'x:4.1.')
row(PLAIN, 'x', ALL, DSET, 1, 65, True, 'x:8.2.')
row(PLAIN, 'x', ALL, DSET, 1, 128, False, 'x:8.2.')
row(PLAIN, 'x', ALL, DSET, 1, 129, False, 'x:16.4.')
row(PLAIN, 'x', ALL, DSET, 1, 200, True, 'x:16.4.')
row(PLAIN, 'x', ALL, (53, 72, 128), 1, 256, True, 'x:16.4.')
# ... sets of single Gaussians: the narrow forms, then chunks of 256
row(PLAIN, 'x', ALL, DSET, 17, 1, False, 'x:4.1.N')
row(PLAIN, 'x', ALL, DSET, 64, 1, True, 'x:4.1.N')
row(PLAIN, 'x', ALL, DSET, 65, 1, True, 'x:8.1.N')
row(PLAIN, 'x', ALL, DSET, 128, 1, False, 'x:8.1.N')
row(PLAIN, 'x', ALL, DSET, 129, 1, False, 'x:16.1.')
row(PLAIN, 'x', ALL, DSET, 300, 1, True, 'x:16.1.*2')
# ... G = 2
row(PLAIN, 'x', ALL, DSET, 9, 2, True, 'x:16.1.')
row(PLAIN, 'x', ALL, DSET, 150, 2, False, 'x:16.1.*2')
# ... groups of 4 / 8 / 16: lane-major without responsibilities
row(PLAIN, 'x', ALL, DSET, 5, 4, False, 'x:16.1.LM')
row(PLAIN, 'x', ALL, DSET, 3, 8, False, 'x:16.1.LM')
row(PLAIN, 'x', ALL, DSET, 2, 16, False, 'x:16.1.LM')
row(PLAIN, 'x', ALL, DSET, 33, 16, False, 'x:16.1.LM*3')
row(PLAIN, 'x', ALL, (53, 72, 128), 65, 4, False, 'x:16.1.LM*2')
row(PLAIN, 'x', ALL, DSET, 5, 4, True, 'x:16.1.')
row(PLAIN, 'x', ALL, DSET, 33, 16, True, 'x:16.1.*3')
# ... groups of 32 .. 256: GQ = 1, 2, 4, LNO without responsibilities
row(PLAIN, 'x', ALL, DSET, 2, 32, False, 'x:16.1.L')
row(PLAIN, 'x', ALL, DSET, 5, 64, False, 'x:16.1.L*2')
row(PLAIN, 'x', ALL, DSET, 5, 64, True, 'x:16.1.*2')
row(PLAIN, 'x', ALL, DSET, 2, 128, False, 'x:16.2.L')
row(PLAIN, 'x', ALL, DSET, 3, 128, False, 'x:16.2.L*2')
row(PLAIN, 'x', ALL, DSET, 2, 128, True, 'x:16.2.')
row(PLAIN, 'x', ALL, DSET, 3, 128, True, 'x:16.2.*2')
row(PLAIN, 'x', ALL, DSET, 2, 256, False, 'x:16.4.L*2')
row(PLAIN, 'x', ALL, DSET, 2, 256, True, 'x:16.4.*2')
# ... groups padded to a power of two (log-normalisers only)
row(PLAIN, 'x', ALL, DSET, 6, 3, False, 'x:16.1.LMD')
row(PLAIN, 'x', ALL, DSET, 4, 5, False, 'x:16.1.LMD')
row(PLAIN, 'x', ALL, DSET, 3, 6, False, 'x:16.1.LMD')
row(PLAIN, 'x', ALL, DSET, 2, 12, False, 'x:16.1.LMD')
row(PLAIN, 'x', ALL, DSET, 40, 12, False, 'x:16.1.LMD*3')
row(PLAIN, 'x', ALL, DSET, 2, 20, False, 'x:16.1.LD')
row(PLAIN, 'x', ALL, DSET, 9, 33, False, 'x:16.1.LD*3')
row(PLAIN, 'x', ALL, DSET, 2, 65, False, 'x:16.2.LD')
row(PLAIN, 'x', ALL, DSET, 3, 65, False, 'x:16.2.LD*2')
row(PLAIN, 'x', ALL, DSET, 2, 129, False, 'x:16.4.LD*2')
# --- llhx_kernel, packed responsibilities: one mixture (X^T left behind from 129 components) ---
row(PACKED, 'x', ALL, DSET, 1, 17, True, 'x:4.1.P', ragged=1)
row(PACKED, 'x', ALL, DSET, 1, 65, True, 'x:8.2.P')
row(PACKED, 'x', FULL, DSET, 1, 129, True, 'x:16.4.PBT', ragged=1)
row(PACKED, 'x', FULL, DSET, 1, 200, True, 'x:16.4.PBT')
row(PACKED, 'x', FULL, DSET, 1, 256, True, 'x:16.4.PT', k1_lds=0)
row(PACKED, 'x', FULL, (53, 72, 128), 1, 200, True, 'x:16.4.PT')
row(PACKED, 'x', DIAGS, DSET, 1, 200, True, 'x:16.4.PT')
# ... mixture sets (full covariance)
row(PACKED, 'x', FULL, DSET, 5, 8, True, 'x:16.1.PB')
row(PACKED, 'x', FULL, DSET, 5, 16, True, 'x:16.1.PB')
row(PACKED, 'x', FULL, DSET, 5, 64, True, 'x:16.1.PB*2')
row(PACKED, 'x', FULL, DSET, 2, 128, True, 'x:16.2.PB')
row(PACKED, 'x', FULL, DSET, 3, 128, True, 'x:16.2.PB*2')
row(PACKED, 'x', FULL, DSET, 2, 32, True, 'x:16.1.P', k1_lds=0)
row(PACKED, 'x', FULL, (53, 72, 128), 33, 16, True, 'x:16.1.P*3')
row(PACKED, 'x', FULL, DSET, 2, 128, True, 'x:16.2.P', k1_lds=0)
row(PACKED, 'x', FULL, (53, 72), 3, 128, True, 'x:16.2.P*2')
# --- lnfi_kernel<NKU, G, NT> over a frame image (diagonal / isotropic) ---
for G_ in (4, 8, 16):
    row(IMAGE, 'x', DIAGS, (1, 4, 5, 12), 64 // G_ + 1, G_, False, f'i:1.{G_}.16', ragged=int(G_ == 8))
    row(IMAGE, 'x', DIAGS, (13, 28), 5, G_, False, f'i:2.{G_}.16')
    row(IMAGE, 'x', DIAGS, (29, 37, 40), 4, G_, False, f'i:3.{G_}.16')
    row(IMAGE, 'x', DIAGS, (1, 4, 5), 528 // G_, G_, False, f'i:1.{G_}.16*3')
    row(IMAGE, 'x', DIAGS, (13, 28), 260 // G_ + 1, G_, False, f'i:2.{G_}.16*2')
    row(IMAGE, 'x', DIAGS, (37, 40), 528 // G_, G_, False, f'i:3.{G_}.16*3')
row(IMAGE, 'x', DIAGS, (41, 44, 48), 5, 4, False, 'i:4.4.8')
row(IMAGE, 'x', DIAGS, (41, 44, 48), 3, 8, False, 'i:4.8.8')
row(IMAGE, 'x', DIAGS, (44, 48), 33, 4, False, 'i:4.4.8*2')
row(IMAGE, 'x', DIAGS, (44, 48), 33, 8, False, 'i:4.8.8*3')
row(IMAGE, 'x', DIAGS, (5, 13, 40), 4, 5, False, 'i:{nku}.8.16')            # padded groups
# --- llhx_kernel<.., LNO, IMG>: where lnfi_kernel does not go ---
row(IMAGE, 'x', DIAGS, (44, 48), 2, 16, False, 'x:16.1.LIM')
row(IMAGE, 'x', DIAGS, (44, 48), 17, 16, False, 'x:16.1.LIM*2')
row(IMAGE, 'x', DIAGS, (44, 48), 2, 9, False, 'x:16.1.LIMD')
row(IMAGE, 'x', DIAGS, DSET, 5, 4, False, 'x:16.1.LIM', lnfi=0, ragged=1)
row(IMAGE, 'x', DIAGS, DSET, 33, 8, False, 'x:16.1.LIM*2', lnfi=0)
row(IMAGE, 'x', DIAGS, DSET, 4, 5, False, 'x:16.1.LIMD', lnfi=0)
row(IMAGE, 'x', DIAGS, DSET, 2, 32, False, 'x:16.1.LI')
row(IMAGE, 'x', DIAGS, DSET, 5, 64, False, 'x:16.1.LI*2')
row(IMAGE, 'x', DIAGS, DSET, 2, 20, False, 'x:16.1.LID')
row(IMAGE, 'x', DIAGS, DSET, 9, 33, False, 'x:16.1.LID*3')
row(IMAGE, 'x', DIAGS, DSET, 2, 128, False, 'x:16.2.LI')
row(IMAGE, 'x', DIAGS, DSET, 3, 128, False, 'x:16.2.LI*2')
row(IMAGE, 'x', DIAGS, DSET, 2, 256, False, 'x:16.4.LI*2')
row(IMAGE, 'x', DIAGS, DSET, 2, 65, False, 'x:16.2.LID')
row(IMAGE, 'x', DIAGS, DSET, 3, 65, False, 'x:16.2.LID*2')
row(IMAGE, 'x', DIAGS, DSET, 2, 129, False, 'x:16.4.LID*2')
row(IMAGE, 'x', DIAGS, (44, 48), 17, 9, False, 'x:16.1.LIMD*2')
# --- the generic kernels: shapes without a matrix-core kernel, or no workspace ---
ANY = 'f64 exact x'
row(PLAIN, ANY, ALL, DSET, 3, 2, True, 'g:2', ragged=1)                   # K < 16
row(PLAIN, ANY, ALL, DSET, 5, 1, False, 'g:2')                            # G = 1: log_norm is w
row(PLAIN, ANY, ALL, DSET, 3, 5, True, 'g:3')                             # 64 % G != 0
row(PLAIN, ANY, ALL, DSET, 1, 100, True, 'g:3', ws=0)                     # two component chunks of 64
row(PLAIN, ANY, ALL, DSET, 2, 128, True, 'g:3', ws=0)
row(PLAIN, ANY, ALL, DSET, 5, 16, True, 'g:2', ws=0)
row(PLAIN, 'x', ALL, (129, 130), 1, 17, True, 'g:3')                      # beyond kMaxDimX
row(PLAIN, 'exact', ALL, (97, 128), 5, 16, True, 'g:2')                   # beyond kMaxDimF32
row(PLAIN, 'f64', ALL, (65, 72), 5, 16, True, 'g:2')                      # beyond kMaxDimF64


def nku_of(D):
    'k-steps (8 slabs each) of diagonal / isotropic statistics: estep_tiles.h diag_walk.'
    items = 2 * ((D + 3) // 4)
    return (items + (items - 1) // 7 + 1 + 7) // 8


def expand(rows):
    cases = []
    for n, r in enumerate(rows):
        for arith in r.ariths:
            for ci, cov in enumerate(r.covs):
                D = r.Ds[(n + 3 * ci + (arith == 'exact')) % len(r.Ds)]
                form = r.form.format(nku=nku_of(D))
                cases.append(Case(r.entry, arith, cov, D, r.S, r.G, r.resps, form, r.opts,
                                  1000 + 7 * n + ci))
    return cases


CASES = expand(ROWS)


def case_id(c):
    opts = ''.join(f'-{k}{v}' for k, v in c.opts if k != 'ragged')
    return (f'{("plain", "packed", "image")[c.entry]}-{c.arith}-{c.cov[:4]}-D{c.D}-{c.S}x{c.G}'
            f'{"-r" if c.resps else ""}{opts}-{c.form.replace(":", "").replace("*", "c")}')


def opt(c, name, default=None):
    return dict(c.opts).get(name, default)


def case_args(c):
    'BEER_ARG_* of the call a case makes.'
    a = _hip.ARG_LOG_NORM | _hip.ARG_LLH_SUM | _hip.ARG_LOG_WEIGHTS
    return a | _hip.ARG_RESPS if c.resps else a


def workspace_bytes(c):
    if opt(c, 'ws') == 0:
        return 0
    return _hip.lib().beer_estep_workspace_bytes(CODE_OF[c.arith] & ~_hip.EXACT, _hip.COV_CODE[c.cov],
                                                 c.D, c.S, c.G)


class options:
    'BEER_OPT_* of a case set for the block, restored in any case.'

    def __init__(self, c):
        self.want = [(k, v) for k, v in c.opts if k in _hip.OPTIONS]

    def __enter__(self):
        self.old = [(k, _hip.set_option(k, v)) for k, v in self.want]

    def __exit__(self, *exc):
        for k, v in reversed(self.old):
            _hip.set_option(k, v)


def case_route(c, args=None, ws_bytes=None):
    with options(c):
        return _hip.estep_route(c.entry, CODE_OF[c.arith], _hip.COV_CODE[c.cov], c.D, c.S, c.G,
                                case_args(c) if args is None else args,
                                workspace_bytes(c) if ws_bytes is None else ws_bytes)


def case_inputs(c, T=TMAX, **kw):
    return et.make(c.cov, c.D, c.S, c.G, T, c.seed, NP_OF[c.arith], **kw)


# --- running a case ----------------------------------------------------------------------------

PAT32, PAT64 = 0x7fc0beef, 0x7ff8dead0000beef
GUARD_ROWS, GUARD_BYTES = 2, 256


def nan_filled(rows, cols, dtype):
    'A [rows, cols] buffer of NaNs with a bit pattern of our own.'
    if dtype == torch.float32:
        return torch.full((rows, cols), PAT32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((rows, cols), PAT64, dtype=torch.int64, device=DEV).view(torch.float64)


def untouched(t):
    if t.dtype == torch.uint8:
        return bool((t == 0xA5).all())
    bits = t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return bool((bits == (PAT32 if t.dtype == torch.float32 else PAT64)).all())


def bytes_buf(n, fill=0xA5):
    return torch.full((n + GUARD_BYTES,), fill, dtype=torch.uint8, device=DEV)


def execute(c, T, inp, labels=None, scale=1., want_pc=False, want_sum=True, want_ln=True):
    '''One call of the case's entry point on the first T frames of `inp`; returns the outputs as
    numpy arrays after checking NaNs, guards and the return code.  T = 0: nothing may be written.'''
    dtype = torch.float64 if c.arith == 'f64' else torch.float32
    cov, D, S, G, K = _hip.COV_CODE[c.cov], c.D, c.S, c.G, c.S * c.G
    X = tt(inp['X'][:max(T, 1)])
    E = tt(inp['E'])
    lw = None if inp['lw'] is None else tt(inp['lw'])
    ln = nan_filled(T + GUARD_ROWS, S, dtype) if want_ln else None
    need_r = c.resps or c.entry == PACKED
    resps = nan_filled(T + GUARD_ROWS, K, dtype) if need_r else None
    pc = nan_filled(T + GUARD_ROWS, K, dtype) if want_pc else None
    total = torch.full((1,), SUM0, dtype=torch.float64, device=DEV) if want_sum else None
    nws = workspace_bytes(c)
    ws = bytes_buf(nws) if nws else None
    lab = None if labels is None else tt(np.asarray(labels[:max(T, 1)], dtype=np.int64))
    packed = image = None
    p = _hip.ptr
    with options(c):
        if c.entry == PLAIN:
            _hip.call('beer_mixtureset_estep', CODE_OF[c.arith], cov, T, D, S, G, p(X), p(E), p(lw),
                      p(lab), scale, p(pc), p(ln), p(resps), p(total), p(ws), nws)
        elif c.entry == PACKED:
            npk = _hip.lib().beer_packed_resps_bytes(T, D, K)
            assert npk >= 256
            packed = bytes_buf(npk, 0xFF)                   # (0xFFFF: a bf16 NaN in every piece)
            if S == 1:
                _hip.call('beer_mixture_estep_packed', cov, T, D, K, p(X), p(E), p(lw), p(ln),
                          p(packed), p(total), p(ws), nws)
            else:
                _hip.call('beer_mixtureset_estep_packed', cov, T, D, S, G, p(X), p(E), p(lw), p(ln),
                          p(packed), p(total), p(ws), nws)
            assert bool((packed[npk:] == 0xFF).all()), 'guard bytes behind the packed buffer'
            if T == 0:
                assert bool((packed == 0xFF).all())
            _hip.call('beer_unpack_resps', T, K, p(packed), p(resps))
        else:
            nimg = _hip.lib().beer_frame_image_bytes(cov, T, D)
            assert nimg > 0
            image = bytes_buf(nimg)
            _hip.call('beer_frame_image', cov, T, D, p(X), p(image), nimg)
            assert untouched(image[nimg:]), 'guard bytes behind the frame image'
            _hip.call('beer_mixtureset_lognorm_image', cov, T, D, S, G, p(X), p(E), p(lw), p(image),
                      p(ln), p(total), p(ws), nws)
    torch.cuda.synchronize()
    out = {}
    for name, buf in (('ln', ln), ('resps', resps), ('pc', pc)):
        if buf is None:
            continue
        assert untouched(buf[T:]), f'guard rows behind {name}'
        out[name] = npy(buf[:T]).astype(np.float64)
        assert not np.isnan(out[name]).any(), f'{name}: elements left unwritten'
    if ws is not None:
        assert untouched(ws[nws:]), 'guard bytes behind the workspace'
        if T == 0:
            assert untouched(ws)
    if total is not None:
        out['sum'] = float(total[0]) - SUM0
        if T == 0:
            assert float(total[0]) == SUM0
    return out


WORST = {}          # (family, output) -> (error / bound, error, case): printed when the module is done


def family_of(c):
    return {'g': 'generic ' + c.arith, 'e': 'exact ' + c.arith, 'x': 'llhx', 'i': 'lnfi'}[c.form[0]]


def compare(c, T, got, ln, resps, what=''):
    'The outputs of a run against the oracle, within the bounds of the module docstring.'
    scale = float(np.abs(ln).max())             # (of the case: every T is held to the same bound)
    ln, resps = ln[:T], resps[:T]
    tol_ln, tol_r = (1e-9, 1e-9) if c.arith == 'f64' else (1e-5 * scale, 2e-5 * scale)
    errs = []
    if 'ln' in got:
        assert got['ln'].shape == ln.shape
        errs.append(('log_norm', float(np.abs(got['ln'] - ln).max()), tol_ln))
    if 'resps' in got:
        assert got['resps'].shape == resps.shape
        errs.append(('resps', float(np.abs(got['resps'] - resps).max()), tol_r))
    if 'sum' in got:
        errs.append(('llh_sum', abs(got['sum'] - float(ln.sum())), T * c.S * tol_ln))
    print(f'{case_id(c)} T={T}{what}: max |ln| {scale:.1f} ' +
          ' '.join(f'{n} {e:.3e} (bound {t:.1e})' for n, e, t in errs))
    for name, err, tol in errs:
        key = (family_of(c), name)
        if err / tol >= WORST.get(key, (-1.,))[0]:
            WORST[key] = (err / tol, err, f'{case_id(c)} T={T}')
    for name, err, tol in errs:
        assert err <= tol, f'{case_id(c)} T={T}{what} {name}: {err:.3e} > {tol:.3e}'


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    for (family, name), (ratio, err, where) in sorted(WORST.items()):
        print(f'\nworst {family:14s} {name:8s} {err:.3e} = {ratio:.3f} of its bound  ({where})', end='')
    print()


def run_case(c, Ts):
    assert case_route(c) == route_value(c.form, c.arith), hex(case_route(c))
    inp = case_inputs(c)
    ln, resps, _ = et.truth(c.cov, inp, c.S, c.G)
    for T in Ts:
        compare(c, T, execute(c, T, inp), ln, resps)
    return inp, ln, resps


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_every_form_against_the_oracle(c):
    inp, _, _ = run_case(c, TS)
    assert execute(c, 0, inp)['sum'] == 0.


RAGGED_CASES = [c for c in CASES if opt(c, 'ragged')]


@pytest.mark.parametrize('c', RAGGED_CASES, ids=case_id)
def test_ragged_tails(c):
    'One form of each kernel template at every tail length around the tiles of 32, 64 and 128.'
    run_case(c, RAGGED)


# --- separate small tests ------------------------------------------------------------------------

def small(entry, arith, cov, D, S, G, resps, form, seed, **opts):
    return Case(entry, arith, cov, D, S, G, resps, form, tuple(sorted(opts.items())), seed)


NOWEIGHTS = [small(PLAIN, 'f64', 'full', 13, 17, 1, False, 'e:16.1.1', 31),
             small(PLAIN, 'exact', 'diagonal', 37, 300, 1, False, 'e:16.1.1*2', 32),
             small(PLAIN, 'x', 'isotropic', 5, 40, 1, False, 'x:4.1.N', 33),
             small(PLAIN, 'x', 'full', 40, 100, 1, False, 'x:8.1.N', 34),
             small(PLAIN, 'x', 'diagonal', 44, 300, 1, False, 'x:16.1.*2', 35),
             small(PLAIN, 'f64', 'diagonal', 4, 5, 1, False, 'g:2', 36)]


@pytest.mark.parametrize('c', NOWEIGHTS, ids=case_id)
def test_no_log_weights_is_normal_llh(c):
    '`log_weights = NULL`, S = K, G = 1: the log-normalisers are the per-component log-likelihoods.'
    args = _hip.ARG_LOG_NORM | _hip.ARG_LLH_SUM
    assert case_route(c, args) == route_value(c.form, c.arith)
    inp = case_inputs(c, weights=False)
    ln, resps, pc = et.truth(c.cov, inp, c.S, c.G)
    np.testing.assert_array_equal(ln, pc)
    for T in TS:
        compare(c, T, execute(c, T, inp), ln, resps, ' no weights')


PHANTOMS = [small(PLAIN, 'f64', 'full', 5, 1, 17, True, 'e:4.1.4', 41),
            small(PLAIN, 'exact', 'diagonal', 13, 5, 16, True, 'e:16.1.4', 42),
            small(PLAIN, 'f64', 'isotropic', 40, 2, 128, True, 'e:16.2.4', 43),
            small(PACKED, 'x', 'full', 13, 5, 16, True, 'x:16.1.PB', 44),
            small(PACKED, 'x', 'full', 37, 3, 128, True, 'x:16.2.PB*2', 45),
            small(PLAIN, 'x', 'diagonal', 40, 3, 8, False, 'x:16.1.LM', 46),
            small(PLAIN, 'x', 'full', 44, 2, 32, False, 'x:16.1.L', 47),
            small(PLAIN, 'x', 'isotropic', 4, 4, 5, False, 'x:16.1.LMD', 48),
            small(IMAGE, 'x', 'diagonal', 37, 5, 16, False, 'i:3.16.16', 49)]


@pytest.mark.parametrize('c', PHANTOMS, ids=case_id)
def test_phantom_component(c):
    '''A component with log-weight -1e30 (the phantom of `wide_mixture_estep`): responsibility
    exactly 0, and the state's normaliser that of the state without it.'''
    assert case_route(c) == route_value(c.form, c.arith)
    inp = case_inputs(c, phantom=True)
    ln, resps, _ = et.truth(c.cov, inp, c.S, c.G)
    gone = np.arange(c.S) * c.G + c.G - 2
    assert (inp['lw'].reshape(-1)[gone] == NP_OF[c.arith](et.PHANTOM)).all() and not resps[:, gone].any()
    keep = np.setdiff1d(np.arange(c.S * c.G), gone)
    without = dict(X=inp['X'], E=inp['E'][keep], lw=inp['lw'].reshape(-1)[keep].reshape(c.S, c.G - 1))
    np.testing.assert_allclose(et.truth(c.cov, without, c.S, c.G - 1)[0], ln, rtol=0, atol=1e-12)
    for T in TS:
        got = execute(c, T, inp)
        compare(c, T, got, ln, resps, ' phantom')
        if 'resps' in got:
            assert not got['resps'][:, gone].any()


OUTLIERS = [small(PLAIN, 'f64', 'full', 13, 5, 16, True, 'e:16.1.4', 51),
            small(PLAIN, 'exact', 'diagonal', 40, 1, 65, True, 'e:8.2.4', 52),
            small(PLAIN, 'x', 'full', 37, 1, 200, True, 'x:16.4.', 53),
            small(PACKED, 'x', 'full', 5, 5, 16, True, 'x:16.1.PB', 54),
            small(PLAIN, 'x', 'isotropic', 44, 3, 8, False, 'x:16.1.LM', 55),
            small(IMAGE, 'x', 'diagonal', 13, 5, 4, False, 'i:2.4.16', 56),
            small(PLAIN, 'x', 'diagonal', 4, 3, 5, True, 'g:3', 57)]


@pytest.mark.parametrize('c', OUTLIERS, ids=case_id)
def test_outlier_frame(c):
    '''One frame 40 standard deviations out: finite outputs, responsibilities that sum to 1, and
    its log-normalisers (thousands of nats) right relative to their own magnitude.'''
    assert case_route(c) == route_value(c.form, c.arith)
    T = 129
    inp = case_inputs(c, T, outlier=True)
    ln, resps, _ = et.truth(c.cov, inp, c.S, c.G)
    t = T // 2
    assert np.abs(ln[t]).min() > 20 * np.abs(np.delete(ln, t, 0)).max()
    got = execute(c, T, inp, want_sum=False)
    assert np.isfinite(got['ln']).all()
    rel = 1e-9 if c.arith == 'f64' else 1e-5
    err = np.abs(got['ln'][t] - ln[t]) / np.abs(ln[t])
    print(f'{case_id(c)} outlier: |ln| {np.abs(ln[t]).max():.0f} relative error {err.max():.3e}')
    assert err.max() <= rel
    rest = np.arange(T) != t
    ordinary = {k: v[rest] for k, v in got.items()}
    compare(c, T - 1, ordinary, ln[rest], resps[rest], ' beside the outlier')
    if 'resps' in got:
        assert np.isfinite(got['resps']).all()
        scale = float(np.abs(ln[rest]).max())
        tol = 1e-9 if c.arith == 'f64' else 2e-5 * scale
        sums = got['resps'].reshape(T, c.S, c.G).sum(2)
        assert np.abs(sums - 1.).max() <= tol
        # the frame's own responsibilities: the oracle's, where it tells the components apart
        assert np.abs(got['resps'][t] - resps[t]).max() <= max(tol, rel * np.abs(ln[t]).max())


@pytest.mark.parametrize('arith', ['f64', 'exact', 'x'])
@pytest.mark.parametrize('cov', et.COVS)
def test_labels(cov, arith):
    '`labels` (mixture.py:85-87): one-hot responsibilities, log_norm[t] = l[t, label].'
    c = small(PLAIN, arith, cov, 13, 1, 17, True, 'g:4', 61)
    args = case_args(c) | _hip.ARG_LABELS
    assert case_route(c, args) == route_value('g:4')
    assert case_route(c, args & ~_hip.ARG_RESPS) == _hip.EINVAL                 # nowhere to put pc_llh
    inp = case_inputs(c)
    labels = np.random.default_rng(5).integers(0, 17, TMAX)
    ln, resps = et.labels_truth(cov, inp, labels)
    for T in TS:
        got = execute(c, T, inp, labels=labels)
        np.testing.assert_array_equal(got['resps'], resps[:T])
        compare(c, T, got, ln, resps, ' labels')
    assert execute(c, 0, inp, labels=labels)['sum'] == 0.


@pytest.mark.parametrize('arith', ['f64', 'exact', 'x'])
@pytest.mark.parametrize('cov', et.COVS)
def test_scaled_statistics_with_pc_llh(cov, arith):
    '''`stat_scale` != 1 (hmm.py:119) and `pc_llh`: the generic kernels, whatever the shape;
    pc_llh alone is pass 1 only.'''
    c = small(PLAIN, arith, cov, 5, 5, 16, True, 'g:2', 71)
    args = case_args(c)
    assert _hip.estep_family(case_route(c, args)) != _hip.ESTEP_GENERIC
    assert case_route(c, args | _hip.ARG_SCALED) == route_value('g:2')
    assert case_route(c, args | _hip.ARG_PC_LLH) == route_value('g:2')
    assert case_route(c, _hip.ARG_PC_LLH | _hip.ARG_LOG_WEIGHTS) == route_value('g:1')
    inp = case_inputs(c)
    X, E = inp['X'].astype(np.float64), inp['E'].astype(np.float64)
    pc = orc.normal_llh(.8 * orc.SUFFSTATS[cov](X), E, c.D)
    w = pc.reshape(-1, c.S, c.G) + inp['lw'].astype(np.float64)[None]
    ln = orc.logsumexp(w, axis=-1)
    resps = np.exp(w - ln[:, :, None]).reshape(-1, c.S * c.G)
    for T in TS:
        got = execute(c, T, inp, scale=.8, want_pc=True)
        compare(c, T, got, ln, resps, ' scaled')
        tol = 1e-9 if arith == 'f64' else 1e-5 * np.abs(pc[:T]).max()
        assert np.abs(got['pc'] - pc[:T]).max() <= tol
        only = execute(small(PLAIN, arith, cov, 5, 5, 16, False, 'g:1', 71), T, inp, scale=.8,
                       want_pc=True, want_sum=False, want_ln=False)
        np.testing.assert_array_equal(only['pc'], got['pc'])


K1_CASES = [small(PACKED, 'x', 'full', 13, 5, 16, True, 'x:16.1.PB', 81),
            small(PACKED, 'x', 'full', 40, 1, 256, True, 'x:16.4.PBT', 82)]


@pytest.mark.parametrize('c', K1_CASES, ids=case_id)
def test_k1_lds_gives_the_same_bits(c):
    '`BEER_OPT_K1_LDS` 1 against 0 at small T: another kernel, the same products in the same order.'
    inp = case_inputs(c)
    off = c._replace(opts=(('k1_lds', 0),), form=c.form.replace('B', ''))
    assert case_route(c) == route_value(c.form) and case_route(off) == route_value(off.form)
    assert case_route(c) != case_route(off)
    for T in TS:
        a, b = execute(c, T, inp), execute(off, T, inp)
        np.testing.assert_array_equal(a['ln'], b['ln'])
        np.testing.assert_array_equal(a['resps'], b['resps'])
