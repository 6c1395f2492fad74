"""Every launch form of the accumulation kernels (csrc/estep.hip, estep_mfma.hip, estep_bf16.hip,
acc_diag.hip behind `beer_normal_accumulate`, `beer_normal_accumulate_packed`,
`beer_mixtureset_accumulate_packed` and `beer_mixtureset_accumulate_fused`) against the float64
oracle (`orc.mixtureset_accumulate`) at small shapes: the seed of the accumulation sweep.

One static table: each row names the form the launchers must pick for it
(`beer_accumulate_route`), and its test first holds the C layer's answer against the table, then
calls the C entry point itself through `_hip.call` at T = 0, 1, 65, 129 and 300 (whole and ragged
tiles of 32 and 64 frames; `acc_diag` at 16384 and 16385, the smallest it takes: eight chains, and
a ninth of one frame) and compares `acc`, which starts from non-zero values because the kernels
add, with the oracle in float64 on the values handed to the kernel: the frames and the
responsibilities rounded to the case's type; for the fused entry point the responsibilities
exp(logit - log_norm) of the log-normalisers `beer_mixtureset_estep` wrote for the same frames.
Packed responsibilities come from `beer_pack_resps`.  The workspace has exactly the advertised
size, is pre-filled with NaN and has 256 guard bytes behind it that must keep their bits, as must
two guard rows behind `acc`; T = 0 returns OK and writes nothing.

Shapes: K = 16 and 20 on the matrix-core families (132 where the form needs more than 128
components, 80 for the 128-component workgroups of `acc_diag`, 64 / 65 for blocks of four states
in the fused kernels), K = 3 and 17 on the generic kernel; D from 1, 5, 13, 40, 64, 96, 128 where
the form exists there, else the smallest D that has it (full covariance D = 9: two statistic
tiles per wave; 49 / 104 / 117 / 119: eight and seven tiles per wave of the packed kernel on
either side of D = 112; 17: two tiles of dimensions in `acc_diag`; 41: four k-steps, the nine
statistic tiles of the fused kernels; 2 and 5 beside 1 for the fused kernel without blocks of states).

Bounds (tests/test_gpu_parity.py, `tol_stats` of the matrix-core parity test, held per block of
the statistics by `assert_stats_close` as there): float64 1e-8, float32 1e-5.

Worst errors observed on an MI355X, as a fraction of the bound (the module prints them at its
end, `pytest -s`): float64 below 0.001; generic float32 0.03; exact fp32 MFMA 0.07; `acc_diag`
0.02; `accx_kernel` 0.08; `accf_kernel` 0.79 and `accfi_kernel` 0.91, both at T = 1 (DESIGN.md
section 17).

The cases `fused-...-D1-5x4-sr-f:6.8` found a launcher that sized the LDS of `accf_kernel`
without its final reduction (D = 1, 2: 6.5e-2 off from 256 frames on); DESIGN.md section 17."""

from collections import namedtuple

import numpy as np
import pytest
import torch

import estep_truth as et
from helpers import assert_stats_close, orc

pytestmark = pytest.mark.gpu

from beer_amd import _hip                                            # noqa: E402
from gpu_helpers import DEV, npy, tt                                 # noqa: E402

TS = (0, 1, 65, 129, 300)
TS_DIAG = (16384, 16385)
PLAIN, PACKED, FUSED = _hip.ACC_PLAIN, _hip.ACC_PACKED, _hip.ACC_FUSED
NP_OF = {'f64': np.float64, 'exact': np.float32, 'x': np.float32}
CODE_OF = {'f64': _hip.F64, 'exact': _hip.F32 | _hip.EXACT, 'x': _hip.F32}
TOL = {'f64': 1e-8, 'exact': 1e-5, 'x': 1e-5}
GUARD = 256


def route_value(spec, arith='x'):
    '''The `beer_accumulate_route` value of a form written as
    'g' (accumulate_kernel), 'e:NQ[.s]' (acc_kernel, float32 or float64 by `arith`; s: HAS_SR),
    'd:NJ2.NC[.p]' (accd_kernel; p: partial sums), 'x:NQ.FLAGS' (accx_kernel; s SR, x one X^T
    tile, t X^T reused), 'f:NQT.W[.b]' (accf_kernel; b BLK) or 'i:NKU.W.NS' (accfi_kernel).'''
    kind, _, rest = spec.partition(':')
    f = rest.split('.')
    if kind == 'g':
        return _hip.ACC_GENERIC
    if kind == 'e':
        fam = _hip.ACC_EXACT_F64 if arith == 'f64' else _hip.ACC_EXACT_F32
        return fam | int(f[0]) | (_hip.ACC_SR if f[1:] == ['s'] else 0)
    if kind == 'd':
        return _hip.ACC_DIAG | int(f[0]) | int(f[1]) << 4 | (_hip.ACC_D_PARTIAL if f[2:] == ['p'] else 0)
    if kind == 'x':
        flags = {'s': _hip.ACC_SR, 'x': _hip.ACC_X_SX, 't': _hip.ACC_X_XT_REUSED}
        return _hip.ACC_ACCX | int(f[0]) | sum(flags[ch] for ch in f[1])
    if kind == 'f':
        return _hip.ACC_ACCF | int(f[0]) | int(f[1]) << 21 | (_hip.ACC_F_BLK if f[2:] == ['b'] else 0)
    assert kind == 'i'
    return _hip.ACC_ACCF | _hip.ACC_F_IMAGE | int(f[0]) << 4 | int(f[1]) << 21 | int(f[2]) << 16


# entry, arithmetic, covariance type, D, S, G, state posteriors given, option ('nows': no
# workspace; 'image8' / 'image4': a frame image, BEER_OPT_ACCFI_WAVES = 8 / 4), the form
C = namedtuple('C', 'entry arith cov D S G sr opt form')
CASES = [
    C(PLAIN, 'f64', 'full', 5, 1, 3, False, '', 'g'),
    C(PLAIN, 'f64', 'full', 13, 17, 1, True, '', 'g'),
    C(PLAIN, 'exact', 'full', 5, 1, 3, False, '', 'g'),
    C(PLAIN, 'exact', 'full', 13, 17, 1, True, '', 'g'),
    C(PLAIN, 'x', 'full', 5, 1, 3, False, '', 'g'),
    C(PLAIN, 'x', 'full', 13, 17, 1, True, '', 'g'),
    C(PLAIN, 'exact', 'full', 1, 1, 16, False, '', 'e:1'),
    C(PLAIN, 'exact', 'full', 1, 5, 4, True, '', 'e:1.s'),
    C(PLAIN, 'exact', 'full', 13, 1, 16, False, '', 'e:4'),
    C(PLAIN, 'exact', 'full', 96, 5, 4, True, '', 'e:4.s'),
    C(PLAIN, 'x', 'diagonal', 96, 1, 20, False, '', 'e:4'),
    C(PLAIN, 'exact', 'full', 9, 1, 16, False, '', 'e:2'),
    C(PLAIN, 'exact', 'full', 9, 5, 4, True, '', 'e:2.s'),
    C(PLAIN, 'f64', 'full', 1, 1, 16, False, '', 'e:1'),
    C(PLAIN, 'f64', 'full', 1, 5, 4, True, '', 'e:1.s'),
    C(PLAIN, 'f64', 'full', 13, 1, 16, False, '', 'e:4'),
    C(PLAIN, 'f64', 'full', 13, 5, 4, True, '', 'e:4.s'),
    C(PLAIN, 'f64', 'full', 9, 1, 16, False, '', 'e:2'),
    C(PLAIN, 'f64', 'full', 9, 5, 4, True, '', 'e:2.s'),
    C(PACKED, 'x', 'full', 1, 1, 16, False, '', 'x:6.'),
    C(PACKED, 'x', 'full', 1, 2, 8, True, '', 'x:6.s'),
    C(PACKED, 'x', 'full', 1, 1, 132, False, '', 'x:6.t'),
    C(PACKED, 'x', 'full', 40, 1, 16, False, '', 'x:7.'),
    C(PACKED, 'x', 'full', 40, 2, 8, True, '', 'x:7.s'),
    C(PACKED, 'x', 'full', 40, 1, 132, False, '', 'x:7.t'),
    C(PACKED, 'x', 'full', 128, 1, 16, False, '', 'x:6.x'),
    C(PACKED, 'x', 'full', 128, 2, 8, True, '', 'x:6.sx'),
    C(PACKED, 'x', 'full', 128, 1, 132, False, '', 'x:6.xt'),
    C(PACKED, 'x', 'full', 49, 1, 16, False, '', 'x:8.'),
    C(PACKED, 'x', 'full', 49, 2, 8, True, '', 'x:8.s'),
    C(PACKED, 'x', 'full', 49, 1, 132, False, '', 'x:8.t'),
    C(PACKED, 'x', 'full', 104, 2, 8, True, '', 'x:8.sx'),
    C(PACKED, 'x', 'full', 117, 2, 8, True, '', 'x:7.sx'),
    C(PACKED, 'x', 'full', 119, 1, 16, False, '', 'x:7.x'),
    C(PACKED, 'x', 'full', 119, 1, 132, False, '', 'x:7.xt'),
    C(PLAIN, 'f64', 'diagonal', 13, 1, 3, False, '', 'g'),
    C(PLAIN, 'f64', 'diagonal', 40, 17, 1, True, '', 'g'),
    C(PLAIN, 'exact', 'diagonal', 13, 1, 3, False, '', 'g'),
    C(PLAIN, 'exact', 'diagonal', 40, 17, 1, True, '', 'g'),
    C(PLAIN, 'x', 'diagonal', 13, 1, 3, False, '', 'g'),
    C(PLAIN, 'x', 'diagonal', 40, 17, 1, True, '', 'g'),
    C(PLAIN, 'exact', 'diagonal', 1, 1, 16, False, '', 'e:1'),
    C(PLAIN, 'exact', 'diagonal', 1, 5, 4, True, '', 'e:1.s'),
    C(PLAIN, 'exact', 'diagonal', 40, 1, 16, False, '', 'e:2'),
    C(PLAIN, 'exact', 'diagonal', 40, 5, 4, True, '', 'e:2.s'),
    C(PLAIN, 'exact', 'diagonal', 64, 1, 16, False, '', 'e:4'),
    C(PLAIN, 'exact', 'diagonal', 64, 5, 4, True, '', 'e:4.s'),
    C(PLAIN, 'f64', 'diagonal', 1, 1, 16, False, '', 'e:1'),
    C(PLAIN, 'f64', 'diagonal', 1, 5, 4, True, '', 'e:1.s'),
    C(PLAIN, 'f64', 'diagonal', 40, 1, 16, False, '', 'e:2'),
    C(PLAIN, 'f64', 'diagonal', 40, 5, 4, True, '', 'e:2.s'),
    C(PLAIN, 'f64', 'diagonal', 64, 1, 16, False, '', 'e:4'),
    C(PLAIN, 'f64', 'diagonal', 64, 5, 4, True, '', 'e:4.s'),
    C(PLAIN, 'x', 'diagonal', 1, 1, 16, False, '', 'd:1.1.p'),
    C(PLAIN, 'x', 'diagonal', 1, 1, 16, False, 'nows', 'd:1.1'),
    C(PLAIN, 'x', 'diagonal', 1, 1, 80, False, '', 'd:1.2.p'),
    C(PLAIN, 'x', 'diagonal', 1, 1, 80, False, 'nows', 'd:1.2'),
    C(PLAIN, 'x', 'diagonal', 40, 1, 16, False, '', 'd:3.1.p'),
    C(PLAIN, 'x', 'diagonal', 40, 1, 16, False, 'nows', 'd:3.1'),
    C(PLAIN, 'x', 'diagonal', 40, 1, 80, False, '', 'd:3.2.p'),
    C(PLAIN, 'x', 'diagonal', 40, 1, 80, False, 'nows', 'd:3.2'),
    C(PLAIN, 'x', 'diagonal', 64, 1, 20, False, '', 'd:4.1.p'),
    C(PLAIN, 'x', 'diagonal', 64, 1, 20, False, 'nows', 'd:4.1'),
    C(PLAIN, 'x', 'diagonal', 64, 1, 80, False, '', 'd:4.2.p'),
    C(PLAIN, 'x', 'diagonal', 64, 1, 80, False, 'nows', 'd:4.2'),
    C(PLAIN, 'x', 'diagonal', 17, 1, 20, False, '', 'd:2.1.p'),
    C(PLAIN, 'x', 'diagonal', 17, 1, 20, False, 'nows', 'd:2.1'),
    C(PLAIN, 'x', 'diagonal', 17, 1, 80, False, '', 'd:2.2.p'),
    C(PLAIN, 'x', 'diagonal', 17, 1, 80, False, 'nows', 'd:2.2'),
    C(PACKED, 'x', 'diagonal', 1, 1, 16, False, '', 'x:6.'),
    C(PACKED, 'x', 'diagonal', 1, 1, 132, False, '', 'x:6.t'),
    C(PACKED, 'x', 'diagonal', 128, 1, 16, False, '', 'x:6.x'),
    C(PACKED, 'x', 'diagonal', 128, 1, 132, False, '', 'x:6.xt'),
    C(FUSED, 'x', 'diagonal', 1, 4, 4, False, '', 'f:6.8.b'),
    C(FUSED, 'x', 'diagonal', 1, 4, 4, False, 'image8', 'i:1.8.4'),
    C(FUSED, 'x', 'diagonal', 1, 4, 4, False, 'image4', 'i:1.4.4'),
    C(FUSED, 'x', 'diagonal', 1, 5, 4, True, '', 'f:6.8'),
    C(FUSED, 'x', 'diagonal', 5, 5, 4, True, '', 'f:6.8'),
    C(FUSED, 'x', 'diagonal', 2, 5, 4, False, '', 'f:6.8'),
    C(FUSED, 'x', 'diagonal', 1, 5, 4, True, 'image8', 'i:1.8.16'),
    C(FUSED, 'x', 'diagonal', 1, 5, 4, True, 'image4', 'i:1.4.16'),
    C(FUSED, 'x', 'diagonal', 13, 4, 4, False, 'image8', 'i:2.8.4'),
    C(FUSED, 'x', 'diagonal', 13, 4, 4, False, 'image4', 'i:2.4.4'),
    C(FUSED, 'x', 'diagonal', 13, 5, 4, True, 'image8', 'i:2.8.16'),
    C(FUSED, 'x', 'diagonal', 13, 5, 4, True, 'image4', 'i:2.4.16'),
    C(FUSED, 'x', 'diagonal', 40, 4, 4, True, 'image8', 'i:3.8.4'),
    C(FUSED, 'x', 'diagonal', 40, 4, 4, True, 'image4', 'i:3.4.4'),
    C(FUSED, 'x', 'diagonal', 40, 5, 4, False, 'image8', 'i:3.8.16'),
    C(FUSED, 'x', 'diagonal', 40, 5, 4, False, 'image4', 'i:3.4.16'),
    C(FUSED, 'x', 'diagonal', 64, 4, 4, True, '', 'f:10.4.b'),
    C(FUSED, 'x', 'diagonal', 64, 5, 4, False, '', 'f:10.4'),
    C(FUSED, 'x', 'diagonal', 41, 4, 4, False, '', 'f:9.4.b'),
    C(FUSED, 'x', 'diagonal', 41, 4, 4, False, 'image8', 'i:4.8.4'),
    C(FUSED, 'x', 'diagonal', 41, 4, 4, False, 'image4', 'i:4.4.4'),
    C(FUSED, 'x', 'diagonal', 41, 5, 4, True, '', 'f:9.4'),
    C(FUSED, 'x', 'diagonal', 41, 5, 4, True, 'image8', 'i:4.8.16'),
    C(FUSED, 'x', 'diagonal', 41, 5, 4, True, 'image4', 'i:4.4.16'),
    C(PLAIN, 'f64', 'isotropic', 40, 1, 3, False, '', 'g'),
    C(PLAIN, 'f64', 'isotropic', 5, 17, 1, True, '', 'g'),
    C(PLAIN, 'exact', 'isotropic', 40, 1, 3, False, '', 'g'),
    C(PLAIN, 'exact', 'isotropic', 5, 17, 1, True, '', 'g'),
    C(PLAIN, 'x', 'isotropic', 40, 1, 3, False, '', 'g'),
    C(PLAIN, 'x', 'isotropic', 5, 17, 1, True, '', 'g'),
    C(PLAIN, 'exact', 'isotropic', 1, 1, 16, False, '', 'e:1'),
    C(PLAIN, 'exact', 'isotropic', 1, 5, 4, True, '', 'e:1.s'),
    C(PLAIN, 'exact', 'isotropic', 40, 1, 16, False, '', 'e:2'),
    C(PLAIN, 'exact', 'isotropic', 40, 5, 4, True, '', 'e:2.s'),
    C(PLAIN, 'exact', 'isotropic', 64, 1, 16, False, '', 'e:4'),
    C(PLAIN, 'exact', 'isotropic', 64, 5, 4, True, '', 'e:4.s'),
    C(PLAIN, 'f64', 'isotropic', 1, 1, 16, False, '', 'e:1'),
    C(PLAIN, 'f64', 'isotropic', 1, 5, 4, True, '', 'e:1.s'),
    C(PLAIN, 'f64', 'isotropic', 40, 1, 16, False, '', 'e:2'),
    C(PLAIN, 'f64', 'isotropic', 40, 5, 4, True, '', 'e:2.s'),
    C(PLAIN, 'f64', 'isotropic', 64, 1, 16, False, '', 'e:4'),
    C(PLAIN, 'f64', 'isotropic', 64, 5, 4, True, '', 'e:4.s'),
    C(PLAIN, 'x', 'isotropic', 1, 1, 16, False, '', 'd:1.1.p'),
    C(PLAIN, 'x', 'isotropic', 1, 1, 16, False, 'nows', 'd:1.1'),
    C(PLAIN, 'x', 'isotropic', 1, 1, 80, False, '', 'd:1.2.p'),
    C(PLAIN, 'x', 'isotropic', 1, 1, 80, False, 'nows', 'd:1.2'),
    C(PLAIN, 'x', 'isotropic', 40, 1, 16, False, '', 'd:3.1.p'),
    C(PLAIN, 'x', 'isotropic', 40, 1, 16, False, 'nows', 'd:3.1'),
    C(PLAIN, 'x', 'isotropic', 40, 1, 80, False, '', 'd:3.2.p'),
    C(PLAIN, 'x', 'isotropic', 40, 1, 80, False, 'nows', 'd:3.2'),
    C(PLAIN, 'x', 'isotropic', 64, 1, 20, False, '', 'd:4.1.p'),
    C(PLAIN, 'x', 'isotropic', 64, 1, 20, False, 'nows', 'd:4.1'),
    C(PLAIN, 'x', 'isotropic', 64, 1, 80, False, '', 'd:4.2.p'),
    C(PLAIN, 'x', 'isotropic', 64, 1, 80, False, 'nows', 'd:4.2'),
    C(PLAIN, 'x', 'isotropic', 17, 1, 20, False, '', 'd:2.1.p'),
    C(PLAIN, 'x', 'isotropic', 17, 1, 20, False, 'nows', 'd:2.1'),
    C(PLAIN, 'x', 'isotropic', 17, 1, 80, False, '', 'd:2.2.p'),
    C(PLAIN, 'x', 'isotropic', 17, 1, 80, False, 'nows', 'd:2.2'),
    C(PACKED, 'x', 'isotropic', 1, 1, 16, False, '', 'x:6.'),
    C(PACKED, 'x', 'isotropic', 1, 1, 132, False, '', 'x:6.t'),
    C(PACKED, 'x', 'isotropic', 128, 1, 16, False, '', 'x:6.x'),
    C(PACKED, 'x', 'isotropic', 128, 1, 132, False, '', 'x:6.xt'),
    C(FUSED, 'x', 'isotropic', 1, 4, 4, False, '', 'f:6.8.b'),
    C(FUSED, 'x', 'isotropic', 1, 4, 4, False, 'image8', 'i:1.8.4'),
    C(FUSED, 'x', 'isotropic', 1, 4, 4, False, 'image4', 'i:1.4.4'),
    C(FUSED, 'x', 'isotropic', 1, 5, 4, True, '', 'f:6.8'),
    C(FUSED, 'x', 'isotropic', 5, 5, 4, True, '', 'f:6.8'),
    C(FUSED, 'x', 'isotropic', 1, 5, 4, True, 'image8', 'i:1.8.16'),
    C(FUSED, 'x', 'isotropic', 1, 5, 4, True, 'image4', 'i:1.4.16'),
    C(FUSED, 'x', 'isotropic', 13, 4, 4, False, 'image8', 'i:2.8.4'),
    C(FUSED, 'x', 'isotropic', 13, 4, 4, False, 'image4', 'i:2.4.4'),
    C(FUSED, 'x', 'isotropic', 13, 5, 4, True, 'image8', 'i:2.8.16'),
    C(FUSED, 'x', 'isotropic', 13, 5, 4, True, 'image4', 'i:2.4.16'),
    C(FUSED, 'x', 'isotropic', 40, 4, 4, True, 'image8', 'i:3.8.4'),
    C(FUSED, 'x', 'isotropic', 40, 4, 4, True, 'image4', 'i:3.4.4'),
    C(FUSED, 'x', 'isotropic', 40, 5, 4, False, 'image8', 'i:3.8.16'),
    C(FUSED, 'x', 'isotropic', 40, 5, 4, False, 'image4', 'i:3.4.16'),
    C(FUSED, 'x', 'isotropic', 64, 4, 4, True, '', 'f:10.4.b'),
    C(FUSED, 'x', 'isotropic', 64, 5, 4, False, '', 'f:10.4'),
    C(FUSED, 'x', 'isotropic', 41, 4, 4, False, '', 'f:9.4.b'),
    C(FUSED, 'x', 'isotropic', 41, 4, 4, False, 'image8', 'i:4.8.4'),
    C(FUSED, 'x', 'isotropic', 41, 4, 4, False, 'image4', 'i:4.4.4'),
    C(FUSED, 'x', 'isotropic', 41, 5, 4, True, '', 'f:9.4'),
    C(FUSED, 'x', 'isotropic', 41, 5, 4, True, 'image8', 'i:4.8.16'),
    C(FUSED, 'x', 'isotropic', 41, 5, 4, True, 'image4', 'i:4.4.16'),
]


def case_id(c):
    return f"{'plain packed fused'.split()[c.entry]}-{c.arith}-{c.cov[:4]}-D{c.D}-{c.S}x{c.G}" \
           f"{'-sr' if c.sr else ''}{'-' + c.opt if c.opt else ''}-{c.form}"


def case_seed(c):
    return 1000 + 131 * c.D + 17 * c.S + c.G + 7 * et.COVS.index(c.cov)


def case_args(c):
    return ((_hip.ARG_RESPS if c.entry != FUSED else 0) | (_hip.ARG_STATE_RESPS if c.sr else 0) |
            (_hip.ARG_IMAGE if c.opt.startswith('image') else 0))


def case_ts(c):
    return TS_DIAG if c.form.startswith('d:') else TS


def case_ws_bytes(c, T):
    'The advertised workspace of the case (what Python sizes its scratch by), 0 with `nows`.'
    lib, cov = _hip.lib(), _hip.COV_CODE[c.cov]
    if c.opt == 'nows':
        return 0
    if c.entry == PLAIN:
        return lib.beer_accumulate_frames_workspace_bytes(CODE_OF[c.arith] & ~_hip.EXACT, cov, T, c.D, c.S, c.G)
    if c.entry == FUSED:
        return lib.beer_accumulate_fused_workspace_bytes(cov, c.D, c.S, c.G)
    if c.sr:
        return lib.beer_mixtureset_accumulate_packed_workspace_bytes(cov, T, c.D, c.S, c.G)
    return lib.beer_accumulate_packed_workspace_bytes(cov, T, c.D, c.S * c.G)


def case_route(c, T):
    old = _hip.set_option('accfi_waves', 4 if c.opt == 'image4' else 8)
    try:
        return _hip.accumulate_route(c.entry, CODE_OF[c.arith], _hip.COV_CODE[c.cov], T, c.D, c.S, c.G,
                                     case_args(c), case_ws_bytes(c, T))
    finally:
        _hip.set_option('accfi_waves', old)


WORST = {}


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    for fam, (frac, cid) in sorted(WORST.items()):
        print(f'\nworst error / bound, {fam}: {frac:.3f} ({cid})', end='')
    print()


def guarded(nbytes):
    'A buffer of `nbytes` of NaN (all bits set) with a guard behind it, and the guard\'s copy.'
    buf = torch.full((nbytes + GUARD,), 0xff, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = torch.arange(GUARD, dtype=torch.uint8, device=DEV)
    return buf


def guard_kept(buf, nbytes):
    return bool((buf[nbytes:] == torch.arange(GUARD, dtype=torch.uint8, device=DEV)).all())


def inputs(c, seed):
    '''What the case hands its kernel for its longest T (a shorter T takes a prefix), in the case's
    type: frames, responsibilities within each state [T, S G], state posteriors [T, S] (sparse,
    the first frame dense), and for the fused entry point E[T] and the log-weights.'''
    rng = np.random.default_rng(seed)
    T, K, dt = max(case_ts(c)), c.S * c.G, NP_OF[c.arith]
    inp = et.make(c.cov, c.D, c.S, c.G, T, seed, dt)
    if c.entry != FUSED:
        inp['X'] = (rng.standard_normal((T, c.D)) * 1.2 + .7).astype(dt)
        r = rng.random((T, c.S, c.G)) * (rng.random((T, c.S, c.G)) < .8) + 1e-3
        inp['r'] = np.ascontiguousarray((r / r.sum(2, keepdims=True)).reshape(T, K).astype(dt))
    sr = rng.random((T, c.S)) * (rng.random((T, c.S)) < .6)
    sr[0] = .25 + .5 * rng.random(c.S)
    inp['sr'] = np.ascontiguousarray(sr.astype(dt)) if c.sr else None
    return inp


def truth(c, inp, T, ln=None):
    'orc.mixtureset_accumulate in float64 on the first T frames of `inp` (fused: with `ln`).'
    X = inp['X'][:T].astype(np.float64)
    stats = orc.SUFFSTATS[c.cov](X)
    if c.entry == FUSED:
        r = orc.mixtureset_estep(stats, inp['E'].astype(np.float64), c.D, inp['lw'].astype(np.float64))[1]
    else:
        r = inp['r'][:T].astype(np.float64).reshape(T, c.S, c.G)
    sr = np.ones((T, c.S)) if inp['sr'] is None else inp['sr'][:T].astype(np.float64)
    return orc.mixtureset_accumulate(stats, r, sr)[1]


def run(c, inp, T):
    'One call of the case\'s entry point on T frames: (acc - acc0 [K, Q], what it must equal).'
    lib, cov, K = _hip.lib(), _hip.COV_CODE[c.cov], c.S * c.G
    Q = {'full': c.D * c.D + c.D + 2, 'diagonal': 2 * c.D + 2, 'isotropic': c.D + 3}[c.cov]
    n = max(T, 1)                                  # (no null pointers at T = 0)
    X = tt(inp['X'][:n])
    sr = tt(inp['sr'][:n]) if c.sr else None
    # acc starts from eighths: (acc0 + sum) - acc0 gives the sum back to 1e-16 of acc0
    acc0 = ((torch.arange((K + 2) * Q, device=DEV) % 7 + 1).double() / 8.).reshape(K + 2, Q)
    acc = acc0.clone()
    nws = case_ws_bytes(c, T)
    ws = guarded(nws) if nws else None
    assert case_route(c, T) == route_value(c.form, c.arith), (case_id(c), T, hex(case_route(c, T)))
    ln = None
    if c.entry == PLAIN:
        _hip.call('beer_normal_accumulate', CODE_OF[c.arith], cov, T, c.D, c.S, c.G, _hip.ptr(X),
                  _hip.ptr(tt(inp['r'][:n])), _hip.ptr(sr), _hip.ptr(acc), _hip.ptr(ws), nws)
    elif c.entry == PACKED:
        npk = lib.beer_packed_resps_bytes(T, c.D, K)
        packed = guarded(npk)
        _hip.call('beer_pack_resps', T, c.D, c.S, c.G, _hip.ptr(X), _hip.ptr(tt(inp['r'][:n])), None,
                  _hip.ptr(packed))
        if c.sr:
            _hip.call('beer_mixtureset_accumulate_packed', cov, T, c.D, c.S, c.G, _hip.ptr(X),
                      _hip.ptr(packed), _hip.ptr(sr), _hip.ptr(acc), _hip.ptr(ws), nws)
        else:
            _hip.call('beer_normal_accumulate_packed', cov, T, c.D, K, _hip.ptr(X), _hip.ptr(packed),
                      _hip.ptr(acc), _hip.ptr(ws), nws)
        assert guard_kept(packed, npk)
    else:
        E, lw = tt(inp['E']), tt(inp['lw'])
        lnt = torch.zeros(n, c.S, dtype=torch.float32, device=DEV)
        nes = lib.beer_estep_workspace_bytes(_hip.F32, cov, c.D, c.S, c.G)
        es = guarded(nes)
        _hip.call('beer_mixtureset_estep', _hip.F32, cov, T, c.D, c.S, c.G, _hip.ptr(X), _hip.ptr(E),
                  _hip.ptr(lw), None, 1., None, _hip.ptr(lnt), None, None, _hip.ptr(es), nes)
        image = None
        if c.opt.startswith('image'):
            nim = lib.beer_frame_image_bytes(cov, T, c.D)
            assert nim > 0
            image = guarded(nim)
            _hip.call('beer_frame_image', cov, T, c.D, _hip.ptr(X), _hip.ptr(image), nim)
        old = _hip.set_option('accfi_waves', 4 if c.opt == 'image4' else 8)
        try:
            _hip.call('beer_mixtureset_accumulate_fused', cov, T, c.D, c.S, c.G, _hip.ptr(X), _hip.ptr(E),
                      _hip.ptr(lw), _hip.ptr(lnt), _hip.ptr(sr), _hip.ptr(image), _hip.ptr(acc),
                      _hip.ptr(ws), nws)
        finally:
            _hip.set_option('accfi_waves', old)
        ln = npy(lnt)[:T]
    torch.cuda.synchronize()
    assert ws is None or guard_kept(ws, nws), 'workspace guard'
    assert torch.equal(acc[K:], acc0[K:]), 'guard rows behind acc'
    if T == 0:
        assert torch.equal(acc, acc0)
        assert ws is None or bool((ws[:nws] == 0xff).all()), 'T = 0 wrote to the workspace'
        return None, None
    return npy(acc[:K] - acc0[:K]), truth(c, inp, T, ln)


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_accumulation_form_vs_oracle(c):
    inp = inputs(c, case_seed(c))
    for T in case_ts(c):
        got, want = run(c, inp, T)
        if T == 0:
            continue
        assert np.isfinite(got).all(), (case_id(c), T)
        errs = assert_stats_close(got, want, c.D, TOL[c.arith], f'{case_id(c)} T={T}')
        fam = c.form.split(':')[0] + ('64' if c.arith == 'f64' else '')
        frac = max(errs.values()) / TOL[c.arith]
        if frac > WORST.get(fam, (0., ''))[0]:
            WORST[fam] = (frac, f'{case_id(c)} T={T}')
