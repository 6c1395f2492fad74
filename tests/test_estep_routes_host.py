"""CPU checks of the E-step dispatch: `beer_estep_route` on both sides of every boundary of the
launch code (csrc/estep.hip estep_plan, estep_mfma.hip llh_form, estep_bf16.hip llhx_form), the
refusals of the entry points themselves, the case table of tests/test_gpu_estep_routes.py (every
case's stated form what the query gives, every form the query can return named by a case), what
Python concludes from the query (`kernels.estep_buffers`), and the
conditions under which the generated inputs of tests/estep_truth.py can tell a wrong kernel from a
right one."""

import ctypes
import os
import re

import numpy as np
import pytest

import estep_truth as et
from helpers import ROOT, orc
import test_gpu_estep_routes as table
from test_gpu_estep_routes import IMAGE, PACKED, PLAIN, route_value

from beer_amd import _hip, kernels

EINVAL = _hip.EINVAL
LN, RESPS, SUM, PC, LABELS, SCALED, LW = (_hip.ARG_LOG_NORM, _hip.ARG_RESPS, _hip.ARG_LLH_SUM,
                                          _hip.ARG_PC_LLH, _hip.ARG_LABELS, _hip.ARG_SCALED,
                                          _hip.ARG_LOG_WEIGHTS)
CODE_OF = table.CODE_OF


def ws_bytes(arith, cov, D, S, G):
    return _hip.lib().beer_estep_workspace_bytes(CODE_OF[arith] & ~_hip.EXACT, _hip.COV_CODE[cov], D, S, G)


def route(entry=PLAIN, arith='x', cov='full', D=13, S=1, G=16, args=LN | SUM | LW, ws=None, opts=()):
    'The query; `ws`: None = the advertised size, else bytes relative to it (0: none at all).'
    full = ws_bytes(arith, cov, D, S, G)
    nbytes = full if ws is None else (0 if ws == 0 else full + ws)
    old = [(k, _hip.set_option(k, v)) for k, v in opts]
    try:
        return _hip.estep_route(entry, CODE_OF[arith], _hip.COV_CODE[cov], D, S, G, args, nbytes)
    finally:
        for k, v in reversed(old):
            _hip.set_option(k, v)


R = LN | SUM | LW | RESPS
NOLNFI, NOK1 = (('lnfi', 0),), (('k1_lds', 0),)
# (arguments of `route`, the form as test_gpu_estep_routes.route_value writes it, or EINVAL)
BOUNDARIES = [
    # one mixture, K at 15|16, 64|65, 128|129, 256|257 -- on every matrix-core arithmetic
    (dict(G=15, args=R), 'g:3'), (dict(G=16), 'x:4.1.'), (dict(G=64), 'x:4.1.'), (dict(G=65), 'x:8.2.'),
    (dict(G=128), 'x:8.2.'), (dict(G=129), 'x:16.4.'), (dict(G=256), 'x:16.4.'),
    (dict(G=257, args=R), 'g:3'), (dict(G=257), EINVAL),
    (dict(arith='exact', G=15, args=R), 'g:3'), (dict(arith='exact', G=16), 'e:4.1.4'),
    (dict(arith='exact', G=64), 'e:4.1.4'), (dict(arith='exact', G=65), 'e:8.2.4'),
    (dict(arith='exact', G=128), 'e:8.2.4'), (dict(arith='exact', G=129), 'e:16.4.4'),
    (dict(arith='exact', G=256), 'e:16.4.4'), (dict(arith='exact', G=257, args=R), 'g:3'),
    (dict(arith='f64', G=15, args=R), 'g:3'), (dict(arith='f64', G=16), 'e:4.1.4'),
    (dict(arith='f64', G=64), 'e:4.1.4'), (dict(arith='f64', G=65), 'e:8.2.4'),
    (dict(arith='f64', G=128), 'e:8.2.4'), (dict(arith='f64', G=129), 'e:16.4.4'),
    (dict(arith='f64', G=256), 'e:16.4.4'), (dict(arith='f64', G=257, args=R), 'g:3'),
    (dict(entry=PACKED, G=15, args=R), EINVAL), (dict(entry=PACKED, G=16, args=R), 'x:4.1.P'),
    (dict(entry=PACKED, G=64, args=R), 'x:4.1.P'), (dict(entry=PACKED, G=65, args=R), 'x:8.2.P'),
    (dict(entry=PACKED, G=128, args=R), 'x:8.2.P'), (dict(entry=PACKED, G=129, args=R), 'x:16.4.PBT'),
    (dict(entry=PACKED, G=256, args=R), 'x:16.4.PBT'), (dict(entry=PACKED, G=257, args=R), EINVAL),
    (dict(entry=PACKED, G=16, args=R & ~LW), EINVAL), (dict(entry=PACKED, G=16, args=LN | LW), EINVAL),
    # D at 64|65 (float64), 96|97 (exact float32), 128|129 (bf16x3)
    (dict(arith='f64', D=64, S=5), 'e:16.1.4'), (dict(arith='f64', D=65, S=5, args=R), 'g:2'),
    (dict(arith='f64', D=65, S=5), EINVAL),
    (dict(arith='exact', D=96, S=5), 'e:16.1.4'), (dict(arith='exact', D=97, S=5, args=R), 'g:2'),
    (dict(arith='exact', D=97, S=5), EINVAL), (dict(D=97, S=5), 'x:16.1.LM'),
    (dict(D=128, S=5, args=R), 'x:16.1.'), (dict(D=129, S=5, args=R), 'g:2'), (dict(D=129, S=5), EINVAL),
    (dict(entry=PACKED, D=128, G=200, args=R), 'x:16.4.PT'), (dict(entry=PACKED, D=129, G=200, args=R), EINVAL),
    (dict(D=0), EINVAL), (dict(S=0), EINVAL), (dict(G=0), EINVAL),
    # G at 1, 2, 3|4 and the powers of two 4 .. 256|512 (S = 5: two chunks from G = 64)
    (dict(S=17, G=1), 'x:4.1.N'), (dict(S=17, G=1, arith='f64'), 'e:16.1.1'),
    (dict(S=9, G=2), 'x:16.1.'), (dict(S=9, G=2, arith='exact'), 'e:16.1.2'),
    (dict(S=6, G=3), 'x:16.1.LMD'), (dict(S=6, G=3, arith='exact', args=R), 'g:3'),
    (dict(S=6, G=3, arith='f64'), EINVAL),
    (dict(S=5, G=4), 'x:16.1.LM'), (dict(S=5, G=8), 'x:16.1.LM'), (dict(S=5, G=16), 'x:16.1.LM'),
    (dict(S=5, G=32), 'x:16.1.L'), (dict(S=5, G=64), 'x:16.1.L*2'), (dict(S=5, G=128), 'x:16.2.L*3'),
    (dict(S=5, G=256), 'x:16.4.L*5'), (dict(S=5, G=512, args=R), 'g:3'), (dict(S=5, G=512), EINVAL),
    (dict(S=5, G=4, args=R), 'x:16.1.'), (dict(S=5, G=64, args=R), 'x:16.1.*2'),
    (dict(S=5, G=128, args=R), 'x:16.2.*3'), (dict(S=5, G=256, args=R), 'x:16.4.*5'),
    (dict(S=5, G=4, arith='f64'), 'e:16.1.4'), (dict(S=5, G=64, arith='f64'), 'e:16.1.4*2'),
    (dict(S=5, G=128, arith='f64'), 'e:16.2.4*3'), (dict(S=5, G=256, arith='f64'), 'e:16.4.4*5'),
    (dict(S=5, G=512, arith='f64', args=R), 'g:3'),
    (dict(entry=PACKED, S=5, G=4, args=R), EINVAL), (dict(entry=PACKED, S=5, G=8, args=R), 'x:16.1.PB'),
    (dict(entry=PACKED, S=5, G=64, args=R), 'x:16.1.PB*2'),
    (dict(entry=PACKED, S=5, G=128, args=R), 'x:16.2.PB*3'), (dict(entry=PACKED, S=5, G=256, args=R), EINVAL),
    (dict(entry=PACKED, S=5, G=12, args=R), EINVAL),
    (dict(entry=PACKED, S=5, G=16, args=R, cov='diagonal'), EINVAL),
    # G not a power of two, with and without responsibilities wanted
    (dict(S=4, G=5), 'x:16.1.LMD'), (dict(S=4, G=5, args=R), 'g:3'), (dict(S=2, G=12), 'x:16.1.LMD'),
    (dict(S=2, G=20), 'x:16.1.LD'), (dict(S=2, G=20, args=R), 'g:3'), (dict(S=3, G=6, args=R), 'g:3'),
    (dict(S=2, G=100), 'x:16.2.LD'), (dict(S=2, G=200), 'x:16.4.LD*2'), (dict(S=2, G=257), EINVAL),
    (dict(S=3, G=3), EINVAL), (dict(S=3, G=3, args=R), 'g:3'),              # 3 x 4 slots: fewer than 16
    (dict(S=3, G=5), 'x:16.1.LMD'),
    (dict(S=1, G=5, args=R), 'g:3'),
    # S G at 256|257: component chunks
    (dict(S=16, G=16), 'x:16.1.LM'), (dict(S=17, G=16), 'x:16.1.LM*2'), (dict(S=32, G=16), 'x:16.1.LM*2'),
    (dict(S=33, G=16), 'x:16.1.LM*3'), (dict(S=256, G=1), 'x:16.1.'), (dict(S=257, G=1), 'x:16.1.*2'),
    (dict(S=16, G=16, arith='f64'), 'e:16.1.4'), (dict(S=17, G=16, arith='f64'), 'e:16.1.4*2'),
    # narrow at K = 64|65 and 128|129 (and K = 15|16)
    (dict(S=15, G=1), 'g:2'), (dict(S=16, G=1), 'x:4.1.N'), (dict(S=64, G=1), 'x:4.1.N'),
    (dict(S=65, G=1), 'x:8.1.N'), (dict(S=128, G=1), 'x:8.1.N'), (dict(S=129, G=1), 'x:16.1.'),
    (dict(S=64, G=1, args=R), 'x:4.1.N'),
    # K1-LDS (BL) at D = 52|53, and with the option off
    (dict(entry=PACKED, D=52, G=200, args=R), 'x:16.4.PBT'), (dict(entry=PACKED, D=53, G=200, args=R), 'x:16.4.PT'),
    (dict(entry=PACKED, D=52, G=200, args=R, opts=NOK1), 'x:16.4.PT'),
    (dict(entry=PACKED, D=52, G=200, args=R, cov='diagonal'), 'x:16.4.PT'),
    (dict(entry=PACKED, D=52, G=64, args=R), 'x:4.1.P'),
    (dict(entry=PACKED, D=52, S=5, G=16, args=R), 'x:16.1.PB'), (dict(entry=PACKED, D=53, S=5, G=16, args=R), 'x:16.1.P'),
    (dict(entry=PACKED, D=52, S=5, G=16, args=R, opts=NOK1), 'x:16.1.P'),
    (dict(entry=PACKED, D=52, S=2, G=128, args=R), 'x:16.2.PB'), (dict(entry=PACKED, D=53, S=2, G=128, args=R), 'x:16.2.P'),
    # lnfi at the k-step boundaries of diagonal / isotropic statistics: D = 12|13, 28|29, 40|41;
    # the image is refused from D = 49
    (dict(entry=IMAGE, cov='diagonal', D=12, S=5), 'i:1.16.16'), (dict(entry=IMAGE, cov='diagonal', D=13, S=5), 'i:2.16.16'),
    (dict(entry=IMAGE, cov='isotropic', D=28, S=5), 'i:2.16.16'), (dict(entry=IMAGE, cov='isotropic', D=29, S=5), 'i:3.16.16'),
    (dict(entry=IMAGE, cov='diagonal', D=40, S=5), 'i:3.16.16'), (dict(entry=IMAGE, cov='diagonal', D=41, S=5), 'x:16.1.LIM'),
    (dict(entry=IMAGE, cov='diagonal', D=48, S=5), 'x:16.1.LIM'), (dict(entry=IMAGE, cov='diagonal', D=49, S=5), EINVAL),
    (dict(entry=IMAGE, cov='isotropic', D=48, S=5, G=8), 'i:4.8.8'), (dict(entry=IMAGE, cov='isotropic', D=49, S=5, G=8), EINVAL),
    (dict(entry=IMAGE, cov='full', D=13, S=5), EINVAL), (dict(entry=IMAGE, cov='diagonal', D=13, S=1, G=64), EINVAL),
    (dict(entry=IMAGE, cov='diagonal', D=13, S=9, G=2), EINVAL), (dict(entry=IMAGE, cov='diagonal', D=13, S=6, G=3), 'i:2.4.16'),
    (dict(entry=IMAGE, cov='diagonal', D=13, S=5, args=R), EINVAL), (dict(entry=IMAGE, cov='diagonal', D=13, S=5, args=SUM | LW), EINVAL),
    # lnfi8 at G = 4, 8 against 16 (four k-steps: D = 41 .. 48), chunks of 128
    (dict(entry=IMAGE, cov='diagonal', D=44, S=5, G=4), 'i:4.4.8'), (dict(entry=IMAGE, cov='diagonal', D=44, S=5, G=8), 'i:4.8.8'),
    (dict(entry=IMAGE, cov='diagonal', D=44, S=5, G=16), 'x:16.1.LIM'), (dict(entry=IMAGE, cov='diagonal', D=44, S=5, G=32), 'x:16.1.LI'),
    (dict(entry=IMAGE, cov='diagonal', D=44, S=32, G=4), 'i:4.4.8'), (dict(entry=IMAGE, cov='diagonal', D=44, S=33, G=4), 'i:4.4.8*2'),
    (dict(entry=IMAGE, cov='diagonal', D=40, S=33, G=4), 'i:3.4.16'), (dict(entry=IMAGE, cov='diagonal', D=40, S=65, G=4), 'i:3.4.16*2'),
    # BEER_OPT_LNFI = 0
    (dict(entry=IMAGE, cov='diagonal', D=13, S=5, opts=NOLNFI), 'x:16.1.LIM'),
    (dict(entry=IMAGE, cov='diagonal', D=44, S=5, G=4, opts=NOLNFI), 'x:16.1.LIM'),
    (dict(entry=IMAGE, cov='diagonal', D=44, S=33, G=4, opts=NOLNFI), 'x:16.1.LIM'),
    (dict(entry=IMAGE, cov='diagonal', D=13, S=5, G=64, opts=NOLNFI), 'x:16.1.LI*2'),
    # labels, scaled statistics and pc_llh all force the generic kernels
    (dict(args=R | LABELS), 'g:4'), (dict(args=R | LABELS, arith='f64'), 'g:4'), (dict(args=LN | LABELS), EINVAL),
    (dict(args=LN | PC | LABELS), 'g:4'), (dict(S=5, args=R | LABELS), EINVAL),
    (dict(S=5, args=R | SCALED), 'g:2'), (dict(S=5, args=LN | SUM | SCALED), EINVAL), (dict(S=5, args=R | PC), 'g:2'),
    (dict(S=5, args=PC), 'g:1'), (dict(S=5, args=PC | SCALED, arith='f64'), 'g:1'), (dict(S=5, args=0), 'g:1'),
    (dict(S=80, G=1, args=LN | SCALED), 'g:2'), (dict(S=80, G=1, args=SUM), 'x:8.1.N'),
    (dict(S=5, G=1, args=SUM), EINVAL), (dict(S=5, G=1, args=LN), 'g:2'),
    (dict(entry=PACKED, S=5, args=R | SCALED), EINVAL), (dict(entry=IMAGE, cov='diagonal', S=5, args=LN | PC), EINVAL),
    (dict(entry=PACKED, arith='exact', args=R), EINVAL), (dict(entry=IMAGE, arith='f64', cov='diagonal', S=5), EINVAL),
    # no workspace; one byte short
    (dict(S=5, ws=0), EINVAL), (dict(S=5, args=R, ws=0), 'g:2'), (dict(S=5, ws=1), 'x:16.1.LM'),
    (dict(S=5, arith='f64', ws=-1), EINVAL), (dict(S=5, arith='f64', args=R, ws=-1), 'g:2'),
    (dict(S=80, G=1, arith='f64', ws=-1), 'g:2'),
    (dict(D=100, S=5, ws=-1), EINVAL), (dict(D=100, S=5, args=R, ws=-1), 'g:2'),
    # (float32 up to D = 96: the advertised size is that of the bf16x3 image, the larger one; a
    #  workspace one byte short still holds the exact kernel's, which then runs)
    (dict(S=5, ws=-1), 'e:16.1.4'), (dict(S=5, args=R, ws=-1), 'e:16.1.4'), (dict(S=80, G=1, ws=-1), 'e:16.1.1'),
    (dict(entry=PACKED, S=5, args=R, ws=-1), EINVAL), (dict(entry=PACKED, G=64, args=R, ws=-1), EINVAL),
    (dict(entry=PACKED, G=64, args=R, ws=0), EINVAL),
    (dict(entry=IMAGE, cov='diagonal', S=5, ws=-1), EINVAL), (dict(entry=IMAGE, cov='diagonal', S=5, ws=0), EINVAL),
    (dict(S=5, arith='exact', ws=-1), 'e:16.1.4'),
]


def want_of(kw, form):
    return EINVAL if form == EINVAL else route_value(form, kw.get('arith', 'x'))


@pytest.mark.parametrize('kw,form', BOUNDARIES, ids=[str(i) for i in range(len(BOUNDARIES))])
def test_route_on_both_sides_of_every_boundary(kw, form):
    got = route(**kw)
    assert got == want_of(kw, form), (kw, form, hex(got))
    assert _hip.estep_route(3, 0, 0, 13, 1, 16, LN, 1 << 20) == EINVAL            # no such entry point
    assert _hip.estep_route(PLAIN, 7, 0, 13, 1, 16, LN, 1 << 20) == EINVAL        # no such dtype
    assert _hip.estep_route(PLAIN, 0, 3, 13, 1, 16, LN, 1 << 20) == EINVAL        # no such covariance type


def test_route_refuses_where_the_entry_points_do():
    '''Every row of the boundary table through its entry point with T = 0 and buffers it never
    reaches: the rows the query refuses are refused before anything is launched, an empty batch of
    the others is accepted.'''
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    lib = _hip.lib()

    def arg(bit, args):
        return buf if args & bit else None

    for kw, form in BOUNDARIES:
        k = dict(entry=PLAIN, arith='x', cov='full', D=13, S=1, G=16, args=LN | SUM | LW, ws=None, opts=())
        k.update(kw)
        full = ws_bytes(k['arith'], k['cov'], k['D'], k['S'], k['G'])
        nws = full if k['ws'] is None else (0 if k['ws'] == 0 else full + k['ws'])
        ws = buf if nws > 0 else None
        a, cov = k['args'], _hip.COV_CODE[k['cov']]
        old = [(o, _hip.set_option(o, v)) for o, v in k['opts']]
        try:
            if k['entry'] == PLAIN:
                rc = lib.beer_mixtureset_estep(CODE_OF[k['arith']], cov, 0, k['D'], k['S'], k['G'], buf, buf,
                                               arg(LW, a), arg(LABELS, a), .5 if a & SCALED else 1.,
                                               arg(PC, a), arg(LN, a), arg(RESPS, a), arg(SUM, a), ws, nws, None)
            elif k['arith'] != 'x' or a & (PC | LABELS | SCALED):
                continue        # (the packed and image entry points have no such argument)
            elif k['entry'] == PACKED and k['S'] == 1:
                rc = lib.beer_mixture_estep_packed(cov, 0, k['D'], k['G'], buf, buf, arg(LW, a), arg(LN, a),
                                                   arg(RESPS, a), arg(SUM, a), ws, nws, None)
            elif k['entry'] == PACKED:
                rc = lib.beer_mixtureset_estep_packed(cov, 0, k['D'], k['S'], k['G'], buf, buf, arg(LW, a),
                                                      arg(LN, a), arg(RESPS, a), arg(SUM, a), ws, nws, None)
            else:
                if a & RESPS:
                    continue    # (no responsibilities argument either)
                rc = lib.beer_mixtureset_lognorm_image(cov, 0, k['D'], k['S'], k['G'], buf, buf, arg(LW, a),
                                                       buf, arg(LN, a), arg(SUM, a), ws, nws, None)
        finally:
            for o, v in reversed(old):
                _hip.set_option(o, v)
        assert rc == (EINVAL if form == EINVAL else 0), (kw, form, rc)


def test_route_is_declared_in_the_header_and_bound():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    assert re.search(r'int beer_estep_route\(int entry, int dtype, int cov, int D, int S, int G, '
                     r'unsigned args,\s+size_t workspace_bytes\);', text)
    assert _hip.SIGNATURES['beer_estep_route'] == [_hip.c_i] * 6 + [ctypes.c_uint, _hip.c_z]
    for name in ('ESTEP_PLAIN', 'ESTEP_PACKED', 'ESTEP_IMAGE', 'ARG_PC_LLH', 'ARG_LOG_NORM', 'ARG_RESPS',
                 'ARG_LLH_SUM', 'ARG_LABELS', 'ARG_SCALED', 'ARG_LOG_WEIGHTS', 'ESTEP_GENERIC',
                 'ESTEP_EXACT_F32', 'ESTEP_EXACT_F64', 'ESTEP_LLHX', 'ESTEP_LNFI', 'ESTEP_GENERIC_PASS1',
                 'ESTEP_GENERIC_FUSED', 'ESTEP_GENERIC_NORMALISE', 'ESTEP_GENERIC_LABELS',
                 'ESTEP_X_PACKED', 'ESTEP_X_LNO', 'ESTEP_X_IMG', 'ESTEP_X_BL', 'ESTEP_X_NARROW',
                 'ESTEP_X_LANE_MAJOR', 'ESTEP_X_PADDED', 'ESTEP_X_XT'):
        m = re.search(rf'#define BEER_{name} (0x[0-9a-fA-F]+|\d+)u?\b', text)
        assert m and int(m.group(1), 0) == getattr(_hip, name), name


# --- the case table ------------------------------------------------------------------------------

def all_cases():
    return (table.CASES + table.NOWEIGHTS + table.PHANTOMS + table.OUTLIERS + table.K1_CASES)


def test_every_case_states_the_route_the_query_gives():
    for c in all_cases():
        args = table.case_args(c) & ~(LW if c in table.NOWEIGHTS else 0)
        assert table.case_route(c, args) == route_value(c.form, c.arith), table.case_id(c)
    ids = [table.case_id(c) for c in table.CASES]
    assert len(set(ids)) == len(ids)
    assert all(c.D == 1 or table.nku_of(c.D) == (_hip.estep_route(IMAGE, 0, 1, c.D, 5, 16, LN, 1 << 24) >> 5 & 7)
               for c in table.CASES if c.D <= 40)


def collapse(r):
    '''A route with its chunk count cut at 2.  The written exception of the coverage test: a kernel
    sees the number of component chunks only as a factor of its grid (`xcd_block`), so one chunk
    (a grid of frame blocks alone) and several are two forms, two chunks and five are one.'''
    chunks = r >> 16 & 0xfff
    return r & ~(0xfff << 16) | min(chunks, 2) << 16


SWEEP_S = (1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 300, 600)
SWEEP_G = tuple(range(1, 21)) + (24, 32, 33, 40, 64, 65, 100, 128, 129, 200, 256, 257, 300, 512, 600)
SWEEP_ARGS = (LN | SUM | LW, LN | SUM | LW | RESPS, R | LABELS, R | SCALED, PC)


def sweep(plain=True):
    '''(entry, arith, cov, D, S, G, args, workspace bytes) over D <= 130, S G <= 600, every entry
    point, arithmetic, output set, with and without a workspace, both values of both options.'''
    lib = _hip.lib()
    for cov in et.COVS:
        code = _hip.COV_CODE[cov]
        for D in range(1, 131):
            for S in SWEEP_S:
                for G in SWEEP_G:
                    if S * G > 600:
                        break
                    for arith in ('f64', 'exact', 'x'):
                        full = lib.beer_estep_workspace_bytes(CODE_OF[arith] & ~_hip.EXACT, code, D, S, G)
                        for args in SWEEP_ARGS if plain else ():
                            for nws in {full, 0}:
                                yield PLAIN, arith, cov, D, S, G, args, nws
                        if arith == 'x' and full:
                            yield PACKED, arith, cov, D, S, G, R, full
                            yield IMAGE, arith, cov, D, S, G, LN | SUM | LW, full


@pytest.fixture(scope='module')
def swept():
    'Every (call, route) of the sweep, for each setting of the two options the launchers read.'
    lib = _hip.lib()
    out = {}
    for k1, lnfi in ((1, 1), (0, 0)):          # (the options reach the packed and the image entry only)
        old = _hip.set_option('k1_lds', k1), _hip.set_option('lnfi', lnfi)
        try:
            out[k1, lnfi] = [(call, lib.beer_estep_route(call[0], CODE_OF[call[1]], _hip.COV_CODE[call[2]],
                                                         *call[3:])) for call in sweep(plain=k1 == 1)]
        finally:
            _hip.set_option('k1_lds', old[0])
            _hip.set_option('lnfi', old[1])
    return out


def test_every_form_the_query_can_return_is_named_by_a_case(swept):
    reachable = {collapse(r) for calls in swept.values() for _, r in calls if r != EINVAL}
    named = {collapse(route_value(c.form, c.arith)) for c in all_cases()}
    named |= {route_value('g:4'), route_value('g:1')}          # test_labels, test_scaled_statistics_with_pc_llh
    assert named - reachable == set(), sorted(hex(r) for r in named - reachable)
    assert reachable - named == set(), sorted(hex(r) for r in reachable - named)
    families = {_hip.estep_family(r) for r in reachable}
    assert families == {_hip.ESTEP_GENERIC, _hip.ESTEP_EXACT_F32, _hip.ESTEP_EXACT_F64, _hip.ESTEP_LLHX,
                        _hip.ESTEP_LNFI}


def test_case_table_covers_what_the_issue_lists():
    cs = table.CASES
    assert {c.D for c in cs} >= set(table.DSET) | {53, 72, 128}
    for cov in et.COVS:
        assert {c.D for c in cs if c.cov == cov} >= set(table.DSET)
    assert {c.S * c.G for c in cs if c.S == 1} >= {17, 65, 129, 200}
    assert {(c.S, c.G) for c in cs} >= {(33, 16), (3, 128), (300, 1)}
    assert {c.G for c in cs if c.S > 1} >= {1, 2, 3, 5, 6, 12, 4, 8, 16, 32, 64, 128, 256}
    assert table.TS == (1, 129, 300) and max(c.S * c.G for c in cs) <= 600
    # one form of each kernel template also at the ragged tails
    ragged = {(c.entry, c.arith, c.form.split('*')[0]) for c in table.RAGGED_CASES}
    assert ragged >= {(PLAIN, 'f64', 'g:2'), (PLAIN, 'exact', 'e:4.1.4'), (PLAIN, 'f64', 'e:4.1.4'),
                      (PLAIN, 'x', 'x:4.1.'), (PACKED, 'x', 'x:4.1.P'), (PACKED, 'x', 'x:16.4.PBT'),
                      (IMAGE, 'x', 'x:16.1.LIM'), (IMAGE, 'x', 'i:1.8.16')}
    assert table.RAGGED == (31, 32, 33, 63, 64, 65, 127, 128, 257)


# --- the refusals, once: entry point and query ---------------------------------------------------

def test_packed_and_image_entry_points_refuse_what_the_query_refuses():
    '''`beer_mixture_estep_packed`, `beer_mixtureset_estep_packed` and `beer_mixtureset_lognorm_image`
    with T = 0 against the query on the rows of the boundary table that name them: the same answer
    on both sides of every boundary, and each of the three on both sides of at least one.'''
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    lib, seen = _hip.lib(), set()
    for kw, _ in BOUNDARIES:
        k = dict(arith='x', cov='full', D=13, S=1, G=16, args=LN | SUM | LW, ws=None, opts=())
        k.update(kw)
        a, cov, D, S, G = k['args'], _hip.COV_CODE[k['cov']], k['D'], k['S'], k['G']
        if k.get('entry', PLAIN) == PLAIN or k['arith'] != 'x' or a & (PC | LABELS | SCALED) or k['opts']:
            continue            # (no such argument; the options move no refusal)
        if k['entry'] == IMAGE and a & RESPS:
            continue
        full = ws_bytes('x', k['cov'], D, S, G)
        nws = full if k['ws'] is None else (0 if k['ws'] == 0 else full + k['ws'])
        given = [buf if a & bit else None for bit in (LW, LN, RESPS, SUM)]
        tail = (buf if nws else None, nws, None)
        if k['entry'] == IMAGE:
            name = 'beer_mixtureset_lognorm_image'
            rc = lib.beer_mixtureset_lognorm_image(cov, 0, D, S, G, buf, buf, given[0], buf, given[1],
                                                   given[3], *tail)
        elif S == 1:
            name = 'beer_mixture_estep_packed'
            rc = lib.beer_mixture_estep_packed(cov, 0, D, G, buf, buf, *given, *tail)
        else:
            name = 'beer_mixtureset_estep_packed'
            rc = lib.beer_mixtureset_estep_packed(cov, 0, D, S, G, buf, buf, *given, *tail)
        refused = _hip.estep_route(k['entry'], _hip.F32, cov, D, S, G, a, nws) == EINVAL
        assert rc in (0, EINVAL) and (rc == EINVAL) == refused, (name, kw, rc)
        seen.add((name, refused))
    assert seen == {(n, r) for n in ('beer_mixture_estep_packed', 'beer_mixtureset_estep_packed',
                                     'beer_mixtureset_lognorm_image') for r in (False, True)}
    # one mixture through the entry point of sets: refused, whatever the query says of S = 1
    assert lib.beer_mixtureset_estep_packed(0, 0, 13, 1, 16, buf, buf, buf, buf, buf, None, buf,
                                            ws_bytes('x', 'full', 13, 1, 16), None) == EINVAL


# --- what Python concludes from the query --------------------------------------------------------

def test_python_plan_agrees_with_the_library(swept):
    '''`kernels.estep_buffers` over the sweep: it asks for a responsibilities buffer whenever the
    library would run the generic kernels with G > 1, it never leaves the matrix cores by asking
    for one the caller does not want, and it never offers a frame image where the library refuses
    one -- by construction now: need_resps is "wanted, or refused without and taken with", image_ok
    is "the image query does not refuse", and a call refused either way raises.  (The predicate it
    replaces disagreed with the library for exact float32 frames at 96 < D <= 128.)'''
    lib = _hip.lib()
    for call, r in swept[1, 1]:
        entry, arith, cov, D, S, G, args, nws = call
        if entry != PLAIN or args == PC:
            continue
        want_resps = bool(args & RESPS)
        code, c = CODE_OF[arith], _hip.COV_CODE[cov]
        with_resps = lib.beer_estep_route(PLAIN, code, c, D, S, G, args | RESPS, nws)
        if (r == EINVAL or want_resps) and with_resps == EINVAL:
            assert S > 1 and args & LABELS, call
            with pytest.raises(_hip.HipInvalid):
                kernels.estep_buffers(code, c, D, S, G, args, nws)
            continue
        need, image = kernels.estep_buffers(code, c, D, S, G, args, nws)
        assert need == (want_resps or (r == EINVAL and with_resps != EINVAL)), call
        assert image == (lib.beer_estep_route(IMAGE, code, c, D, S, G, args, nws) != EINVAL), call
        got = with_resps if need else r
        assert got != EINVAL, call
        if _hip.estep_family(got) == _hip.ESTEP_GENERIC and G > 1:
            assert need, call
        if not want_resps and r != EINVAL:
            assert not need, call                       # the library needs none: ask for none
        if image and lib.beer_frame_image_bytes(c, 300, D) > 0:
            assert lib.beer_estep_route(IMAGE, _hip.F32, c, D, S, G, LN | SUM | LW, nws) != EINVAL, call
        assert not (image and (need or arith != 'x'))


# --- the generator -------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def truths():
    memo = {}

    def get(c, **kw):
        key = (c, tuple(sorted(kw.items())))
        if key not in memo:
            inp = table.case_inputs(c, **kw)
            memo[key] = (inp,) + et.truth(c.cov, inp, c.S, c.G)
        return memo[key]
    return get


def test_inputs_can_tell_a_wrong_kernel_from_a_right_one(truths):
    '''Every case of the GPU table: log-normalisers below 100 nats (the float32 bound then is at
    most 1e-3, a misplaced slab moves a logit by 0.1 .. 10), and in every state at least two
    components that reach a responsibility of 1e-3 in some frame.'''
    for c in table.CASES + table.NOWEIGHTS:
        inp, ln, resps, pc = truths(c, **({'weights': False} if c in table.NOWEIGHTS else {}))
        assert ln.shape == (table.TMAX, c.S) and resps.shape == (table.TMAX, c.S * c.G)
        assert np.abs(ln).max() < 100., table.case_id(c)
        np.testing.assert_allclose(resps.reshape(-1, c.S, c.G).sum(2), 1., rtol=0, atol=1e-12)
        if c.G >= 2:
            alive = (resps.reshape(-1, c.S, c.G) > 1e-3).any(0).sum(1)
            assert alive.min() >= 2, table.case_id(c)
        # the terms of a logit are larger than their sum
        if c.D >= 4 and (c.cov != 'full' or c.D <= 40):
            X, E = inp['X'].astype(np.float64), inp['E'].astype(np.float64)
            linear = np.abs(X[:8] @ E[:, :c.D].T)
            assert np.median(linear) > 3 * np.median(np.abs(pc[:8])), table.case_id(c)
        assert inp['X'].dtype == inp['E'].dtype == table.NP_OF[c.arith]


def test_generator_makes_every_parameter_its_own():
    assert [et.ksteps('diagonal', D) for D in (12, 13, 28, 29, 40, 41, 48)] == [1, 2, 2, 3, 3, 4, 4]
    assert et.ksteps('full', 40) == 27 and et.ksteps('isotropic', 128) == 10
    for cov in et.COVS:
        mean, scale, a, b = et.std_params(cov, 5, 12, 3, S=3)
        assert len(np.unique(mean)) == mean.size
        E = orc.FAMILIES[cov]['exp'](mean, scale, a, b)
        assert E.shape == (12, orc.stats_dim(cov, 5))
        second = E[:, 5:-2]
        if cov == 'full':
            P = second.reshape(12, 5, 5)
            np.testing.assert_allclose(P, P.transpose(0, 2, 1), rtol=1e-12)
            off = P[:, np.triu_indices(5, 1)[0], np.triu_indices(5, 1)[1]]
            assert len(np.unique(np.round(off, 12))) == off.size and np.abs(off).min() > 1e-6
            assert np.linalg.eigvalsh(P).min() > 0
        assert len(np.unique(second if cov != 'full' else np.einsum('kii->ki', P))) == \
            (12 if cov == 'isotropic' else 60)
    lw = et.log_weights(4, 16, 9)
    np.testing.assert_allclose(orc.logsumexp(lw, 1), 0., atol=1e-12)
    assert np.exp(lw[0]).max() > .7 and np.exp(lw[1]).max() < .08 and len(np.unique(lw)) == lw.size
    assert (et.log_weights(4, 16, 9, phantom=True)[:, 14] == et.PHANTOM).all()
    # a shorter batch is a prefix of a longer one; float32 inputs are float64's, rounded
    a, b = et.make('diagonal', 5, 2, 4, 300, 1), et.make('diagonal', 5, 2, 4, 33, 1, np.float32)
    np.testing.assert_array_equal(a['X'][:33].astype(np.float32), b['X'])
    np.testing.assert_array_equal(a['E'].astype(np.float32), b['E'])
    out = et.make('full', 13, 1, 16, 129, 1, outlier=True)['X']
    offset, spread = et.geometry('full', 13)
    np.testing.assert_allclose(np.abs(out[64] - offset), 40 * spread)


def test_truth_is_the_oracle_on_the_values_given(truths):
    'float32 cases: the oracle in float64 on the ROUNDED values; phantom and absent component agree.'
    c = next(c for c in table.CASES if c.arith == 'x' and c.cov == 'full' and c.S > 1 and c.G >= 4)
    inp, ln, resps, pc = truths(c)
    stats = orc.SUFFSTATS[c.cov](inp['X'].astype(np.float64))
    want_ln, want_r = orc.mixtureset_estep(stats, inp['E'].astype(np.float64), c.D,
                                           inp['lw'].astype(np.float64))
    np.testing.assert_array_equal(ln, want_ln)
    np.testing.assert_array_equal(resps, want_r.reshape(len(ln), -1))
    exact = et.truth(c.cov, table.case_inputs(c._replace(arith='f64')), c.S, c.G)[0]
    assert 0 < np.abs(exact - ln).max() < 1e-3              # (the rounding of the inputs is visible)
    for p in table.PHANTOMS:
        inp, ln, resps, _ = truths(p, phantom=True)
        gone = np.arange(p.S) * p.G + p.G - 2
        assert not resps[:, gone].any() and np.isfinite(ln).all()
