"""CPU checks of the accumulation dispatch: `beer_accumulate_route` on both sides of every boundary
of the launch code (csrc/estep.hip accumulate_plan, estep_mfma.hip acc_form, estep_bf16.hip
accx_form / accf_form, acc_diag.hip accd_form), the refusals of the entry points themselves, the
workspace sizes against the values recorded before the layouts were gathered into one function
each (tests/golden/accumulate_workspace_bytes.json), and the case table of
tests/test_gpu_accumulate_routes.py: every case's stated form what the query gives, every form
the query can return named by a case."""

import ctypes
import json
import os
import re

import pytest

from helpers import ROOT
import test_gpu_accumulate_routes as table
from test_gpu_accumulate_routes import FUSED, PACKED, PLAIN, route_value

from beer_amd import _hip

EINVAL = _hip.EINVAL
R, SR, IMG = _hip.ARG_RESPS, _hip.ARG_STATE_RESPS, _hip.ARG_IMAGE
CODE_OF = table.CODE_OF
COVS = ('full', 'diagonal', 'isotropic')


def ws_bytes(entry, arith, cov, T, D, S, G, args):
    'The advertised workspace of a call: the query Python sizes its scratch by.'
    return table.case_ws_bytes(table.C(entry, arith, cov, D, S, G, bool(args & SR), '', ''), T)


def route(entry=PLAIN, arith='x', cov='full', T=300, D=13, S=1, G=16, args=R, ws=None, waves=None):
    'The query; `ws`: None = the advertised size, else bytes relative to it (0: none at all).'
    full = ws_bytes(entry, arith, cov, T, D, S, G, args)
    nbytes = full if ws is None else (0 if ws == 0 else full + ws)
    old = _hip.set_option('accfi_waves', waves) if waves else None
    try:
        return _hip.accumulate_route(entry, CODE_OF[arith], _hip.COV_CODE[cov], T, D, S, G, args, nbytes)
    finally:
        if waves:
            _hip.set_option('accfi_waves', old)


PK, PKS, FU = dict(entry=PACKED), dict(entry=PACKED, args=R | SR), dict(entry=FUSED, cov='diagonal', args=0)
DG = dict(cov='diagonal', T=16384)
# (arguments of `route`, the form as test_gpu_accumulate_routes.route_value writes it, or EINVAL)
BOUNDARIES = [
    # K at 15|16 and K % 4, on every matrix-core family
    (dict(G=15), 'g'), (dict(G=16), 'e:4'), (dict(G=17), 'g'), (dict(G=18), 'g'), (dict(G=20), 'e:4'),
    (dict(arith='f64', G=15), 'g'), (dict(arith='f64', G=16), 'e:4'), (dict(arith='f64', G=18), 'g'),
    (dict(arith='exact', S=5, G=3), 'g'), (dict(arith='exact', S=5, G=4, args=R | SR), 'e:4.s'),
    (dict(PK, G=15), EINVAL), (dict(PK, G=16), 'x:6.'), (dict(PK, G=18), EINVAL), (dict(PK, G=20), 'x:6.'),
    (dict(DG, G=15), 'g'), (dict(DG, G=16), 'd:1.1.p'), (dict(DG, G=17), 'd:1.1.p'),
    # D at 64|65 (float64), 96|97 (exact float32), 128|129 (packed), 64|65 (fused and diag)
    (dict(arith='f64', cov='diagonal', D=64), 'e:4'), (dict(arith='f64', cov='diagonal', D=65), 'g'),
    (dict(arith='exact', D=96), 'e:4'), (dict(arith='exact', D=97), 'g'), (dict(D=96), 'e:4'), (dict(D=97), 'g'),
    (dict(PK, D=128), 'x:6.x'), (dict(PK, D=129), EINVAL), (dict(PK, D=0), EINVAL),
    (dict(FU, D=64, S=5, G=4), 'f:10.4'), (dict(FU, D=65, S=5, G=4), EINVAL), (dict(FU, D=0, S=5, G=4), EINVAL),
    (dict(DG, D=64), 'd:4.1.p'), (dict(DG, D=65), 'e:4'), (dict(DG, D=97), 'g'),
    (dict(D=0), EINVAL), (dict(S=0), EINVAL), (dict(G=0), EINVAL), (dict(T=-1), EINVAL),
    # statistic tiles of acc_kernel at 4|5 and 8|9: diagonal D = 28|29 and 56|57 (14, 16 | 19 and
    # 32 | 35 slabs), full D = 8|9 and 12|13 (15 | 25 and 28 | 42 slabs)
    (dict(arith='exact', cov='diagonal', D=28), 'e:1'), (dict(arith='exact', cov='diagonal', D=29), 'e:2'),
    (dict(arith='exact', cov='diagonal', D=56), 'e:2'), (dict(arith='exact', cov='diagonal', D=57), 'e:4'),
    (dict(arith='f64', cov='isotropic', D=28), 'e:1'), (dict(arith='f64', cov='isotropic', D=29), 'e:2'),
    (dict(arith='f64', cov='isotropic', D=56), 'e:2'), (dict(arith='f64', cov='isotropic', D=57), 'e:4'),
    (dict(arith='f64', D=8), 'e:1'), (dict(arith='f64', D=9), 'e:2'), (dict(arith='f64', D=12), 'e:2'),
    (dict(arith='f64', D=13, S=5, G=4, args=R | SR), 'e:4.s'),
    # no responsibilities, no workspace, a workspace one byte short: the generic kernel
    (dict(args=0), 'g'), (dict(ws=0), 'g'), (dict(ws=-1), 'g'), (dict(arith='f64', ws=-1), 'g'), (dict(ws=1), 'e:4'),
    # the three values of accx_nq: 6 / 7 / 8 tiles per wave at 24|25 and 28|29 tiles (full D = 24|25,
    # 48|49); diagonal statistics never leave 6
    (dict(PK, D=24), 'x:6.'), (dict(PK, D=25), 'x:7.'), (dict(PK, D=28), 'x:7.'), (dict(PK, D=29), 'x:6.'),
    (dict(PK, D=48), 'x:7.'), (dict(PK, D=49), 'x:8.'), (dict(PK, D=52), 'x:8.'), (dict(PK, D=53), 'x:7.'),
    (dict(PK, cov='diagonal', D=64), 'x:6.'), (dict(PKS, S=2, G=8, D=49), 'x:8.s'),
    # one X^T tile (sx): two tiles and two R buffers fill the LDS up to D = 118, with the state
    # posteriors' buffers up to D = 103
    (dict(PK, D=118), 'x:7.'), (dict(PK, D=119), 'x:7.x'), (dict(PK, cov='isotropic', D=118), 'x:6.'),
    (dict(PK, cov='isotropic', D=119), 'x:6.x'), (dict(PKS, S=2, G=8, D=103), 'x:8.s'),
    (dict(PKS, S=2, G=8, D=104), 'x:8.sx'),
    # the X^T image behind the packed tiles: one mixture of 129 .. 256 components
    (dict(PK, G=128), 'x:6.'), (dict(PK, G=132), 'x:6.t'), (dict(PK, G=256), 'x:6.t'), (dict(PK, G=260), 'x:6.'),
    (dict(PK, S=2, G=66), 'x:6.t'), (dict(PKS, S=2, G=128), 'x:6.s'), (dict(PK, G=132, D=119), 'x:7.xt'),
    # packed sets: G at 7|8, 128|256, not a power of two; full covariance only
    (dict(PKS, S=4, G=4), EINVAL), (dict(PKS, S=2, G=8), 'x:6.s'), (dict(PKS, S=2, G=128), 'x:6.s'),
    (dict(PKS, S=2, G=256), EINVAL), (dict(PKS, S=2, G=12), EINVAL), (dict(PKS, S=1, G=16), EINVAL),
    (dict(PKS, S=2, G=8, cov='diagonal'), EINVAL), (dict(PK, S=2, G=8, cov='diagonal'), 'x:6.'),
    (dict(PK, args=0), EINVAL), (dict(PK, arith='exact'), EINVAL), (dict(PK, arith='f64'), EINVAL),
    (dict(PK, ws=-1), EINVAL), (dict(PK, ws=0), EINVAL), (dict(PKS, S=2, G=8, ws=-1), EINVAL), (dict(PK, ws=1), 'x:6.'),
    # fused: NQT 6 / 9 / 10 at 96|97..144|145 statistic columns (D = 40|41, 60|61), full refused
    (dict(FU, D=40, S=5, G=4), 'f:6.8'), (dict(FU, D=41, S=5, G=4), 'f:9.4'), (dict(FU, D=60, S=5, G=4), 'f:9.4'),
    (dict(FU, D=61, S=5, G=4), 'f:10.4'), (dict(FU, cov='isotropic', D=40, S=5, G=4), 'f:6.8'),
    (dict(FU, cov='isotropic', D=41, S=5, G=4), 'f:9.4'), (dict(FU, cov='full', S=5, G=4), EINVAL),
    (dict(FU, S=1, G=256), 'f:6.8'), (dict(FU, S=1, G=257), EINVAL), (dict(FU, S=5, G=4, args=SR), 'f:6.8'),
    (dict(FU, S=5, G=4, ws=-1), EINVAL), (dict(FU, S=5, G=4, ws=0), EINVAL), (dict(FU, S=5, G=4, arith='f64'), EINVAL),
    # ... blocks of 4 states (blk): S >= 4 and no 64-slot chunk over more than 4 states; a chunk of
    # 5 x 12 slots, or of 16 x 4, straddles more
    (dict(FU, S=3, G=16), 'f:6.8'), (dict(FU, S=4, G=16), 'f:6.8.b'), (dict(FU, S=4, G=13), 'f:6.8.b'),
    (dict(FU, S=4, G=12), 'f:6.8.b'), (dict(FU, S=5, G=12), 'f:6.8'), (dict(FU, S=5, G=13), 'f:6.8.b'),
    (dict(FU, S=4, G=4), 'f:6.8.b'), (dict(FU, S=16, G=4), 'f:6.8'), (dict(FU, S=150, G=4), 'f:6.8'),
    (dict(FU, D=64, S=5, G=13), 'f:10.4.b'), (dict(FU, D=41, S=5, G=13), 'f:9.4.b'),
    # ... over a frame image: NKU 1 .. 4 at D = 12|13, 28|29, 40|41, no image kernel from D = 49;
    # blocks of 4 or 16 states (groups hold at least 4 slots: no chunk straddles more than 16, the
    # kernel without an image for ns_img = 0 is out of reach); 8 or 4 waves by BEER_OPT_ACCFI_WAVES
    (dict(FU, D=12, S=5, G=4, args=IMG, waves=8), 'i:1.8.16'), (dict(FU, D=13, S=5, G=4, args=IMG, waves=8), 'i:2.8.16'),
    (dict(FU, D=28, S=5, G=4, args=IMG, waves=4), 'i:2.4.16'), (dict(FU, D=29, S=5, G=4, args=IMG, waves=4), 'i:3.4.16'),
    (dict(FU, D=40, S=5, G=13, args=IMG, waves=8), 'i:3.8.4'), (dict(FU, D=41, S=5, G=13, args=IMG, waves=8), 'i:4.8.4'),
    (dict(FU, D=48, S=5, G=13, args=IMG, waves=4), 'i:4.4.4'), (dict(FU, D=49, S=5, G=13, args=IMG, waves=4), 'f:9.4.b'),
    (dict(FU, D=13, S=64, G=3, args=IMG | SR, waves=4), 'i:2.4.16'), (dict(FU, D=13, S=150, G=4, args=IMG, waves=8), 'i:2.8.16'),
    (dict(FU, D=13, S=4, G=12, args=IMG, waves=4), 'i:2.4.4'), (dict(FU, D=13, S=5, G=12, args=IMG, waves=4), 'i:2.4.16'),
    (dict(FU, D=13, S=5, G=4, args=0, waves=4), 'f:6.8'),
    # acc_diag: T at 16383|16384, K at 64|65, float32 bf16x3 only, no state posteriors, not full
    (dict(DG, T=16383), 'e:1'), (dict(DG), 'd:1.1.p'), (dict(DG, G=64), 'd:1.1.p'), (dict(DG, G=65), 'd:1.2.p'),
    (dict(DG, D=16), 'd:1.1.p'), (dict(DG, D=17), 'd:2.1.p'), (dict(DG, D=32), 'd:2.1.p'), (dict(DG, D=33), 'd:3.1.p'),
    (dict(DG, D=48), 'd:3.1.p'), (dict(DG, D=49, cov='isotropic'), 'd:4.1.p'),
    (dict(DG, arith='exact'), 'e:1'), (dict(DG, arith='f64'), 'e:1'), (dict(DG, S=4, G=4, args=R | SR), 'e:1.s'),
    (dict(DG, cov='full'), 'e:4'), (dict(DG, args=0), 'g'), (dict(DG, S=16, G=1), 'd:1.1.p'),
    # ... the partial-sum workspace present, one byte short, absent: a route, not a refusal; one
    # chain of frames does not exist from 16384 frames on
    (dict(DG, ws=-1), 'd:1.1'), (dict(DG, ws=0), 'd:1.1'), (dict(DG, G=80, D=40, ws=0), 'd:3.2'),
    (dict(DG, G=80, D=40, ws=-1), 'd:3.2'), (dict(DG, G=80, D=40), 'd:3.2.p'),
]


def want_of(kw, form):
    return EINVAL if form == EINVAL else route_value(form, kw.get('arith', 'x'))


@pytest.mark.parametrize('kw,form', BOUNDARIES, ids=[str(i) for i in range(len(BOUNDARIES))])
def test_route_on_both_sides_of_every_boundary(kw, form):
    got = route(**kw)
    assert got == want_of(kw, form), (kw, form, hex(got))
    assert _hip.accumulate_route(3, 0, 0, 300, 13, 1, 16, R, 1 << 20) == EINVAL        # no such entry point
    assert _hip.accumulate_route(PLAIN, 7, 0, 300, 13, 1, 16, R, 1 << 20) == EINVAL    # no such dtype
    assert _hip.accumulate_route(PLAIN, 0, 3, 300, 13, 1, 16, R, 1 << 20) == EINVAL    # no such covariance


def test_route_refuses_where_the_entry_points_do():
    '''Every row of the boundary table through its entry point with T = 0 (a negative T as it is)
    and buffers it never reaches: the rows the query refuses are refused before anything is
    launched, an empty batch of the others is accepted.  An empty batch of a refused shape is
    refused like a full one -- as before the query existed: every accumulation entry point checked
    its shape and workspace ahead of its T == 0 return.'''
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    lib = _hip.lib()
    for kw, form in BOUNDARIES:
        k = dict(entry=PLAIN, arith='x', cov='full', T=300, D=13, S=1, G=16, args=R, ws=None, waves=None)
        k.update(kw)
        if k['entry'] != PLAIN and k['arith'] != 'x':
            continue            # (the packed and the fused entry points have no such argument)
        a, cov, T0 = k['args'], _hip.COV_CODE[k['cov']], min(k['T'], 0)
        # (the workspace of the empty batch: the query at T = 0, moved as the row moves it)
        full = ws_bytes(k['entry'], k['arith'], k['cov'], 0, k['D'], k['S'], k['G'], a)
        nws = full if k['ws'] is None else (0 if k['ws'] == 0 else full + k['ws'])
        ws = buf if nws > 0 else None
        want = EINVAL if route(**dict(k, T=T0)) == EINVAL else 0
        if k['entry'] == PLAIN:
            rc = lib.beer_normal_accumulate(CODE_OF[k['arith']], cov, T0, k['D'], k['S'], k['G'], buf,
                                            buf if a & R else None, buf if a & SR else None, buf, ws, nws, None)
        elif k['entry'] == FUSED:
            rc = lib.beer_mixtureset_accumulate_fused(cov, T0, k['D'], k['S'], k['G'], buf, buf, buf, buf,
                                                      buf if a & SR else None, buf if a & IMG else None,
                                                      buf, ws, nws, None)
        elif a & SR:
            rc = lib.beer_mixtureset_accumulate_packed(cov, T0, k['D'], k['S'], k['G'], buf,
                                                       buf if a & R else None, buf, buf, ws, nws, None)
        else:
            rc = lib.beer_normal_accumulate_packed(cov, T0, k['D'], k['S'] * k['G'], buf,
                                                   buf if a & R else None, buf, ws, nws, None)
        assert rc == want, (kw, form, rc)
        if k['T'] == 300 and k['entry'] != PLAIN:       # (T-independent forms: the row's own verdict)
            assert want == (EINVAL if form == EINVAL else 0), (kw, form)


def test_route_is_declared_in_the_header_and_bound():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    assert re.search(r'int beer_accumulate_route\(int entry, int dtype, int cov, int64_t T, int D, int S, '
                     r'int G,\s+unsigned args, size_t workspace_bytes\);', text)
    assert _hip.SIGNATURES['beer_accumulate_route'] == \
        [_hip.c_i] * 3 + [_hip.c_l] + [_hip.c_i] * 3 + [ctypes.c_uint, _hip.c_z]
    for name in ('ACC_PLAIN', 'ACC_PACKED', 'ACC_FUSED', 'ARG_RESPS', 'ARG_STATE_RESPS', 'ARG_IMAGE',
                 'ACC_GENERIC', 'ACC_EXACT_F32', 'ACC_EXACT_F64', 'ACC_DIAG', 'ACC_ACCX', 'ACC_ACCF', 'ACC_SR',
                 'ACC_D_PARTIAL', 'ACC_X_SX', 'ACC_X_XT_REUSED', 'ACC_F_BLK', 'ACC_F_IMAGE'):
        m = re.search(rf'#define BEER_{name} (0x[0-9a-fA-F]+|\d+)u?\b', text)
        assert m and int(m.group(1), 0) == getattr(_hip, name), name


# --- the workspace layouts -----------------------------------------------------------------------

def size_queries(cov, T, D, S, G):
    lib = _hip.lib()
    return [lib.beer_accumulate_workspace_bytes(_hip.F32, cov, D, S, G),
            lib.beer_accumulate_workspace_bytes(_hip.F64, cov, D, S, G),
            lib.beer_accumulate_frames_workspace_bytes(_hip.F32, cov, T, D, S, G),
            lib.beer_accumulate_packed_workspace_bytes(cov, T, D, S * G),
            lib.beer_mixtureset_accumulate_packed_workspace_bytes(cov, T, D, S, G),
            lib.beer_accumulate_fused_workspace_bytes(cov, D, S, G)]


def test_advertised_workspace_sizes_are_the_recorded_ones():
    '''The six size queries at 48 shapes (D <= 129, S G <= 600, T from 0 to 100000), recorded from
    the library as it was when every size was a sum written next to its launcher: exactly equal.'''
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'accumulate_workspace_bytes.json')))
    assert len(g['rows']) >= 40 and sum(any(r[5:]) for r in g['rows']) >= 30
    for cov, T, D, S, G, *sizes in g['rows']:
        assert size_queries(cov, T, D, S, G) == sizes, (cov, T, D, S, G)


def test_workspace_sizes_grow_with_the_frames_only_where_the_layout_holds_frames():
    for cov in range(3):
        for D, S, G in ((13, 1, 16), (40, 2, 8), (64, 5, 4), (128, 1, 132)):
            a, b = size_queries(cov, 64, D, S, G), size_queries(cov, 65, D, S, G)
            assert a[:3] == b[:3] and a[5] == b[5]
            assert all(y > x for x, y in zip(a[3:5], b[3:5]) if x)          # one more X^T tile
            assert a[4] == 0 or a[4] > a[3]                                 # ... and its posteriors


# --- the case table ------------------------------------------------------------------------------

def test_every_case_states_the_route_the_query_gives():
    for c in table.CASES:
        for T in table.case_ts(c):
            assert table.case_route(c, T) == route_value(c.form, c.arith), (table.case_id(c), T)
    ids = [table.case_id(c) for c in table.CASES]
    assert len(set(ids)) == len(ids)


SWEEP_S = (1, 2, 3, 4, 5, 9, 17, 33, 65, 129, 257, 300, 600)
SWEEP_G = tuple(range(1, 21)) + (24, 32, 33, 40, 64, 65, 100, 128, 129, 132, 200, 256, 257, 300, 512, 600)


def sweep():
    '''Routes over D <= 130, S G <= 600, T = 300 and 16385, every entry point, arithmetic and
    argument set, with the advertised workspace and without one, both values of the option.'''
    lib = _hip.lib()
    q = lib.beer_accumulate_route
    for cov in range(3):
        for D in range(1, 131):
            for S in SWEEP_S:
                for G in SWEEP_G:
                    if S * G > 600:
                        break
                    for T in (300, 16385):
                        for arith in ('f64', 'exact', 'x'):
                            code = CODE_OF[arith]
                            full = lib.beer_accumulate_frames_workspace_bytes(code & ~_hip.EXACT, cov, T, D, S, G)
                            for args in (R, R | SR, 0):
                                for nws in {full, 0}:
                                    yield q(PLAIN, code, cov, T, D, S, G, args, nws)
                        yield q(PACKED, _hip.F32, cov, T, D, S, G, R,
                                lib.beer_accumulate_packed_workspace_bytes(cov, T, D, S * G))
                        yield q(PACKED, _hip.F32, cov, T, D, S, G, R | SR,
                                lib.beer_mixtureset_accumulate_packed_workspace_bytes(cov, T, D, S, G))
                    nws = lib.beer_accumulate_fused_workspace_bytes(cov, D, S, G)
                    for args in (0, IMG, IMG | SR):
                        yield q(FUSED, _hip.F32, cov, 300, D, S, G, args, nws)


def test_every_form_the_query_can_return_is_named_by_a_case():
    reachable = set()
    for waves in (8, 4):
        old = _hip.set_option('accfi_waves', waves)
        try:
            reachable |= set(sweep())
        finally:
            _hip.set_option('accfi_waves', old)
    reachable.discard(EINVAL)
    named = {route_value(c.form, c.arith) for c in table.CASES}
    assert named - reachable == set(), sorted(hex(r) for r in named - reachable)
    assert reachable - named == set(), sorted(hex(r) for r in reachable - named)
    assert {_hip.accumulate_family(r) for r in reachable} == {
        _hip.ACC_GENERIC, _hip.ACC_EXACT_F32, _hip.ACC_EXACT_F64, _hip.ACC_DIAG, _hip.ACC_ACCX, _hip.ACC_ACCF}
    assert len(reachable) == 67
    # (the written exception: accfi_kernel exists for blocks of 4 and 16 states only and
    #  accf_form keeps ns_img = 0 for chunks over more; with groups of at least 4 slots a
    #  64-slot chunk never is, so the fused call with an image always takes an image kernel
    #  up to D = 48)
    assert not any(_hip.accumulate_family(r) == _hip.ACC_ACCF and r & _hip.ACC_F_IMAGE and not r >> 16 & 31
                   for r in reachable)


def test_case_table_covers_what_the_issue_lists():
    cs = table.CASES
    assert table.TS == (0, 1, 65, 129, 300) and table.TS_DIAG == (16384, 16385)
    assert {c.D for c in cs} >= {1, 5, 13, 40, 64, 96, 128}
    assert {c.S * c.G for c in cs if c.form == 'g'} == {3, 17}
    assert {c.S * c.G for c in cs if c.form != 'g'} >= {16, 20}
    for fam, covs in (('g', COVS), ('e', COVS), ('x', COVS), ('d', COVS[1:]), ('f', COVS[1:]), ('i', COVS[1:])):
        assert {c.cov for c in cs if c.form.split(':')[0] == fam} == set(covs), fam
