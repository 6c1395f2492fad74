"""CPU checks of the dispatch of the kernels behind a VAE's prior: `beer_dense_route` and
`beer_frames_llh_backward_route` on both sides of every boundary of the launch code (csrc/dense.hip:
big_shape, gemm3_fits, g3_tile, g3_chain; csrc/sample_grad.hip: sg_fast, sd_fast, sg_blocks,
sd_tiles, sg_chunk_frames), the workspace query against the route's chunk length, the case tables
of tests/test_gpu_vae_prior_routes.py (every case's stated form what the query gives, every form
the query can return named by a case) and the refusal of `kernels.dense_accumulate`."""

import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT
import test_gpu_vae_prior_routes as table
from test_gpu_vae_prior_routes import ACC, BWD, LLH, dense_value, frames_value

from beer_amd import _hip, kernels

EINVAL = _hip.EINVAL
F32, F64 = _hip.F32, _hip.F64
FULL, DIAG, ISO = _hip.FULL, _hip.DIAG, _hip.ISO


def dense(op=LLH, dtype=F32, T=8192, Q=512, K=17):
    r = _hip.dense_route(op, dtype, T, Q, K)
    return r if r < 0 else r & ~0xFF00


DENSE_BOUNDARIES = [
    # T at 8191 | 8192, Q at 511 | 512, every op
    (dict(T=8191), 'p'), (dict(T=8192), '3:128x64.ak.bk'), (dict(Q=511), 'p'), (dict(Q=512), '3:128x64.ak.bk'),
    (dict(op=BWD, T=8191), 'p'), (dict(op=BWD, T=8192), '3:128x128.ak'), (dict(op=BWD, Q=511), 'p'),
    (dict(op=ACC, T=8191), 'p'), (dict(op=ACC, T=8192), '3:64x128'), (dict(op=ACC, Q=511), 'p'),
    # the tile: N = K at 64 | 65 (llh), M = K at 64 | 65 (accumulate); backward: always 128 x 128
    (dict(K=64), '3:128x64.ak.bk'), (dict(K=65), '3:128x128.ak.bk'), (dict(K=1), '3:128x64.ak.bk'),
    (dict(op=ACC, K=64), '3:64x128'), (dict(op=ACC, K=65), '3:128x128'), (dict(op=ACC, K=1), '3:64x128'),
    (dict(op=BWD, K=1), '3:128x128.ak'), (dict(op=BWD, K=64), '3:128x128.ak'), (dict(op=BWD, K=65), '3:128x128.ak'),
    # dtype
    (dict(dtype=F64), 'p'), (dict(op=BWD, dtype=F64), 'p'), (dict(op=ACC, dtype=F64), 'p'),
    (dict(dtype=F64, T=1 << 20, Q=4162, K=120), 'p'),
    # the 2^22 stride limit of gemm3_fits: Q is a stride of all three, K of backward and accumulate
    (dict(Q=(1 << 22) - 1), '3:128x64.ak.bk'), (dict(Q=1 << 22), 'p'),
    (dict(op=BWD, Q=(1 << 22) - 1), '3:128x128.ak'), (dict(op=BWD, Q=1 << 22), 'p'),
    (dict(op=ACC, Q=(1 << 22) - 1), '3:64x128'), (dict(op=ACC, Q=1 << 22), 'p'),
    (dict(op=BWD, K=(1 << 22) - 1), '3:128x128.ak'), (dict(op=BWD, K=1 << 22), 'p'),
    (dict(op=ACC, K=(1 << 22) - 1), '3:128x128'), (dict(op=ACC, K=1 << 22), 'p'),
    (dict(K=1 << 22), '3:128x128.ak.bk'),                     # (llh: K is no stride)
    # empty batch: nothing runs, the plain family
    (dict(T=0), 'p'),
    # invalid arguments
    (dict(op=3), EINVAL), (dict(op=-1), EINVAL), (dict(dtype=2), EINVAL), (dict(dtype=F32 | _hip.EXACT), EINVAL),
    (dict(T=-1), EINVAL), (dict(Q=0), EINVAL), (dict(K=0), EINVAL),
]


@pytest.mark.parametrize('kw,form', DENSE_BOUNDARIES, ids=[str(i) for i in range(len(DENSE_BOUNDARIES))])
def test_dense_route_on_both_sides_of_every_boundary(kw, form):
    got = dense(**kw)
    assert got == (EINVAL if form == EINVAL else dense_value(form)), (kw, form, hex(got))


def test_dense_route_reports_the_chain_of_the_accumulation():
    '''The frames a workgroup sums in float32: multiples of 32, at most 4096; short where few
    tiles leave room to split, 2048 at config 4's shape, 4096 for the long-chain case.'''
    assert _hip.dense_chain(_hip.dense_route(LLH, F32, 8192, 512, 17)) == 0
    assert _hip.dense_chain(_hip.dense_route(BWD, F32, 8192, 512, 17)) == 0
    assert _hip.dense_chain(_hip.dense_route(ACC, F32, 8192, 512, 64)) == 64
    assert _hip.dense_chain(_hip.dense_route(ACC, F32, 1 << 20, 4162, 120)) == 2048
    c = table.LONG
    assert _hip.dense_chain(_hip.dense_route(ACC, F32, c.ts[0], c.Q, c.S * c.G)) == 4096 > 2048
    assert c.ts[0] * c.Q < 3e8
    for T in (8192, 8193, 10000, 65536, 1 << 20):
        for Q in (512, 600, 4162):
            for K in (1, 64, 65, 120, 512):
                chain = _hip.dense_chain(_hip.dense_route(ACC, F32, T, Q, K))
                assert 32 <= chain <= 4096 and chain % 32 == 0, (T, Q, K, chain)


def ws_bytes(dtype, cov, T, D, K):
    return _hip.lib().beer_frames_llh_backward_workspace_bytes(dtype, cov, T, D, K)


def frames(dtype=F32, cov=FULL, T=4096, D=13, K=3, ws=None):
    'The query; `ws`: None = the advertised size, else bytes relative to it (0: none at all).'
    full = ws_bytes(dtype, cov, T, D, K)
    r = _hip.frames_llh_backward_route(dtype, cov, T, D, K, full if ws is None else (0 if ws == 0 else full + ws))
    return _hip.SGRAD_CHUNKED if r > 0 and _hip.sgrad_family(r) == _hip.SGRAD_CHUNKED else r


DG, IS = dict(cov=DIAG), dict(cov=ISO)
FRAME_BOUNDARIES = [
    # T at 4095 | 4096 on every family
    (dict(T=4095), 'gen'), (dict(T=4096), 'sg:1'), (dict(DG, T=4095), 'gen'), (dict(DG, T=4096), 'sd:2'),
    (dict(dtype=F64, T=4095), 'gen'), (dict(dtype=F64, T=4096), 'ch'), (dict(T=0), 'gen'),
    # full covariance: D at 7 | 8, 32 | 33, 64 | 65
    (dict(D=7), 'ch'), (dict(D=8), 'sg:1'), (dict(D=32), 'sg:1'), (dict(D=33), 'sg:2'), (dict(D=64), 'sg:2'),
    (dict(D=65), 'ch'), (dict(D=1), 'ch'),
    # diagonal / isotropic: D at 32 | 33, 48 | 49, 64 | 65, 128 | 129
    (dict(DG, D=1), 'sd:2'), (dict(DG, D=32), 'sd:2'), (dict(DG, D=33), 'sd:3'), (dict(DG, D=48), 'sd:3'),
    (dict(DG, D=49), 'sd:4'), (dict(DG, D=64), 'sd:4'), (dict(DG, D=65), 'sd:8'), (dict(DG, D=128), 'sd:8'),
    (dict(DG, D=129), 'ch'), (dict(IS, D=32), 'sd:2'), (dict(IS, D=33), 'sd:3'), (dict(IS, D=48), 'sd:3'),
    (dict(IS, D=49), 'sd:4'), (dict(IS, D=64), 'sd:4'), (dict(IS, D=65), 'sd:8'), (dict(IS, D=128), 'sd:8'),
    (dict(IS, D=129), 'ch'), (dict(DG, D=7), 'sd:2'), (dict(DG, D=8), 'sd:2'),
    # dtype: float64 never reaches the matrix cores
    (dict(dtype=F64), 'ch'), (dict(DG, dtype=F64), 'ch'), (dict(IS, dtype=F64, D=64), 'ch'),
    # the workspace present, one byte short, absent, one byte more
    (dict(ws=-1), 'gen'), (dict(ws=0), 'gen'), (dict(ws=1), 'sg:1'), (dict(DG, ws=-1), 'gen'), (dict(DG, ws=0), 'gen'),
    (dict(dtype=F64, ws=-1), 'gen'), (dict(dtype=F64, ws=0), 'gen'), (dict(D=72, ws=-1), 'gen'), (dict(D=72), 'ch'),
    # invalid arguments
    (dict(T=-1), EINVAL), (dict(D=0), EINVAL), (dict(K=0), EINVAL), (dict(cov=3), EINVAL), (dict(cov=-1), EINVAL),
    (dict(dtype=2), EINVAL), (dict(dtype=F32 | _hip.EXACT), EINVAL),
]


@pytest.mark.parametrize('kw,form', FRAME_BOUNDARIES, ids=[str(i) for i in range(len(FRAME_BOUNDARIES))])
def test_frames_route_on_both_sides_of_every_boundary(kw, form):
    got = frames(**kw)
    assert got == (EINVAL if form == EINVAL else frames_value(form)), (kw, form, hex(got))


def test_a_workspace_short_of_the_fragment_image_is_not_used_for_chunks():
    'More than the image: the matrix cores; one byte less, which holds no chunk either: generic.'
    assert _hip.frames_llh_backward_route(F32, FULL, 4100, 13, 3, 1 << 30) == frames_value('sg:1')
    full = ws_bytes(F32, FULL, 4100, 13, 3)
    assert _hip.frames_llh_backward_route(F32, FULL, 4100, 13, 3, full - 1) == _hip.SGRAD_GENERIC


def test_workspace_query_agrees_with_the_chunk_length_of_the_route():
    for dtype, elem in ((F32, 4), (F64, 8)):
        for cov, name in ((FULL, 'full'), (DIAG, 'diagonal'), (ISO, 'isotropic')):
            for D in (1, 5, 7, 8, 64, 65, 72, 128, 129, 130, 300):
                for T in (4096, 4100, 9000, 12766, 1 << 20, 1 << 25):
                    nws = ws_bytes(dtype, cov, T, D, 3)
                    r = _hip.frames_llh_backward_route(dtype, cov, T, D, 3, nws)
                    assert nws > 0
                    if _hip.sgrad_family(r) != _hip.SGRAD_CHUNKED:
                        assert dtype == F32 and D <= (64 if cov == FULL else 128)
                        continue
                    Q = table.vt.stats_dim(name, D)
                    chunk = _hip.sgrad_form(r)
                    assert nws == chunk * Q * elem, (dtype, cov, T, D)
                    assert chunk == min(T, max(1024, (256 << 20) // (Q * elem)))
    assert ws_bytes(F32, FULL, 4095, 13, 3) == 0


def test_routes_are_declared_in_the_header_and_bound():
    text = open(os.path.join(ROOT, 'include', 'beer_hip.h')).read()
    assert re.search(r'int beer_dense_route\(int op, int dtype, int64_t T, int Q, int K\);', text)
    assert re.search(r'int beer_frames_llh_backward_route\(int dtype, int cov, int64_t T, int D, int K,\s+'
                     r'size_t workspace_bytes\);', text)
    assert _hip.SIGNATURES['beer_dense_route'] == [_hip.c_i, _hip.c_i, _hip.c_l, _hip.c_i, _hip.c_i]
    assert _hip.SIGNATURES['beer_frames_llh_backward_route'] == \
        [_hip.c_i, _hip.c_i, _hip.c_l, _hip.c_i, _hip.c_i, _hip.c_z]
    for name in ('DENSE_LLH', 'DENSE_BACKWARD', 'DENSE_ACCUMULATE', 'DENSE_PLAIN', 'DENSE_GEMM3', 'DENSE_T64x128',
                 'DENSE_T128x64', 'DENSE_T128x128', 'DENSE_AK', 'DENSE_BK', 'SGRAD_GENERIC', 'SGRAD_FULL',
                 'SGRAD_DIAG', 'SGRAD_CHUNKED'):
        m = re.search(rf'#define BEER_{name} (0x[0-9a-fA-F]+|\d+)u?\b', text)
        assert m and int(m.group(1), 0) == getattr(_hip, name), name
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'beer_dense_route' in doc and 'beer_frames_llh_backward_route' in doc


# --- the case tables -----------------------------------------------------------------------------

def test_every_case_states_the_route_the_query_gives():
    for c in table.DENSE_CASES + [table.LONG]:
        for T in c.ts:
            assert table.dense_route(c, T) == dense_value(c.form if T else 'p'), (table.dense_id(c), T)
    frame_cases = table.FRAME_CASES + [table.GENERIC_STRIDE]
    for c in frame_cases:
        for T in c.ts:
            assert table.frame_route(c, T) == frames_value(c.form if T else 'gen'), (table.frame_id(c), T)
    for ids in ([table.dense_id(c) for c in table.DENSE_CASES], [table.frame_id(c) for c in frame_cases],
                [table.stat_id(c) for c in table.STAT_CASES]):
        assert len(set(ids)) == len(ids)


def test_every_form_the_queries_can_return_is_named_by_a_case():
    reachable = set()
    for op in (LLH, BWD, ACC):
        for dtype in (F32, F64):
            for T in (1, 300, 8191, 8192, 8193, 20001, 1 << 20):
                for Q in (1, 130, 511, 512, 513, 4162):
                    for K in (1, 17, 63, 64, 65, 129, 512):
                        reachable.add(dense(op, dtype, T, Q, K))
    named = {dense_value(c.form) for c in table.DENSE_CASES}
    assert reachable == named, sorted(hex(r) for r in reachable ^ named)
    assert len(named) == 6       # plain; llh on two tiles, backward on one, accumulate on two
    reachable = set()
    for dtype in (F32, F64):
        for cov in (FULL, DIAG, ISO):
            for T in (1, 300, 4095, 4096, 4100, 20001):
                for D in list(range(1, 140)) + [300]:
                    for K in (1, 3, 33, 120):
                        for ws in (None, 0, -1):
                            reachable.add(frames(dtype, cov, T, D, K, ws))
    named = {frames_value(c.form) for c in table.FRAME_CASES}
    assert reachable == named, sorted(hex(r) for r in reachable ^ named)
    assert named == {frames_value(f) for f in ('gen', 'ch', 'sg:1', 'sg:2', 'sd:2', 'sd:3', 'sd:4', 'sd:8')}


def test_grid_stride_cases_run_their_loops_twice():
    'The launchers cap their grids at 65536 workgroups of 256 threads (of 4 frames, a wave each).'
    for w, c in table.STRIDE_CASES:
        Q = table.vt.stats_dim(c.cov, c.D)
        full = w == 'backward' and c.cov == 'full' and 8 <= c.D <= 64
        n = c.ts[0] * Q if w == 'mean' else (c.ts[0] / 4 * 256 if full else c.ts[0] * c.ns * c.D)
        assert 65536 * 256 < n < 1.01 * 65536 * 256 + 2048, (w, c)
    assert {(w, c.cov == 'full') for w, c in table.STRIDE_CASES} == {('mean', False), ('backward', False), ('backward', True)}
    g = table.GENERIC_STRIDE
    assert 65536 * 256 < g.ts[0] * g.D < 1.01 * 65536 * 256 and g.ws == 'nows'


def test_dense_weights_differ_from_frame_to_frame_and_component_to_component():
    'No case hands a product constant weights: a misplaced row or column of them must show.'
    for c in table.DENSE_CASES:
        if c.op == LLH or max(c.ts) > 1000:
            continue
        inp = table.vt.dense_inputs(max(c.ts), c.Q, c.S * c.G, c.S, table.dense_seed(c), table.NP_OF[c.arith])
        for name in ('w', 'ws'):
            w = inp[name]
            assert (w.std(0) > 0).all(), (table.dense_id(c), name)
            assert c.S * c.G == 1 or (w.std(1) > 0).all(), (table.dense_id(c), name)
        assert (inp['w'] == 0).any() and (inp['w'] >= 0).all()


# --- kernels.dense_accumulate --------------------------------------------------------------------

def test_dense_accumulate_refuses_weights_that_are_not_T_by_K(monkeypatch):
    '''`comp_resps=None` with [T, S] state posteriors and G > 1 used to hand the library K = S G
    columns of a [T, S] buffer; every shape other than [T, K] is refused before any launch.'''
    monkeypatch.setattr(_hip, 'on_device', lambda t, dtype=None: t if dtype is None else t.to(dtype))

    def no_launch(*a):
        raise AssertionError('a kernel was launched')
    monkeypatch.setattr(_hip, 'call', no_launch)
    T, Q, S, G = 6, 5, 3, 4
    st = torch.zeros(T, Q)
    with pytest.raises(ValueError):
        kernels.dense_accumulate(st, None, torch.zeros(T, S), S, G)
    with pytest.raises(ValueError):
        kernels.dense_accumulate(st, torch.zeros(T, S), None, S, G)
    with pytest.raises(ValueError):
        kernels.dense_accumulate(st, torch.zeros(T - 1, S * G), None, S, G)
    with pytest.raises(ValueError):
        kernels.dense_accumulate(st, torch.zeros(T, S * G), torch.zeros(T, S * G), S, G)
    with pytest.raises(ValueError):
        kernels.dense_accumulate(st, torch.zeros(T, S * G), torch.zeros(T, S), S, G, acc=torch.zeros(S, Q).double())
    # the shapes the callers pass get as far as the launch
    for args in ((torch.zeros(T, S * G), torch.zeros(T, S), S, G), (torch.zeros(T, S * G), None, S * G, 1),
                 (None, None, 1, 1), (None, torch.zeros(T, S), S, 1)):
        with pytest.raises(AssertionError, match='launched'):
            kernels.dense_accumulate(st, *args)
