"""CPU checks of what the block kernels of the HMM families share (csrc/hmm_block.h): one refusal
of a batch and one byte formula for the arcs staged beside their categories.  With neutral extras
the routes of the six families refuse exactly the same batches, and the four category kernels
stage their arcs in LDS for exactly the same batches, on a grid that crosses every threshold of
the shared part."""

import ctypes

from beer_amd import _hip

F32, F64 = _hip.F32, _hip.F64
STATES = (1, 64, 120, 300, 2000, 6136, 6137, 10232, 10233, 32767, 32768)
N_CAT = 3


def desc(max_states, max_arcs, nutt=3):
    'A beer_batch with only its scalar fields filled: all the queries may read.'
    return _hip.Batch(nutt, max_states, max_arcs, max(max_states, 1), 0, 1,
                      None, None, None, None, None, None, 0, 0, 0, 0, None)


def arc_counts(S, w):
    'Nothing, sparse, dense, and the last count whose out-CSR with categories is staged and the next.'
    # rows (2 S + 16) 8, arcs (S + 2 + 2 A) 4 + (A + 1) w: together within 64 KiB
    a = (64 * 1024 - (2 * S + 16) * 8 - 4 * (S + 2) - w) // (8 + w)
    return sorted(v for v in {0, S, 12 * S, a, a + 1} if v >= 0)


def grid():
    for S in STATES:
        for dtype, w in ((F32, 4), (F64, 8), (7, 4)):
            for A in arc_counts(S, w):
                yield S, A, dtype


def routes(S, A, dtype):
    'The six routes of one batch, with neutral extras: frames and utterance bins wanted.'
    lib, b = _hip.lib(), ctypes.byref(desc(S, A))
    return {'arcs': lib.beer_hmm_arcs_route(dtype, b, N_CAT, 1),
            'segposts': lib.beer_hmm_segposts_route(dtype, b, N_CAT, 0),
            'segments': lib.beer_hmm_segments_route(dtype, b, N_CAT, 0),
            'maxmarg': lib.beer_hmm_maxmarg_route(dtype, b, N_CAT, 1, 1, 1),
            'evidence': lib.beer_hmm_evidence_route(dtype, b),
            'sample': lib.beer_hmm_sample_route(dtype, b, 1)}


ARCS_LDS = {'arcs': _hip.ARCS_ARCS_LDS, 'segposts': _hip.SEGPOSTS_ARCS_LDS,
            'segments': _hip.SEGMENTS_ARCS_LDS, 'maxmarg': _hip.MAXMARG_ARCS_LDS}


def test_the_six_routes_refuse_the_same_batches():
    refused, served = 0, 0
    for S, A, dtype in grid():
        got = routes(S, A, dtype)
        no = {name for name, r in got.items() if r == _hip.EINVAL}
        assert no in (set(), set(got)), (S, A, dtype, got)
        # ... and where the header says: the dtype, the states, two fp64 rows within a CU's LDS
        assert bool(no) == (dtype == 7 or S > 10232), (S, A, dtype)
        assert all(r == _hip.EINVAL or r > 0 for r in got.values()), (S, A, dtype, got)
        refused += bool(no)
        served += not no
    assert refused and served
    lib = _hip.lib()
    for b in (None, desc(0, 0), desc(8, -1), desc(8, 16, nutt=-1)):
        p = ctypes.byref(b) if b is not None else None
        assert lib.beer_hmm_arcs_route(F64, p, N_CAT, 1) == _hip.EINVAL
        assert lib.beer_hmm_segposts_route(F64, p, N_CAT, 0) == _hip.EINVAL
        assert lib.beer_hmm_segments_route(F64, p, N_CAT, 0) == _hip.EINVAL
        assert lib.beer_hmm_maxmarg_route(F64, p, N_CAT, 1, 1, 1) == _hip.EINVAL
        assert lib.beer_hmm_evidence_route(F64, p) == _hip.EINVAL
        assert lib.beer_hmm_sample_route(F64, p, 1) == _hip.EINVAL


def test_the_four_category_kernels_stage_their_arcs_for_the_same_batches():
    seen = set()
    for S, A, dtype in grid():
        got = routes(S, A, dtype)
        if got['arcs'] == _hip.EINVAL:
            continue
        bits = {name: bool(got[name] & bit) for name, bit in ARCS_LDS.items()}
        assert len(set(bits.values())) == 1, (S, A, dtype, bits)
        w = 4 if dtype == F32 else 8
        assert bits['arcs'] == ((2 * S + 16) * 8 + (S + 2 + 2 * A) * 4 + (A + 1) * w <= 64 * 1024), \
            (S, A, dtype)
        seen.add(bits['arcs'])
    assert seen == {False, True}
