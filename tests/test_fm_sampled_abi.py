"""CPU: the sampled FM index entry points (include/archon_hip.h, archon_hip_fm_sample, _block_fm_index, _fm_read_samples,
_fm_locate, _fm_extract, _fm_extract_dev, _get_fm_walk_stats) are declared, exported and bound; their statistics mirror has
the C layout; they refuse bad arguments and, without a GPU, fail loudly.  And the rule of the header (fm_sampled_naive.py)
is pinned to brute force on every short string: samples, locate with its exact LF steps, extract."""
import ctypes
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_naive
import fm_sampled_naive as M

FUNCTIONS = ["archon_hip_fm_sample", "archon_hip_block_fm_index", "archon_hip_fm_read_samples", "archon_hip_fm_locate",
             "archon_hip_fm_extract", "archon_hip_fm_extract_dev", "archon_hip_get_fm_walk_stats"]
RATES = (1, 2, 4, 8, 64)


def test_sampled_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert "FM_SAMPLE_WALK" in pyarchon._ROUTE_NAMES
    for name in ("FmWalkStats", "fm_walk_stats"):
        assert hasattr(pyarchon, name), name
    for name in ("sample", "samples", "locate", "extract", "extract_dev"):
        assert hasattr(pyarchon.FmIndex, name), name
    assert hasattr(pyarchon.Block, "fm_index")


def test_fm_walk_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_walk_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmWalkStats._fields_]
    got = _layout(tmp_path, "archon_hip_fm_walk_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmWalkStats)
    assert got[1:] == [getattr(pyarchon.FmWalkStats, k).offset for k in names]


def test_sampled_bad_arguments():
    """null pointers are ARCHON_E_ARG, with or without a device (bad rates: tests/test_gpu_fm_sampled.py); the route is known"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    h = ctypes.c_void_p(None)
    starts, off = np.zeros(1, np.uint32), np.array([0, 1], np.uint32)
    out = np.zeros(4, np.uint8)
    pos = np.zeros(4, np.uint32)
    total = ctypes.c_uint64(0)
    cnt = ctypes.c_uint32(0)
    assert L.archon_hip_fm_sample(None, 32) == E
    assert L.archon_hip_block_fm_index(None, 32, ctypes.byref(h)) == E
    assert L.archon_hip_fm_read_samples(None, _p(pos), 4, ctypes.byref(cnt)) == E
    assert L.archon_hip_fm_locate(None, _p(out), _p(off), 1, _p(pos), 4, ctypes.byref(total)) == E
    assert L.archon_hip_fm_extract(None, _p(starts), _p(off), 1, _p(out)) == E
    assert L.archon_hip_fm_extract_dev(None, _p(starts), _p(off), 1, _p(out), None) == E
    assert L.archon_hip_get_fm_walk_stats(0, None) == E
    assert L.archon_hip_test_route(b"FM_SAMPLE_WALK", 1) == 0
    assert L.archon_hip_test_route(b"RESET", 0) == 0
    if pyarchon.device_count() == 0:
        # a thread that ran no sampled call has no statistics
        assert L.archon_hip_get_fm_walk_stats(0, ctypes.byref(pyarchon.FmWalkStats())) == E


def test_sampled_no_gpu_fails_loudly():
    """without a device the handles cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).sample(2)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block()


def test_model_banana():
    """the worked example of the header"""
    sa, bwt, base = M.a7_forward(b"banana")
    assert (sa, bwt, base) == ([2, 4, 6, 1, 3, 5], b"nnbaaa", 2)
    m = M.Model(bwt, base, 2)
    assert m.isa == [2, 0, 1]
    assert sorted(m.marked) == [0, 1, 2]
    assert m.lf[4] == 1 and m.lf[5] == 2
    starts, steps = m.locate(b"an")
    assert starts == [1, 3] and steps == [1, 1]
    # x[3 .. 5): from isa_s[1] = row 0 one step to row 4 ('a'); cut at item 4, whose walk starts at isa_s[2] = row 1 ('n')
    assert m.segments(3, 2) == [(1, 3, 4), (2, 4, 5)]
    assert m.lf[0] == 4 and m.bwt[4] == ord("a") and m.bwt[1] == ord("n")
    assert m.extract(3, 2) == (b"an", 1)
    assert list(M.expected_isa(sa, base, 2)) == [2, 0, 1]


def _strings():
    for n in range(1, 7):
        yield from itertools.product((0, 1, 255), repeat=n)


def test_model_against_brute_force():
    """every string of length <= 6 over {0, 1, 255}, every pattern of length <= 3, rates 1, 2, 4, 8 and 64: the samples are
    the inverse of the suffix array at the items kS, locate gives sa[r] - m on every row of the range with the exact LF
    steps, extract gives x for every start and length with the exact LF steps"""
    patterns = [b""] + [bytes(p) for m in range(1, 4) for p in itertools.product((0, 1, 255), repeat=m)]
    for t in _strings():
        x = bytes(t)
        n = len(x)
        sa, bwt, base = M.a7_forward(x)
        for S in RATES:
            m = M.Model(bwt, base, S)
            assert m.isa == list(M.expected_isa(sa, base, S)), (x, S)
            # every row's sa value and steps
            for r in range(n):
                s, steps = m.sa_of(r)
                assert s == sa[r], (x, S, r)
                assert steps == M.locate_steps(sa, [r], S)[0], (x, S, r)
                assert steps <= min(S - 1, n - 1)
            for p in patterns:
                starts, steps = m.locate(p)
                lo, hi, _ = fm_naive.backward_search(bwt, base, p)
                assert starts == [sa[r] - len(p) for r in range(lo, hi)], (x, S, p)
                assert sorted(starts) == [q for q in range(n - len(p) + 1) if x[q:q + len(p)] == p and q + len(p) >= 1], (x, S, p)
                assert sum(steps) == int(M.locate_steps(sa, range(lo, hi), S).sum())
            for a in range(n + 1):
                for L in range(n - a + 1):
                    got, steps = m.extract(a, L)
                    assert got == x[a:a + L], (x, S, a, L)
                    assert steps == M.extract_steps([a], [L], S)
                    assert all(v - k * S - 1 <= S - 1 for k, _, v in m.segments(a, L))
