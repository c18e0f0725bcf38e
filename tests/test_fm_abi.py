"""CPU: the FM index entry points (include/archon_hip.h, archon_hip_fm_*) are declared, exported and bound; their statistics
mirror has the C layout; they refuse bad arguments and, without a GPU, fail loudly.  And the expected answers of the GPU
tests are pinned to the definition: tests/fm_naive.c against brute force, the search rule of the header (fm_naive.py)
against every occurrence of every short pattern in every short string."""
import ctypes
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_naive

FM_FUNCTIONS = ["archon_hip_fm_create", "archon_hip_fm_create_dev", "archon_hip_fm_destroy", "archon_hip_fm_count", "archon_hip_fm_count_dev",
                "archon_hip_block_fm_count", "archon_hip_block_fm_locate", "archon_hip_get_fm_stats"]
BANANA_BWT = b"nnbaaa"          # a7 order of "banana": primary row 2, sa = 2 4 6 1 3 5 (test_abi.py)


def test_fm_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FM_FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert "FM_SUB_ROWS" in pyarchon._ROUTE_NAMES and "FM_SUPER_ROWS" in pyarchon._ROUTE_NAMES
    for name in ("FmIndex", "fm_stats", "FmStats"):
        assert hasattr(pyarchon, name), name
    for name in ("fm_count", "fm_locate"):
        assert hasattr(pyarchon.Block, name), name
    for name in ("from_dev", "count", "count_dev", "close"):
        assert hasattr(pyarchon.FmIndex, name), name


def test_fm_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmStats._fields_]
    got = _layout(tmp_path, "archon_hip_fm_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmStats)
    assert got[1:] == [getattr(pyarchon.FmStats, k).offset for k in names]


def test_fm_bad_arguments():
    """null pointers, n = 0 and a primary row >= n are ARCHON_E_ARG, with or without a device; so are test routes out of range"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    bwt = np.frombuffer(BANANA_BWT, np.uint8).copy()
    pat = np.frombuffer(b"an", np.uint8).copy()
    off = np.array([0, 2], np.uint32)
    lo, hi = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    h = ctypes.c_void_p(None)
    out = ctypes.byref(h)
    assert L.archon_hip_fm_create(None, 6, 2, 0, out) == E
    assert L.archon_hip_fm_create(_p(bwt), 6, 2, 0, None) == E
    assert L.archon_hip_fm_create(_p(bwt), 0, 0, 0, out) == E
    assert L.archon_hip_fm_create(_p(bwt), 6, 6, 0, out) == E
    assert L.archon_hip_fm_create(_p(bwt), 6, 0xFFFFFFFF, 0, out) == E
    assert L.archon_hip_fm_create_dev(None, 6, 2, 0, None, out) == E
    assert L.archon_hip_fm_create_dev(_p(bwt), 6, 2, 0, None, None) == E
    assert L.archon_hip_fm_create_dev(_p(bwt), 0, 0, 0, None, out) == E
    assert L.archon_hip_fm_create_dev(_p(bwt), 6, 7, 0, None, out) == E
    assert h.value is None
    assert L.archon_hip_fm_count(None, _p(pat), _p(off), 1, _p(lo), _p(hi)) == E
    assert L.archon_hip_fm_count_dev(None, _p(pat), _p(off), 1, _p(lo), _p(hi), None) == E
    assert L.archon_hip_block_fm_count(None, _p(pat), _p(off), 1, _p(lo), _p(hi)) == E
    total = ctypes.c_uint64(0)
    assert L.archon_hip_block_fm_locate(None, _p(pat), _p(off), 1, _p(lo), 1, ctypes.cast(ctypes.byref(total), ctypes.c_void_p)) == E
    assert L.archon_hip_get_fm_stats(0, None) == E
    L.archon_hip_fm_destroy(None)                 # a null handle is nothing to free
    for name, value in (("FM_SUB_ROWS", 8), ("FM_SUB_ROWS", 2048), ("FM_SUB_ROWS", 100), ("FM_SUB_ROWS", -16),
                        ("FM_SUPER_ROWS", 131072), ("FM_SUPER_ROWS", 3000), ("FM_SUPER_ROWS", 8), ("FM_SUPER_ROWS", -1)):
        assert L.archon_hip_test_route(name.encode(), value) == E, (name, value)
    for name, value in (("FM_SUB_ROWS", 16), ("FM_SUB_ROWS", 1024), ("FM_SUB_ROWS", 0), ("FM_SUPER_ROWS", 64), ("FM_SUPER_ROWS", 65536),
                        ("FM_SUPER_ROWS", 0)):
        assert L.archon_hip_test_route(name.encode(), value) == 0, (name, value)
    assert L.archon_hip_test_route(b"RESET", 0) == 0


def test_fm_without_a_device():
    """no CPU fallback: without a GPU every FM entry point that can be reached is ARCHON_E_NODEVICE (with one, the host
    form answers "banana" as the header says)"""
    import pyarchon
    L = pyarchon.lib()
    bwt = np.frombuffer(BANANA_BWT, np.uint8).copy()
    if pyarchon.device_count() > 0:
        f = pyarchon.FmIndex(bwt, 2)
        lo, hi = f.count([b"an", b"ana", b"ab", b""])
        f.close()
        assert list(zip(lo.tolist(), hi.tolist()))[:2] == [(4, 6), (1, 3)] and lo[2] == hi[2] and (lo[3], hi[3]) == (0, 6)
        return
    h = ctypes.c_void_p(None)
    assert L.archon_hip_fm_create(_p(bwt), 6, 2, 0, ctypes.byref(h)) == pyarchon.E_NODEVICE
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_fm_create_dev(_p(bwt), 6, 2, 0, None, ctypes.byref(h)) == pyarchon.E_NODEVICE
    assert h.value is None
    assert L.archon_hip_block_create(0, ctypes.byref(h)) == pyarchon.E_NODEVICE    # so no handle reaches block_fm_*
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(bwt, 2)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.fm_stats()


def _occurrences(x, p):
    """the definition: starts q with x[q .. q+m) == p and 1 <= q + m <= n"""
    n, m = len(x), len(p)
    return [q for q in range(n - m + 1) if x[q:q + m] == p and q + m >= 1]


def _longest_prefix(x, p):
    return max(l for l in range(len(p) + 1) if l == 0 or _occurrences(x, p[:l]))


def test_naive_helper_is_the_definition(tmp_path):
    """tests/fm_naive.c against brute force: every string of length 1-6 over {0, 1, 255} with every pattern of length 0-3
    over {0, 1, 255}, overlapping matches included; then long periodic strings, where KMP's borders matter"""
    naive = fm_naive.build(tmp_path)
    pats = [bytes(t) for m in range(4) for t in itertools.product((0, 1, 255), repeat=m)]
    for n in range(1, 7):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            count, L, starts = naive(np.frombuffer(x, np.uint8), pats, starts=True)
            for j, p in enumerate(pats):
                want = _occurrences(x, p)
                assert count[j] == len(want) and starts[j].tolist() == want, (x, p)
                assert L[j] == _longest_prefix(x, p), (x, p)
    x = b"abaababaabaababaababa" * 3 + b"aaaaaaab"
    pats = [b"aba", b"abaab", b"aa", b"aaaa", b"aaaaaaab", b"aaaaaaaab", b"babaa", x, x + b"a", b"aab" + x]
    count, L, starts = naive(np.frombuffer(x, np.uint8), pats, starts=True)
    for j, p in enumerate(pats):
        want = _occurrences(x, p)
        assert count[j] == len(want) and starts[j].tolist() == want, p
        assert L[j] == _longest_prefix(x, p), p


def test_search_rule_on_banana():
    """the header's example: "an" gives [0, 3) then [4, 6); "ana" gives [1, 3); "ab" is empty at its second step"""
    assert fm_naive.backward_search(BANANA_BWT, 2, b"a") == (0, 3, 0)
    assert fm_naive.backward_search(BANANA_BWT, 2, b"an") == (4, 6, 1)
    assert fm_naive.backward_search(BANANA_BWT, 2, b"ana") == (1, 3, 2)
    lo, hi, steps = fm_naive.backward_search(BANANA_BWT, 2, b"ab")
    assert lo == hi and steps == 1
    assert fm_naive.backward_search(BANANA_BWT, 2, b"") == (0, 6, 0)
    assert fm_naive.backward_search(BANANA_BWT, 2, b"bananas") == (0, 0, 0)


def test_search_rule_is_the_definition(oracle):
    """the rule of the header (fm_naive.backward_search) on every string of length 1-6 over {0, 1, 255} and every pattern of
    length 0-3 over {0, 1, 2, 255}: hi - lo is the number of occurrences, sa[r] - m over [lo, hi) are their starts, and the
    rank steps are those fm_naive.expected_steps gives.  SA and BWT from the oracle."""
    pats = [bytes(t) for m in range(4) for t in itertools.product((0, 1, 2, 255), repeat=m)]
    for n in range(1, 7):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            sa, bwt, base = oracle.forward(np.frombuffer(x, np.uint8))
            for p in pats:
                lo, hi, steps = fm_naive.backward_search(bwt.tobytes(), base, p)
                want = _occurrences(x, p)
                assert 0 <= lo <= hi <= n and hi - lo == len(want), (x, p)
                assert sorted(int(sa[r]) - len(p) for r in range(lo, hi)) == want, (x, p)
                assert steps == fm_naive.expected_steps(len(p), n, _longest_prefix(x, p)), (x, p)
