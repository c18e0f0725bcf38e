"""CPU: the edit-distance search entry points (include/archon_hip.h, archon_hip_fm_edit, _fm_edit_dev, _block_fm_edit,
_get_fm_edit_stats) are declared, exported and bound; the hit and statistics mirrors have the C layout; the test routes
exist and refuse bad values; bad arguments are refused before the handle is used and, without a GPU, the calls fail loudly.
And the models the GPU tests take their answers from (fm_edit_naive) are pinned to each other: the rule to the definition,
the filter and the band to the rule."""
import ctypes
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_edit_naive as E

FUNCTIONS = ["archon_hip_fm_edit", "archon_hip_fm_edit_dev", "archon_hip_block_fm_edit", "archon_hip_get_fm_edit_stats"]


def test_edit_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmEditStats", "fm_edit_stats", "FM_EDIT"):
        assert hasattr(pyarchon, name), name
    for name in ("edit", "edit_dev"):
        assert hasattr(pyarchon.FmIndex, name), name
    assert hasattr(pyarchon.Block, "fm_edit")


def test_fm_edit_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_edit_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmEditStats._fields_]
    assert names == ["n", "patterns", "max_errors", "tile", "batches", "built", "pattern_bytes", "seed_rows", "tiles", "rows", "hits", "lf_steps",
                     "kernel_launches", "host_syncs", "ms_build", "ms_seed", "ms_extract", "ms_count", "ms_emit"]
    got = _layout(tmp_path, "archon_hip_fm_edit_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmEditStats)
    assert got[1:] == [getattr(pyarchon.FmEditStats, k).offset for k in names]


def test_fm_edit_hit_struct_layout(tmp_path):
    """FM_EDIT is archon_hip_fm_edit_hit byte for byte"""
    import pyarchon
    names = list(pyarchon.FM_EDIT.names)
    assert names == ["start", "end", "distance", "pattern"]
    got = _layout(tmp_path, "archon_hip_fm_edit_hit", names)
    assert got[0] == pyarchon.FM_EDIT.itemsize
    assert got[1:] == [pyarchon.FM_EDIT.fields[k][1] for k in names]


def test_edit_routes():
    """EDIT_TILE and EDIT_BATCH are routes of the test hook and of the binding, refuse values out of range, and go back with RESET"""
    import pyarchon
    L = pyarchon.lib()
    assert "EDIT_TILE" in pyarchon._ROUTE_NAMES and "EDIT_BATCH" in pyarchon._ROUTE_NAMES
    try:
        for name, good, bad in ((b"EDIT_TILE", (0, 1, 5, 32, 64), (-1, 65, 1000)), (b"EDIT_BATCH", (0, 1, 3, 1 << 20), (-1, 1 << 31))):
            for v in good:
                assert L.archon_hip_test_route(name, v) == 0, (name, v)
            for v in bad:
                assert L.archon_hip_test_route(name, v) == pyarchon.E_ARG, (name, v)
        # a tile too wide for the errors of a call is refused by the call, before the handle is used
        assert L.archon_hip_test_route(b"EDIT_TILE", 61) == 0
        pat, off, nh = np.zeros(8, np.uint8), np.array([0, 4, 8], np.uint32), np.zeros(2, np.uint32)
        total = ctypes.c_uint64(0)
        stand_in = _p(np.zeros(64, np.uint8))
        assert L.archon_hip_fm_edit(stand_in, _p(pat), _p(off), 2, 2, _p(nh), None, 0, ctypes.byref(total)) == pyarchon.E_ARG
        assert "EDIT_TILE" in L.archon_hip_last_error().decode()
    finally:
        assert L.archon_hip_test_route(b"RESET", 0) == 0


def test_edit_bad_arguments():
    """null pointers, K > 8, decreasing offsets, m <= K and m > 4096 are ARCHON_E_ARG with or without a device: they are
    refused before the handle is used (a stand-in handle is never read)"""
    import pyarchon
    L = pyarchon.lib()
    E_ARG = pyarchon.E_ARG
    pat = np.zeros(5000, np.uint8)
    off, bad_off = np.array([0, 2, 4], np.uint32), np.array([0, 3, 2], np.uint32)
    short_off, long_off = np.array([0, 2, 5], np.uint32), np.array([0, 4097, 4100], np.uint32)
    nh = np.zeros(2, np.uint32)
    hits = np.zeros(4, pyarchon.FM_EDIT)
    total = ctypes.c_uint64(0)
    tp = ctypes.byref(total)
    stand_in = _p(np.zeros(64, np.uint8))
    for fn in (L.archon_hip_fm_edit, L.archon_hip_block_fm_edit):
        assert fn(None, _p(pat), _p(off), 2, 1, _p(nh), _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, None, _p(off), 2, 1, _p(nh), _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, _p(pat), None, 2, 1, _p(nh), _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, _p(pat), _p(off), 2, 1, None, _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, _p(pat), _p(off), 2, 1, _p(nh), _p(hits), 4, None) == E_ARG
        assert fn(stand_in, _p(pat), _p(off), 2, 9, _p(nh), _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, _p(pat), _p(off), 2, 99, _p(nh), None, 0, tp) == E_ARG
        assert fn(stand_in, _p(pat), _p(bad_off), 2, 1, _p(nh), _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, _p(pat), _p(short_off), 2, 2, _p(nh), _p(hits), 4, tp) == E_ARG      # m = 2 <= K = 2
        assert fn(stand_in, _p(pat), _p(off), 2, 2, _p(nh), _p(hits), 4, tp) == E_ARG
        assert fn(stand_in, _p(pat), _p(long_off), 2, 1, _p(nh), _p(hits), 4, tp) == E_ARG       # m = 4097
        assert "4097" in L.archon_hip_last_error().decode()
    assert (nh == 0).all() and total.value == 0 and (hits["end"] == 0).all()
    dv = L.archon_hip_fm_edit_dev
    assert dv(None, _p(pat), _p(off), 2, 1, _p(nh), None, 0, tp, None) == E_ARG
    assert dv(stand_in, _p(pat), _p(off), 2, 9, _p(nh), None, 0, tp, None) == E_ARG
    assert dv(stand_in, _p(pat), _p(off), 2, 1, None, None, 0, tp, None) == E_ARG
    assert dv(stand_in, _p(pat), _p(off), 2, 1, _p(nh), None, 0, None, None) == E_ARG
    assert L.archon_hip_get_fm_edit_stats(0, None) == E_ARG
    if pyarchon.device_count() == 0:
        # a thread that ran no edit call has no statistics
        assert L.archon_hip_get_fm_edit_stats(0, ctypes.byref(pyarchon.FmEditStats())) == E_ARG


def test_edit_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).edit([b"bnan"], 1)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_edit([b"bnan"], 1)


def test_rule_banana():
    """the worked example of the header"""
    for fn in (E.definition, E.rule, E.rule_np):
        assert fn(b"banana", b"bnan", 1) == [(0, 3, 1), (2, 5, 1)]
        assert fn(b"banana", b"nab", 1) == [(2, 4, 1), (2, 5, 1), (4, 6, 1)]
    assert E.tile_model(b"banana", b"bnan", 1, 32) == ([(0, 3, 1), (2, 5, 1)], {"seed_rows": 2, "tiles": 1, "rows": 4, "hits": 2})
    assert E.pieces(9, 8) == list(range(10)) and E.pieces(7, 2) == [0, 2, 4, 7]


def _all_tiles(x, P, K, W):
    n, m = len(x), len(P)
    return range((n - m + K) // W + 1) if n - m + K >= 0 else range(0)


def test_models_agree_exhaustively():
    """every string of length <= 5 over two symbols, every pattern of length <= 4, every K < min(m, 3): the rule is the
    definition; the filter (W = 1, 3, 32) finds exactly the rule's matches; the band over every tile, marked or not, gives
    the rule's matches too"""
    patterns = [bytes(p) for m in range(1, 5) for p in itertools.product((0, 1), repeat=m)]
    for n in range(0, 6):
        for tt in itertools.product((0, 1), repeat=n):
            x = bytes(tt)
            for P in patterns:
                for K in range(min(len(P), 3)):
                    want = E.rule(x, P, K)
                    assert want == E.definition(x, P, K), (x, P, K)
                    assert want == E.rule_np(x, P, K), (x, P, K)
                    for W in (1, 3, 32):
                        assert E.tile_model(x, P, K, W)[0] == want, (x, P, K, W)
                        band = [h for t in _all_tiles(x, P, K, W) for h in E.band_model(x, P, K, W, t)]
                        assert band == want, (x, P, K, W)


def test_models_agree_on_random_cases():
    """seeded random cases over 1, 2, 4 and 26 symbols, n < 400, m < 40, K <= 8: rule_np is the rule, and the filter and the
    band over the marked tiles give the rule's matches at W = 1, 5, 32 and 64 - 2K"""
    rng = np.random.default_rng(1)
    for trial in range(120):
        sigma = int(rng.choice([1, 2, 4, 26]))
        n, m = int(rng.integers(0, 400)), int(rng.integers(1, 40))
        K = int(rng.integers(0, min(m, 9)))
        x = bytes(rng.integers(0, sigma, n, dtype=np.uint8))
        if n > m and rng.random() < 0.7:
            q = int(rng.integers(0, n - m))
            P = bytearray(x[q:q + m])
            for _ in range(K):
                P[int(rng.integers(0, m))] = int(rng.integers(0, sigma))
            P = bytes(P)
        else:
            P = bytes(rng.integers(0, sigma, m, dtype=np.uint8))
        want = E.rule_np(x, P, K)
        if trial < 40:
            assert want == E.rule(x, P, K), trial
        for W in (1, 5, 32, 64 - 2 * K):
            hits, counters = E.tile_model(x, P, K, W)
            assert hits == want, (trial, W)
            assert counters["hits"] == len(want) and counters["rows"] == counters["tiles"] * m
            tiles, _ = E.marked_tiles(x, P, K, W)
            assert [h for t in tiles for h in E.band_model(x, P, K, W, t)] == want, (trial, W)
