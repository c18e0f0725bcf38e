"""CPU: the attached LCP array and the matching statistics (include/archon_hip.h: archon_hip_fm_attach_lcp, _fm_attach_lcp_dev,
_block_fm_attach_lcp, _fm_ms, _fm_ms_dev, _get_fm_ms_stats) are declared, exported and bound; the statistics mirror has the C
layout; bad arguments are refused and, without a GPU, the calls fail loudly.  And the procedure of the header
(fm_ms_naive.Rule) is pinned to the DEFINITION from the text alone on every short string -- the records, the SMEMs that follow
from them, the bounds on both work counters; the C brute force the GPU tests use (fm_ms_naive.c) agrees with it."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_mem_naive
import fm_ms_naive as N
import lcp_kasai
import repeats_naive

FUNCTIONS = ["archon_hip_fm_attach_lcp", "archon_hip_fm_attach_lcp_dev", "archon_hip_block_fm_attach_lcp", "archon_hip_fm_ms",
             "archon_hip_fm_ms_dev", "archon_hip_get_fm_ms_stats"]


def test_ms_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmMsStats", "fm_ms_stats", "ms_smems"):
        assert hasattr(pyarchon, name), name
    for name in ("attach_lcp", "attach_lcp_dev", "ms", "ms_dev"):
        assert hasattr(pyarchon.FmIndex, name), name
    params = inspect.signature(pyarchon.Block.fm_index).parameters
    assert list(params)[-1] == "lcp" and params["lcp"].default is False and params["mirror"].default is False
    assert list(inspect.signature(pyarchon.ms_smems).parameters) == ["len", "lo", "hi", "offsets", "min_len"]
    assert inspect.signature(pyarchon.FmIndex.ms).parameters["rows"].default is True


def test_fm_ms_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_ms_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmMsStats._fields_]
    assert names == ["n", "patterns", "fan", "levels", "attached", "pattern_bytes", "steps", "parents", "probes", "matched", "longest",
                     "lcp_bytes", "kernel_launches", "host_syncs", "ms_lcp", "ms_attach", "ms_query"]
    got = _layout(tmp_path, "archon_hip_fm_ms_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmMsStats)
    assert got[1:] == [getattr(pyarchon.FmMsStats, k).offset for k in names]


def test_ms_bad_arguments():
    """null pointers, lo without hi and decreasing offsets are ARCHON_E_ARG with or without a device: they are refused before
    the handle is used (a stand-in handle is never read)"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    pat = np.zeros(8, np.uint8)
    off, bad_off = np.array([0, 2, 4], np.uint32), np.array([0, 3, 2], np.uint32)
    ln, lo, hi = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    lcp = np.zeros(8, np.uint32)
    stand_in = _p(np.zeros(64, np.uint8))
    fn = L.archon_hip_fm_ms
    assert fn(None, _p(pat), _p(off), 2, _p(ln), _p(lo), _p(hi)) == E
    assert fn(stand_in, None, _p(off), 2, _p(ln), _p(lo), _p(hi)) == E
    assert fn(stand_in, _p(pat), None, 2, _p(ln), _p(lo), _p(hi)) == E
    assert fn(stand_in, _p(pat), _p(off), 2, None, _p(lo), _p(hi)) == E
    assert fn(stand_in, _p(pat), _p(off), 2, _p(ln), _p(lo), None) == E
    assert fn(stand_in, _p(pat), _p(off), 2, _p(ln), None, _p(hi)) == E
    assert fn(stand_in, _p(pat), _p(bad_off), 2, _p(ln), _p(lo), _p(hi)) == E
    assert fn(stand_in, _p(pat), _p(bad_off), 2, _p(ln), None, None) == E
    dv = L.archon_hip_fm_ms_dev
    assert dv(None, _p(pat), _p(off), 2, _p(ln), _p(lo), _p(hi), None) == E
    assert dv(stand_in, None, _p(off), 2, _p(ln), _p(lo), _p(hi), None) == E
    assert dv(stand_in, _p(pat), None, 2, _p(ln), _p(lo), _p(hi), None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, None, _p(lo), _p(hi), None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, _p(ln), _p(lo), None, None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, _p(ln), None, _p(hi), None) == E
    assert L.archon_hip_fm_attach_lcp(None, _p(lcp)) == E
    assert L.archon_hip_fm_attach_lcp(stand_in, None) == E
    assert L.archon_hip_fm_attach_lcp_dev(None, _p(lcp), None) == E
    assert L.archon_hip_fm_attach_lcp_dev(stand_in, None, None) == E
    assert L.archon_hip_block_fm_attach_lcp(None, stand_in) == E
    assert L.archon_hip_block_fm_attach_lcp(stand_in, None) == E
    assert L.archon_hip_get_fm_ms_stats(0, None) == E
    assert (ln == 0).all() and (lo == 0).all() and (hi == 0).all()
    if pyarchon.device_count() == 0:
        # a thread that ran no matching-statistics call has no statistics
        assert L.archon_hip_get_fm_ms_stats(0, ctypes.byref(pyarchon.FmMsStats())) == E


def test_ms_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).attach_lcp(np.array([0, 1, 3, 0, 0, 2], np.uint32)).ms([b"nanb"])
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_index(32, lcp=True)


def _as_arrays(records_of_patterns):
    """the records of several patterns as FmIndex.ms returns them: (len, lo, hi, offsets)"""
    flat = [r for recs in records_of_patterns for r in recs]
    off = np.zeros(len(records_of_patterns) + 1, np.uint32)
    np.cumsum([len(recs) for recs in records_of_patterns], out=off[1:])
    cols = [np.array([r[i] for r in flat], np.uint32) for i in range(3)]
    return cols[0], cols[1], cols[2], off


def test_rule_header_examples():
    """the two worked examples of the header, literally"""
    import pyarchon
    sa, lcp, bwt, base = repeats_naive.a7_arrays(b"banana")
    assert (bwt, base, sa, lcp) == (b"nnbaaa", 2, [2, 4, 6, 1, 3, 5], [0, 1, 3, 0, 0, 2])
    r = N.Rule(b"banana")
    assert r.search(b"nanb") == ([(1, 4, 6), (2, 1, 3), (3, 5, 6), (1, 3, 4)], 4, 2)
    assert N.smems(r.search(b"nanb")[0]) == [(5, 6, 0, 3), (3, 4, 3, 4)]
    assert N.smems(r.search(b"nanb")[0]) == fm_mem_naive.Rule(b"banana").search(b"nanb")[0]
    got = pyarchon.ms_smems(*_as_arrays([r.search(b"nanb")[0]]))
    assert [tuple(int(q[k]) for k in ("lo", "hi", "start", "end", "pattern")) for q in got] == [(5, 6, 0, 3, 0), (3, 4, 3, 4, 0)]
    assert r.search(b"") == ([], 0, 0)
    assert repeats_naive.a7_arrays(b"aaaa")[1] == [0, 3, 2, 1]
    assert N.Rule(b"aaaa").search(b"aaaab") == ([(1, 0, 4), (2, 0, 3), (3, 0, 2), (4, 0, 1), (0, 0, 4)], 7, 4)


def test_rule_against_the_definition():
    """every block of <= 6 bytes over two symbols, every pattern of <= 4 bytes over those symbols and an absent one: the
    procedure's records are the definition's; the SMEMs that pyarchon.ms_smems derives from them are those of the SMEM
    definition, in its order, with the rows of the pieces, for min_len 1 and 2; steps <= 2 m and parents <= m"""
    import pyarchon
    patterns = [bytes(p) for m in range(0, 5) for p in itertools.product((0, 1, 7), repeat=m)]
    cases = 0
    for n in range(1, 7):
        for tt in itertools.product((0, 1), repeat=n):
            x = bytes(tt)
            r = N.Rule(x)
            got = [r.search(P) for P in patterns]
            for P, (recs, steps, parents) in zip(patterns, got):
                assert recs == N.definition(x, P), (x, P)
                assert steps <= 2 * len(P) and parents <= len(P), (x, P)
                want = fm_mem_naive.definition(x, P)
                assert [(b, e) for _, _, b, e in N.smems(recs)] == want, (x, P)
                cases += 1
            arrays = _as_arrays([g[0] for g in got])
            for min_len in (1, 2):
                mems = pyarchon.ms_smems(*arrays, min_len=min_len)
                want = [(lo, hi, b, e, j) for j, g in enumerate(got) for lo, hi, b, e in N.smems(g[0], min_len)]
                assert [tuple(int(q[k]) for k in ("lo", "hi", "start", "end", "pattern")) for q in mems] == want, x
                assert (mems["reserved0"] == 0).all()
    assert cases == 126 * 121


def test_rule_ends_on_any_array():
    """a wrong array gives unspecified records but the same bounds: steps <= 2 m, parents <= m, every range inside [0, n]"""
    rng = np.random.default_rng(9)
    for trial in range(60):
        n = int(rng.integers(1, 12))
        x = bytes(rng.integers(0, 2, n, dtype=np.uint8))
        r = N.Rule(x, lcp=[int(v) for v in rng.integers(0, n, n)])
        for _ in range(5):
            P = bytes(rng.integers(0, 3, int(rng.integers(0, 12)), dtype=np.uint8))
            recs, steps, parents = r.search(P)
            assert steps <= 2 * len(P) and parents <= len(P)
            assert all(0 <= lo < hi <= n for _, lo, hi in recs)


def test_c_brute_force_agrees_with_rule(tmp_path):
    """fm_ms_naive.c (the GPU tests' reference on large blocks) against the procedure on random blocks of <= 200 bytes"""
    naive = N.build(tmp_path)
    kasai = lcp_kasai.build(tmp_path)
    rng = np.random.default_rng(5)
    for trial in range(30):
        n = int(rng.integers(1, 201))
        sigma = int(rng.choice([2, 4, 256]))
        x = bytes(rng.integers(0, sigma, n, dtype=np.uint8))
        r = N.Rule(x)
        lcp = kasai(np.frombuffer(x, np.uint8), r.sa)
        assert lcp[1:].tolist() == r.lcp[1:]
        pats = []
        for _ in range(6):
            m = int(rng.integers(0, 40))
            q = int(rng.integers(0, n))
            P = bytearray(np.resize(np.frombuffer(x, np.uint8)[q:], m).tobytes()) if m else bytearray()
            for _ in range(int(rng.integers(0, 3)) if m else 0):
                P[int(rng.integers(0, m))] = int(rng.integers(0, sigma + 1)) & 255
            pats.append(bytes(P))
        pats += [b"", np.resize(np.frombuffer(x, np.uint8), n + 3).tobytes()]
        length, lo, hi, off, steps, parents, matched, longest = naive(np.frombuffer(x, np.uint8), r.sa, lcp, pats)
        want = [r.search(P) for P in pats]
        flat = [rec for w in want for rec in w[0]]
        assert list(zip(length.tolist(), lo.tolist(), hi.tolist())) == flat, (x, pats)
        assert off.tolist() == np.cumsum([0] + [len(P) for P in pats]).tolist()
        assert (steps, parents) == (sum(w[1] for w in want), sum(w[2] for w in want)), (x, pats)
        assert matched == sum(rec[0] for rec in flat) and longest == max([rec[0] for rec in flat] + [0])
