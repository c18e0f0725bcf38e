"""CPU: the mirror and SMEM entry points (include/archon_hip.h: archon_hip_fm_mirror, _fm_mirror_dev, _block_fm_mirror,
_fm_read_mirror, _fm_smems, _fm_smems_dev, _fm_locate_mems, _block_fm_locate_mems, _get_fm_mem_stats) are declared,
exported and bound; the SMEM and statistics mirrors have the C layout; bad arguments are refused and, without a GPU, the
calls fail loudly.  And the procedure of the header (fm_mem_naive.Rule) is pinned to the brute-force DEFINITION of an SMEM on
every short string: the SMEMs, their order, their rows, and both work counters; the C brute force the GPU tests use
(fm_mem_naive.c) agrees with it."""
import ctypes
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_mem_naive as N
import fm_naive
import fm_sampled_naive as M

FUNCTIONS = ["archon_hip_fm_mirror", "archon_hip_fm_mirror_dev", "archon_hip_block_fm_mirror", "archon_hip_fm_read_mirror",
             "archon_hip_fm_smems", "archon_hip_fm_smems_dev", "archon_hip_fm_locate_mems", "archon_hip_block_fm_locate_mems",
             "archon_hip_get_fm_mem_stats"]


def test_mem_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmMemStats", "fm_mem_stats", "FM_MEM"):
        assert hasattr(pyarchon, name), name
    for name in ("mirror", "read_mirror", "smems", "smems_dev", "locate_mems"):
        assert hasattr(pyarchon.FmIndex, name), name
    assert hasattr(pyarchon.Block, "fm_locate_mems")
    import inspect
    assert inspect.signature(pyarchon.Block.fm_index).parameters["mirror"].default is False


def test_fm_mem_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_mem_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmMemStats._fields_]
    assert names == ["n", "patterns", "min_len", "built", "pattern_bytes", "fwd_steps", "bwd_steps", "found", "mems", "occurrences",
                     "lf_steps", "mirror_bytes", "kernel_launches", "host_syncs", "ms_mirror", "ms_count", "ms_emit", "ms_locate"]
    got = _layout(tmp_path, "archon_hip_fm_mem_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmMemStats)
    assert got[1:] == [getattr(pyarchon.FmMemStats, k).offset for k in names]


def test_fm_mem_struct_layout(tmp_path):
    """FM_MEM is archon_hip_fm_mem byte for byte: 24 bytes"""
    import pyarchon
    names = list(pyarchon.FM_MEM.names)
    assert names == ["lo", "hi", "start", "end", "pattern", "reserved0"]
    got = _layout(tmp_path, "archon_hip_fm_mem", names)
    assert got[0] == pyarchon.FM_MEM.itemsize == 24
    assert got[1:] == [pyarchon.FM_MEM.fields[k][1] for k in names]
    assert N.MEM == pyarchon.FM_MEM


def test_mem_bad_arguments():
    """null pointers and decreasing offsets are ARCHON_E_ARG with or without a device: they are refused before the handle is
    used (a stand-in handle is never read)"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    pat = np.zeros(8, np.uint8)
    off, bad_off = np.array([0, 2, 4], np.uint32), np.array([0, 3, 2], np.uint32)
    nm, no = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    mems = np.zeros(4, pyarchon.FM_MEM)
    pos = np.zeros(4, np.uint32)
    total = ctypes.c_uint64(0)
    tp = ctypes.byref(total)
    stand_in = _p(np.zeros(64, np.uint8))
    fn = L.archon_hip_fm_smems
    assert fn(None, _p(pat), _p(off), 2, 1, _p(nm), _p(no), _p(mems), 4, tp) == E
    assert fn(stand_in, None, _p(off), 2, 1, _p(nm), _p(no), _p(mems), 4, tp) == E
    assert fn(stand_in, _p(pat), None, 2, 1, _p(nm), _p(no), _p(mems), 4, tp) == E
    assert fn(stand_in, _p(pat), _p(off), 2, 1, None, _p(no), _p(mems), 4, tp) == E
    assert fn(stand_in, _p(pat), _p(off), 2, 1, _p(nm), None, _p(mems), 4, tp) == E
    assert fn(stand_in, _p(pat), _p(off), 2, 1, _p(nm), _p(no), _p(mems), 4, None) == E
    assert fn(stand_in, _p(pat), _p(bad_off), 2, 1, _p(nm), _p(no), _p(mems), 4, tp) == E
    dv = L.archon_hip_fm_smems_dev
    assert dv(None, _p(pat), _p(off), 2, 1, _p(nm), _p(no), None, 0, tp, None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, 1, _p(nm), _p(no), None, 0, None, None) == E
    assert L.archon_hip_fm_mirror(None) == E
    assert L.archon_hip_fm_mirror_dev(None, _p(pat), None) == E
    assert L.archon_hip_fm_mirror_dev(stand_in, None, None) == E
    assert L.archon_hip_block_fm_mirror(None, stand_in) == E
    assert L.archon_hip_block_fm_mirror(stand_in, None) == E
    assert L.archon_hip_fm_read_mirror(None, _p(pat), 8, ctypes.byref(ctypes.c_uint32(0))) == E
    for fn in (L.archon_hip_fm_locate_mems, L.archon_hip_block_fm_locate_mems):
        assert fn(None, _p(mems), 4, _p(pos), 4, tp) == E
        assert fn(stand_in, None, 4, _p(pos), 4, tp) == E
    assert L.archon_hip_get_fm_mem_stats(0, None) == E
    if pyarchon.device_count() == 0:
        # a thread that ran no SMEM call has no statistics
        assert L.archon_hip_get_fm_mem_stats(0, ctypes.byref(pyarchon.FmMemStats())) == E


def test_mem_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).mirror().smems([b"nanb"])
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_locate_mems(np.zeros(1, pyarchon.FM_MEM))


def test_rule_banana():
    """the worked example of the header"""
    sa, bwt, base = M.a7_forward(b"banana")
    assert (bwt, base, sa) == (b"nnbaaa", 2, [2, 4, 6, 1, 3, 5])
    r = N.Rule(b"banana")
    assert (r.mirror_bwt, r.mirror_base) == (b"bnnaaa", 3)
    assert r.search(b"nanb") == ([(5, 6, 0, 3), (3, 4, 3, 4)], 3, 1, 2)
    assert sa[5] - 3 == 2 and sa[3] - 1 == 0
    assert r.search(b"nanb", 2) == ([(5, 6, 0, 3)], 3, 1, 2)
    assert r.search(b"") == ([], 0, 0, 0)
    assert r.search(b"bananas") == ([(2, 3, 0, 6)], 6, 0, 1)
    assert r.search(b"xbanx") == ([(4, 5, 1, 4)], 3, 0, 1)


def test_rule_against_the_definition():
    """every string of length <= 6 over {0, 1, 255}, every pattern of length <= 4 over {0, 1, 2, 255}, min_len 1 .. 3: the
    procedure's SMEMs are the definition's, in ascending start; their rows are what the search rule gives for the piece; the
    counters are those of the header's closed forms (a step per matched byte after a phase's first, plus the failing one)
    and do not depend on min_len"""
    patterns = [bytes(p) for m in range(0, 5) for p in itertools.product((0, 1, 2, 255), repeat=m)]
    for n in range(1, 7):
        for tt in itertools.product((0, 1, 255), repeat=n):
            x = bytes(tt)
            r = N.Rule(x)
            bwt, base = r.primary.bwt, r.primary.base
            for P in patterns:
                m = len(P)
                want = N.definition(x, P)
                # the counters from the definition's SMEMs alone
                fwd = sum((e - b) if e < m else (e - b - 1) for b, e in want)
                bwd = 0
                for i, (b, e) in enumerate(want):
                    if e == m:
                        continue
                    nb = want[i + 1][0] if i + 1 < len(want) and want[i + 1][0] <= e else None
                    if nb is not None:
                        bwd += (e - nb + 1) if nb > b + 1 else (e - nb)
                for min_len in (1, 2, 3):
                    out, f, bw, found = r.search(P, min_len)
                    assert [(b, e) for _, _, b, e in out] == [(b, e) for b, e in want if e - b >= min_len], (x, P, min_len)
                    assert (f, bw, found) == (fwd, bwd, len(want)), (x, P, min_len)
                    for lo, hi, b, e in out:
                        assert (lo, hi) == fm_naive.backward_search(bwt, base, P[b:e])[:2], (x, P, b, e)
                        assert lo < hi


def test_c_brute_force_agrees_with_rule(tmp_path):
    """fm_mem_naive.c (the GPU tests' reference on large blocks) against the procedure on random short texts"""
    naive = N.build(tmp_path)
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 300))
        sigma = int(rng.choice([2, 4, 256]))
        x = bytes(rng.integers(0, sigma, n, dtype=np.uint8))
        sa, _, _ = M.a7_forward(x)
        r = N.Rule(x)
        pats = []
        for _ in range(6):
            m = int(rng.integers(0, 40))
            q = int(rng.integers(0, n))
            P = bytearray(np.resize(np.frombuffer(x, np.uint8)[q:], m).tobytes()) if m else bytearray()
            for _ in range(int(rng.integers(0, 3)) if m else 0):
                P[int(rng.integers(0, m))] = int(rng.integers(0, sigma + 1)) & 255
            pats.append(bytes(P))
        for min_len in (1, 3):
            mems, nmems, nocc, fwd, bwd, found = naive(np.frombuffer(x, np.uint8), sa, pats, min_len)
            want = [r.search(P, min_len) for P in pats]
            assert (fwd, bwd, found) == (sum(w[1] for w in want), sum(w[2] for w in want), sum(w[3] for w in want)), (x, pats)
            assert [int(c) for c in nmems] == [len(w[0]) for w in want]
            assert [int(c) for c in nocc] == [sum(hi - lo for lo, hi, _, _ in w[0]) for w in want]
            flat = [(lo, hi, b, e, j) for j, w in enumerate(want) for lo, hi, b, e in w[0]]
            assert [tuple(int(v) for v in (q["lo"], q["hi"], q["start"], q["end"], q["pattern"])) for q in mems] == flat, (x, pats)
