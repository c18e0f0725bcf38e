"""CPU: the approximate FM search entry points (include/archon_hip.h, archon_hip_fm_approx, _fm_approx_dev,
_block_fm_approx, _fm_locate_hits, _block_fm_locate_hits, _get_fm_approx_stats) are declared, exported and bound; the hit
and statistics mirrors have the C layout; bad arguments are refused and, without a GPU, the calls fail loudly.  And the rule
of the header (fm_approx_naive.Rule) is pinned to brute force on every short string: hit sets, starts, distances, the order
and both work counters; the C brute force the GPU tests use (fm_approx_naive.c) agrees with it."""
import ctypes
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_approx_naive as A
import fm_sampled_naive as M

FUNCTIONS = ["archon_hip_fm_approx", "archon_hip_fm_approx_dev", "archon_hip_block_fm_approx", "archon_hip_fm_locate_hits",
             "archon_hip_block_fm_locate_hits", "archon_hip_get_fm_approx_stats"]


def test_approx_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmApproxStats", "fm_approx_stats", "FM_HIT"):
        assert hasattr(pyarchon, name), name
    for name in ("approx", "approx_dev", "locate_hits"):
        assert hasattr(pyarchon.FmIndex, name), name
    for name in ("fm_approx", "fm_locate_hits"):
        assert hasattr(pyarchon.Block, name), name


def test_fm_approx_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_approx_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmApproxStats._fields_]
    got = _layout(tmp_path, "archon_hip_fm_approx_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmApproxStats)
    assert got[1:] == [getattr(pyarchon.FmApproxStats, k).offset for k in names]


def test_fm_hit_struct_layout(tmp_path):
    """FM_HIT is archon_hip_fm_hit byte for byte"""
    import pyarchon
    names = list(pyarchon.FM_HIT.names)
    assert names == ["lo", "hi", "mismatches", "pattern"]
    got = _layout(tmp_path, "archon_hip_fm_hit", names)
    assert got[0] == pyarchon.FM_HIT.itemsize
    assert got[1:] == [pyarchon.FM_HIT.fields[k][1] for k in names]


def test_approx_bad_arguments():
    """null pointers, K > 4 and decreasing offsets are ARCHON_E_ARG with or without a device: they are refused before the
    handle is used (a stand-in handle is never read)"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    pat = np.zeros(8, np.uint8)
    off, bad_off = np.array([0, 2, 4], np.uint32), np.array([0, 3, 2], np.uint32)
    nh, no = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    hits = np.zeros(4, pyarchon.FM_HIT)
    pos = np.zeros(4, np.uint32)
    total = ctypes.c_uint64(0)
    tp = ctypes.byref(total)
    stand_in = _p(np.zeros(64, np.uint8))
    for fn in (L.archon_hip_fm_approx, L.archon_hip_block_fm_approx):
        assert fn(None, _p(pat), _p(off), 2, 1, _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, None, _p(off), 2, 1, _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), None, 2, 1, _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, 1, None, _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, 1, _p(nh), None, _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, 1, _p(nh), _p(no), _p(hits), 4, None) == E
        assert fn(stand_in, _p(pat), _p(off), 2, 5, _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, 99, _p(nh), _p(no), None, 0, tp) == E
        assert fn(stand_in, _p(pat), _p(bad_off), 2, 1, _p(nh), _p(no), _p(hits), 4, tp) == E
    dv = L.archon_hip_fm_approx_dev
    assert dv(None, _p(pat), _p(off), 2, 1, _p(nh), _p(no), None, 0, tp, None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, 5, _p(nh), _p(no), None, 0, tp, None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, 1, _p(nh), _p(no), None, 0, None, None) == E
    for fn in (L.archon_hip_fm_locate_hits, L.archon_hip_block_fm_locate_hits):
        assert fn(None, _p(off), 2, _p(hits), 4, _p(pos), 4, tp) == E
    assert L.archon_hip_get_fm_approx_stats(0, None) == E
    if pyarchon.device_count() == 0:
        # a thread that ran no approximate call has no statistics
        assert L.archon_hip_get_fm_approx_stats(0, ctypes.byref(pyarchon.FmApproxStats())) == E


def test_approx_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).approx([b"an"], 1)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_approx([b"an"], 1)


def test_rule_banana():
    """the worked example of the header"""
    sa, bwt, base = M.a7_forward(b"banana")
    assert (bwt, base) == (b"nnbaaa", 2)
    r = A.Rule(bwt, base)
    assert r.search(b"bn", 1) == ([(4, 6, 1), (0, 1, 1)], 1, 2)
    assert r.search(b"an", 1)[0] == [(4, 6, 0)]
    assert [sa[q] - 2 for q in range(4, 6)] == [1, 3] and sa[0] - 2 == 0
    assert r.search(b"", 3) == ([(0, 6, 0)], 0, 0)
    assert r.search(b"bananas", 2) == ([], 0, 0)


def _order_key(w, P):
    """the rule's order: the mismatch list (p, w[p]) ascending, a list that ends after every longer list that starts with it"""
    return [(p, w[p]) for p in range(len(P)) if w[p] != P[p]] + [(len(P) + 1, 0)]


def _brute(x, P, K):
    """{w: (d, sorted starts)} and the two counters of the closed forms"""
    n, m = len(x), len(P)
    hits = {}
    for q in range(n - m + 1):
        w = x[q:q + m]
        d = sum(a != b for a, b in zip(w, P))
        if d <= K:
            hits.setdefault(w, (d, []))[1].append(q)
    ex = st = 0
    for t in range(1, m):
        for u in {x[q:q + t] for q in range(n - t + 1)}:
            d = sum(a != b for a, b in zip(u, P))
            ex += d < K
            st += d == K
    return hits, ex, st


def test_rule_against_brute_force():
    """every string of length <= 6 over {0, 1, 255}, every pattern of length <= 3 over {0, 1, 2, 255}, K = 0 .. 3: the hits
    are the distinct strings within distance K with their starts and distances, in the rule's order, with disjoint ranges;
    the counters equal the closed forms"""
    patterns = [bytes(p) for m in range(1, 4) for p in itertools.product((0, 1, 2, 255), repeat=m)]
    for n in range(1, 7):
        for tt in itertools.product((0, 1, 255), repeat=n):
            x = bytes(tt)
            sa, bwt, base = M.a7_forward(x)
            r = A.Rule(bwt, base)
            for P in patterns:
                m = len(P)
                for K in range(4):
                    hits, ex, st = r.search(P, K)
                    want, wex, wst = _brute(x, P, K)
                    if m > n:
                        assert (hits, ex, st) == ([], 0, 0)
                        continue
                    assert (ex, st) == (wex, wst), (x, P, K)
                    got = {}
                    for lo, hi, d in hits:
                        starts = sorted(sa[q] - m for q in range(lo, hi))
                        got[x[starts[0]:starts[0] + m]] = (d, starts)
                    assert len(got) == len(hits)
                    assert got == want, (x, P, K)
                    keys = [_order_key(x[sa[lo] - m:sa[lo]], P) for lo, _, _ in hits]
                    assert keys == sorted(keys), (x, P, K)
                    rows = sorted((lo, hi) for lo, hi, _ in hits)
                    assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:]))


def test_c_brute_force_agrees_with_rule(tmp_path):
    """fm_approx_naive.c (the GPU tests' reference on large blocks) against the rule on random short texts"""
    naive = A.build(tmp_path)
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 300))
        sigma = int(rng.choice([2, 4, 256]))
        x = bytes(rng.integers(0, sigma, n, dtype=np.uint8))
        sa, bwt, base = M.a7_forward(x)
        r = A.Rule(bwt, base)
        for _ in range(6):
            m = int(rng.integers(1, 9))
            q = int(rng.integers(0, max(n - m, 0) + 1))
            P = bytearray(x[q:q + m].ljust(m, b"\0"))
            for _ in range(int(rng.integers(0, 3))):
                P[int(rng.integers(0, m))] = int(rng.integers(0, sigma))
            for K in range(3):
                hits, ex, st = r.search(bytes(P), K)
                groups, nex, nst = naive(np.frombuffer(x, np.uint8), bytes(P), K)
                assert (nex, nst) == (ex, st), (x, bytes(P), K)
                got = sorted((d, sorted(sa[q] - m for q in range(lo, hi))) for lo, hi, d in hits)
                assert got == sorted(groups), (x, bytes(P), K)
