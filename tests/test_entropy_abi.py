"""CPU: the entropy and complexity entry points (include/archon_hip.h, archon_hip_entropy*, archon_hip_complexity*) are declared,
exported and bound; the two records and the statistics mirror have the C layout; they refuse bad arguments with the records
zeroed and, without a GPU, fail loudly; the getter refuses as its siblings do.  And the expected answers of the GPU tests,
tests/entropy_naive.py: the header's examples, and the row rules pinned to the definitions by the text on every string of length
1 to 7 over {0, 1, 255}."""
import ctypes
import itertools
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import entropy_naive as E
import kmers_naive as K
import repeats_naive as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["archon_hip_entropy", "archon_hip_entropy_dev", "archon_hip_block_entropy", "archon_hip_complexity", "archon_hip_complexity_dev",
             "archon_hip_block_complexity", "archon_hip_entropy_last_stats"]
STATS = ["n", "nk", "what", "tile", "direct_rows", "built", "kernel_launches", "host_syncs", "groups_direct", "groups_table", "groups_in_wave",
         "ms_lcp", "ms_build", "ms_count"]
ENTROPY = ["k", "reserved", "contexts", "deterministic", "pairs", "symbols", "bits"]
COMPLEXITY = ["n", "max_len", "lcp_max", "delta_len", "delta_count", "delta_exact", "longest_run", "reserved", "lcp_sum", "substrings", "runs"]
BANANA_BITS = 8.754887502163468
ABRA_BITS = 22.44410733057346


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(archon_[a-z0-9_]+)\s*\(", src))


def test_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
    for name in ("ENTROPY", "EntropyStats", "Complexity", "entropy", "entropy_dev", "complexity", "complexity_dev", "entropy_stats"):
        assert hasattr(pyarchon, name), name
    assert hasattr(pyarchon.Block, "entropy") and hasattr(pyarchon.Block, "complexity")
    assert [k for k, _ in pyarchon.EntropyStats._fields_] == STATS
    assert [k for k, _ in pyarchon.Complexity._fields_] == COMPLEXITY
    assert list(pyarchon.ENTROPY.names) == ENTROPY and pyarchon.ENTROPY == E.ENTROPY


def test_struct_layouts(tmp_path):
    """struct archon_hip_entropy is 48 bytes in the order of the numpy dtype; the ctypes mirrors of struct archon_hip_complexity
    and archon_hip_entropy_stats have the sizes and the field offsets the C header gives them"""
    import pyarchon
    parts = (("struct archon_hip_entropy", ENTROPY), ("struct archon_hip_complexity", COMPLEXITY), ("archon_hip_entropy_stats", STATS))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){'
                   + "".join('printf("%%zu ", sizeof(%s));' % t + "".join('printf("%%zu ", offsetof(%s, %s));' % (t, f) for f in fields)
                             for t, fields in parts) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    a, b = 1 + len(ENTROPY), 2 + len(ENTROPY) + len(COMPLEXITY)
    assert got[0] == 48 == pyarchon.ENTROPY.itemsize
    assert got[1:a] == [pyarchon.ENTROPY.fields[f][1] for f in ENTROPY] == [0, 4, 8, 16, 24, 32, 40]
    assert got[a] == 56 == ctypes.sizeof(pyarchon.Complexity)
    assert got[a + 1:b] == [getattr(pyarchon.Complexity, f).offset for f in COMPLEXITY]
    assert got[b] == ctypes.sizeof(pyarchon.EntropyStats)
    assert got[b + 1:] == [getattr(pyarchon.EntropyStats, f).offset for f in STATS]


def _banana():
    return (np.array([2, 4, 6, 1, 3, 5], np.uint32), np.array([0, 1, 3, 0, 0, 2], np.uint32), np.frombuffer(b"nnbaaa", np.uint8).copy(), 2)


def test_bad_arguments():
    """null pointers, n = 0, nk outside 1..64 and base_id >= n are ARCHON_E_ARG, with or without a device, and the records are
    zeroed; counts stays untouched"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp, bwt, base = _banana()
    ks = np.array([0, 1, 2], np.uint32)
    out = np.zeros(66, pyarchon.ENTROPY)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    A = pyarchon.E_ARG

    def dirty():
        out.view(np.uint8)[:] = 0xA5

    for fn, tail in ((L.archon_hip_entropy, (0,)), (L.archon_hip_entropy_dev, (0, None))):
        for a, b, c, n, bid, kp, nk in ((None, p(lcp), p(bwt), 6, base, p(ks), 3), (p(sa), None, p(bwt), 6, base, p(ks), 3), (p(sa), p(lcp), None, 6, base, p(ks), 3),
                                        (p(sa), p(lcp), p(bwt), 0, 0, p(ks), 3), (p(sa), p(lcp), p(bwt), 6, 6, p(ks), 3), (p(sa), p(lcp), p(bwt), 6, 7, p(ks), 3),
                                        (p(sa), p(lcp), p(bwt), 6, base, None, 3), (p(sa), p(lcp), p(bwt), 6, base, p(ks), 0),
                                        (p(sa), p(lcp), p(bwt), 6, base, p(ks), 65)):
            dirty()
            assert fn(a, b, c, n, bid, kp, nk, p(out), *tail) == A, (n, bid, nk)
            zeroed = min(nk, 64)
            assert not out[:zeroed].view(np.uint8).any() and (out[zeroed:].view(np.uint8) == 0xA5).all()
        assert fn(p(sa), p(lcp), p(bwt), 6, base, p(ks), 3, None, *tail) == A
    dirty()
    assert L.archon_hip_block_entropy(None, p(ks), 3, p(out)) == A and not out[:3].view(np.uint8).any()
    assert L.archon_hip_block_entropy(None, p(ks), 3, None) == A
    counts = np.full(8, 7, np.uint32)
    for fn, tail in ((L.archon_hip_complexity, (0,)), (L.archon_hip_complexity_dev, (0, None))):
        for a, n in ((None, 6), (p(lcp), 0)):
            rec = pyarchon.Complexity(n=9, runs=9, lcp_sum=9)
            assert fn(a, p(bwt), n, 0, p(counts), ctypes.byref(rec), *tail) == A
            assert not any(rec.asdict().values())
        assert fn(p(lcp), p(bwt), 6, 0, p(counts), None, *tail) == A
    rec = pyarchon.Complexity(n=9, runs=9)
    assert L.archon_hip_block_complexity(None, 0, p(counts), ctypes.byref(rec)) == A and not any(rec.asdict().values())
    assert L.archon_hip_block_complexity(None, 0, p(counts), None) == A
    assert (counts == 7).all()


def test_getter_refusals():
    """a null out is "null pointer"; a thread that has run no such call is told so, with the device's number"""
    import pyarchon
    L = pyarchon.lib()
    got = {}

    def ask():
        st = pyarchon.EntropyStats()
        got["null"] = (L.archon_hip_entropy_last_stats(0, None), L.archon_hip_last_error())
        got["none"] = (L.archon_hip_entropy_last_stats(3, ctypes.byref(st)), L.archon_hip_last_error())

    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got["null"] == (pyarchon.E_ARG, b"null pointer")
    assert got["none"] == (pyarchon.E_ARG, b"the calling thread has run no entropy call on device 3")


def test_without_a_device():
    """no CPU fallback: without a GPU a good call is ARCHON_E_NODEVICE (with one, the host forms answer the header's example)"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp, bwt, base = _banana()
    ks = np.array([0, 1, 2, 3], np.uint32)
    out = np.zeros(4, pyarchon.ENTROPY)
    rec = pyarchon.Complexity()
    counts = np.zeros(6, np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    if pyarchon.device_count() > 0:
        assert L.archon_hip_entropy(p(sa), p(lcp), p(bwt), 6, base, p(ks), 4, p(out), 0) == 0
        assert [tuple(r)[2:6] for r in out.tolist()] == [(1, 0, 3, 6), (3, 3, 3, 5), (3, 3, 3, 4), (3, 3, 3, 3)]
        assert abs(out["bits"][0] - BANANA_BITS) <= 2.0 ** -48 * 6 + 2.0 ** -52 * 3 * BANANA_BITS and not out["bits"][1:].any()
        assert L.archon_hip_complexity(p(lcp), p(bwt), 6, 6, p(counts), ctypes.byref(rec), 0) == 0
        assert counts.tolist() == [3, 3, 3, 3, 2, 1] and (rec.substrings, rec.runs, rec.longest_run, rec.delta_len, rec.delta_count) == (15, 3, 3, 1, 3)
        return
    N = pyarchon.E_NODEVICE
    assert L.archon_hip_entropy(p(sa), p(lcp), p(bwt), 6, base, p(ks), 4, p(out), 0) == N
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_entropy_dev(p(sa), p(lcp), p(bwt), 6, base, p(ks), 4, p(out), 0, None) == N
    assert L.archon_hip_complexity(p(lcp), p(bwt), 6, 0, p(counts), ctypes.byref(rec), 0) == N
    assert L.archon_hip_complexity_dev(p(lcp), p(bwt), 6, 0, p(counts), ctypes.byref(rec), 0, None) == N
    for call in (lambda: pyarchon.entropy(sa, lcp, bwt, base, [0, 1]), lambda: pyarchon.complexity(lcp, bwt), lambda: pyarchon.complexity(lcp),
                 pyarchon.entropy_stats):
        with pytest.raises(pyarchon.ArchonError):
            call()
    assert not out.view(np.uint8).any() and not counts.any() and not any(rec.asdict().values())


def _all_helpers(x, k):
    """the record of order k through the text, the windows and the rows: the integers equal, the bits within a few ulp"""
    sa, lcp, bwt, base = R.a7_arrays(x)
    a, b, (c, _) = E.order_text(x, k), E.order_windows(np.frombuffer(x, np.uint8), k), E.order_rows(sa, lcp, bwt, base, k)
    assert a[:4] == b[:4] == c[:4], (x, k)
    assert abs(a[4] - b[4]) <= 1e-12 * max(a[4], 1) and abs(a[4] - c[4]) <= 1e-12 * max(a[4], 1), (x, k)
    return a


def test_worked_examples():
    """the header's examples through all helpers"""
    x = b"banana"
    sa, lcp, bwt, base = R.a7_arrays(x)
    assert (bwt, base) == (b"nnbaaa", 2)
    assert _all_helpers(x, 0) == (1, 0, 3, 6, BANANA_BITS)
    for k in (1, 2, 3):
        assert _all_helpers(x, k) == (3, 3, 3, 6 - k, 0.0)
    assert E.distinct_text(x) == [3, 3, 3, 3, 2, 1]
    rec, counts = E.complexity_rows(lcp, bwt, 6)
    assert counts.tolist() == [3, 3, 3, 3, 2, 1]
    assert rec == dict(n=6, max_len=6, lcp_max=3, delta_len=1, delta_count=3, delta_exact=1, longest_run=3, lcp_sum=6, substrings=15, runs=3)

    x = b"abracadabra"
    sa, lcp, bwt, base = R.a7_arrays(x)
    assert _all_helpers(x, 0) == (1, 0, 5, 11, ABRA_BITS)
    assert _all_helpers(x, 1) == (5, 4, 7, 10, 6.0)
    assert _all_helpers(x, 2) == (7, 7, 7, 9, 0.0)
    assert E.distinct_text(x) == [5, 7, 7, 7, 7, 6, 5, 4, 3, 2, 1]
    rec, counts = E.complexity_rows(lcp, bwt, 11)
    assert counts.tolist() == E.distinct_text(x)
    assert rec == dict(n=11, max_len=11, lcp_max=4, delta_len=1, delta_count=5, delta_exact=1, longest_run=4, lcp_sum=12, substrings=54, runs=7)
    # without a bwt no runs; a shorter max_len is exact here because d_1 / 1 already beats (n - max_len) / (max_len + 1)
    rec, counts = E.complexity_rows(lcp, None, 3)
    assert counts.tolist() == [5, 7, 7] and (rec["runs"], rec["longest_run"], rec["max_len"], rec["delta_exact"]) == (0, 0, 3, 1)
    assert E.complexity_rows(lcp, bwt, 0)[0]["max_len"] == 11 == E.complexity_rows(lcp, bwt, 99)[0]["max_len"]


def test_rules_are_the_definitions():
    """every string of length 1-7 over {0, 1, 255}: the row rules against the text rules for every k in 0 .. n+1 and every l;
    pairs(k) is the number of distinct (k+1)-mers, bits never grows with k, and the group model covers every k-mer group once"""
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            sa, lcp, bwt, base = R.a7_arrays(x)
            last = None
            for k in range(0, n + 2):
                want = E.order_text(x, k)
                for tile in (4, E.DEFAULT_TILE):
                    got, groups = E.order_rows(sa, lcp, bwt, base, k, tile)
                    assert got[:4] == want[:4] and abs(got[4] - want[4]) <= 1e-12 * max(want[4], 1), (x, k)
                    if k >= 1:
                        assert sum(groups) == len(K.counts(x, k)) and groups[1] == 0, (x, k)
                assert want[2] == len(K.counts(x, k + 1)), (x, k)
                assert want[3] == max(n - k, 0) and want[1] <= want[0] <= want[2]
                assert last is None or want[4] <= last + 1e-12, (x, k)
                last = want[4]
            d = E.distinct_text(x)
            for L in range(1, n + 1):
                rec, counts = E.complexity_rows(lcp, bwt, L)
                assert counts.tolist() == d[:L], (x, L)
                assert (rec["delta_len"], rec["delta_count"]) == E.delta_of(d[:L])
                assert rec["delta_exact"] == 0 or E.delta_of(d) == E.delta_of(d[:L]), (x, L)
            rec, _ = E.complexity_rows(lcp, bwt, n)
            assert rec["substrings"] == sum(d) == len({x[p:q] for p in range(n) for q in range(p + 1, n + 1)})
            assert (rec["runs"], rec["longest_run"]) == E.runs_of(bwt) and rec["delta_exact"] == 1
            assert rec["runs"] == 1 + sum(bwt[i] != bwt[i - 1] for i in range(1, n))
