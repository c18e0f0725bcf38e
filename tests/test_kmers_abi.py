"""CPU: the k-mer entry points (include/archon_hip.h, archon_hip_kmers*, archon_hip_kmer_occ*, archon_hip_sus*) are declared,
exported and bound; the record and the statistics mirror have the C layout; they refuse bad arguments and, without a GPU, fail
loudly.  And the expected answers of the GPU tests, tests/kmers_naive.py: the header's examples through the helpers, and the
array-based helper pinned to the text-based one."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import kmers_naive as K
import repeats_naive as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["archon_hip_kmers", "archon_hip_kmers_dev", "archon_hip_block_kmers", "archon_hip_kmer_occ", "archon_hip_kmer_occ_dev",
             "archon_hip_block_kmer_occ", "archon_hip_sus", "archon_hip_sus_dev", "archon_hip_block_sus", "archon_hip_get_kmer_stats"]


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
    assert "KMER_TILE" in pyarchon._ROUTE_NAMES
    assert "KMER_TILE" in open(os.path.join(ROOT, "include", "archon_hip_test.h")).read()
    assert "KMER_TILE" in open(os.path.join(ROOT, "README.md")).read()
    for name in ("KMER", "KmerStats", "kmer_stats", "kmers", "kmers_dev", "kmer_occ", "kmer_occ_dev", "sus", "sus_dev", "kmer_bytes"):
        assert hasattr(pyarchon, name), name
    for name in ("kmers", "kmer_occ", "sus", "locate_kmers"):
        assert hasattr(pyarchon.Block, name), name
    assert hasattr(pyarchon.FmIndex, "locate_kmers")


def test_struct_layouts(tmp_path):
    """archon_hip_kmer is 12 bytes in the order of the numpy dtype; the ctypes mirror of archon_hip_kmer_stats has the size and
    the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.KmerStats._fields_]
    fields = ["lo", "hi", "item"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%zu", sizeof(archon_hip_kmer_stats));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_kmer_stats, %s));' % k for k in names)
                   + 'printf(" %zu", sizeof(archon_hip_kmer));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_kmer, %s));' % k for k in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = len(names)
    assert got[0] == ctypes.sizeof(pyarchon.KmerStats)
    assert got[1:1 + k] == [getattr(pyarchon.KmerStats, f).offset for f in names]
    assert got[1 + k] == 12 == pyarchon.KMER.itemsize == K.KMER.itemsize
    assert got[2 + k:] == [pyarchon.KMER.fields[f][1] for f in fields] == [0, 4, 8]
    assert pyarchon.KMER == K.KMER


def _banana():
    return np.array([2, 4, 6, 1, 3, 5], np.uint32), np.array([0, 1, 3, 0, 0, 2], np.uint32)


def test_bad_arguments():
    """null pointers, n = 0, k = 0, 1 bin, 4097 bins, a histogram with 0 bins and bins without a histogram are ARCHON_E_ARG, with
    or without a device, and *total is written 0; so is a tile that is no power of two in [4, 2048]"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp = _banana()
    out = np.zeros(8, pyarchon.KMER)
    hist = np.zeros(4100, np.uint32)
    words = np.zeros(8, np.uint32)
    total = ctypes.c_uint64(7)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    E = pyarchon.E_ARG
    for fn, tail in ((L.archon_hip_kmers, (0,)), (L.archon_hip_kmers_dev, (0, None))):
        assert fn(None, p(lcp), 6, 2, 1, 0, p(out), 8, tp, None, 0, *tail) == E
        assert fn(p(sa), None, 6, 2, 1, 0, p(out), 8, tp, None, 0, *tail) == E
        assert fn(p(sa), p(lcp), 6, 2, 1, 0, p(out), 8, None, None, 0, *tail) == E
        for n, k, hp, bins in ((0, 2, None, 0), (6, 0, None, 0), (6, 2, p(hist), 1), (6, 2, p(hist), 4097), (6, 2, p(hist), 0), (6, 2, None, 5)):
            total.value = 7
            assert fn(p(sa), p(lcp), n, k, 1, 0, p(out), 8, tp, hp, bins, *tail) == E, (n, k, bins)
            assert total.value == 0
    for fn, tail in ((L.archon_hip_kmer_occ, (0,)), (L.archon_hip_kmer_occ_dev, (0, None))):
        assert fn(None, p(lcp), 6, 2, p(words), *tail) == E
        assert fn(p(sa), None, 6, 2, p(words), *tail) == E
        assert fn(p(sa), p(lcp), 6, 2, None, *tail) == E
        assert fn(p(sa), p(lcp), 0, 2, p(words), *tail) == E
        assert fn(p(sa), p(lcp), 6, 0, p(words), *tail) == E
    for fn, tail in ((L.archon_hip_sus, (0,)), (L.archon_hip_sus_dev, (0, None))):
        assert fn(None, p(lcp), 6, p(words), *tail) == E
        assert fn(p(sa), None, 6, p(words), *tail) == E
        assert fn(p(sa), p(lcp), 6, None, *tail) == E
        assert fn(p(sa), p(lcp), 0, p(words), *tail) == E
    assert L.archon_hip_block_kmers(None, 2, 1, 0, p(out), 8, tp, None, 0) == E
    assert L.archon_hip_block_kmer_occ(None, 2, p(words)) == E
    assert L.archon_hip_block_sus(None, p(words)) == E
    assert L.archon_hip_get_kmer_stats(0, None) == E
    assert not out.view(np.uint32).any() and not hist.any() and not words.any()
    for bad in (3, 6, 2, 1, -4, 4096, 3000):
        assert L.archon_hip_test_route(b"KMER_TILE", bad) == E, bad
    for good in (4, 8, 16, 256, 1024, 2048, 0):
        assert L.archon_hip_test_route(b"KMER_TILE", good) == 0, good
    assert L.archon_hip_test_route(b"RESET", 0) == 0


def test_without_a_device():
    """no CPU fallback: without a GPU every entry point of the family is ARCHON_E_NODEVICE (with one, the host forms answer)"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp = _banana()
    out = np.zeros(8, pyarchon.KMER)
    words = np.zeros(8, np.uint32)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    if pyarchon.device_count() > 0:
        assert L.archon_hip_kmers(p(sa), p(lcp), 6, 2, 1, 0, p(out), 8, tp, None, 0, 0) == 0
        assert total.value == 3 and out[:3].tolist() == [(0, 1, 2), (1, 3, 4), (4, 6, 3)]
        assert L.archon_hip_kmer_occ(p(sa), p(lcp), 6, 2, p(words), 0) == 0 and words[:5].tolist() == [1, 2, 2, 2, 2]
        assert L.archon_hip_sus(p(sa), p(lcp), 6, p(words), 0) == 0 and words[:6].tolist() == [1, 2, 3, 4, 3, 4]
        return
    N = pyarchon.E_NODEVICE
    assert L.archon_hip_kmers(p(sa), p(lcp), 6, 2, 1, 0, p(out), 8, tp, None, 0, 0) == N
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_kmers_dev(p(sa), p(lcp), 6, 2, 1, 0, p(out), 8, tp, None, 0, 0, None) == N
    assert L.archon_hip_kmer_occ(p(sa), p(lcp), 6, 2, p(words), 0) == N
    assert L.archon_hip_kmer_occ_dev(p(sa), p(lcp), 6, 2, p(words), 0, None) == N
    assert L.archon_hip_sus(p(sa), p(lcp), 6, p(words), 0) == N
    assert L.archon_hip_sus_dev(p(sa), p(lcp), 6, p(words), 0, None) == N
    h = ctypes.c_void_p(None)
    assert L.archon_hip_block_create(0, ctypes.byref(h)) == N       # so no handle reaches the block forms
    for call in (lambda: pyarchon.kmers(sa, lcp, 2), lambda: pyarchon.kmers(sa, lcp, 2, count_only=True, bins=4),
                 lambda: pyarchon.kmer_occ(sa, lcp, 2), lambda: pyarchon.sus(sa, lcp), pyarchon.kmer_stats):
        with pytest.raises(pyarchon.ArchonError):
            call()
    assert not out.view(np.uint32).any() and not words.any()


KMERS = {1: [(0, 3, 2), (3, 4, 1), (4, 6, 3)], 2: [(0, 1, 2), (1, 3, 4), (4, 6, 3)], 3: [(1, 3, 4), (4, 5, 3), (5, 6, 5)]}
BYTES = {1: [b"a", b"b", b"n"], 2: [b"ba", b"na", b"an"], 3: [b"ana", b"ban", b"nan"]}
OCC = {1: [1, 3, 2, 3, 2, 3], 2: [1, 2, 2, 2, 2], 3: [1, 2, 1, 2]}


@pytest.mark.parametrize("k", [1, 2, 3])
def test_worked_examples(k):
    """the examples of the header, through the text-based helpers, the array helper and pyarchon.kmer_bytes"""
    import pyarchon
    x = b"banana"
    sa, lcp, _, _ = R.a7_arrays(x)
    assert (sa, lcp) == ([2, 4, 6, 1, 3, 5], [0, 1, 3, 0, 0, 2])
    recs, nshort = K.kmers_text(x, k, sa)
    assert recs.tolist() == KMERS[k] and nshort == k - 1
    assert K.kmers_windows(np.frombuffer(x, np.uint8), k, sa)[0].tolist() == KMERS[k]
    by_rule, groups, shorts = K.kmers_arrays(sa, lcp, k)
    assert by_rule.tolist() == KMERS[k] and shorts == k - 1 and groups == len(KMERS[k]) + shorts
    assert [bytes(r) for r in pyarchon.kmer_bytes(x, recs, k)] == BYTES[k]
    assert K.occ_text(x, k).tolist() == K.occ_windows(np.frombuffer(x, np.uint8), k).tolist() == K.occ_arrays(sa, lcp, k).tolist() == OCC[k]
    assert K.sus_text(x).tolist() == K.sus_arrays(sa, lcp).tolist() == [1, 2, 3, 4, 3, 4]
    K.check_sus_sample(x, K.sus_text(x), range(1, 7))
    assert K.hist_of([3, 1, 2], 3).tolist() == [0, 1, 2]


def test_array_helper_is_the_text_helper():
    """the boundary rule in numpy against the text-based helpers on every string of length 1-7 over {0, 1, 255}, every k in
    1 .. n+1: records and order, groups and short rows, occ, sus; the two invariants of the counts; and occ[p] == 1 exactly when
    0 < sus[p+k-1] <= k"""
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            xa = np.frombuffer(x, np.uint8)
            sa, lcp, _, _ = R.a7_arrays(x)
            sus = K.sus_text(x)
            assert K.sus_arrays(sa, lcp).tolist() == sus.tolist(), x
            for k in range(1, n + 2):
                want, nshort = K.kmers_text(x, k, sa)
                got, groups, shorts = K.kmers_arrays(sa, lcp, k)
                assert got.tolist() == want.tolist(), (x, k)
                assert shorts == nshort == min(k - 1, n) and groups == want.size + shorts
                assert K.kmers_windows(xa, k, sa)[0].tolist() == want.tolist()
                occ = K.occ_text(x, k)
                assert K.occ_arrays(sa, lcp, k).tolist() == occ.tolist() == K.occ_windows(xa, k).tolist(), (x, k)
                sizes = want["hi"].astype(np.int64) - want["lo"]
                assert int(sizes.sum()) == max(n - k + 1, 0)
                assert ((occ == 1) == ((sus[k - 1:] > 0) & (sus[k - 1:] <= k))).all(), (x, k)
