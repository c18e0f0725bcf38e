"""The expected answers of the FM index tests (TEST INFRASTRUCTURE ONLY): tests/fm_naive.c, compiled with gcc into a
directory the test names, and the search rule of include/archon_hip.h in pure Python over (bwt, primary row)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def pack(patterns):
    """a list of bytes / uint8 arrays -> (packed uint8, uint32 offsets[k + 1])"""
    parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p, np.uint8).ravel() for p in patterns]
    off = np.zeros(len(parts) + 1, np.uint32)
    np.cumsum([q.size for q in parts], out=off[1:])
    return np.concatenate(parts + [np.zeros(1, np.uint8)]), off


def expected_steps(m, n, L):
    """rank steps of one pattern of length m whose longest occurring prefix has length L: none for m > n or L = 0, L when
    the search stops early (L < m), m - 1 for a pattern that occurs"""
    if m == 0 or m > n or L == 0:
        return 0
    return L if L < m else m - 1


def build(directory):
    """compile fm_naive.c into `directory`; returns naive(x, patterns, starts=False) -> (count, L[, list of start arrays])"""
    so = os.path.join(str(directory), "libfm_naive.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "fm_naive.c")], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.fm_naive.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64]
    lib.fm_naive.restype = ctypes.c_int64

    def naive(x, patterns, starts=False):
        x = np.ascontiguousarray(x, np.uint8)
        packed, off = pack(patterns)
        k = off.size - 1
        count, L = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        p = lambda a: vp(a.ctypes.data)      # noqa: E731
        total = lib.fm_naive(p(x), x.size, p(packed), p(off), k, p(count), p(L), None, 0)
        assert total >= 0
        if not starts:
            return count, L
        out = np.zeros(max(total, 1), np.uint32)
        assert lib.fm_naive(p(x), x.size, p(packed), p(off), k, p(count), p(L), p(out), total) == total
        cuts = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
        return count, L, [out[cuts[j]:cuts[j + 1]] for j in range(k)]

    return naive


def backward_search(bwt, base, pattern):
    """the rule of include/archon_hip.h, literally: (lo, hi, rank steps).  P[0] first; R counted over the whole BWT; occ'
    leaves the primary row out"""
    bwt = bytes(bwt)
    n, m = len(bwt), len(pattern)
    if m == 0:
        return 0, n, 0
    if m > n:
        return 0, 0, 0
    R = [0] * 257
    for c in bwt:
        R[c + 1] += 1
    for c in range(256):
        R[c + 1] += R[c]

    def occ(c, i):
        return sum(1 for j in range(i) if bwt[j] == c and j != base)

    lo, hi, steps = R[pattern[0]], R[pattern[0] + 1], 0
    for c in pattern[1:]:
        if lo >= hi:
            break
        steps += 1
        lo, hi = R[c] + occ(c, lo), R[c] + occ(c, hi)
    return lo, hi, steps
