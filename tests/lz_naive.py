"""The expected answer of the LZ tests (TEST INFRASTRUCTURE ONLY): tests/lz_naive.c -- the longest previous factors from (sa,
lcp, dir) with two stacks, the parse as a plain walk -- compiled with gcc into a directory the test names; and the brute-force
DEFINITIONS in terms of the text to pin it to: the longest common suffix of two prefixes, and the textbook greedy LZ77."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

LPF = np.dtype([("len", "<u4"), ("src", "<u4")])
PHRASE = np.dtype([("end", "<u4"), ("len", "<u4"), ("src", "<u4")])


class Naive:
    def __init__(self, lib):
        self.lib = lib

    def lpf(self, sa, lcp, dir=0):
        """the LPF array of (sa, lcp): record of item s at index s - 1"""
        sa = np.ascontiguousarray(sa, np.uint32)
        lcp = np.ascontiguousarray(lcp, np.uint32)
        assert sa.size == lcp.size and sa.size and sa.min() >= 1 and sa.max() <= sa.size
        out = np.zeros(sa.size, LPF)
        assert self.lib.lpf_naive(sa.ctypes.data, lcp.ctypes.data, sa.size, int(dir), out.ctypes.data) == 0
        return out

    def parse(self, lpf):
        """the phrases of the len words of an LPF array, the one ending at n first"""
        lpf = np.ascontiguousarray(lpf, LPF)
        total = self.lib.parse_naive(lpf.ctypes.data, lpf.size, None, 0)
        out = np.zeros(max(total, 1), PHRASE)
        assert self.lib.parse_naive(lpf.ctypes.data, lpf.size, out.ctypes.data, total) == total
        return out[:total]


def build(directory):
    """compile lz_naive.c into `directory`; returns a Naive"""
    so = os.path.join(str(directory), "liblz_naive.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "lz_naive.c")], check=True)
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.lpf_naive.argtypes = [vp, vp, u32, u32, vp]
    lib.lpf_naive.restype = ctypes.c_int
    lib.parse_naive.argtypes = [vp, u32, vp, ctypes.c_uint64]
    lib.parse_naive.restype = ctypes.c_int64
    return Naive(lib)


def key(x, s):
    """the key of item s in a7 order, INF as 256"""
    return [x[s - 1 - j] for j in range(s)] + [256]


def a7_arrays(x):
    """(sa, lcp) of x by the definition: items sorted by their keys, neighbours compared symbol by symbol"""
    x = bytes(x)
    n = len(x)
    sa = sorted(range(1, n + 1), key=lambda s: key(x, s))
    lcp = [0]
    for i in range(1, n):
        a, b = key(x, sa[i - 1]), key(x, sa[i])
        m = 0
        while a[m] == b[m] and a[m] != 256:
            m += 1
        lcp.append(m)
    return sa, lcp


def common_suffix(x, s, t):
    """the largest l with x[s-l .. s) == x[t-l .. t)"""
    m = 0
    while m < min(s, t) and x[s - 1 - m] == x[t - 1 - m]:
        m += 1
    return m


def lpf_by_text(x, dir):
    """len of every item by the text alone: the maximum of common_suffix over the admissible items"""
    n = len(x)
    return [max([common_suffix(x, s, t) for t in (range(1, s) if dir == 0 else range(s + 1, n + 1))], default=0) for s in range(1, n + 1)]


def lz77_by_text(z):
    """the textbook greedy LZ77 of z, left to right: (pos, len) with len = the longest match of z[pos:] that starts before pos
    (overlap allowed), 0 for a literal"""
    z = bytes(z)
    n, i, out = len(z), 0, []
    while i < n:
        best = 0
        for j in range(i):
            m = 0
            while i + m < n and z[j + m] == z[i + m]:
                m += 1
            best = max(best, m)
        out.append((i, best))
        i += max(best, 1)
    return out
