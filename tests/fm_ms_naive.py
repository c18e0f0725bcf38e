"""The matching-statistics procedure of include/archon_hip.h in pure Python (TEST INFRASTRUCTURE ONLY) over the naive index
of fm_mem_naive (the bucket of a byte and one rank step) and the arrays of repeats_naive.a7_arrays (sa, lcp, bwt and primary
row by the definition); the DEFINITION from the text alone to pin it to; and tests/fm_ms_naive.c, the brute force of the GPU
tests, compiled with gcc into a directory the test names."""
import ctypes
import os
import subprocess

import numpy as np

import fm_mem_naive
import fm_naive
import repeats_naive

HERE = os.path.dirname(os.path.abspath(__file__))


class Rule:
    """search(P) -> ([(len, lo, hi)] one per byte of P, steps, parents): the procedure of the header, literally.  lcp: another
    array to run it over (any n words: the procedure ends whatever they hold)"""

    def __init__(self, x, lcp=None):
        x = bytes(x)
        self.sa, true_lcp, bwt, base = repeats_naive.a7_arrays(x)
        self.n = len(x)
        self.lcp = list(true_lcp if lcp is None else lcp)
        self.index = fm_mem_naive.Index(bwt, base)

    def _lcp(self, i):
        return self.lcp[i] if 0 < i < self.n else 0        # lcp[0] is read as 0 and lcp[n] as 0

    def search(self, P):
        P = bytes(P)
        n, ix = self.n, self.index
        lo, hi, l = 0, n, 0
        out, steps, parents = [], 0, 0
        for c in P:
            while True:
                if l == 0:
                    a, b = ix.bucket(c)
                    lo, hi, l = (a, b, 1) if a < b else (0, n, 0)
                    break
                steps += 1
                a, b = ix.step(c, lo, hi)
                if a < b:
                    lo, hi, l = a, b, l + 1
                    break
                parents += 1
                lp = min(max(self._lcp(lo), self._lcp(hi)), l - 1)
                if lp == 0:
                    lo, hi, l = 0, n, 0
                else:
                    lo = max(p for p in range(lo + 1) if self._lcp(p) < lp)
                    hi = min([q for q in range(hi, n) if self._lcp(q) < lp] + [n])
                    l = lp
            out.append((l, lo, hi))
        return out, steps, parents


def definition(x, P):
    """the records of P in x from the text alone: for every end e the largest l <= e with P[e-l .. e) in x, and the rows of
    that piece -- the places, among the items sorted by their keys, of the items where an occurrence ends -- or (0, 0, n)"""
    x, P = bytes(x), bytes(P)
    n = len(x)
    order = sorted(range(1, n + 1), key=lambda s: repeats_naive.key(x, s))
    out = []
    for e in range(1, len(P) + 1):
        l = next((l for l in range(e, 0, -1) if P[e - l:e] in x), 0)
        if l == 0:
            out.append((0, 0, n))
            continue
        rows = [r for r, s in enumerate(order) if s >= l and x[s - l:s] == P[e - l:e]]
        assert rows == list(range(rows[0], rows[-1] + 1))
        out.append((l, rows[0], rows[-1] + 1))
    return out


def smems(records, min_len=1):
    """[(lo, hi, start, end)] that follow from one pattern's records: P[e-len .. e) is an SMEM exactly when len > 0 and (e == m
    or len(e+1) <= len(e))"""
    m = len(records)
    return [(lo, hi, e - l, e) for e, (l, lo, hi) in enumerate(records, 1)
            if l > 0 and (e == m or records[e][0] <= l) and l >= min_len]


def build(directory):
    """compile fm_ms_naive.c into `directory`; returns naive(x, sa, lcp, patterns) -> (len, lo, hi, offsets, steps, parents,
    matched, longest): sa the a7 suffix array of x (the oracle's), lcp its LCP array (Kasai's)"""
    so = os.path.join(str(directory), "libfm_ms_naive.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "fm_ms_naive.c")], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.fm_ms_naive.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp]
    lib.fm_ms_naive.restype = ctypes.c_int

    def naive(x, sa, lcp, patterns):
        x = np.ascontiguousarray(x, np.uint8)
        sa = np.ascontiguousarray(sa, np.uint32)
        lcp = np.ascontiguousarray(lcp, np.uint32)
        assert sa.size == x.size == lcp.size
        packed, off = fm_naive.pack(patterns)
        k = off.size - 1
        total = int(off[-1])
        length, lo, hi = (np.zeros(total + 1, np.uint32) for _ in range(3))
        counters = np.zeros(4, np.uint64)
        p = lambda a: vp(a.ctypes.data)      # noqa: E731
        rc = lib.fm_ms_naive(p(x), x.size, p(sa), p(lcp), p(packed), p(off), k, p(length), p(lo), p(hi), p(counters))
        assert rc == 0, "the procedure's walk disagrees with the definition"
        return (length[:total], lo[:total], hi[:total], off) + tuple(int(c) for c in counters)

    return naive
