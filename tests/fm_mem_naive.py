"""The SMEM procedure of include/archon_hip.h in pure Python (TEST INFRASTRUCTURE ONLY) over two naive indexes -- the a7
transform of x and of x reversed (fm_sampled_naive.a7_forward) -- the brute-force DEFINITION to pin it to, and
tests/fm_mem_naive.c, the brute force of the GPU tests, compiled with gcc into a directory the test names."""
import ctypes
import os
import subprocess

import numpy as np

import fm_naive
import fm_sampled_naive as M

HERE = os.path.dirname(os.path.abspath(__file__))


class Index:
    """the count rule over (bwt, primary row): the bucket of a byte, and one rank step"""

    def __init__(self, bwt, base):
        self.bwt, self.base, self.n = bytes(bwt), base, len(bwt)
        self.R = [0] * 257
        for c in self.bwt:
            self.R[c + 1] += 1
        for c in range(256):
            self.R[c + 1] += self.R[c]

    def bucket(self, c):
        return self.R[c], self.R[c + 1]

    def occ(self, c, i):
        return sum(1 for j in range(i) if self.bwt[j] == c and j != self.base)

    def step(self, c, lo, hi):
        return self.R[c] + self.occ(c, lo), self.R[c] + self.occ(c, hi)


class Rule:
    """search(P, min_len) -> ([(lo, hi, start, end)], fwd_steps, bwd_steps, found): the procedure of the header, literally"""

    def __init__(self, x):
        x = bytes(x)
        _, bwt, base = M.a7_forward(x)
        _, mbwt, mbase = M.a7_forward(x[::-1])
        self.primary, self.mirror = Index(bwt, base), Index(mbwt, mbase)
        self.mirror_bwt, self.mirror_base = mbwt, mbase

    @staticmethod
    def _run(ix, symbols):
        """the count rule over `symbols` until the range is empty or they end: (bytes matched, lo, hi, steps taken)"""
        lo, hi = ix.bucket(symbols[0])
        if lo >= hi:
            return 0, lo, hi, 0
        matched = 1
        steps = 0
        for c in symbols[1:]:
            steps += 1
            nlo, nhi = ix.step(c, lo, hi)
            if nlo >= nhi:
                break
            lo, hi = nlo, nhi
            matched += 1
        return matched, lo, hi, steps

    def search(self, P, min_len=1):
        P = bytes(P)
        m = len(P)
        out, fwd, bwd, found = [], 0, 0, 0
        b = 0
        while b < m:
            l, lo, hi, steps = self._run(self.primary, P[b:])
            if l == 0:
                b += 1
                continue
            assert steps == (l if b + l < m else l - 1)
            fwd += steps
            e = b + l
            found += 1
            if e - b >= min_len:
                out.append((lo, hi, b, e))
            if e == m:
                break
            g, _, _, steps = self._run(self.mirror, P[e:b:-1])      # P[e], P[e-1], ..., P[b+1]
            if g == 0:
                b = e + 1
                continue
            nb = e - g + 1
            assert steps == (g if nb > b + 1 else g - 1)
            bwd += steps
            b = nb
        return out, fwd, bwd, found


def definition(x, P):
    """the SMEMs of P in x by the definition: the occurring pieces (b, e) of P that no other occurring piece contains,
    ascending in b"""
    x, P = bytes(x), bytes(P)
    m = len(P)
    occurs = {(b, e) for b in range(m) for e in range(b + 1, m + 1) if P[b:e] in x}
    return sorted((b, e) for b, e in occurs
                  if (b == 0 or (b - 1, e) not in occurs) and (e == m or (b, e + 1) not in occurs))


MEM = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("start", "<u4"), ("end", "<u4"), ("pattern", "<u4"), ("reserved0", "<u4")])


def build(directory):
    """compile fm_mem_naive.c into `directory`; returns naive(x, sa, patterns, min_len) -> (mems, nmems, nocc, fwd, bwd, found):
    sa the a7 suffix array of x (the oracle's); mems a MEM array in the procedure's order"""
    so = os.path.join(str(directory), "libfm_mem_naive.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "fm_mem_naive.c")], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.fm_mem_naive.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp]
    lib.fm_mem_naive.restype = ctypes.c_int64

    def naive(x, sa, patterns, min_len=1):
        x = np.ascontiguousarray(x, np.uint8)
        sa = np.ascontiguousarray(sa, np.uint32)
        packed, off = fm_naive.pack(patterns)
        k = off.size - 1
        nmems, nocc = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        counters = np.zeros(3, np.uint64)
        p = lambda a: vp(a.ctypes.data)      # noqa: E731
        cap = int(off[-1]) + 1
        mems = np.zeros(cap, MEM)
        total = lib.fm_mem_naive(p(x), x.size, p(sa), p(packed), p(off), k, int(min_len), p(nmems), p(nocc), p(mems), cap, p(counters))
        assert 0 <= total <= cap
        return mems[:total], nmems, nocc, int(counters[0]), int(counters[1]), int(counters[2])

    return naive
