"""The expected answers of the approximate FM search tests (TEST INFRASTRUCTURE ONLY): the rule of include/archon_hip.h in
Python over (bwt, primary row), with its hits in order and both work counters; and tests/fm_approx_naive.c, a brute force
over the text compiled with gcc into a directory the test names."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class Rule:
    """R and occ' of a BWT as numpy tables: occ[c, i] = rows j < i with bwt[j] == c, the primary row left out (256 x (n + 1)
    u32: blocks up to about 64 KiB)"""

    def __init__(self, bwt, base):
        b = np.frombuffer(bytes(bwt), np.uint8) if isinstance(bwt, (bytes, bytearray)) else np.ascontiguousarray(bwt, np.uint8)
        self.n = n = b.size
        counts = np.bincount(b, minlength=256).astype(np.int64)
        self.R = np.zeros(257, np.int64)
        np.cumsum(counts, out=self.R[1:])
        keep = np.ones(n, bool)
        keep[base] = False
        self.occ = np.zeros((256, n + 1), np.uint32)
        for c in np.nonzero(counts)[0]:
            np.cumsum((b == c) & keep, out=self.occ[c, 1:])

    def children(self, lo, hi):
        return self.R[:256] + self.occ[:, lo], self.R[:256] + self.occ[:, hi]

    def search(self, P, K):
        """(hits [(lo, hi, d)] in the rule's order, expansions, steps)"""
        P = bytes(P)
        m, n = len(P), self.n
        if m == 0:
            return [(0, n, 0)], 0, 0
        if m > n:
            return [], 0, 0
        hits, work = [], [0, 0]
        R = self.R

        def frame(d, t, lo, hi):
            while True:
                if t == m:
                    hits.append((lo, hi, d))
                    return
                c = P[t]
                if d < K:
                    if t == 0:
                        clo, chi = R[:256], R[1:]
                    else:
                        work[0] += 1
                        clo, chi = self.children(lo, hi)
                    for e in np.nonzero(clo < chi)[0]:
                        if e != c:
                            frame(d + 1, t + 1, int(clo[e]), int(chi[e]))
                    lo, hi = int(clo[c]), int(chi[c])
                elif t == 0:
                    lo, hi = int(R[c]), int(R[c + 1])
                else:
                    work[1] += 1
                    lo, hi = int(R[c] + self.occ[c, lo]), int(R[c] + self.occ[c, hi])
                if lo >= hi:
                    return
                t += 1

        frame(0, 0, 0, n)
        return hits, work[0], work[1]


def build(directory):
    """compile fm_approx_naive.c into `directory`; returns naive(x, P, K) -> (groups, expansions, steps): groups a list of
    (distance, sorted starts), one per distinct string within distance K, in the byte order of the strings"""
    so = os.path.join(str(directory), "libfm_approx_naive.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "fm_approx_naive.c")], check=True)
    lib = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.fma_naive.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp, vp, vp, u64]
    lib.fma_naive.restype = ctypes.c_int64

    def naive(x, P, K):
        x = np.ascontiguousarray(x, np.uint8)
        P = np.frombuffer(bytes(P), np.uint8).copy() if isinstance(P, (bytes, bytearray)) else np.ascontiguousarray(P, np.uint8)
        p = lambda a: vp(a.ctypes.data)      # noqa: E731
        ex, st, nh = u64(0), u64(0), u64(0)
        refs = [ctypes.byref(ex), ctypes.byref(st), ctypes.byref(nh)]
        Pb = np.concatenate([P, np.zeros(1, np.uint8)])
        total = lib.fma_naive(p(x), x.size, p(Pb), P.size, K, *refs, None, None, 0)
        assert total >= 0
        starts, group = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint32)
        assert lib.fma_naive(p(x), x.size, p(Pb), P.size, K, *refs, p(starts), p(group), total) == total
        groups = []
        for i in range(total):
            if i == 0 or group[i] != group[i - 1]:
                w = x[starts[i]:starts[i] + P.size]
                groups.append((int(np.count_nonzero(w != P)), []))
            groups[-1][1].append(int(starts[i]))
        assert len(groups) == nh.value
        return [(d, sorted(s)) for d, s in groups], ex.value, st.value

    return naive
