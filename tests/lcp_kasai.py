"""The expected answer of the LCP tests: tests/lcp_kasai.c, compiled with gcc into a directory the test names
(TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def build(directory):
    """compile lcp_kasai.c into `directory`; returns kasai(x, sa) -> uint32[n]"""
    so = os.path.join(str(directory), "liblcp_kasai.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "lcp_kasai.c")], check=True)
    L = ctypes.CDLL(so)
    L.lcp_kasai.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.lcp_kasai.restype = ctypes.c_int

    def kasai(x, sa):
        x = np.ascontiguousarray(x, dtype=np.uint8)
        sa = np.ascontiguousarray(sa, dtype=np.uint32)
        out = np.empty(x.size, np.uint32)
        assert L.lcp_kasai(ctypes.c_void_p(x.ctypes.data), x.size, ctypes.c_void_p(sa.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == 0
        return out

    return kasai


def irreducible_rows(x, sa):
    """rows whose value archon_hip_lcp finds by comparing key bytes: row 0, rows whose item or whose upper neighbour's
    item is n, and rows where bwt[i] != bwt[i-1] (bwt[i] = x[sa[i]])"""
    n = x.size
    sa = np.asarray(sa, np.int64)
    c = x[np.minimum(sa, n - 1)].astype(np.int64)
    irr = np.ones(n, bool)
    irr[1:] = (sa[1:] == n) | (sa[:-1] == n) | (c[1:] != c[:-1])
    return irr
