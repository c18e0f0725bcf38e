"""The expected answer of the repeats tests (TEST INFRASTRUCTURE ONLY): tests/repeats_naive.c, the one-pass stack
enumeration of LCP intervals, compiled with gcc into a directory the test names; and the brute-force DEFINITION in terms of
the text -- occurrence lists, preceding and following byte sets, containment among maximal repeats -- to pin it to."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

REPEAT = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("len", "<u4"), ("row", "<u4")])


def build(directory):
    """compile repeats_naive.c into `directory`; returns naive(lcp, bwt, base, kind, min_len, min_occ, count_only) ->
    (repeats as a REPEAT array in representative-row order, or their number; intervals; occurrences; longest)"""
    so = os.path.join(str(directory), "librepeats_naive.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "repeats_naive.c")], check=True)
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.repeats_naive.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, ctypes.c_uint64, vp]
    lib.repeats_naive.restype = ctypes.c_int64

    def naive(lcp, bwt, base, kind=1, min_len=1, min_occ=2, count_only=False):
        lcp = np.ascontiguousarray(lcp, np.uint32)
        bwt = np.ascontiguousarray(bwt, np.uint8)
        counters = np.zeros(3, np.uint64)
        p = lambda a: vp(a.ctypes.data)      # noqa: E731
        args = (p(lcp), p(bwt), bwt.size, int(base), int(kind), int(min_len), int(min_occ))
        total = lib.repeats_naive(*args, None, 0, p(counters))
        assert total >= 0
        stats = tuple(int(c) for c in counters)
        if count_only:
            return (total,) + stats
        out = np.zeros(max(total, 1), REPEAT)
        assert lib.repeats_naive(*args, p(out), total, p(counters)) == total
        return (out[:total],) + stats

    return naive


def key(x, s):
    """the key of item s in a7 order, INF as 256"""
    return [x[s - 1 - j] for j in range(s)] + [256]


def a7_arrays(x):
    """(sa, lcp, bwt, base) of x by the definition: items sorted by their keys, neighbours compared symbol by symbol"""
    x = bytes(x)
    n = len(x)
    sa = sorted(range(1, n + 1), key=lambda s: key(x, s))
    lcp = [0]
    for i in range(1, n):
        a, b = key(x, sa[i - 1]), key(x, sa[i])
        L = 0
        while a[L] == b[L] and a[L] != 256:
            L += 1
        lcp.append(L)
    bwt = bytes(x[s] if s < n else x[0] for s in sa)
    return sa, lcp, bwt, sa.index(n)


def definition(x, kind, min_len=1, min_occ=2):
    """the repeats of x by the text alone: {string u: sorted starts} of every u that occurs at least twice (min_occ times),
    whose occurrences are not all preceded by the same byte (the start of the text differs from every byte), for kind >= 1
    not all followed by the same byte (the end of the text differs from every byte), and for kind 2 is a substring of no other
    maximal repeat"""
    x = bytes(x)
    n = len(x)
    occ = {}
    for p in range(n):
        for m in range(1, n - p + 1):
            occ.setdefault(x[p:p + m], []).append(p)
    left_open = {u: ps for u, ps in occ.items() if len(ps) >= 2 and len({x[p - 1] if p else -1 for p in ps}) >= 2}
    if kind == 0:
        picked = left_open
    else:
        maximal = {u: ps for u, ps in left_open.items() if len({x[p + len(u)] if p + len(u) < n else -1 for p in ps}) >= 2}
        picked = maximal if kind == 1 else {u: ps for u, ps in maximal.items() if not any(u != w and u in w for w in maximal)}
    return {u: ps for u, ps in picked.items() if len(u) >= max(min_len, 1) and len(ps) >= max(min_occ, 2)}, len(occ)


def rows_of(x, sa, lcp, u, starts):
    """(lo, hi, len, row) of the string u with the given starts: its rows are those of the items where an occurrence ends; they
    must be adjacent; row is the first one inside that holds len"""
    m = len(u)
    rows = sorted(sa.index(p + m) for p in starts)
    lo, hi = rows[0], rows[-1] + 1
    assert rows == list(range(lo, hi)), (x, u)
    row = next(k for k in range(lo + 1, hi) if lcp[k] == m)
    assert all(lcp[k] >= m for k in range(lo + 1, hi))
    return lo, hi, m, row
