"""The matching statistics of a long text in chunks, in pure Python (TEST INFRASTRUCTURE ONLY): the walk, the sweep and the fix
of include/archon_hip.h (archon_hip_fm_ms_text) with the join rule, literally, over the procedure of fm_ms_naive.Rule and the
arrays of repeats_naive.a7_arrays; the counters that follow from the block, the text and the chunk alone; and the chain of the
relative LZ parse."""
import numpy as np

import fm_ms_naive


def chunks_of(m, C):
    return (m + C - 1) // C


def counters(walk_len, C):
    """saturated, full_chunks, runs and longest_run from the lengths of the walk's records alone (walk_len[e - 1] of end e).
    A record is saturated when its len is e - s_c; a chunk is full when its last record is; chunk c >= 2 depends on chunk c - 1
    when that one is full, and a run is a maximal row of dependent chunks: its joins are the sweep's chain"""
    m = len(walk_len)
    k = chunks_of(m, C)
    if isinstance(walk_len, np.ndarray):        # (long texts: the same two lines on arrays)
        e = np.arange(1, m + 1, dtype=np.int64)
        sat = walk_len.astype(np.int64) == e - ((e - 1) // C) * C
        saturated = int(sat[C:].sum())
    else:
        sat = [l == e - ((e - 1) // C) * C for e, l in enumerate(walk_len, 1)]
        saturated = sum(sat[C:])
    full = [bool(sat[min(m, (c + 1) * C) - 1]) for c in range(k)]
    runs, longest, cur = 0, 0, 0
    for c in range(2, k):
        if full[c - 1]:
            cur += 1
            if cur == 1:
                runs += 1
            longest = max(longest, cur)
        else:
            cur = 0
    return {"chunks": k, "saturated": saturated, "full_chunks": sum(full), "runs": runs, "longest_run": longest}


def walk_len_of(exact_len, C):
    """the lengths the walk leaves, from the exact ones: min(ms(e), e - s_c)"""
    if isinstance(exact_len, np.ndarray):
        e = np.arange(1, exact_len.size + 1, dtype=np.int64)
        return np.minimum(exact_len.astype(np.int64), e - ((e - 1) // C) * C)
    return [min(l, e - ((e - 1) // C) * C) for e, l in enumerate(exact_len, 1)]


class Model:
    """run(P, C) -> ([(len, lo, hi)] one per byte of P, counters): walk, sweep and fix; joins counts the joins of both"""

    def __init__(self, x):
        self.rule = fm_ms_naive.Rule(x)
        self.n = self.rule.n
        self.sa = self.rule.sa
        self.isa = [self.n] * (self.n + 1)
        for r, s in enumerate(self.sa):
            self.isa[s] = r
        self.joins = 0
        self._chunks = {}           # the walk's records of a chunk, by its bytes

    def _lcp(self, i):
        return self.rule.lcp[i] if 0 < i < self.n else 0

    def _q(self, r, y):
        s = self.sa[r]
        return self.n if s <= y else self.isa[s - y]

    def _first(self, lo, hi, y, t):
        """the first r in [lo, hi) with q(r) >= t, or hi: a binary search (q is strictly increasing there)"""
        while lo < hi:
            mid = (lo + hi) // 2
            if self._q(mid, y) >= t:
                hi = mid
            else:
                lo = mid + 1
        return lo

    def join(self, state, y, lo, hi):
        """the exact record at e from the exact state (L, lo_s, hi_s) at s and the rows [lo, hi) of Y = P[s .. e), |Y| = y"""
        self.joins += 1
        L, lo_s, hi_s = state
        if L == 0:
            return (y, lo, hi)
        a, b = self._first(lo, hi, y, lo_s), self._first(lo, hi, y, hi_s)
        if a < b:
            return (y + L, a, b)
        lp = min(self._lcp(i) for i in range(self._q(a - 1, y) + 1, lo_s + 1)) if a > lo else 0
        ls = min(self._lcp(i) for i in range(hi_s, self._q(a, y) + 1)) if a < hi else 0
        l = max(lp, ls)
        if l == 0:
            return (y, lo, hi)
        u = max(p for p in range(lo_s + 1) if self._lcp(p) < l)
        v = min([p for p in range(hi_s, self.n) if self._lcp(p) < l] + [self.n])
        return (y + l, self._first(lo, hi, y, u), self._first(lo, hi, y, v))

    def walk(self, P, C):
        P = bytes(P)
        out = []
        for s in range(0, len(P), C):
            piece = P[s:s + C]
            if piece not in self._chunks:
                self._chunks[piece] = self.rule.search(piece)[0]
            out += self._chunks[piece]
        return out

    def run(self, P, C):
        P = bytes(P)
        m = len(P)
        rec = self.walk(P, C)
        k = chunks_of(m, C)
        sat = [rec[e - 1][0] == e - ((e - 1) // C) * C for e in range(1, m + 1)]
        # sweep: start[c], the exact record at end s_c = c C
        start = [None] * k
        for c in range(1, k):
            last = rec[c * C - 1]
            if c == 1 or not sat[c * C - 1]:
                start[c] = last
            else:
                start[c] = self.join(start[c - 1], C, last[1], last[2])
        # fix
        out = list(rec)
        for e in range(C + 1, m + 1):
            if sat[e - 1]:
                c = (e - 1) // C
                out[e - 1] = self.join(start[c], e - c * C, rec[e - 1][1], rec[e - 1][2])
        return out, counters([r[0] for r in rec], C)


def rlz_records(records, sa):
    """(len, src) of every end from its record: src = sa[lo], or 0 when len is 0"""
    return [(l, sa[lo] if l else 0) for l, lo, _ in records]


def chain(lpf):
    """the parse of include/archon_hip.h over (len, src) records: [(end, len, src)] from e = m down"""
    out, e = [], len(lpf)
    while e > 0:
        l, s = lpf[e - 1]
        out.append((e, l, s))
        e -= min(max(1, l), e)
    return out
