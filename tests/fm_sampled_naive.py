"""The sampled FM index rule of include/archon_hip.h in pure Python (TEST INFRASTRUCTURE ONLY): LF with the primary row's
special case, ISA / SA samples, locate by LF walks to a sampled row, extract by LF walks from the ISA samples, and the a7
suffix array by brute force to pin them to."""
import numpy as np

import fm_naive


def a7_forward(x):
    """(sa, bwt, base) of x by sorting the keys: item s is x[s-1], ..., x[0], INF"""
    x = bytes(x)
    n = len(x)
    sa = sorted(range(1, n + 1), key=lambda s: tuple(reversed(x[:s])) + (256,))
    bwt = bytes(x[s] if s < n else x[0] for s in sa)
    return sa, bwt, sa.index(n)


class Model:
    def __init__(self, bwt, base, rate):
        self.bwt, self.base, self.rate = bytes(bwt), base, rate
        n = self.n = len(self.bwt)
        self.R = [0] * 257
        for c in self.bwt:
            self.R[c + 1] += 1
        for c in range(256):
            self.R[c + 1] += self.R[c]
        # LF of every row, by the rule: R[c] + occ'(c, r), the primary row to the end of its bucket
        seen = [0] * 256
        self.lf = [0] * n
        for r, c in enumerate(self.bwt):
            if r == base:
                self.lf[r] = self.R[c + 1] - 1
            else:
                self.lf[r] = self.R[c] + seen[c]
                seen[c] += 1
        # ISA samples: the row of item kS, item 0 the primary row, item p + 1 = LF(row of item p)
        ns = (n + rate - 1) // rate
        self.isa = []
        r = base
        for p in range(n):
            if p % rate == 0:
                self.isa.append(r)
            r = self.lf[r]
        assert len(self.isa) == ns
        sampled = sorted((row, k * rate if k else n) for k, row in enumerate(self.isa))
        self.marked = set(row for row, _ in sampled)
        self.sa_s = [v for _, v in sampled]
        self.slot = {row: i for i, (row, _) in enumerate(sampled)}

    def sa_of(self, r):
        """(sa[r], LF steps) by walking to a sampled row"""
        t = 0
        while r not in self.marked:
            r = self.lf[r]
            t += 1
        return self.sa_s[self.slot[r]] - t, t

    def locate(self, pattern):
        """(starts in row order, LF steps of each) of one pattern"""
        lo, hi, _ = fm_naive.backward_search(self.bwt, self.base, pattern)
        out, steps = [], []
        for r in range(lo, hi):
            s, t = self.sa_of(r)
            out.append(s - len(pattern))
            steps.append(t)
        return out, steps

    def segments(self, a, length):
        """(k, u, v) of the request x[a .. a + length): its range cut at the multiples of S"""
        S, out, u = self.rate, [], a
        while u < a + length:
            k = u // S
            v = min(a + length, (k + 1) * S)
            out.append((k, u, v))
            u = v
        return out

    def extract(self, a, length):
        """(bytes, LF steps) of x[a .. a + length)"""
        out, steps = bytearray(), 0
        for k, u, v in self.segments(a, length):
            r = self.isa[k]
            for _ in range(k * self.rate, u):
                r = self.lf[r]
                steps += 1
            for p in range(u, v):
                out.append(self.bwt[r])
                if p + 1 < v:
                    r = self.lf[r]
                    steps += 1
        return bytes(out), steps


def expected_isa(sa, base, rate):
    """the ISA samples from a suffix array: the row of item kS, base for k = 0"""
    sa = np.asarray(sa, np.int64)
    n = sa.size
    isa = np.zeros((n + rate - 1) // rate, np.uint32)
    rows = np.nonzero((sa % rate == 0) & (sa < n))[0]
    isa[sa[rows] // rate] = rows
    isa[0] = base
    return isa


def locate_steps(sa, rows, rate):
    """the exact LF steps of locating the rows: the least t >= 0 with (s + t) mod S == 0 or s + t == n, s = sa[r]"""
    sa = np.asarray(sa, np.int64)
    n = sa.size
    s = sa[np.asarray(rows, np.int64)]
    return np.minimum((-s) % rate, n - s)


def extract_steps(starts, lengths, rate):
    """the exact LF steps of extracting the requests: per segment [u, v) inside [kS, (k+1)S), v - kS - 1; over the segments
    k0 .. k1 of a request [a, e) that is (k1 - k0)(S - 1) + e - k1 S - 1"""
    total = 0
    for a, L in zip(starts, lengths):
        a, L = int(a), int(L)
        if L:
            e = a + L
            k0, k1 = a // rate, (e - 1) // rate
            total += (k1 - k0) * (rate - 1) + e - k1 * rate - 1
    return total
