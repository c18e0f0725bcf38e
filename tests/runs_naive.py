"""The expected answer of the runs tests (TEST INFRASTRUCTURE ONLY): the runs of a block by the DEFINITION (runs_text, brute
force), by the RULE of include/archon_hip.h with its counters (runs_rule, over repeats_naive.a7_arrays and a plain lce), an
independent vectorised finder of the runs of short period (runs_short), and a numpy LCE over a sparse table for blocks too
long for the plain one."""
import itertools

import numpy as np

import repeats_naive

RUN = np.dtype([("start", "<u4"), ("end", "<u4"), ("period", "<u4"), ("root", "<u4")])


def tiny_strings():
    """every string of length 1-10 over {0, 1} and of length 1-7 over {0, 1, 255}: what the rule is pinned to the definition on"""
    for alpha, top in (((0, 1), 10), ((0, 1, 255), 7)):
        for n in range(1, top + 1):
            for tup in itertools.product(alpha, repeat=n):
                yield bytes(tup)


def smallest_period(w):
    """the smallest p >= 1 with w[i] == w[i + p] for every i"""
    for p in range(1, len(w) + 1):
        if w[p:] == w[:len(w) - p]:
            return p
    return 0


def is_run(x, start, end, p):
    """the definition, by slices: x[start:end] has smallest period p, at least two copies, and extends neither way"""
    x = bytes(x)
    n = len(x)
    if not (0 <= start < end <= n and p >= 1 and end - start >= 2 * p):
        return False
    if smallest_period(x[start:end]) != p:
        return False
    if start > 0 and x[start - 1] == x[start - 1 + p]:
        return False
    if end < n and x[end] == x[end - p]:
        return False
    return True


def is_run_fast(x, start, end, p):
    """is_run for long runs, by whole-slice comparisons: the period by one, the smallest period by one per prime factor of p (a
    run of period p and length >= 2p has a smaller period only if its root is a power, so a period p / r with r prime)"""
    n = len(x)
    if not (0 <= start < end <= n and p >= 1 and end - start >= 2 * p):
        return False
    if x[start:end - p] != x[start + p:end]:
        return False
    if start > 0 and x[start - 1] == x[start - 1 + p]:
        return False
    if end < n and x[end] == x[end - p]:
        return False
    m, r = p, 2
    while m > 1:
        if r * r > m:
            r = m
        if m % r == 0:
            q = p // r
            if x[start:start + p - q] == x[start + q:start + p]:
                return False
            while m % r == 0:
                m //= r
        r += 1
    return True


def runs_text(x):
    """the set of (start, end, period) of x by the definition: every p, every maximal stretch of x[i] == x[i + p] of length
    >= p, kept when p is the smallest period of the stretch it spans"""
    x = bytes(x)
    n = len(x)
    out = set()
    for p in range(1, n // 2 + 1):
        i = 0
        while i + p < n:
            if x[i] != x[i + p]:
                i += 1
                continue
            j = i
            while j + p < n and x[j] == x[j + p]:
                j += 1
            if j - i >= p and smallest_period(x[i:j + p]) == p:
                out.add((i, j + p, p))
            i = j + 1
    return out


def passes(rec, min_period=0, max_period=0, min_copies=2, min_len=0):
    """the copies and length filters of the rule's step 6 (the period filter acts in step 1)"""
    start, end, p = rec[0], rec[1], rec[2]
    return end - start >= min_copies * p and end - start >= min_len


def plain_lce(x):
    """lce(s, t) of the header by comparing bytes"""
    x = bytes(x)

    def lce(s, t):
        if s == t:
            return s
        k = 0
        while k < s and k < t and x[s - 1 - k] == x[t - 1 - k]:
            k += 1
        return k
    return lce


def ranks(x):
    """(rank0, rank1): the row of every item 1..n in the a7 suffix array of x and of its complement (index 0 unused)"""
    x = bytes(x)
    n = len(x)
    out = []
    for y in (x, bytes(255 - c for c in x)):
        sa = repeats_naive.a7_arrays(y)[0]
        r = [0] * (n + 1)
        for row, s in enumerate(sa):
            r[s] = row
        out.append(r)
    return out


def runs_rule(x, min_period=0, max_period=0, min_copies=2, min_len=0, lce=None, rank=None):
    """the rule of include/archon_hip.h: (records (start, end, period, root) in output order, counters) with counters a dict
    of candidates, roots, lce_queries, runs, emitted, longest_period.  lce and rank: given for long blocks (sparse_lce,
    ranks_fast), else by the definition"""
    x = bytes(x)
    n = len(x)
    lce = lce or plain_lce(x)
    rank = rank or ranks(x)
    c = dict(candidates=0, roots=0, lce_queries=0, runs=0, emitted=0, longest_period=0)
    out = []
    # the nearest earlier item of greater rank, for every item and both orders, by a stack
    prev = []
    for r in rank:
        pv = [0] * (n + 1)
        st = []
        for s in range(1, n + 1):
            while st and r[st[-1]] < r[s]:
                st.pop()
            pv[s] = st[-1] if st else 0
            st.append(s)
        prev.append(pv)
    rank0 = rank[0]
    for s in range(1, n + 1):
        for l in (0, 1):
            t = prev[l][s]
            if not t:
                continue
            p = s - t
            if p < min_period or (max_period and p > max_period):
                continue
            c["candidates"] += 1
            c["lce_queries"] += 1
            R = lce(s, t)
            if R == 0:
                continue
            if s + p <= n:
                c["lce_queries"] += 1
                if lce(s + p, s) >= p:
                    continue
            c["roots"] += 1
            lo, hi = 0, min(p - 1, n - s)
            while lo < hi:
                m = (lo + hi + 1) >> 1
                c["lce_queries"] += 1
                if lce(s + m, t + m) >= m:
                    lo = m
                else:
                    hi = m - 1
            L = lo
            if R + L < p:
                continue
            start, end = t - R, s + L
            if start == 0:
                keep = l == 0
            elif l == 0:
                keep = rank0[start] > rank0[start + p]
            else:
                keep = rank0[start] < rank0[start + p]
            if not keep:
                continue
            c["runs"] += 1
            if not passes((start, end, p), min_period, max_period, min_copies, min_len):
                continue
            c["emitted"] += 1
            c["longest_period"] = max(c["longest_period"], p)
            out.append((start, end, p, s))
    return out, c


# ---- long blocks: the arrays by numpy, the lce by a sparse table
def a7_fast(x):
    """(sa, lcp) of x as uint32 arrays by prefix doubling over the reversed text (n up to about 2^17): the same arrays as
    repeats_naive.a7_arrays"""
    x = np.frombuffer(bytes(x), np.uint8)
    n = x.size
    # item s = key x[s-1], x[s-2], ..., x[0], INF: the suffix of z = reversed x at n - s, the end GREATEST
    z = x[::-1].astype(np.int64)
    rank = z.copy()
    k = 1
    idx = np.arange(n)
    while True:
        nxt = np.full(n, 1 << 40, np.int64)         # past the end: INF, the greatest
        nxt[:n - k] = rank[k:] if k < n else nxt[:0]
        order = np.lexsort((nxt, rank))
        r2, n2 = rank[order], nxt[order]
        new = np.zeros(n, np.int64)
        new[1:] = np.cumsum((r2[1:] != r2[:-1]) | (n2[1:] != n2[:-1]))
        rank = np.empty(n, np.int64)
        rank[order] = new
        if new[-1] == n - 1 or k >= n:
            break
        k *= 2
    sa_z = np.empty(n, np.int64)
    sa_z[rank] = idx
    sa = (n - sa_z).astype(np.uint32)               # suffix of z at j is item n - j
    # lcp by Kasai over z
    lcp = np.zeros(n, np.uint32)
    zb = z
    h = 0
    rk = rank
    for j in range(n):
        r = rk[j]
        if r == 0:
            h = 0
            continue
        i = sa_z[r - 1]
        while j + h < n and i + h < n and zb[j + h] == zb[i + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return sa, lcp


def ranks_fast(x):
    """ranks() by a7_fast, as lists"""
    x = bytes(x)
    n = len(x)
    out = []
    for y in (x, bytes(255 - c for c in x)):
        sa = a7_fast(y)[0]
        r = np.zeros(n + 1, np.int64)
        r[sa] = np.arange(n)
        out.append(r.tolist())
    return out


class SparseLce:
    """lce(s, t) of the header from sa and lcp: range minima over a sparse table (n up to about 70 000: n log n words)"""

    def __init__(self, sa, lcp):
        sa = np.asarray(sa, np.int64)
        n = sa.size
        self.n = n
        self.isa = np.zeros(n + 1, np.int64)
        self.isa[sa] = np.arange(n)
        lv = np.asarray(lcp, np.int64).copy()
        lv[0] = 0
        self.tab = [lv]
        j = 1
        while 2 * j <= n:
            prev = self.tab[-1]
            self.tab.append(np.minimum(prev[:prev.size - j], prev[j:]))
            j *= 2

    def many(self, s, t):
        """the lce of every pair of the arrays s, t (items in 0..n)"""
        s = np.asarray(s, np.int64)
        t = np.asarray(t, np.int64)
        a, b = self.isa[s], self.isa[t]
        lo, hi = np.minimum(a, b) + 1, np.maximum(a, b)         # rows lo .. hi inclusive
        out = np.zeros(s.size, np.int64)
        ok = (s != t) & (s > 0) & (t > 0)
        span = np.where(ok, hi - lo + 1, 1)
        k = np.floor(np.log2(span)).astype(np.int64)
        for lev in np.unique(k[ok]) if ok.any() else []:
            m = ok & (k == lev)
            tab = self.tab[lev]
            out[m] = np.minimum(tab[lo[m]], tab[hi[m] - (1 << lev) + 1])
        out[s == t] = s[s == t]
        return out

    def scalar(self):
        """lce(s, t) for one pair at a time over plain lists: what runs_rule asks a few hundred thousand times"""
        isa, tab = self.isa.tolist(), [t.tolist() for t in self.tab]

        def lce(s, t):
            if s == t:
                return s
            if not s or not t:
                return 0
            a, b = isa[s], isa[t]
            lo, hi = (a + 1, b) if a < b else (b + 1, a)
            k = (hi - lo + 1).bit_length() - 1
            u, v = tab[k][lo], tab[k][hi - (1 << k) + 1]
            return u if u < v else v
        return lce

    def __call__(self, s, t):
        return int(self.many([s], [t])[0])


def runs_short(x, P):
    """the set of (start, end, period) of the runs of x with period <= P, independently of the rule: for every p the maximal
    stretches of x[:-p] == x[p:] of length >= p (numpy), then the primitivity check by slices"""
    x = bytes(x)
    n = len(x)
    a = np.frombuffer(x, np.uint8)
    out = set()
    for p in range(1, min(P, n // 2) + 1):
        eq = np.concatenate(([0], (a[:-p] == a[p:]).astype(np.int8), [0]))
        d = np.diff(eq)
        begins, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
        long_enough = ends - begins >= p
        for i, j in zip(begins[long_enough].tolist(), ends[long_enough].tolist()):
            w = x[i:i + p]
            # the stretch has period p; p is its smallest exactly when the root is primitive (no proper divisor period)
            if any(p % q == 0 and w == w[:q] * (p // q) for q in range(1, p // 2 + 1)):
                continue
            out.add((i, j + p, p))
    return out


def fibonacci(k):
    """the Fibonacci string of length F(k), F(1) = F(2) = 1, k >= 2: a, ab, aba, abaab, ... (each term the previous one followed
    by the one before it)"""
    a, b = b"b", b"a"
    for _ in range(k - 2):
        a, b = b, b + a
    return b
