"""The suffix-prefix overlaps of include/archon_hip.h (archon_hip_fm_overlaps) twice over.

The MODEL works on rows, as the device does: the walk of a query over the suffix array's BWT gives the rows [lo, hi) of each of
its prefixes, the end rows of the documents (the rows r with sa[r] = ends[d]) inside a range are the overlaps of that length.  It
gives the records in the header's order, novl, and every counter that follows from the data alone: steps, tested, hit, overlaps
and longest.

The DEFINITION works on the text alone: document d overlaps Q by l when l <= ends[d] and x[ends[d]-l : ends[d]] == Q[:l].
test_fm_ovl_abi.py pins the first to the second."""
import bisect
import functools

import numpy as np

FM_OVL = np.dtype([("query", "<u4"), ("doc", "<u4"), ("len", "<u4"), ("row", "<u4")])


def end_bytes(n, D):
    """bytes of the attachment: ends | erow | edoc padded to 256 bytes together, then one bit-vector level over the rows"""
    B = (n + 255) // 256
    r256 = lambda v: (v + 255) // 256 * 256        # noqa: E731
    return r256(12 * D) + r256(4 * (9 * B + 1))


class Walker:
    """the search rule over (x, sa): R, occ' (the primary row left out) and the walk of a pattern's prefixes.  Built once per
    block; the tables hold one row of n + 1 counts per distinct byte of x"""

    def __init__(self, x, sa):
        x = np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)
        sa = np.asarray(sa, np.int64)
        n = x.size
        assert sa.size == n and n >= 1
        self.n = n
        self.sa = sa
        self.isa = np.zeros(n + 1, np.int64)            # isa[item] = its row
        self.isa[sa] = np.arange(n)
        counts = np.bincount(x, minlength=256)
        self.R = np.concatenate([[0], np.cumsum(counts)]).tolist()
        # bwt[r] = x[sa[r]]; the primary row (sa[r] = n) holds no byte that counts
        inner = sa < n
        bwt = np.where(inner, x[np.minimum(sa, n - 1)], 0)
        self.occ = {}
        for c in np.flatnonzero(counts).tolist():
            t = np.zeros(n + 1, np.int32)
            np.cumsum((bwt == c) & inner, out=t[1:])
            self.occ[c] = t

    def walk(self, pattern):
        """([(lo, hi) of the prefix of 1, 2, ... bytes while it holds rows], rank steps): the pattern's first n bytes, P[0] first;
        a step is every byte after the first that is consumed, the one that empties the range included"""
        P = bytes(pattern)[:self.n]
        ranges, steps = [], 0
        lo = hi = 0
        for i, c in enumerate(P):
            if i == 0:
                lo, hi = self.R[c], self.R[c + 1]
            else:
                steps += 1
                t = self.occ.get(c)
                lo, hi = (self.R[c] + int(t[lo]), self.R[c] + int(t[hi])) if t is not None else (0, 0)
            if lo >= hi:
                break
            ranges.append((lo, hi))
        return ranges, steps


def end_rows(walker, ends):
    """(erow ascending, edoc): the end rows of the documents and the document of each"""
    ends = np.asarray(ends, np.int64)
    assert ends.size >= 1 and ends[0] >= 1 and ends[-1] <= walker.n and (np.diff(ends) > 0).all()
    rows = walker.isa[ends]
    order = np.argsort(rows, kind="stable")
    return rows[order].tolist(), order.tolist()


def model(walker, ends, patterns, min_len, walks=None):
    """(records, novl, counters) of the queries: records an FM_OVL array query by query, by ascending len and by ascending row;
    novl[j] the overlaps of query j; counters steps, tested, hit, overlaps, longest.  walks: walker.walk of every pattern, when
    the caller has them already (they do not depend on the ends)"""
    assert min_len >= 1
    erow, edoc = end_rows(walker, ends)
    rec = []
    novl = np.zeros(len(patterns), np.uint32)
    ctr = {"steps": 0, "tested": 0, "hit": 0, "overlaps": 0, "longest": 0}
    for j, P in enumerate(patterns):
        ranges, steps = walks[j] if walks is not None else walker.walk(P)
        ctr["steps"] += steps
        mine = 0
        for l in range(min_len, len(ranges) + 1):
            lo, hi = ranges[l - 1]
            ctr["tested"] += 1
            a, b = bisect.bisect_left(erow, lo), bisect.bisect_left(erow, hi)
            if b > a:
                ctr["hit"] += 1
                ctr["longest"] = max(ctr["longest"], l)
                mine += b - a
                rec += [(j, edoc[i], l, erow[i]) for i in range(a, b)]
        novl[j] = mine
        ctr["overlaps"] += mine
    return np.array(rec, FM_OVL) if rec else np.zeros(0, FM_OVL), novl, ctr


@functools.lru_cache(maxsize=None)
def items_ending_with(x, piece):
    """the items e in len(piece) .. n with x[e - len(piece) : e] == piece, from the text alone"""
    l = len(piece)
    return frozenset(e for e in range(l, len(x) + 1) if x[e - l:e] == piece)


def definition(x, ends, patterns, min_len):
    """the set of (query, doc, len): document d overlaps Q by l, min_len <= l <= min(m, n), when l <= ends[d] and
    x[ends[d] - l : ends[d]] == Q[:l]"""
    x = bytes(x)
    got = set()
    for j, Q in enumerate(patterns):
        Q = bytes(Q)
        for l in range(min_len, min(len(Q), len(x)) + 1):
            at = items_ending_with(x, Q[:l])
            got.update((j, d, l) for d, e in enumerate(ends) if e in at)
    return got


def text_counters(x, patterns, min_len):
    """steps and tested from the text alone: with L the longest prefix of the query's first n bytes that occurs in x, the walk
    takes L steps when it stops early and m' - 1 when the whole m' = min(m, n) bytes occur, none when L = 0; it tests the lengths
    min_len .. L"""
    x = bytes(x)
    steps = tested = 0
    for Q in patterns:
        Q = bytes(Q)[:len(x)]
        L = 0
        while L < len(Q) and Q[:L + 1] in x:
            L += 1
        steps += 0 if L == 0 else (L if L < len(Q) else len(Q) - 1)
        tested += max(0, L - min_len + 1)
    return steps, tested


def best_loop(records):
    """best_overlaps by a plain loop: the longest record of every (query, doc) pair, in the records' order"""
    last = {}
    for i, r in enumerate(records):
        key = (int(r["query"]), int(r["doc"]))
        if key not in last or int(r["len"]) >= int(records[last[key]]["len"]):
            last[key] = i
    return records[sorted(last.values())]
