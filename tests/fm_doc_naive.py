"""The document listing of include/archon_hip.h in numpy: the model of the listing over a suffix array (rows, their documents, the
records of a row range and the counters that follow from the ranges and the tile alone), and the DEFINITION from the text alone
(which documents hold the last byte of an occurrence, and how often).  test_fm_doc_abi.py pins the first to the second."""
import bisect

import numpy as np

FM_DOC = np.dtype([("doc", "<u4"), ("tf", "<u4"), ("row", "<u4"), ("range", "<u4")])
DEFAULT_TILE = 4096


def boundary_sets(n):
    """every bounds[0 .. D] of a block of n bytes: 0 and n with every subset of 1 .. n - 1 between them"""
    for mask in range(1 << (n - 1)):
        yield [0] + [c for c in range(1, n) if mask >> (c - 1) & 1] + [n]


def doc_of_items(bounds, items):
    """the d with bounds[d] < s <= bounds[d + 1] for every item s in 1 .. n: the document that holds byte s - 1"""
    return (np.searchsorted(np.asarray(bounds, np.int64), np.asarray(items, np.int64) - 1, side="right") - 1).astype(np.uint32)


def row_docs(sa, bounds):
    """the document of every row: that of sa[r]"""
    return doc_of_items(bounds, sa)


def listing(sa, bounds, ranges, T=DEFAULT_TILE):
    """(records, ndocs, counters) of the row ranges [(lo, hi), ...]: records an FM_DOC array range by range and, within a range,
    by ascending first row; ndocs[j] the distinct documents of range j; counters rows, tiles and listed"""
    docs = row_docs(sa, bounds).astype(np.int64)
    lo = np.array([r[0] for r in ranges], np.int64).reshape(-1)
    hi = np.array([r[1] for r in ranges], np.int64).reshape(-1)
    assert ((0 <= lo) & (lo <= hi) & (hi <= docs.size)).all()
    cnt = hi - lo
    ctr = {"rows": int(cnt.sum()), "tiles": int(((cnt + T - 1) // T).sum())}
    # every (range, row) pair, range by range and by ascending row
    j = np.repeat(np.arange(lo.size), cnt)
    row = np.arange(j.size) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    d = docs[row]
    # grouped by (range, document), rows ascending inside a group: the head of a group is the first row, its length the tf
    order = np.lexsort((row, d, j))
    js, ds, rs = j[order], d[order], row[order]
    head = np.ones(js.size, bool)
    head[1:] = (js[1:] != js[:-1]) | (ds[1:] != ds[:-1])
    at = np.flatnonzero(head)
    tf = np.diff(np.append(at, js.size))
    back = np.lexsort((rs[at], js[at]))
    rec = np.zeros(at.size, FM_DOC)
    rec["doc"], rec["tf"], rec["row"], rec["range"] = ds[at][back], tf[back], rs[at][back], js[at][back]
    ctr["listed"] = int(rec.size)
    return rec, np.bincount(js[at], minlength=lo.size).astype(np.uint32), ctr


def pattern_rows(x, sa, pattern):
    """the rows [lo, hi) of a pattern by brute force: row r holds it when x[sa[r] - m .. sa[r]) is the pattern (the rows of a
    pattern are contiguous; (0, 0) when it does not occur)"""
    x, P = bytes(x), bytes(pattern)
    m = len(P)
    hit = [r for r, s in enumerate(sa) if s >= m and x[s - m:s] == P]
    if not hit:
        return 0, 0
    assert hit == list(range(hit[0], hit[-1] + 1)), "the rows of a pattern are contiguous"
    return hit[0], hit[-1] + 1


def definition(x, bounds, pattern):
    """{document: occurrences} from the text alone: every start p with x[p .. p + m) == pattern counts for the document that holds
    byte p + m - 1, the occurrence's last"""
    x, P = bytes(x), bytes(pattern)
    m = len(P)
    assert m >= 1
    got = {}
    for p in range(len(x) - m + 1):
        if x[p:p + m] == P:
            last = p + m - 1
            d = bisect.bisect_right(bounds, last) - 1        # bounds[d] <= last < bounds[d + 1]
            got[d] = got.get(d, 0) + 1
    return got
