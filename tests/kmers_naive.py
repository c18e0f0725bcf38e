"""The expected answers of the k-mer tests (TEST INFRASTRUCTURE ONLY), FROM THE TEXT ALONE: which k-mers a text has and how
often (collections.Counter at tiny sizes, windows through np.unique above them), their rows by sorting the reversed k-mers
together with the short prefixes (a7 order) -- the suffix array only names the item of a row and is checked against the text
on the way --, and the shortest unique substrings by brute force.  Beside them the boundary rule of include/archon_hip.h in
numpy over (sa, lcp), for inputs the text-based helpers are too slow for or that are the arrays of no text;
tests/test_kmers_abi.py pins it to the text-based ones."""
import collections

import numpy as np

KMER = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("item", "<u4")])


# ---------------------------------------------------------------- from the text, pure Python (tiny n)
def counts(x, k):
    """Counter of the k-mers of x"""
    x = bytes(x)
    return collections.Counter(x[p:p + k] for p in range(len(x) - k + 1))


def occ_text(x, k):
    """occ[p], p in 0 .. n-k: how often x[p .. p+k) occurs in x"""
    x = bytes(x)
    c = counts(x, k)
    return np.array([c[x[p:p + k]] for p in range(len(x) - k + 1)], np.uint32)


def kmers_text(x, k, sa):
    """(KMER records of all k-mers in ascending row, number of short rows).  The k-mers in a7 order are the distinct windows
    sorted by their reversed bytes; the short rows, items s < k with key x[s-1] .. x[0] INF, sort among them with INF = 256.
    Every row of a k-mer must hold the end of one of its occurrences, every short row its item: sa is checked, not trusted"""
    x = bytes(x)
    n = len(x)
    c = counts(x, k)
    entries = [(list(w[::-1]), cnt, w) for w, cnt in c.items()]
    entries += [(list(x[:s][::-1]) + [256], 1, None) for s in range(1, min(k - 1, n) + 1)]
    entries.sort(key=lambda e: e[0])
    recs, row = [], 0
    for key, cnt, w in entries:
        if w is None:
            assert sa[row] == len(key) - 1, (x, k)
        else:
            assert sorted(int(sa[r]) for r in range(row, row + cnt)) == [p + k for p in range(n - k + 1) if x[p:p + k] == w], (x, k, w)
            recs.append((row, row + cnt, int(sa[row])))
        row += cnt
    assert row == n
    return np.array(recs, KMER).reshape(-1), min(k - 1, n)


def count_occ(x, w, stop=None):
    """occurrences of w in x, overlapping ones included (counting stops at `stop`)"""
    c, p = 0, x.find(w)
    while p >= 0 and (stop is None or c < stop):
        c += 1
        p = x.find(w, p + 1)
    return c


def sus_text(x):
    """sus[e-1]: the least L with x[e-L .. e) occurring once, 0 when even x[0 .. e) occurs twice -- by brute force"""
    x = bytes(x)
    return np.array([next((L for L in range(1, e + 1) if count_occ(x, x[e - L:e], 2) == 1), 0) for e in range(1, len(x) + 1)], np.uint32)


def check_sus_sample(x, sus, positions):
    """the identity "least L with count 1" at the items e in positions: x[e-L .. e) occurs once and its suffix one shorter
    twice; L = 0: the whole prefix occurs again"""
    x = bytes(x)
    for e in positions:
        L = int(sus[e - 1])
        if L == 0:
            assert count_occ(x, x[:e], 2) == 2, e
        else:
            assert L <= e and count_occ(x, x[e - L:e], 2) == 1, (e, L)
            assert L == 1 or count_occ(x, x[e - L + 1:e], 2) == 2, (e, L)


def hist_of(sizes, bins):
    """hist[c] = entries of sizes equal to c, the last bin those >= bins - 1; bin 0 stays 0"""
    h = np.zeros(bins, np.uint32)
    np.add.at(h, np.minimum(np.asarray(sizes, np.int64), bins - 1), 1)
    return h


# ---------------------------------------------------------------- from the text, numpy (any n)
def _void_rows(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype((np.void, a.dtype.itemsize * a.shape[1]))).ravel()


def occ_windows(x, k):
    """occ_text for any n: the windows of x as byte strings through np.unique"""
    x = np.ascontiguousarray(x, np.uint8)
    if k > x.size:
        return np.zeros(0, np.uint32)
    _, inv, cnt = np.unique(_void_rows(np.lib.stride_tricks.sliding_window_view(x, k)), return_inverse=True, return_counts=True)
    return cnt[inv.ravel()].astype(np.uint32)


def kmers_windows(x, k, sa):
    """kmers_text for any n: the reversed windows through np.unique (memcmp order of the reversed bytes is a7 order), the short
    rows sorted among them as rows of 16-bit symbols, high byte first, with INF = 256.  sa is checked against the windows"""
    x = np.ascontiguousarray(x, np.uint8)
    sa = np.asarray(sa, np.int64)
    n = x.size
    nshort = min(k - 1, n)
    if k <= n:
        rev = np.lib.stride_tricks.sliding_window_view(x, k)[:, ::-1]
        uniq, inv, cnt = np.unique(_void_rows(rev), return_inverse=True, return_counts=True)
        inv = inv.ravel()
        keys = np.frombuffer(uniq.tobytes(), np.uint8).reshape(-1, k).astype(np.uint16)
    else:
        inv, cnt, keys = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, k), np.uint16)
    short = np.zeros((nshort, k), np.uint16)
    for s in range(1, nshort + 1):
        short[s - 1, :s] = x[:s][::-1]
        short[s - 1, s] = 256
    d = cnt.size
    both = np.concatenate([keys, short])
    order = np.argsort(_void_rows(np.stack([both >> 8, both & 255], axis=-1).astype(np.uint8).reshape(both.shape[0], 2 * k)), kind="stable")
    sizes = np.concatenate([cnt, np.ones(nshort, np.int64)])[order]
    lo = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    assert int(sizes.sum()) == n
    is_kmer = order < d
    # every row of a k-mer holds the end of an occurrence of THAT k-mer; a short row holds its item
    which = np.repeat(order, sizes)
    rows_kmer = which < d
    assert (sa[rows_kmer] >= k).all() and (inv[sa[rows_kmer] - k] == which[rows_kmer]).all()
    assert (sa[~rows_kmer] == which[~rows_kmer] - d + 1).all()
    recs = np.zeros(int(is_kmer.sum()), KMER)
    recs["lo"] = lo[is_kmer]
    recs["hi"] = lo[is_kmer] + sizes[is_kmer]
    recs["item"] = sa[lo[is_kmer]]
    return recs, nshort


# ---------------------------------------------------------------- from the arrays: the rule of the header in numpy
def kmers_arrays(sa, lcp, k):
    """(KMER records of all k-mer groups in ascending row, groups, short rows) by the boundary rule: row i starts a group when
    i == 0 or lcp[i] < k; a group is a k-mer when its first item is at least k"""
    sa = np.asarray(sa, np.int64)
    below = np.asarray(lcp, np.int64) < k
    below[0] = True
    starts = np.flatnonzero(below)
    ends = np.append(starts[1:], sa.size)
    keep = sa[starts] >= k
    recs = np.zeros(int(keep.sum()), KMER)
    recs["lo"], recs["hi"], recs["item"] = starts[keep], ends[keep], sa[starts][keep]
    return recs, starts.size, int((~keep).sum())


def occ_arrays(sa, lcp, k):
    """occ by the rule: a row r of a k-mer group of c rows gives occ[sa[r] - k] = c"""
    sa = np.asarray(sa, np.int64)
    n = sa.size
    below = np.asarray(lcp, np.int64) < k
    below[0] = True
    starts = np.flatnonzero(below)
    sizes = np.diff(np.append(starts, n))
    per_row = np.repeat(sizes, sizes)
    occ = np.zeros(max(n - k + 1, 0), np.uint32)
    rows = sa >= k
    occ[sa[rows] - k] = per_row[rows]
    return occ


def sus_arrays(sa, lcp):
    """sus by the rule: m = max(lcp[r], lcp[r+1]) (lcp[0] and lcp[n] read as 0); sus[sa[r]-1] = m + 1 if m + 1 <= sa[r] else 0"""
    sa = np.asarray(sa, np.int64)
    l = np.asarray(lcp, np.int64).copy()
    l[0] = 0
    m = np.maximum(l, np.append(l[1:], 0))
    sus = np.zeros(sa.size, np.uint32)
    sus[sa - 1] = np.where(m < sa, m + 1, 0)
    return sus
