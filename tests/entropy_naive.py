"""The expected answers of the entropy and complexity tests (TEST INFRASTRUCTURE ONLY).  FROM THE TEXT ALONE: the followers of
every context (collections.Counter, math.fsum) and the distinct substrings of every length at tiny sizes, (k+1)-byte windows
through np.unique above them.  Beside them the row rules of include/archon_hip.h in numpy over (sa, lcp, bwt, base), with the
model of which group the follower pass settles where; tests/test_entropy_abi.py pins the rules to the text-based helpers."""
import collections
import math

import numpy as np

ENTROPY = np.dtype([("k", "<u4"), ("reserved", "<u4"), ("contexts", "<u8"), ("deterministic", "<u8"), ("pairs", "<u8"), ("symbols", "<u8"),
                    ("bits", "<f8")])
DIRECT_ROWS = 64                # entropy.hiph kDirectRows
WAVE = 64                       # rows of a wave's window
DEFAULT_TILE = 2048             # kmers.hiph kDefaultTile
DEFAULT_MAX_LEN = 4095


def bits_of(followers):
    """sum over the contexts (an iterable of iterables of counts) of c log2(m / c), m the context's total: math.fsum of the
    correctly rounded terms' factors"""
    terms = []
    for counts in followers:
        counts = [int(c) for c in counts]
        m = sum(counts)
        terms += [c * math.log2(m / c) for c in counts if c != m]
    return math.fsum(terms)


def summary(followers, n, k):
    """(contexts, deterministic, pairs, symbols, bits) of the per-context follower counts"""
    followers = [list(f) for f in followers]
    return (len(followers), sum(len(f) == 1 for f in followers), sum(len(f) for f in followers), max(n - k, 0), bits_of(followers))


# ---------------------------------------------------------------- from the text, pure Python (tiny n)
def order_text(x, k):
    """the order-k record of x by the definition: F_w = the bytes x[p], k <= p < n, with x[p-k .. p) = w"""
    x = bytes(x)
    F = collections.defaultdict(collections.Counter)
    for p in range(k, len(x)):
        F[x[p - k:p]][x[p]] += 1
    return summary([c.values() for c in F.values()], len(x), k)


def distinct_text(x):
    """d[l-1] = the distinct substrings of length l, l = 1 .. n"""
    x = bytes(x)
    return [len({x[p:p + l] for p in range(len(x) - l + 1)}) for l in range(1, len(x) + 1)]


def delta_of(d):
    """(length, count) of the largest d_l / l over the given prefix of d, ties to the smallest l, by integers"""
    bl, bd = 1, d[0]
    for l, c in enumerate(d, 1):
        if c * bl > bd * l:
            bl, bd = l, c
    return bl, bd


def runs_of(bwt):
    """(runs, longest run) of a byte string"""
    b = np.frombuffer(bytes(bwt), np.uint8)
    starts = np.flatnonzero(np.concatenate(([True], b[1:] != b[:-1])))
    return starts.size, int(np.diff(np.append(starts, b.size)).max())


# ---------------------------------------------------------------- from the text, numpy (any n)
def _void_rows(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype((np.void, a.dtype.itemsize * a.shape[1]))).ravel()


def order_windows(x, k):
    """order_text for any n: the (k+1)-byte windows through np.unique; the windows of one context are neighbours there"""
    x = np.ascontiguousarray(x, np.uint8)
    n = x.size
    if k >= n:
        return (0, 0, 0, max(n - k, 0), 0.0)
    uniq, cnt = np.unique(_void_rows(np.lib.stride_tricks.sliding_window_view(x, k + 1)), return_counts=True)
    rows = np.frombuffer(uniq.tobytes(), np.uint8).reshape(-1, k + 1)[:, :k]
    new = np.concatenate(([True], (rows[1:] != rows[:-1]).any(axis=1))) if k else np.concatenate(([True], np.zeros(cnt.size - 1, bool)))
    ctx = np.cumsum(new) - 1
    m = np.bincount(ctx, weights=cnt).astype(np.int64)
    per_ctx = np.bincount(ctx)
    keep = cnt != m[ctx]
    bits = math.fsum(int(c) * math.log2(int(t) / int(c)) for c, t in zip(cnt[keep], m[ctx][keep]))
    return (int(m.size), int((per_ctx == 1).sum()), int(cnt.size), n - k, bits)


# ---------------------------------------------------------------- from the arrays: the rules of the header in numpy
def window_of(rows, tile):
    """the window of the follower pass a row lies in: its tile and the wave's step inside it"""
    rows = np.asarray(rows, np.int64)
    return rows // tile * (1 << 32) + rows % tile // WAVE


def group_kinds(sa, lcp, k, tile=DEFAULT_TILE):
    """(lo, hi, kind) of the k-mer groups in ascending row, k >= 1: kind 0 direct (at most DIRECT_ROWS rows, ending past the window
    of its first row), 1 table (more rows), 2 inside one window"""
    sa = np.asarray(sa, np.int64)
    below = np.asarray(lcp, np.int64) < k
    below[0] = True
    starts = np.flatnonzero(below)
    ends = np.append(starts[1:], sa.size)
    keep = sa[starts] >= k
    lo, hi = starts[keep], ends[keep]
    table = hi - lo > DIRECT_ROWS
    in_wave = window_of(lo, tile) == window_of(hi - 1, tile)
    assert not (table & in_wave).any()
    return lo, hi, np.where(table, 1, np.where(in_wave, 2, 0))


def order_rows(sa, lcp, bwt, base, k, tile=DEFAULT_TILE):
    """((contexts, deterministic, pairs, symbols, bits), (groups_direct, groups_table, groups_in_wave)) by the row rule: the k-mer
    groups of archon_hip_kmers, F = bwt[r] for r in [lo, hi), r != base; k = 0: one group [0, n) with bwt[base] counted"""
    bwt = np.frombuffer(bytes(bwt), np.uint8) if isinstance(bwt, (bytes, bytearray)) else np.asarray(bwt, np.uint8)
    n = len(sa)
    if k > n:
        return (0, 0, 0, 0, 0.0), (0, 0, 0)
    if k == 0:
        return summary([np.bincount(bwt)[np.bincount(bwt) > 0]], n, 0), (0, 1, 0)
    lo, hi, kind = group_kinds(sa, lcp, k, tile)
    size = hi - lo
    # the followers: (group, byte) pairs over the rows of the k-mer groups, the primary row left out
    gid = np.repeat(np.arange(lo.size), size)
    rows = np.arange(size.sum()) - np.repeat(np.cumsum(size) - size, size) + np.repeat(lo, size)
    live = rows != base
    pair, cnt = np.unique(gid[live] * 256 + bwt[rows[live]], return_counts=True)
    followers = [[] for _ in range(lo.size)]
    for g, c in zip(pair // 256, cnt):
        followers[g].append(int(c))
    return summary([f for f in followers if f], n, k), tuple(int((kind == j).sum()) for j in (0, 1, 2))


def complexity_rows(lcp, bwt=None, max_len=0):
    """(record as a dict, counts) by the row rule: d_l = n - l + 1 - #{i >= 1 : lcp[i] >= l}"""
    l = np.asarray(lcp, np.int64).copy()
    n = l.size
    l[0] = 0
    L = min(max_len or DEFAULT_MAX_LEN, n)
    hist = np.bincount(np.minimum(l[1:], L), minlength=L + 1)
    at_least = np.cumsum(hist[::-1])[::-1]                  # at_least[v] = rows with lcp >= v
    d = [(n - v + 1 - int(at_least[v])) % (1 << 32) for v in range(1, L + 1)]       # (unsigned words: an lcp of nothing can pass n - l + 1)
    dl, dc = delta_of(d)
    rec = dict(n=n, max_len=L, lcp_max=int(l.max()), delta_len=dl, delta_count=dc, delta_exact=int(L == n or dc * (L + 1) >= (n - L) * dl),
               longest_run=0, lcp_sum=int(l.sum()), substrings=(n * (n + 1) // 2 - int(l.sum())) % (1 << 64), runs=0)
    if bwt is not None:
        rec["runs"], rec["longest_run"] = runs_of(bwt)
    return rec, np.array(d, np.uint32)


def bits_bound(n, pairs, want):
    """what a sum of `pairs` non-negative terms, each within a few ulp of c log2(m / c) <= a few ulp of c, may differ from the
    exact sum `want` by, in any order: 2^-48 n + 2^-52 pairs want"""
    return 2.0 ** -48 * n + 2.0 ** -52 * pairs * want
