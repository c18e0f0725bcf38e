"""The windows of a row range in text order (include/archon_hip.h, archon_hip_fm_win_*) by their definition in numpy: sort
sa[lo:hi], cut by the item window [a, b), take the first `most`.  And the two rules of the header that the statistics follow:
`walks` from the queries and n alone, `wm_bytes` from n alone."""
import numpy as np

FM_WIN = np.dtype([("item", "<u4"), ("range", "<u4")])


def levels(n):
    """L: the bit length of n, at least 1"""
    return max(int(n).bit_length(), 1)


def wm_bytes(n):
    """L levels of 8 B words of bits and B + 1 directory words, B = ceil(n / 256), each level padded to 256 bytes"""
    B = -(-n // 256)
    return levels(n) * 256 * -(-4 * (9 * B + 1) // 256)


def valid(n, lo, hi, a, b):
    return lo <= hi <= n and a <= b <= n + 1


def window(sa, lo, hi, a=None, b=None):
    """the items of rows [lo, hi) inside [a, b), ascending (a and b None: the whole block)"""
    n = len(sa)
    a, b = (0, n + 1) if a is None else (a, b)
    assert valid(n, lo, hi, a, b), (n, lo, hi, a, b)
    s = np.sort(np.asarray(sa[lo:hi], dtype=np.int64))
    return s[(s >= a) & (s < b)]


def bound_walks(n, lo, hi, a=None, b=None):
    """walks the two bounds of a query make: none in an empty range, none for a bound of 0 or >= 2^L, one for every other"""
    if lo >= hi:
        return 0
    a, b = (0, n + 1) if a is None else (a, b)
    top = 1 << levels(n)
    return int(0 < a < top) + int(0 < b < top)


def windows(sa, lo, hi, a=None, b=None):
    """the window of every query: what count, select and listing take as `wins` when several of them share the queries"""
    k = len(lo)
    return [window(sa, int(lo[j]), int(hi[j]), None if a is None else int(a[j]), None if b is None else int(b[j])) for j in range(k)]


def _counters(sa, lo, hi, a, b, wins):
    n = len(sa)
    k = len(lo)
    return {"rows": int(sum(int(hi[j]) - int(lo[j]) for j in range(k))), "in_window": int(sum(w.size for w in wins)),
            "walks": sum(bound_walks(n, int(lo[j]), int(hi[j]), None if a is None else int(a[j]), None if b is None else int(b[j])) for j in range(k)),
            "listed": 0}


def count(sa, lo, hi, a=None, b=None, wins=None):
    """(count[k], counters)"""
    wins = windows(sa, lo, hi, a, b) if wins is None else wins
    return np.array([w.size for w in wins], np.uint32), _counters(sa, lo, hi, a, b, wins)


def select(sa, lo, hi, idx, a=None, b=None, wins=None):
    """(item[k], counters): the idx-th smallest item of every window, 0 when it has idx items or fewer; a select that returns an
    item makes one walk more"""
    wins = windows(sa, lo, hi, a, b) if wins is None else wins
    item = np.array([int(w[int(i)]) if int(i) < w.size else 0 for w, i in zip(wins, idx)], np.uint32)
    c = _counters(sa, lo, hi, a, b, wins)
    c["walks"] += int(np.count_nonzero(item))
    return item, c


def listing(sa, lo, hi, a=None, b=None, most=0, emit=True, wins=None):
    """(count[k], records, counters): every window's min(count, most) smallest items (most 0: all) as {item, range}, range by
    range; every emitted record makes one walk more.  emit False: no records, no walks for them"""
    wins = windows(sa, lo, hi, a, b) if wins is None else wins
    cnt = np.array([w.size for w in wins], np.uint32)
    parts = [w[:most] if most else w for w in wins]
    recs = np.zeros(sum(p.size for p in parts), FM_WIN)
    at = 0
    for j, p in enumerate(parts):
        recs["item"][at:at + p.size] = p
        recs["range"][at:at + p.size] = j
        at += p.size
    c = _counters(sa, lo, hi, a, b, wins)
    if emit:
        c["walks"] += recs.size
        c["listed"] = recs.size
    return cnt, (recs if emit else None), c
