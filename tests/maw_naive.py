"""The expected answer of the minimal-absent-words tests (TEST INFRASTRUCTURE ONLY): the DEFINITION in terms of the text alone,
and the node/child rule of include/archon_hip.h over the arrays, in plain Python -- records in the rule's order and the
counters of the record that follow from the input.  tests/test_maw_abi.py pins the second to the first."""
import numpy as np

MAW = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("len", "<u4"), ("item", "<u4"), ("last", "<u4")])


def definition(x):
    """the minimal absent words of x of length >= 2 by the text alone, as a set of bytes: a.w.b with a.w in x, w.b in x and
    a.w.b not in x.  Every substring is taken: quadratic in space, for n up to about 40"""
    x = bytes(x)
    n = len(x)
    subs = {x[p:q] for p in range(n) for q in range(p + 1, n + 1)}
    letters = sorted(set(x))
    words = set()
    for aw in subs:
        for b in letters:
            wb = aw[1:] + bytes([b])
            if wb in subs and aw + bytes([b]) not in subs:
                words.add(aw + bytes([b]))
    return words


def intervals(lcp):
    """every LCP interval (lo, hi, l, k) in ascending representative row k: l = lcp[k] > 0, lo the greatest p < k with
    lcp[p] < l and no row of (lo, k) holding l, hi the least q > k with lcp[q] < l or n; lcp[0] reads as 0"""
    L = [int(v) for v in lcp]
    n = len(L)
    L[0] = 0
    nxt, st = [n] * n, []
    for i in range(n):
        while st and L[st[-1]] > L[i]:
            nxt[st.pop()] = i
        st.append(i)
    out, st = [], []
    for k in range(n):
        while st and L[st[-1]] > L[k]:
            st.pop()
        if k and L[k]:
            p = st[-1]                  # the greatest p < k with lcp[p] <= l: row 0 holds 0
            if L[p] < L[k]:
                out.append((p, nxt[k], L[k], k))
        st.append(k)
    return out


def _set(bwt, base, p, q):
    """B([p, q)): the bytes of bwt[p .. q) without the primary row"""
    if p <= base < q:
        return set(bwt[p:base]) | set(bwt[base + 1:q])
    return set(bwt[p:q])


def model(sa, lcp, bwt, base, min_len=2, max_len=0, direct_rows=64):
    """(records as a MAW array in the rule's order, counters): the rule over the arrays.  counters: intervals, nodes, children,
    sets_direct, sets_table, words, shortest, longest, absent_bytes"""
    sa = [int(v) for v in sa]
    lcp_a = np.asarray(lcp, np.int64).copy()
    lcp_a[0] = 0
    bwt = bytes(bwt) if isinstance(bwt, (bytes, bytearray)) else np.ascontiguousarray(bwt, np.uint8).tobytes()
    n = len(sa)
    base = int(base)
    lo_len = max(int(min_len), 2)
    hi_len = int(max_len) if max_len else 1 << 40
    ivs = intervals(lcp_a)
    c = dict(intervals=len(ivs), nodes=0, children=0, sets_direct=0, sets_table=0, words=0, shortest=0, longest=0,
             absent_bytes=256 - len(set(bwt)))
    # flags as the repeats section has them: right-uniform exactly when no flag lies in (lo, hi)
    flags = np.zeros(n + 1, np.int64)
    b = np.frombuffer(bwt, np.uint8)
    flags[1:n] = b[1:] != b[:-1]
    flags[base] |= base > 0
    if base + 1 < n:
        flags[base + 1] = 1
    S = np.concatenate(([0], np.cumsum(flags)))         # S[k] = flags of rows < k
    recs = []

    def took(rows):
        c["sets_direct" if rows <= direct_rows else "sets_table"] += 1

    for lo, hi, l, k in [(0, n, 0, 0)] + ivs:
        if not lo_len <= l + 2 <= hi_len:
            continue
        if l and S[hi] == S[lo + 1]:
            continue
        c["nodes"] += 1
        node = _set(bwt, base, lo, hi)
        if l == 0:
            node = node | {bwt[base]}
        took(hi - lo)
        cuts = [lo] + (lo + 1 + np.nonzero(lcp_a[lo + 1:hi] == l)[0]).tolist() + [hi]
        for clo, chi in zip(cuts[:-1], cuts[1:]):
            c["children"] += 1
            if sa[clo] == l:
                assert chi == clo + 1
                continue
            took(chi - clo)
            for last in sorted(node - _set(bwt, base, clo, chi)):
                recs.append((clo, chi, l + 2, sa[clo], last))
    out = np.array(recs, MAW) if recs else np.zeros(0, MAW)
    c["words"] = out.size
    if out.size:
        c["shortest"], c["longest"] = int(out["len"].min()), int(out["len"].max())
    return out, c


def word(x, rec):
    """the bytes of a record: x[item-len+1 .. item) followed by last"""
    x = bytes(x)
    lo, hi, ln, item, last = (int(v) for v in rec)
    return x[item - ln + 1:item] + bytes([last])


def _codes(c, m):
    """the 2-bit codes of every m-mer of the letters c (values 0 .. 3), first letter in the highest bits"""
    count = c.size - m + 1
    code = np.zeros(max(count, 0), np.int64)
    for i in range(m):
        code = code * 4 + c[i:count + i]
    return code


def words_of_length(x, L, first=97):
    """the minimal absent words of exactly L >= 2 bytes of a block over the four letters first .. first + 3, by the definition
    and without the arrays, as ascending 2-bit codes (the first byte in the highest bits): presence bitmaps of all (L-1)-mers
    and all L-mers; a code is a word when it is absent while its first and its last L - 1 letters are present"""
    c = np.asarray(x, np.uint8).astype(np.int64) - first
    assert L >= 2 and c.size and c.min() >= 0 and c.max() <= 3
    present = []
    for m in (L - 1, L):
        P = np.zeros(4 ** m, bool)
        P[_codes(c, m)] = True
        present.append(P)
    short, full = present
    return np.flatnonzero(~full & np.repeat(short, 4) & np.tile(short, 4))


def record_codes(x, recs, L, first=97):
    """the 2-bit codes of the words of records that all have len L: x[item - L + 1 .. item) followed by last"""
    c = np.asarray(x, np.uint8).astype(np.int64) - first
    assert (recs["len"] == L).all()
    start = recs["item"].astype(np.int64) - L + 1
    code = np.zeros(recs.size, np.int64)
    for i in range(L - 1):
        code = code * 4 + c[start + i]
    return code * 4 + (recs["last"].astype(np.int64) - first)


def code_bytes(code, L, first=97):
    return bytes(first + ((int(code) >> (2 * (L - 1 - i))) & 3) for i in range(L))
