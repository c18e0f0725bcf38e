"""The expected answers of the edit-distance search tests (TEST INFRASTRUCTURE ONLY): the rule of include/archon_hip.h in
plain Python and numpy, five ways.

  definition(x, P, K)        straight from ed() over all (s, e)
  rule(x, P, K)              the recurrence of the header over cells (d, s)
  rule_np(x, P, K)           the same by rows in numpy, fast enough for blocks of 1 MiB
  tile_model(x, P, K, W)     the filter: pieces, seeds, marked tiles, the rule on each marked tile's window; hits and counters
  band_model(x, P, K, W, t)  one tile as k_fm_edit computes it: 64 lanes, the packed key, the cap and the saturation

A hit is (start, end, distance); every function returns a pattern's hits by ascending end."""
import numpy as np


def _b(v):
    return bytes(v) if isinstance(v, (bytes, bytearray)) else np.ascontiguousarray(v, np.uint8).tobytes()


def _ed_ends(P, y):
    """ed(P, y[0 .. e)) for every e in [0, len(y)]"""
    m = len(P)
    col = list(range(m + 1))            # col[i] = ed(P[:i], y[:e])
    out = [col[m]]
    for ch in y:
        new = [col[0] + 1] * (m + 1)    # the empty prefix of P against y[:e] costs e
        for i in range(1, m + 1):
            new[i] = min(col[i - 1] + (P[i - 1] != ch), col[i] + 1, new[i - 1] + 1)
        col = new
        out.append(col[m])
    return out


def definition(x, P, K):
    """D(e) = min over s of ed(P, x[s .. e)); a match is an e with D(e) <= K, its start the largest s that reaches D(e)"""
    x, P = _b(x), _b(P)
    n = len(x)
    best = [(None, None)] * (n + 1)
    for s in range(n + 1):
        for e, d in enumerate(_ed_ends(P, x[s:]), start=s):
            if best[e][0] is None or d <= best[e][0]:       # ascending s: a tie keeps the larger s
                best[e] = (d, s)
    return [(s, e, d) for e, (d, s) in enumerate(best) if d <= K]


def rule(x, P, K):
    """the recurrence: (0, j) = (0, j), (i, 0) = (i, 0), else the least of diag + [P[i-1] != x[j-1]], up + 1, left + 1 with
    the largest start among the candidates that reach it"""
    x, P = _b(x), _b(P)
    n, m = len(x), len(P)
    prev = [(0, j) for j in range(n + 1)]
    for i in range(1, m + 1):
        cur = [(i, 0)]
        for j in range(1, n + 1):
            cands = [(prev[j - 1][0] + (P[i - 1] != x[j - 1]), prev[j - 1][1]), (prev[j][0] + 1, prev[j][1]), (cur[j - 1][0] + 1, cur[j - 1][1])]
            d = min(c[0] for c in cands)
            cur.append((d, max(c[1] for c in cands if c[0] == d)))
        prev = cur
    return [(s, j, d) for j, (d, s) in enumerate(prev) if d <= K]


_ONE = np.int64(1) << 32


def rule_cells(x, P):
    """row m of the recurrence by rows: (d, s) of every end as two int64 arrays.  A cell is d * 2^32 + (2^32 - 1 - s), whose
    plain minimum is the least d with the largest s; `left` is a running minimum of the row shifted by j * 2^32"""
    x = np.frombuffer(_b(x), np.uint8)
    P = _b(P)
    n = x.size
    j = np.arange(n + 1, dtype=np.int64)
    row = (_ONE - 1) - j
    shift = j * _ONE
    a = np.empty(n + 1, np.int64)
    for i in range(1, len(P) + 1):
        a[0] = i * _ONE + (_ONE - 1)
        np.minimum(row[:-1] + (x != P[i - 1]) * _ONE, row[1:] + _ONE, out=a[1:])
        a -= shift
        row = np.minimum.accumulate(a)
        row += shift
    return row >> 32, (_ONE - 1) - (row & (_ONE - 1))


def rule_np(x, P, K):
    """the matches from rule_cells"""
    d, s = rule_cells(x, P)
    e = np.flatnonzero(d <= K)
    return [(int(a), int(b), int(c)) for a, b, c in zip(s[e], e, d[e])]


def pieces(m, K):
    """o_0 .. o_{K+1}: piece i is P[o_i .. o_{i+1})"""
    return [i * m // (K + 1) for i in range(K + 2)]


def _occurrences(x, piece):
    """the starts of piece in x (numpy uint8), overlapping ones included"""
    L, n = len(piece), x.size
    if L > n:
        return np.zeros(0, np.int64)
    at = np.flatnonzero(x[:n - L + 1] == piece[0])
    for q in range(1, L):
        if not at.size:
            break
        at = at[x[at + q] == piece[q]]
    return at.astype(np.int64)


def marked_tiles(x, P, K, W):
    """(sorted marked tiles of the pattern, seed_rows): a seed of piece i at p has diagonal g = p - o_i and marks the tiles
    of u in [max(g, 0), min(g + 2K, n - m + K)]"""
    xb, P = _b(x), _b(P)
    x = np.frombuffer(xb, np.uint8)
    n, m = x.size, len(P)
    o = pieces(m, K)
    tiles, rows = set(), 0
    if n <= 64:                     # (the same in plain Python: the exhaustive tests make many thousand tiny calls)
        for i in range(K + 1):
            piece = P[o[i]:o[i + 1]]
            for p in range(n - len(piece) + 1):
                if xb[p:p + len(piece)] == piece:
                    rows += 1
                    lo, hi = max(p - o[i], 0), min(p - o[i] + 2 * K, n - m + K)
                    if lo <= hi:
                        tiles.update(range(lo // W, hi // W + 1))
        return sorted(tiles), rows
    for i in range(K + 1):
        g = _occurrences(x, P[o[i]:o[i + 1]]) - o[i]
        rows += g.size
        lo, hi = np.maximum(g, 0), np.minimum(g + 2 * K, n - m + K)
        ok = lo <= hi
        lo, hi = lo[ok] // W, hi[ok] // W
        for step in range(2 * K // W + 2):
            t = lo + step
            tiles.update(np.unique(t[t <= hi]).tolist())
    return sorted(tiles), rows


def window(n, m, K, W, t):
    """the text a tile reads: x[max(0, W t - 2K) .. min(n, W t + W - 1 + m - K))"""
    return max(0, W * t - 2 * K), min(n, W * t + W - 1 + m - K)


def tile_model(x, P, K, W, with_hits=True):
    """(hits, counters): every marked tile reports all the matches it owns (the ends e with (e - (m - K)) // W == t), found
    by the rule on the tile's window alone"""
    xb, P = _b(x), _b(P)
    n, m = len(xb), len(P)
    tiles, seed_rows = marked_tiles(xb, P, K, W)
    hits = []
    if with_hits:
        for t in tiles:
            ws, we = window(n, m, K, W, t)
            for s, e, d in rule_np(xb[ws:we], P, K):
                u = e + ws - (m - K)
                if u >= 0 and u // W == t:
                    hits.append((s + ws, e + ws, d))
    return hits, {"seed_rows": seed_rows, "tiles": len(tiles), "rows": len(tiles) * m, "hits": len(hits)}


def band_model(x, P, K, W, t):
    """tile t as one wave of k_fm_edit: lane l holds diagonal W t - 2K + l, a cell is d * 64 + (63 - l0) with l0 the lane of
    origin of its start, cells outside 0 <= j <= the window's end and lanes from W + 2K on hold the cap, values saturate"""
    x, P = _b(x), _b(P)
    n, m = len(x), len(P)
    assert W + 2 * K <= 64
    cap = (K + 1) * 64 + 63
    base = W * t - 2 * K
    jmax = min(n, W * t + W - 1 + m - K)
    lanes = np.arange(64, dtype=np.int64)
    live = lanes < W + 2 * K

    def valid(i):
        j = i + base + lanes
        return live & (j >= 0) & (j <= jmax), j

    ok, j = valid(0)
    key = np.where(ok, 63 - lanes, cap)
    col0 = 63 - (2 * K - W * t)             # the key of start 0 at distance 0
    for i in range(1, m + 1):
        ok, j = valid(i)
        tb = np.array([x[q - 1] if 1 <= q <= n else 0 for q in j.tolist()], np.int64)
        up = np.append(key[1:], cap)
        a = np.minimum(key + 64 * (tb != P[i - 1]), up + 64)
        a = np.where(j == 0, i * 64 + col0, a)
        a = np.where(ok, a, cap)
        cur = np.minimum.accumulate(a - 64 * lanes) + 64 * lanes
        key = np.where(ok & (cur < (K + 1) * 64), cur, cap)
    hits = []
    for l in range(K, K + W):
        e = m + base + l
        if 0 <= e <= n and key[l] < (K + 1) * 64:
            hits.append((max(0, base + 63 - int(key[l] & 63)), e, int(key[l] >> 6)))
    return hits
