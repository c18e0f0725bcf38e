"""The expected answers of the class search tests (TEST INFRASTRUCTURE ONLY): the rule of include/archon_hip.h
(archon_hip_fm_classes) in Python over fm_approx_naive.Rule, with its hits in order, both work counters and the pattern's
width; and a brute force over the text for the hit set and the closed forms of the counters."""
import numpy as np

MAX_WIDTH = 1024


def table_sets(table):
    """a (256, 8) uint32 class table as 256 lists of accepted bytes, ascending"""
    t = np.ascontiguousarray(table, np.uint32).reshape(256, 8)
    bits = np.unpackbits(t.view(np.uint8).reshape(256, 32), axis=1, bitorder="little")
    return [np.nonzero(row)[0].tolist() for row in bits]


def effective(rule, P, sets):
    """M_t of every position: classes[P[t]] cut to the bytes that occur in the block"""
    here = rule.R[1:] > rule.R[:256]
    return [[c for c in sets[b] if here[c]] for b in bytes(P)]


def width(rule, P, sets):
    """W of a pattern that is searched; a pattern that does no work (longer than the block, or with an empty M_t) has none"""
    M = effective(rule, P, sets)
    if len(M) > rule.n or any(not s for s in M):
        return 0
    return sum(len(s) - 1 for s in M)


def search(rule, P, table, sets=None):
    """(hits [(lo, hi, d)] in the rule's order, expansions, steps); the most frames pending at once in search.pending"""
    P = bytes(P)
    sets = table_sets(table) if sets is None else sets
    m, n = len(P), rule.n
    search.pending = 0
    M = effective(rule, P, sets)
    if any(not s for s in M):
        return [], 0, 0
    if m == 0:
        return [(0, n, 0)], 0, 0
    if m > n:
        return [], 0, 0
    hits, work = [], [0, 0]
    R = rule.R
    stack = [(0, 0, n, 0)]
    while stack:
        search.pending = max(search.pending, len(stack) - 1)
        t, lo, hi, d = stack.pop()
        while True:
            if t == m:
                hits.append((lo, hi, d))
                break
            if len(M[t]) == 1:
                c = M[t][0]
                if t == 0:
                    lo, hi = int(R[c]), int(R[c + 1])
                else:
                    work[1] += 1
                    lo, hi = int(R[c] + rule.occ[c, lo]), int(R[c] + rule.occ[c, hi])
                if lo >= hi:
                    break
                d += c != P[t]
                t += 1
                continue
            if t == 0:
                clo, chi = R[:256], R[1:]
            else:
                work[0] += 1
                clo, chi = rule.children(lo, hi)
            kids = [(t + 1, int(clo[c]), int(chi[c]), d + (c != P[t])) for c in M[t] if clo[c] < chi[c]]
            stack.extend(reversed(kids))
            break
    return hits, work[0], work[1]


search.pending = 0


def brute(x, P, sets):
    """{w: (mismatches, sorted starts)} and the two counters of the closed forms, the classes cut to the bytes of x"""
    x, P = bytes(x), bytes(P)
    n, m = len(x), len(P)
    here = set(x)
    M = [[c for c in sets[b] if c in here] for b in P]
    if any(not s for s in M) or m > n:
        return {}, 0, 0
    ok = [set(s) for s in M]
    hits = {}
    for q in range(n - m + 1):
        w = x[q:q + m]
        if all(w[t] in ok[t] for t in range(m)):
            hits.setdefault(w, (sum(a != b for a, b in zip(w, P)), []))[1].append(q)
    ex = st = 0
    for t in range(1, m):
        subs = {x[q:q + t] for q in range(n - t + 1)}
        count = sum(all(u[i] in ok[i] for i in range(t)) for u in subs)
        if len(M[t]) >= 2:
            ex += count
        else:
            st += count
    return hits, ex, st
