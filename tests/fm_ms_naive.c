/* Brute force for the matching-statistics tests (TEST INFRASTRUCTURE ONLY): the record (len, lo, hi) of every position of
 * every pattern by the DEFINITION, with "occurs" decided by binary search in the a7 suffix array the caller gives (the
 * oracle's), as fm_mem_naive.c does.  Nothing here steps through a BWT or reads a hierarchy.
 *
 * Item s (1 .. n) has the key x[s-1], x[s-2], ..., x[0], INF; sa holds the items in ascending key order.  A piece Q occurs
 * ending at s exactly when the key of s begins with Q reversed, so the rows of Q are one interval of sa: what
 * archon_hip_fm_count returns for Q.
 *
 * len(e) <= len(e-1) + 1 (a piece of an occurring piece occurs), so len(e) is the first length from len(e-1) + 1 downwards
 * whose piece ending at e occurs.
 *
 * The work counters of the header's procedure come from a second walk that keeps the procedure's state (lo, hi, l): a rank
 * step for P[t] succeeds exactly when P[t-l .. t] occurs, and a parent move goes to l' = min(max(lcp[lo], lcp[hi]), l - 1)
 * with the rows of P[t-l' .. t) -- the caller's LCP array (Kasai's, of the same suffix array), read as 0 at 0 and at n.  The
 * walk's lengths must be the definition's: -1 when they are not. */
#include <stdint.h>
#include <stdlib.h>

/* the key of item s against q[0 .. l) read backwards from q[l-1]: -1 key smaller, 0 the key begins with it, 1 key larger */
static int cmp_key(const uint8_t *x, uint32_t s, const uint8_t *q, uint32_t l)
{
    for (uint32_t i = 0; i < l; ++i) {
        if (i >= s) return 1;                       /* INF */
        const uint8_t a = x[s - 1 - i], c = q[l - 1 - i];
        if (a != c) return a < c ? -1 : 1;
    }
    return 0;
}

/* rows [lo, hi) whose keys begin with q reversed */
static void rows_of(const uint8_t *x, uint32_t n, const uint32_t *sa, const uint8_t *q, uint32_t l, uint32_t *lo, uint32_t *hi)
{
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (cmp_key(x, sa[mid], q, l) < 0) a = mid + 1; else b = mid;
    }
    *lo = a;
    b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (cmp_key(x, sa[mid], q, l) <= 0) a = mid + 1; else b = mid;
    }
    *hi = a;
}

/* len, lo, hi: off[k] words, the record of end e of pattern j at off[j] + e - 1.  counters = steps, parents, matched, longest.
 * Returns 0, or -1 when the procedure's walk disagrees with the definition. */
int fm_ms_naive(const uint8_t *x, uint32_t n, const uint32_t *sa, const uint32_t *lcp, const uint8_t *pat, const uint32_t *off, uint32_t k,
                uint32_t *len, uint32_t *lo, uint32_t *hi, uint64_t *counters)
{
    uint64_t steps = 0, parents = 0, matched = 0, longest = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const uint8_t *P = pat + off[j];
        const uint32_t m = off[j + 1] - off[j];
        uint32_t *rl = len + off[j], *rlo = lo + off[j], *rhi = hi + off[j];
        /* the definition */
        uint32_t prev = 0;
        for (uint32_t t = 0; t < m; ++t) {
            uint32_t l = prev + 1, a = 0, b = n;
            for (; l > 0; --l) {
                rows_of(x, n, sa, P + t + 1 - l, l, &a, &b);
                if (a < b) break;
            }
            if (l == 0) { a = 0; b = n; }
            rl[t] = l;
            rlo[t] = a;
            rhi[t] = b;
            prev = l;
            matched += l;
            if (l > longest) longest = l;
        }
        /* the procedure's counters */
        uint32_t slo = 0, shi = n, l = 0;
        for (uint32_t t = 0; t < m; ++t) {
            for (;;) {
                uint32_t a, b;
                if (l == 0) {
                    rows_of(x, n, sa, P + t, 1, &a, &b);
                    if (a < b) { slo = a; shi = b; l = 1; } else { slo = 0; shi = n; }
                    break;
                }
                ++steps;
                rows_of(x, n, sa, P + t - l, l + 1, &a, &b);
                if (a < b) { slo = a; shi = b; ++l; break; }
                ++parents;
                const uint32_t vl = slo ? lcp[slo] : 0, vh = shi < n ? lcp[shi] : 0;
                uint32_t lp = vl > vh ? vl : vh;
                if (lp > l - 1) lp = l - 1;
                l = lp;
                if (l == 0) { slo = 0; shi = n; }
                else rows_of(x, n, sa, P + t - l, l, &slo, &shi);
            }
            if (l != rl[t] || slo != rlo[t] || shi != rhi[t]) return -1;
        }
    }
    counters[0] = steps;
    counters[1] = parents;
    counters[2] = matched;
    counters[3] = longest;
    return 0;
}
