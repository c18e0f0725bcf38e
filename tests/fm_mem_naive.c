/* Brute force for the SMEM tests (TEST INFRASTRUCTURE ONLY): the super-maximal exact matches of patterns in x by their
 * DEFINITION, with "occurs" decided by binary search in the a7 suffix array the caller gives (the oracle's), so a block of a
 * few MiB stays cheap.  Nothing here steps through a BWT.
 *
 * Item s (1 .. n) has the key x[s-1], x[s-2], ..., x[0], INF; sa holds the items in ascending key order.  A piece Q occurs
 * ending at s exactly when the key of s begins with Q reversed, so the rows of Q are one interval of sa: what
 * archon_hip_fm_count returns for Q.
 *
 * ms[b] = the length of the longest piece of P that starts at b and occurs.  b + ms[b] never decreases (a piece of an occurring
 * piece occurs), so (b, b + ms[b]) is an SMEM exactly when ms[b] > 0 and (b == 0 or b - 1 + ms[b-1] < b + ms[b]).  The work
 * counters of the header's procedure follow from ms alone:
 *   an SMEM (b, e) costs e - b steps on the primary index when e < m, else e - b - 1;
 *   when e < m, with b' the next position after b with b' + ms[b'] > e: no step when b' > e (P[e] is not in x), else
 *   e - b' + 1 steps on the mirror when b' > b + 1, one fewer when b' == b + 1. */
#include <stdint.h>
#include <stdlib.h>

typedef struct { uint32_t lo, hi, start, end, pattern, reserved0; } mem_t;

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

/* returns the number of SMEMs of at least min_len bytes over all patterns (-1: more than cap); counters = fwd_steps, bwd_steps,
 * found */
int64_t fm_mem_naive(const uint8_t *x, uint32_t n, const uint32_t *sa, const uint8_t *pat, const uint32_t *off, uint32_t k, uint32_t min_len,
                     uint32_t *nmems, uint32_t *nocc, mem_t *mems, uint64_t cap, uint64_t *counters)
{
    uint64_t total = 0, fwd = 0, bwd = 0, found = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const uint8_t *P = pat + off[j];
        const uint32_t m = off[j + 1] - off[j];
        uint32_t *ms = (uint32_t *)malloc(((size_t)m + 1) * sizeof(uint32_t));
        uint32_t e = 0, lo, hi;
        for (uint32_t b = 0; b < m; ++b) {
            if (e < b) e = b;
            while (e < m) {
                rows_of(x, n, sa, P + b, e + 1 - b, &lo, &hi);
                if (lo >= hi) break;
                ++e;
            }
            ms[b] = e - b;
        }
        nmems[j] = nocc[j] = 0;
        for (uint32_t b = 0; b < m; ++b) {
            if (!ms[b] || (b && b - 1 + ms[b - 1] >= b + ms[b])) continue;
            const uint32_t end = b + ms[b];
            ++found;
            fwd += end < m ? ms[b] : ms[b] - 1;
            if (end < m) {
                uint32_t nb = b + 1;
                while (nb <= end && nb + ms[nb] <= end) ++nb;       /* (nb <= end < m: ms[nb] exists) */
                if (nb <= end) bwd += nb > b + 1 ? end - nb + 1 : end - nb;
            }
            if (ms[b] < min_len) continue;
            rows_of(x, n, sa, P + b, ms[b], &lo, &hi);
            if (total >= cap) { free(ms); return -1; }
            mems[total].lo = lo;
            mems[total].hi = hi;
            mems[total].start = b;
            mems[total].end = end;
            mems[total].pattern = j;
            mems[total].reserved0 = 0;
            ++total;
            ++nmems[j];
            nocc[j] += hi - lo;
        }
        free(ms);
    }
    counters[0] = fwd;
    counters[1] = bwd;
    counters[2] = found;
    return (int64_t)total;
}
