/* The expected answer of the LZ tests (TEST INFRASTRUCTURE ONLY): the longest previous factor of every item from (sa, lcp,
 * dir) by the definition of include/archon_hip.h with two stacks -- one sweep over the rows from the left for (p, L), one from
 * the right for (q, R) --, and the parse as a plain walk.  Deliberately not the library's algorithm (two minimum hierarchies
 * and one tree walk per side; tiles of first-node-below pointers).
 *
 * A sweep keeps a stack of (item, m): the rows seen so far that can still be the nearest admissible row of a later one, each
 * with the minimum of lcp between the entry below it (exclusive) and itself.  A row pops every entry that is not admissible
 * for its item, folding their minima into its own; what is left on top is its nearest admissible row. */
#include <stdint.h>
#include <stdlib.h>

typedef struct { uint32_t len, src; } lpf_t;
typedef struct { uint32_t end, len, src; } phrase_t;
typedef struct { uint32_t item, m; } frame_t;

static int admissible(uint32_t t, uint32_t s, uint32_t dir) { return dir ? t > s : t < s; }

/* side[s - 1] = (min, item of the nearest admissible row) seen from the left (reverse 0) or from the right (reverse 1) */
static int sweep(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t dir, int reverse, lpf_t *side)
{
    frame_t *st = malloc((size_t)n * sizeof *st);
    size_t depth = 0;
    if (!st) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t row = reverse ? n - 1 - i : i;
        const uint32_t s = sa[row];
        /* lcp between this row and the one swept before it: lcp[row] from the left, lcp[row + 1] from the right */
        uint32_t m = i == 0 ? 0 : reverse ? lcp[row + 1] : lcp[row];
        while (depth && !admissible(st[depth - 1].item, s, dir)) {
            --depth;
            if (st[depth].m < m) m = st[depth].m;
        }
        if (depth && m > 0) {
            side[s - 1].len = m;
            side[s - 1].src = st[depth - 1].item;
        } else {
            side[s - 1].len = side[s - 1].src = 0;
        }
        st[depth].item = s;
        st[depth].m = m;
        ++depth;
    }
    free(st);
    return 0;
}

/* out[s - 1] = the record of item s; every sa value must lie in 1..n.  Returns 0, or -1 when memory runs out */
int lpf_naive(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t dir, lpf_t *out)
{
    lpf_t *right = malloc((size_t)n * sizeof *right);
    if (!right) return -1;
    if (sweep(sa, lcp, n, dir, 0, out) || sweep(sa, lcp, n, dir, 1, right)) { free(right); return -1; }
    for (uint32_t k = 0; k < n; ++k) {
        const lpf_t L = out[k], R = right[k];
        if (L.len >= R.len && L.len > 0) out[k] = L;
        else if (R.len > 0) out[k] = R;
        else out[k].len = out[k].src = 0;
    }
    free(right);
    return 0;
}

/* the phrases of the len words of lpf[n], the one ending at n first: returns their number, the first cap of them in out (may be
 * NULL with cap 0) */
int64_t parse_naive(const lpf_t *lpf, uint32_t n, phrase_t *out, uint64_t cap)
{
    uint64_t z = 0;
    for (uint32_t e = n; e > 0;) {
        const uint32_t len = lpf[e - 1].len;
        uint32_t step = len ? len : 1;
        if (step > e) step = e;
        if (z < cap) out[z] = (phrase_t){e, len, lpf[e - 1].src};
        ++z;
        e -= step;
    }
    return (int64_t)z;
}
