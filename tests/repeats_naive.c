/* The expected answer of the repeats tests (TEST INFRASTRUCTURE ONLY): the LCP intervals of a block by the usual one-pass
 * stack enumeration over its LCP array, each with the set of its rows' following bytes, so that the two maximality tests
 * are questions to that set.  Deliberately not the library's algorithm (nearest smaller values in a minimum hierarchy).
 *
 * Conventions of include/archon_hip.h: lcp[k] belongs to rows k-1 and k, lcp[0] is read as 0; bwt[r] is the byte that
 * follows row r's occurrence, the primary row `base` has none.  An interval (lo, hi, len) is reported when the boundary
 * that closes it is reached; its representative row is the boundary that opened it (the first row in (lo, hi) that holds len).
 *   kind 0  every interval
 *   kind 1  its following bytes are not all equal (two different bytes, or the primary row among at least two rows)
 *   kind 2  kind 1, no interval inside it (every inner lcp equals len), no byte twice
 * The output is sorted by representative row. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { uint32_t lo, hi, len, row; } rep_t;

typedef struct {
    uint32_t len, lo, row;
    uint64_t set[4];        /* following bytes of the rows gathered so far (the primary row apart) */
    int twice;              /* some byte follows two of them */
    int primary;            /* the primary row is one of them */
    int child;              /* an interval lies inside */
} frame_t;

static void add_row(frame_t *f, const uint8_t *bwt, uint32_t base, uint32_t r)
{
    if (r == base) { f->primary = 1; return; }
    const uint64_t bit = 1ull << (bwt[r] & 63);
    if (f->set[bwt[r] >> 6] & bit) f->twice = 1;
    f->set[bwt[r] >> 6] |= bit;
}

static void merge(frame_t *into, const frame_t *f)
{
    for (int w = 0; w < 4; ++w) {
        if (into->set[w] & f->set[w]) into->twice = 1;
        into->set[w] |= f->set[w];
    }
    into->twice |= f->twice;
    into->primary |= f->primary;
    into->child = 1;
}

static int distinct_bytes(const frame_t *f)
{
    int c = 0;
    for (int w = 0; w < 4; ++w) c += __builtin_popcountll(f->set[w]);
    return c;
}

static int by_row(const void *a, const void *b)
{
    const rep_t *p = a, *q = b;
    return p->row < q->row ? -1 : p->row > q->row;
}

/* returns the number of repeats that pass kind and filters (min_len 0 as 1, min_occ 0 and 1 as 2), the first cap of them in
 * representative-row order in out (may be NULL with cap 0); counters[0] = all intervals, [1] = rows summed over the repeats,
 * [2] = the longest repeat; -1 when memory runs out */
int64_t repeats_naive(const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base, uint32_t kind, uint32_t min_len,
                      uint32_t min_occ, rep_t *out, uint64_t cap, uint64_t *counters)
{
    size_t room = 1024, depth = 0, found = 0, found_room = 1024;
    frame_t *st = malloc(room * sizeof *st);
    rep_t *all = malloc(found_room * sizeof *all);
    if (!st || !all) return -1;
    if (min_len < 1) min_len = 1;
    if (min_occ < 2) min_occ = 2;
    counters[0] = counters[1] = counters[2] = 0;
    memset(&st[0], 0, sizeof st[0]);        /* the root: len 0, never closed */
    depth = 1;
    for (uint32_t i = 1; i <= n; ++i) {
        const uint32_t cur = i < n ? lcp[i] : 0;
        frame_t *top = &st[depth - 1];
        if (cur > top->len) {               /* row i-1 opens an interval with row i */
            if (depth == room) {
                room *= 2;
                st = realloc(st, room * sizeof *st);
                if (!st) return -1;
            }
            frame_t *f = &st[depth++];
            memset(f, 0, sizeof *f);
            f->len = cur;
            f->lo = i - 1;
            f->row = i;
            add_row(f, bwt, base, i - 1);
            continue;
        }
        add_row(top, bwt, base, i - 1);     /* row i-1 is the last row of the deepest open interval */
        while (cur < st[depth - 1].len) {
            const frame_t f = st[--depth];
            const uint32_t hi = i;
            ++counters[0];
            int ok = f.len >= min_len && hi - f.lo >= min_occ;
            const int maximal = distinct_bytes(&f) + f.primary >= 2;
            if (kind >= 1) ok = ok && maximal;
            if (kind == 2) ok = ok && !f.child && !f.twice;
            if (ok) {
                if (found == found_room) {
                    found_room *= 2;
                    all = realloc(all, found_room * sizeof *all);
                    if (!all) return -1;
                }
                all[found++] = (rep_t){f.lo, hi, f.len, f.row};
                counters[1] += hi - f.lo;
                if (f.len > counters[2]) counters[2] = f.len;
            }
            if (cur > st[depth - 1].len) {  /* what was closed is the first part of a shallower interval that opens here */
                frame_t *g = &st[depth++];  /* (the slot just vacated) */
                const frame_t inner = f;
                memset(g, 0, sizeof *g);
                g->len = cur;
                g->lo = inner.lo;
                g->row = i;
                merge(g, &inner);
                break;
            }
            merge(&st[depth - 1], &f);
        }
    }
    qsort(all, found, sizeof *all, by_row);
    for (size_t k = 0; k < found && k < cap; ++k) out[k] = all[k];
    free(all);
    free(st);
    return (int64_t)found;
}
