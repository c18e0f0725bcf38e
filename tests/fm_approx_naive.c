/*
 * fm_approx_naive.c -- TEST HELPER: the expected answers of the approximate FM search (include/archon_hip.h,
 * archon_hip_fm_approx) on the CPU, straight from the text.  Pattern P of length m >= 1 at distance K:
 *   the hits        the distinct strings w = x[p .. p+m), p + m <= n, with Hamming distance d(w, P) <= K
 *   *expansions     sum over t = 1 .. m-1 of the distinct u = x[p .. p+t) with d(u, P[0 .. t)) <  K
 *   *steps          sum over t = 1 .. m-1 of the distinct u = x[p .. p+t) with d(u, P[0 .. t)) == K
 *   *nhits          the number of distinct hits
 *   starts, group   when not NULL (cap entries at most): every hit's starts, sorted by (w, p); group[i] numbers the distinct
 *                   string of starts[i] (0, 1, ... in the byte order of the strings)
 * One pass over the starts p extends d(x[p .. p+t), P[0 .. t)) with t until it passes K; the distinct strings of one length
 * are counted by sorting their starts.  Returns the number of starts of all hits, or -1 when a list cannot be allocated.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static const uint8_t *g_x;
static uint32_t g_len;

static int by_string(const void *a, const void *b)
{
    const uint32_t p = *(const uint32_t *)a, q = *(const uint32_t *)b;
    const int c = memcmp(g_x + p, g_x + q, g_len);
    return c ? c : (p > q) - (p < q);
}

typedef struct {
    uint32_t *v;
    uint64_t n, cap;
} list;

static int push(list *l, uint32_t p)
{
    if (l->n == l->cap) {
        const uint64_t c = l->cap ? 2 * l->cap : 64;
        uint32_t *v = realloc(l->v, c * 4);
        if (!v) return -1;
        l->v = v;
        l->cap = c;
    }
    l->v[l->n++] = p;
    return 0;
}

/* sorts the starts of l by their strings of length t; returns the number of distinct strings */
static uint64_t distinct(const uint8_t *x, list *l, uint32_t t)
{
    if (!l->n) return 0;
    g_x = x;
    g_len = t;
    qsort(l->v, l->n, 4, by_string);
    uint64_t d = 1;
    for (uint64_t i = 1; i < l->n; ++i) d += memcmp(x + l->v[i - 1], x + l->v[i], t) != 0;
    return d;
}

int64_t fma_naive(const uint8_t *x, uint32_t n, const uint8_t *P, uint32_t m, uint32_t K, uint64_t *expansions, uint64_t *steps,
                  uint64_t *nhits, uint32_t *starts, uint32_t *group, uint64_t cap)
{
    *expansions = *steps = *nhits = 0;
    if (m == 0 || m > n) return 0;
    list *below = calloc(m, sizeof(list)), *at = calloc(m, sizeof(list));     /* [t]: starts with d < K, d == K at length t */
    list hits = {0, 0, 0};
    int64_t rc = 0;
    if (!below || !at) { rc = -1; goto out; }
    for (uint32_t p = 0; p < n && rc == 0; ++p) {
        uint32_t d = 0;
        for (uint32_t t = 1; t <= m && p + t <= n; ++t) {
            d += x[p + t - 1] != P[t - 1];
            if (d > K) break;
            if (t == m) {
                if (push(&hits, p)) rc = -1;
            } else if (push(d < K ? &below[t] : &at[t], p)) {
                rc = -1;
            }
        }
    }
    if (rc) goto out;
    for (uint32_t t = 1; t < m; ++t) {
        *expansions += distinct(x, &below[t], t);
        *steps += distinct(x, &at[t], t);
    }
    *nhits = distinct(x, &hits, m);
    rc = (int64_t)hits.n;
    if (starts && group) {
        uint32_t g = 0;
        for (uint64_t i = 0; i < hits.n && i < cap; ++i) {
            if (i && memcmp(x + hits.v[i - 1], x + hits.v[i], m)) ++g;
            starts[i] = hits.v[i];
            group[i] = g;
        }
    }
out:
    for (uint32_t t = 0; below && at && t < m; ++t) {
        free(below[t].v);
        free(at[t].v);
    }
    free(below);
    free(at);
    free(hits.v);
    return rc;
}
