/*
 * fm_naive.c -- TEST HELPER: the expected answers of the FM index (include/archon_hip.h, archon_hip_fm_*) on the CPU,
 * straight from the text, by a Knuth-Morris-Pratt scan of x per pattern.  Pattern j = pat[off[j] .. off[j+1]) of length m:
 *   count[j]   the starts p with x[p .. p+m) == P and 1 <= p + m <= n (for m = 0: p = 1 .. n, the rows [0, n))
 *   L[j]       the longest prefix of P that occurs in x (0 for m = 0)
 *   starts     when not NULL: every pattern's starts in ascending order, one pattern after the other (cap entries at most)
 * Returns the number of starts of all patterns (whether or not they fit), or -1 when a table cannot be allocated.
 */
#include <stdint.h>
#include <stdlib.h>

int64_t fm_naive(const uint8_t *x, uint32_t n, const uint8_t *pat, const uint32_t *off, uint32_t k, uint32_t *count, uint32_t *L,
                 uint32_t *starts, uint64_t cap)
{
    uint64_t total = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const uint8_t *P = pat + off[j];
        const uint32_t m = off[j + 1] - off[j];
        uint32_t cnt = 0, best = 0;
        if (m == 0) {
            for (uint32_t p = 1; p <= n; ++p, ++cnt)
                if (starts && total + cnt < cap) starts[total + cnt] = p;
        } else {
            uint32_t *fail = malloc(4ull * m);
            if (!fail) return -1;
            fail[0] = 0;
            for (uint32_t i = 1, q = 0; i < m; ++i) {       /* fail[i]: longest proper border of P[0 .. i] */
                while (q && P[i] != P[q]) q = fail[q - 1];
                if (P[i] == P[q]) ++q;
                fail[i] = q;
            }
            for (uint32_t i = 0, q = 0; i < n; ++i) {       /* q: longest prefix of P that ends at x[i] */
                if (q == m) q = fail[q - 1];
                while (q && x[i] != P[q]) q = fail[q - 1];
                if (x[i] == P[q]) ++q;
                if (q > best) best = q;
                if (q == m) {
                    if (starts && total + cnt < cap) starts[total + cnt] = i + 1 - m;
                    ++cnt;
                }
            }
            free(fail);
        }
        count[j] = cnt;
        L[j] = best;
        total += cnt;
    }
    return (int64_t)total;
}
