/*
 * lcp_kasai.c -- TEST HELPER: the LCP array of a suffix array in a7 order on the CPU, the expected answer of
 * archon_hip_lcp (include/archon_hip.h).  Kasai's pass over items s = n .. 1, as tools/lcp_stats.c does it: the key of
 * item s is x[s-1], x[s-2], ..., x[0], INF, and key(s-1) is key(s) without its first byte, so the lcp of the row holding
 * s-1 is at least that of the row holding s, minus one.  sa must be a permutation of 1..n.
 * Returns 0, or -1 when the rank table cannot be allocated.
 */
#include <stdint.h>
#include <stdlib.h>

int lcp_kasai(const uint8_t *x, uint32_t n, const uint32_t *sa, uint32_t *lcp)
{
    uint32_t *rank = malloc(4ull * ((uint64_t)n + 1));
    if (!rank) return -1;
    for (uint32_t i = 0; i < n; ++i) rank[sa[i]] = i;
    uint32_t l = 0;
    for (uint32_t s = n; s >= 1; --s) {
        const uint32_t r = rank[s];
        if (r == 0) { lcp[0] = 0; l = 0; continue; }
        const uint32_t t = sa[r - 1];
        while (l < s && l < t && x[s - 1 - l] == x[t - 1 - l]) ++l;
        lcp[r] = l;
        if (l) --l;
    }
    free(rank);
    return 0;
}
