/*
 * archon_hip_test.h -- TEST-ONLY entry point of libarchon_hip.so.
 *
 * The forward / inverse pipelines choose between several routes (streaming first stage or 7-pass sort, alphabet
 * compaction, run shortcut, text rounds, pair chains, rank writer, ...), every one of which yields the same a7 order
 * (SURVEY.md 8(a0)).  The tests force each of them in turn through this call; the product never does, and the library
 * reads no routing from the environment of whoever links it.  Not part of the drop-in boundary (include/archon_hip.h).
 *
 *   name      value
 *   RESET     -            every knob back to its default
 *   FORCE_PATH   0 / 1 / -1   7-pass first stage / streaming first stage / the block decides
 *   PASS_RANGES  1..1024 / 0  ranges the streaming passes are cut into (0: one per CU)
 *   SMALL_BLOCK  bytes / -1   blocks below this size take the byte count + LSB passes instead of the streaming stage (-1: 8 MiB)
 *   ALIGNED_MIN  bytes / -1   blocks from this size on may run pass B in bucket mode (-1: 16 MiB)
 *   REL_MIN_SEG  places / -1  bucket mode moves range-relative records when a bucket's segments average at least this many places (-1: 4096)
 *   KEY_BYTES    3..6 / 0     7-pass first stage: key bytes the LSB passes sort on (0, or any other value: the library's own choice)
 *   INV_SLAB, INV_SBITS, INV_WALK_WGS   inverse: slab bytes per chain, log2 rows per chain head, walk workgroups per CU.
 *                                       INV_SBITS is clamped to 3..12 (any value >= 0 counts as set; negative: the product's rule).
 *                                       INV_SLAB is cut to a multiple of 16 and taken only where it is at least 16 and below the
 *                                       default of 16 << sbits.  INV_WALK_WGS = 0 means one chain per lane (k_walk_store whatever
 *                                       the number of chains and INV_ROWS); 1.. = workgroups of 512 lanes per CU of the queue and
 *                                       rows walks (128-byte rows take at most 2); negative: the product's 3
 *   INV_ROWS                            inverse: 0 = every lane of the walk stores its own 16 bytes, 1 / 2 = slabs written by quads through
 *                                       128- / 64-byte rows of LDS, -1 = the product's rule (rows above 128 MiB)
 *   LCP_CAP      1..4096 / 0  LCP: key bytes a lane of stage A compares before a row goes to the long list (0: 32)
 *   LCP_WINDOW   bytes / 0    LCP: the first window of the long comparisons, doubled every round (0: 256; at most 2^30)
 *   FM_SUB_ROWS    16..1024 / 0   FM index: rows of a sub-chunk of the rank table, a power of two (0: 1024)
 *   FM_SUPER_ROWS  ..65536 / 0    FM index: rows of a superblock, a power of two, a multiple of the sub-chunk (0: 65536; checked
 *                                 when a table is built).  Neither changes a result: tiny blocks cross many table boundaries
 *   FM_SAMPLE_WALK 0 / nonzero    sampled FM index: nonzero makes archon_hip_block_fm_index take the LF walk route even when the
 *                                 block's SA is resident (the walk route honours INV_SBITS; it stores no slabs, so INV_SLAB has
 *                                 nothing to change there).  Neither route changes a sample
 *   REP_FAN        2..64 / 0      repeats: fan-out of the minimum hierarchy over lcp, a power of two (0: 16).  It changes no result:
 *                                 at 2, blocks of seven bytes cross three levels
 *   LZ_FAN         2..64 / 0      LZ: fan-out of the two hierarchies of the LPF pass, a power of two (0: 16).  It changes no result
 *   LZ_TILE        2..4096 / 0    LZ: items of a tile of the parse, a power of two (0: 256).  It changes no result: at 2, blocks of
 *                                 seven bytes cross three parse levels
 *   KMER_TILE      4..2048 / 0    k-mers: rows of a tile of the passes (and groups of a tile of the group passes), a power of two
 *                                 (0: 2048).  It changes no result: at 4, blocks of seven bytes cross a tile boundary, and
 *                                 65536 rows at 16 give every lane of the tile scan four words
 *   MS_CHUNK       1.. / 0        text matching statistics: bytes of a chunk of the walk, any C >= 1 (0: 1024).  It changes no
 *                                 record: at 1 every end after the first is a join
 *   EDIT_TILE      1..64 / 0      edit-distance search: ends a tile owns, W (0: 32).  A call whose K makes W + 2K > 64 is ARCHON_E_ARG.
 *                                 It changes no match: at 1 every end is a tile of its own
 *   EDIT_BATCH     1.. / 0        edit-distance search: patterns of a batch at most (0: what the scratch budget holds).  It changes
 *                                 no match: at 1 every pattern is marked, swept and checked alone
 *   DOC_TILE       64..2^20 / 0   document listing: rows of a tile, a multiple of 64 (0: 4096).  It changes no record: at 64 a range of
 *                                 65 rows is two tiles
 *   STRIDE_GRID    1..2048 / 0    analyses (FM count / locate / walk, approximate, class, edit, SMEM, matching statistics, text MS /
 *                                 RLZ, document listing, repeats, LZ, k-mers, MAW, entropy, runs / LCE): the most workgroups a stride
 *                                 kernel is launched with (0: 2048; k_fm_locate keeps its own 8192 where that is less).  It changes no
 *                                 result and no counter: at 1 one workgroup (four waves) takes every tile and every pattern.  No
 *                                 kernel of these families waits on another workgroup.  The entropy sums are added per tile in tile
 *                                 order (k_ent_follow fills one slot per tile, k_ent_reduce adds the slots in a fixed order), so
 *                                 `bits` is the same 64 bits at every grid
 *   NO_ALIGNED NO_BREAK_ROUND NO_CHAINS NO_PACK NO_PAIR_CHAINS NO_PERIOD_HINT NO_PERIOD_STREAM NO_RANK_WRITER NO_TEXT_ROUNDS
 *   NO_MID NO_SHALLOW NO_CLOSED_FORM NO_REL_RECORDS      nonzero switches the named step off
 * Returns 0, or ARCHON_E_ARG for an unknown name / a value out of range.  Process-wide; not thread-safe against
 * concurrent transforms (tests run one at a time).
 */
#ifndef ARCHON_HIP_TEST_H
#define ARCHON_HIP_TEST_H
#ifdef __cplusplus
extern "C" {
#endif
int archon_hip_test_route(const char *name, long value);
#ifdef __cplusplus
}
#endif
#endif
