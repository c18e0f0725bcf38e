/*
 * archon_hip.h -- C ABI of libarchon_hip.so: the MI355X (gfx950) kernels behind
 * the Archon a7 BWT hot path.  Plain pointers and sizes, no exceptions, no
 * torch/HIP types in any signature (a HIP stream crosses as void*).
 *
 * What each entry point replaces in kvark/dark-archon (paths under bwt/a7/src):
 *
 *   archon_hip_forward      Archon::enCompute (archon.cpp:882-885 -> Constructor<byte>
 *                           784-819) + the gather loop of Archon::enWrite (887-900)
 *   archon_hip_inverse      Archon::deCompute (917-935) + the LF walk of Archon::deWrite (937-943)
 *   archon_hip_hist256      Constructor::makeBuckets (118-126); tool/radix_dir/radix.c:31-36
 *   archon_hip_validate     Archon::validate (862-874)
 *   archon_hip_sa_to_bwt    the gather loop of Archon::enWrite alone (887-900), for a caller's own SA
 *   archon_hip_radix_scatter  the counting-sort scatter of tool/radix_dir/radix.c:40-44
 *   archon_hip_lms_select   Constructor::findLMS (160-172): the subset a7 sorts directly (a4 IT-2: bwt/a4/src/archon.c:163-169)
 *   archon_hip_lcp          nothing: the LCP array of the suffix array, below
 *   archon_hip_fm_*         nothing: counting and locating patterns by backward search on the BWT (an FM index), below;
 *                           with a sampled SA and ISA it locates and extracts without the block's suffix array, and it
 *                           finds patterns with up to K substituted bytes (archon_hip_fm_approx)
 *                           and with up to K substituted, inserted or deleted bytes (archon_hip_fm_edit), and patterns
 *                           whose positions each accept a set of bytes (archon_hip_fm_classes)
 *   archon_hip_fm_smems     nothing: the super-maximal exact matches of patterns, with a mirror index (archon_hip_fm_mirror)
 *   archon_hip_fm_ms        nothing: the matching statistics of patterns -- for every position the longest piece ending there
 *                           that occurs, and its rows -- with the block's LCP array beside the index (archon_hip_fm_attach_lcp)
 *   archon_hip_repeats*     nothing: the LCP intervals, maximal and supermaximal repeats of a block from its LCP array and BWT
 *   archon_hip_lpf*, _lz_*  nothing: the longest previous factor of every item and the LZ77 parse, from the SA and LCP array
 *   archon_hip_kmers*, _kmer_occ*, _sus*   nothing: the k-mers of a block with their counts, the count of the k-mer at every
 *                           position and the shortest unique substring ending at every item, from the SA and LCP array
 *   archon_hip_maws*        nothing: the minimal absent words of a block, from the SA, the LCP array and the BWT
 *   archon_hip_entropy*, _complexity*   nothing: the order-k statistics and entropy of a block, its substring complexity and the
 *                           runs of its BWT, from the SA, the LCP array and the BWT
 *
 * Ordering convention ("a7 order"): item s in 1..N names the
 * reversed prefix x[s-1],x[s-2],...,x[0],INF with INF > 255; sa[0..N) lists the
 * items in ascending key order; bwt[i] = x[sa[i]] (x[0] where sa[i]==N);
 * *base_id = the i with sa[i]==N.
 *
 * Error model: 0 = ok, negative = ARCHON_E_* below (the reference returns int
 * from every Archon method, archon.h:16-28).  The library owns device memory and
 * streams: up to eight compute contexts per device (arena, staging buffers, stream each:
 * about 145 MB of fixed tables plus 27 N .. 96 N of arena for the largest block it has
 * seen, kept until archon_hip_release), created lazily.  A host thread is bound to one
 * context PER DEVICE: the k-th thread that comes to device d takes context k mod 2 of
 * that device (threads never spread over more than two by themselves), or the one it
 * names with archon_hip_bind_context (0..7: the batch entry points and the container's
 * worker pools do).  One thread sees strictly serial behaviour; two
 * threads feeding one GPU overlap one block's copies with the other's kernels;
 * separate devices run concurrently.  A context holds NO results between calls:
 * what outlives a call (the resident block of a block-coder object) belongs to an
 * archon_hip_block handle, and the statistics of a call to the thread that made it.
 * Callers own every buffer they pass.  There is NO CPU fallback: without a HIP
 * device every compute entry point returns ARCHON_E_NODEVICE.
 *
 * Limits: 1 <= n <= ARCHON_HIP_MAX_N (the reference needs n < 2^30 for its
 * default tracking path, archon.cpp:802).
 */
#ifndef ARCHON_HIP_H
#define ARCHON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARCHON_HIP_MAX_N      0x3FFFFF00u

#define ARCHON_OK             0
#define ARCHON_E_ARG        (-1)   /* null pointer / n out of range / bad base_id */
#define ARCHON_E_NODEVICE   (-2)   /* no HIP device, or dev out of range */
#define ARCHON_E_NOMEM      (-3)   /* device or host allocation failed */
#define ARCHON_E_HIP        (-4)   /* a HIP runtime call failed (see archon_hip_last_error) */
#define ARCHON_E_INTERNAL   (-5)   /* device-side consistency flag raised (e.g. look-back spin bound) */
#define ARCHON_E_CORRUPT    (-6)   /* inverse: LF walk does not close (not a BWT of this format) */

/* number of HIP devices visible (0 when none); never fails */
int archon_hip_device_count(void);

/* human-readable text for the last error raised on the calling thread */
const char *archon_hip_last_error(void);

/* ---- host-buffer entry points (what the C host / cgo-style bindings call) ---- */

/* x[n] -> sa (optional, may be NULL), bwt[n], *base_id.  All host pointers. */
int archon_hip_forward(const uint8_t *x, uint32_t n, uint32_t *sa_or_null,
                       uint8_t *bwt, uint32_t *base_id, int dev);

/* ---- resident blocks: the device side of ONE block-coder object (class Archon, bwt/a7/src/archon.h:8-29) ----------
 * The reference's caller runs read -> enCompute -> validate -> enWrite on one object (main.cpp:39-46), and the host
 * must stay within 5N + O(1) bytes.  So enCompute leaves the block, its suffix array and its BWT resident in HBM, in
 * buffers that belong to the handle (6N device bytes): validate then checks what is there (no upload; the resident BWT
 * is compared with its gather x[sa[i]] row by row), enWrite reads the BWT back in pieces through any O(1) bounce buffer.  Any number of handles,
 * on any threads; a handle is used by one thread at a time (as an Archon object is: a7 is re-entrant per object). */
typedef struct archon_hip_block archon_hip_block;
int  archon_hip_block_create(int dev, archon_hip_block **out);
void archon_hip_block_destroy(archon_hip_block *b);
/* Archon::enCompute (archon.cpp:882-885): x[n] (host) -> sa[n] (host, optional) and *base_id; x, SA, BWT stay resident */
int  archon_hip_block_forward(archon_hip_block *b, const uint8_t *x, uint32_t n, uint32_t *sa_or_null, uint32_t *base_id);
/* the gather loop of Archon::enWrite (archon.cpp:887-900), already done on the device: bytes [offset, offset+len) of the BWT */
int  archon_hip_block_read_bwt(archon_hip_block *b, uint32_t offset, uint32_t len, uint8_t *dst);
/* Archon::validate (archon.cpp:862-874) on the resident block, by archon_hip_validate_resident_dev: 1 if and only if the
 * resident SA is the a7 suffix array of the resident block, the resident BWT its BWT and the primary index its row of n;
 * 0 = not, <0 = error (ARCHON_E_ARG when the last forward on the handle kept no suffix array). */
int  archon_hip_block_validate(archon_hip_block *b);
/* (archon_hip_stats is defined under "measurement" below) */
struct archon_hip_stats;
int  archon_hip_block_stats(archon_hip_block *b, struct archon_hip_stats *out);      /* of the handle's last forward */

/* The same keyed by device, on a default handle that belongs to the CALLING THREAD (so two threads never see each
 * other's BWT): forward_keep = block_forward, read_bwt = block_read_bwt, validate_keep = block_validate. */
int archon_hip_forward_keep(const uint8_t *x, uint32_t n, uint32_t *sa_or_null,
                            uint32_t *base_id, int dev);
int archon_hip_read_bwt(int dev, uint32_t offset, uint32_t len, uint8_t *dst);
int archon_hip_validate_keep(int dev);

/* pinned host memory for block buffers (faster PCIe copies); plain malloc works too */
void *archon_hip_host_alloc(size_t bytes);
void archon_hip_host_free(void *p);

/* bwt[n] + base_id -> x_out[n].  All host pointers. */
int archon_hip_inverse(const uint8_t *bwt, uint32_t n, uint32_t base_id,
                       uint8_t *x_out, int dev);

/* 256-bin histogram of x[n] (host pointers). */
int archon_hip_hist256(const uint8_t *x, size_t n, uint32_t out[256], int dev);

/* Archon::validate, stricter: returns 1 if and only if sa is the a7 suffix array of x, 0 = not, <0 = error.
 * The check: every sa[i] in 1..n, exactly one row holds n (the primary row), and with bwt[i] = x[sa[i]] (x[0] on the
 * primary row) the LF rule sa[T[i]] == sa[i] + 1 on every other row, T the LF table of (bwt, primary row).  Its buckets
 * come from the byte counts in byte order with the primary row ranked last in its bucket, so it pins the order itself:
 * the counts fix the first column, each LF step extends the sorted prefix by one byte, the end of the string sorts last.
 * (a7's own Archon::validate takes its buckets from sa and accepts some permutations that are not the suffix array.) */
int archon_hip_validate(const uint8_t *x, uint32_t n, const uint32_t *sa, int dev);

/* SA -> BWT + primary index for a suffix array the caller already holds (Archon::enWrite, archon.cpp:887-900):
 * bwt[i] = x[sa[i]] (x[0] where sa[i]==n), *base_id = the row holding n.  ARCHON_E_CORRUPT when sa holds a value
 * outside 1..n or not exactly one n. */
int archon_hip_sa_to_bwt(const uint8_t *x, uint32_t n, const uint32_t *sa, uint8_t *bwt, uint32_t *base_id, int dev);

/* The subset the reference sorts directly: a7's LMS items, Constructor::findLMS (archon.cpp:160-172;
 * a4's IT-2 rule, bwt/a4/src/archon.c:163-169, is the same step in a4's convention).  count[c] = LMS items whose first
 * key byte x[i-1] is c; items[] = the buckets' tails one after the other as a7 fills them (P[--RE[c]] = i: ascending
 * slots hold decreasing items); *n1 = their number (<= n/2: items must hold n/2 + 8 words).  The GPU sorter itself
 * sorts all N items -- this is the bucket-setup step as an operator of its own. */
int archon_hip_lms_select(const uint8_t *x, uint32_t n, uint32_t count[256], uint32_t *items, uint32_t *n1, int dev);

/* dst = src stably sorted by byte value (tool/radix_dir scatter), host pointers. */
int archon_hip_radix_scatter(const uint8_t *src, size_t n, uint8_t *dst, int dev);

/* ---- device-resident entry points (inputs already in HBM) ---------------------
 * Every pointer is a device pointer on device `dev`; `stream` is a hipStream_t
 * passed as void* (NULL = the context's own stream).  Work is enqueued on that
 * stream; the forward/inverse pipelines contain host-side decision points
 * (number of unresolved suffix groups), so these calls synchronise the stream
 * internally and the outputs are complete when they return. */
int archon_hip_forward_dev(const uint8_t *d_x, uint32_t n, uint32_t *d_sa_or_null,
                           uint8_t *d_bwt, uint32_t *d_base_id, int dev, void *stream);
int archon_hip_inverse_dev(const uint8_t *d_bwt, uint32_t n, uint32_t base_id,
                           uint8_t *d_x_out, int dev, void *stream);
int archon_hip_hist256_dev(const uint8_t *d_x, size_t n, uint32_t *d_out256, int dev, void *stream);
int archon_hip_validate_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, int dev, void *stream);
/* Archon::validate for a caller that holds the forward pass's outputs on the device: returns 1 if and only if d_sa is the
 * a7 suffix array of d_x, d_bwt its BWT and base_id its primary index (the row that holds n); 0 = not, <0 = error.  The LF
 * table is built from d_bwt, and one sweep checks archon_hip_validate_dev's rules together with d_bwt[i] == d_x[d_sa[i]]
 * (d_x[0] on the primary row) -- the same rows as archon_hip_validate_dev on d_x, plus the BWT and the primary index.  This
 * is what archon_hip_block_validate runs. */
int archon_hip_validate_resident_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, const uint8_t *d_bwt, uint32_t base_id,
                                     int dev, void *stream);
int archon_hip_sa_to_bwt_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, uint8_t *d_bwt, uint32_t *d_base_id,
                             int dev, void *stream);
int archon_hip_radix_scatter_dev(const uint8_t *d_src, size_t n, uint8_t *d_dst, int dev, void *stream);
/* d_items: n/2 + 8 words; *n1 is a HOST pointer (the count is needed on the host to size the launches) */
int archon_hip_lms_select_dev(const uint8_t *d_x, uint32_t n, uint32_t *d_count256, uint32_t *d_items, uint32_t *n1, int dev, void *stream);

/* ---- several small blocks per call (x3's block loop, bwt/final/x3/archon.c:120-142, at its default 4 MiB block) ------------
 * One small block cannot fill the chip: a batch call deals blocks x[0..count) of n[i] bytes to `workers` host threads inside
 * the library, each on a compute context of its own, so that the blocks' copies, kernels and launch gaps overlap
 * (workers <= 0: 8 for blocks up to 4 MiB, 4 up to 16 MiB, 2 beyond; at most 8).  Every block is an independent a7
 * transform with its own primary index; the first error stops the batch and is returned.  Host pointers; the _dev
 * forms take device pointers (d_sa_or_null: NULL, or one pointer per block, each NULL or a buffer of n[i] words). */
int archon_hip_forward_batch(const uint8_t *const *x, const uint32_t *n, uint32_t count, uint8_t *const *bwt, uint32_t *base_id, int dev, int workers);
int archon_hip_inverse_batch(const uint8_t *const *bwt, const uint32_t *n, const uint32_t *base_id, uint32_t count, uint8_t *const *x_out, int dev, int workers);
int archon_hip_forward_batch_dev(const uint8_t *const *d_x, const uint32_t *n, uint32_t count, uint32_t *const *d_sa_or_null, uint8_t *const *d_bwt,
                                 uint32_t *const *d_base_id, int dev, int workers);
int archon_hip_inverse_batch_dev(const uint8_t *const *d_bwt, const uint32_t *n, const uint32_t *base_id, uint32_t count, uint8_t *const *d_x_out, int dev, int workers);

/* ---- workspace / lifetime ---------------------------------------------------- */

/* Pre-size the arena of the calling thread's context on `dev` for blocks up to n bytes (optional; the arena grows on
 * demand; the thread that reserves should be the one that transforms, or have bound itself to the same context).
 * Returns bytes reserved via *bytes_or_null. */
int archon_hip_reserve(uint32_t n, int dev, size_t *bytes_or_null);

/* Bind the calling thread to compute context `slot` (0 .. 7; threads that do not ask are dealt to 0 and 1) of `dev` -- what a pool of workers does so that the two
 * workers of one GPU never share a context whatever order they start in (host/archon_container.cpp: worker w of G GPUs
 * drives GPU w mod G on context w / G).  Without it the k-th thread to reach a device gets context k mod 2 of that
 * device.  archon_hip_context_of_thread returns the binding (and makes the default one if there is none yet). */
int archon_hip_bind_context(int dev, int slot);
int archon_hip_context_of_thread(int dev);

/* Product options, per device; read by every transform on that device when it starts.
 *   "pass_ranges"     ranges the two streaming LSB passes are cut into: 0 = one per CU (default), 1..1024.  A pass workgroup
 *                     takes a whole CU: fewer ranges than CUs leave CUs to kernels that run beside the sort (RCCL's copy
 *                     kernels while an exchange overlaps the next blocks: bench.py asks for 224 at N > 1); more, shorter
 *                     ranges shorten the tail instead, at 9 % of the passes' speed.
 *   "pass_b_buckets"  1 (default): LSB pass B deals whole second-byte buckets, one per workgroup, when the block is
 *                     balanced; 0: always by ranges (every workgroup the same work: again for a chip that is shared).
 * Every setting yields the same output. */
int archon_hip_set_option(int dev, const char *name, long value);
int archon_hip_get_option(int dev, const char *name, long *value);

/* Free the device's contexts (arenas, staging buffers, streams, events). */
int archon_hip_release(int dev);

/* ---- the MTF + zero-run + order-0 Huffman stage of the container's `-m` blocks, on the device --------
 * PARITY UNPINNED: the reference has no such stage (kvark/dark-archon README.md:2 only promises "compression schemes
 * eventually"); dark-archon_amd/host/archon_post.cpp states the format, these entry points produce the same bytes.
 * Stream of a block: u32 pieces | u32 bytes of each piece | the pieces; a piece codes 32 KiB of the BWT:
 * u32 n | 258 code lengths | bits (LSB first). */
size_t archon_hip_post_bound(uint32_t n);      /* bytes the stream of an n-byte block can take at most */
/* BWT on the device -> its stream on the device; *out_bytes = the stream's length (returned after a stream sync) */
int archon_hip_post_encode_dev(const uint8_t *d_bwt, uint32_t n, uint8_t *d_out, size_t cap, size_t *out_bytes, int dev, void *stream);
/* host block -> forward BWT -> stream, host buffers: only the packed stream and the primary index come back over the link.
 * cap may be below archon_hip_post_bound(n): a stream longer than cap makes the call fail with ARCHON_E_ARG (nothing is cut). */
int archon_hip_forward_post(const uint8_t *x, uint32_t n, uint8_t *out, size_t cap, size_t *out_bytes, uint32_t *base_id, int dev);

/* the way back (round 4): a block's stream on the device -> its BWT on the device (d_bwt holds cap bytes); *n_out = the block's length
 * (host pointer; returned after a stream sync).  ARCHON_E_CORRUPT for a malformed stream. */
int archon_hip_post_decode_dev(const uint8_t *d_in, size_t in_bytes, uint8_t *d_bwt, uint32_t cap, uint32_t *n_out, int dev, void *stream);
/* host stream + primary index -> the block (x_out holds cap bytes), host buffers: stream decoded and BWT inverted on the device, only the
 * packed stream goes up the link */
int archon_hip_inverse_post(const uint8_t *in, size_t in_bytes, uint32_t base_id, uint8_t *x_out, uint32_t cap, uint32_t *n_out, int dev);

/* ---- the LCP array of a suffix array (no counterpart in the reference: what its users compute next) -------------------
 * lcp[0] = 0; for i >= 1, lcp[i] = the largest L such that the keys of items sa[i-1] and sa[i] agree in their first L
 * symbols, keys in a7 order as above (item s: x[s-1], x[s-2], ..., x[0], INF).  INF matches nothing, so
 * lcp[i] <= min(sa[i-1], sa[i]).  Orientation: for z[k] = 255 - x[n-1-k] (the block reversed, bytes complemented), item s
 * is z's suffix at n - s and ascending a7 order is DESCENDING lexicographic order of z's suffixes, so with SA_z and LCP_z
 * the textbook suffix and LCP arrays of z (LCP_z[k] = lcp of SA_z[k-1] and SA_z[k]): sa[i] = n - SA_z[n-1-i] and
 * lcp[i] = LCP_z[n-i] for i >= 1.  A caller who wants the textbook arrays of a text z passes x[k] = 255 - z[n-1-k].
 * Work: only rows where bwt[i] != bwt[i-1] (or that touch the item n, or row 0) compare key bytes; every other row follows
 * from the row of item sa[i] + 1 by the LF rule.  Those comparisons sum to at most 2 n log2 n bytes (Kärkkäinen, Manzini
 * and Puglisi, CPM 2009), and one row with a long lcp (a block of one repeated byte) runs over the whole device.
 * Bad input: an sa that is not a permutation of 1..n (a value outside 1..n, or one value twice) is refused with
 * ARCHON_E_CORRUPT before any key byte is compared.  A permutation that is not the a7 suffix array of x returns ARCHON_OK
 * with unspecified contents: every access stays inside x, sa and lcp.  Check sa with archon_hip_validate first when it is
 * not known to be right.  Workspace: about 8n bytes of the calling thread's context arena (grown on demand). */
/* host buffers; lcp[n] */
int archon_hip_lcp(const uint8_t *x, uint32_t n, const uint32_t *sa, uint32_t *lcp, int dev);
/* device pointers; enqueued on `stream` (NULL = the context's own) like archon_hip_validate_dev, complete on return.
 * d_lcp must not overlap d_x or d_sa (it is scratch of the call until its last kernel writes it). */
int archon_hip_lcp_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, uint32_t *d_lcp, int dev, void *stream);
/* the resident block of the handle's last forward (x, SA and BWT on the device; the BWT stands in for x[sa[i]]); lcp[n]
 * is a host buffer.  ARCHON_E_ARG when that forward kept no suffix array. */
int archon_hip_block_lcp(archon_hip_block *b, uint32_t *lcp);
/* the same on the calling thread's default block (archon_hip_forward_keep) */
int archon_hip_lcp_keep(int dev, uint32_t *lcp);
/* work counters and device time of the CALLING THREAD's last LCP call on `dev` (LCP calls leave archon_hip_stats alone) */
typedef struct archon_hip_lcp_stats {
    uint32_t n;                 /* block size of the call */
    uint32_t long_rounds;       /* rounds of the long comparisons (one host wait each) */
    uint32_t max_lcp;           /* the largest value of the array */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint64_t irreducible;       /* rows whose value was found by comparing key bytes */
    uint64_t long_items;        /* of them, rows that outgrew the per-lane cap K */
    uint64_t compared_bytes;    /* key bytes compared, all stages */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_total;             /* device time of the call (HIP events on its stream) */
} archon_hip_lcp_stats;
int archon_hip_get_lcp_stats(int dev, archon_hip_lcp_stats *out);

/* ---- patterns in a block's BWT: an FM index (no counterpart in the reference) ------------------------------------------
 * The search rule in a7 order.  An LF step prepends bwt[i] to a key, so a pattern P of length m is consumed in TEXT
 * order, P[0] first (not last, as in the textbook backward search):
 *   P[0] = c            [lo, hi) = [R[c], R[c+1]), R the starts of the 256 buckets counted over the BWT, primary row included
 *   each later P[t] = c [lo, hi) = [R[c] + occ'(c, lo), R[c] + occ'(c, hi)), occ'(c, i) = the rows j < i with bwt[j] == c,
 *                       the primary row EXCLUDED (it holds x[0] only as a stand-in: its item n has no item n + 1)
 *   stop as soon as lo >= hi.  Each later symbol is one rank step.
 * The occurrences are the rows r in [lo, hi), and P starts at offset sa[r] - m of x (every p with x[p .. p+m) == P and
 * 1 <= p + m <= n).  m = 0 gives [0, n) (starts 1 .. n); a pattern that does not occur gives lo == hi; a pattern longer than
 * the block gives lo == hi == 0 with no rank step.  Example: "banana" (BWT nnbaaa, primary row 2, sa = 2 4 6 1 3 5): "an"
 * gives [0, 3) then [4, 6), starts 1 and 3; "ab" is empty at its second step.
 * Table: superblocks of 65 536 rows hold R[c] + occ'(c, start) (u32), sub-chunks of 1024 rows hold counts relative to
 * their superblock (u16): 0.5 n + n / 64 bytes plus one entry for i = n, beside the BWT as it is.  A rank step reads the
 * two table entries of lo and of hi and counts the rest in the 1024 BWT bytes of their sub-chunk (one load when lo and hi
 * share it).  Ranges stay inside [0, n] for any bytes: a BWT that is not a BWT returns ARCHON_OK with unspecified ranges.
 * Patterns: pattern j is patterns[offsets[j] .. offsets[j+1]), offsets[0 .. k] nondecreasing (else ARCHON_E_ARG); k = 0
 * returns ARCHON_OK and writes nothing.  Results lo[k], hi[k]. */
typedef struct archon_hip_fm archon_hip_fm;    /* rank table + the handle's own copy of the BWT; one thread at a time */
/* host BWT of n bytes with primary row base_id (< n): builds the table on device `dev`; ARCHON_E_ARG for n = 0 or
 * base_id >= n.  The handle owns its device memory until archon_hip_fm_destroy. */
int  archon_hip_fm_create(const uint8_t *bwt, uint32_t n, uint32_t base_id, int dev, archon_hip_fm **out);
/* the same from a device BWT (any address), enqueued on `stream` (NULL = the context's own), complete on return */
int  archon_hip_fm_create_dev(const uint8_t *d_bwt, uint32_t n, uint32_t base_id, int dev, void *stream, archon_hip_fm **out);
void archon_hip_fm_destroy(archon_hip_fm *f);
/* host patterns, offsets[k+1] and ranges lo[k], hi[k] */
int  archon_hip_fm_count(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *lo, uint32_t *hi);
/* device pointers, on `stream` (NULL = the context's own), complete on return; decreasing offsets are found on the device */
int  archon_hip_fm_count_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k,
                             uint32_t *d_lo, uint32_t *d_hi, void *stream);
/* the resident block of the handle's last forward: the table is built over the block's own BWT on the first call after a
 * forward and kept with the handle (a forward drops it).  Needs no suffix array.  ARCHON_E_ARG before any forward. */
int  archon_hip_block_fm_count(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *lo, uint32_t *hi);
/* starts of every occurrence, pattern by pattern, each in row order (not sorted); *total = their number.  ARCHON_E_ARG
 * (nothing written, *total set) when cap < total; ARCHON_E_ARG when the last forward kept no suffix array */
int  archon_hip_block_fm_locate(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k,
                                uint32_t *pos, uint64_t cap, uint64_t *total);
/* work counters and device time of the CALLING THREAD's last FM call on `dev` (FM calls leave the other stats alone) */
typedef struct archon_hip_fm_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t patterns;          /* patterns of the call (0 for a create) */
    uint64_t pattern_bytes;     /* their bytes */
    uint64_t steps;             /* rank steps executed */
    uint64_t shared_steps;      /* of them, steps whose lo and hi shared one sub-chunk load */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    uint32_t built;             /* 1 when the call built a table */
    uint64_t table_bytes;       /* bytes of the rank table (without the BWT) */
    float ms_build;             /* device time of the table build (HIP events), 0 without one */
    float ms_query;             /* device time of the count and locate kernels (HIP events) */
} archon_hip_fm_stats;
int  archon_hip_get_fm_stats(int dev, archon_hip_fm_stats *out);

/* ---- locate and extract without the suffix array: a sampled FM index --------------------------------------------------
 * The rule in a7 order.  Item s is the key x[s-1], x[s-2], ..., x[0], INF (s = 1 .. n); bwt[r] = x[sa[r]], except at the
 * primary row `base`, which holds item n and stores x[0] as a stand-in.  R and occ' are those of the search rule above.
 * LF moves from item s to item s + 1:
 *   LF(r)    = R[bwt[r]] + occ'(bwt[r], r)     r != base
 *   LF(base) = R[bwt[base] + 1] - 1            the row of item 1 (x[0], INF is the last key of its bucket)
 * Walking LF from the row of item s visits items s+1, s+2, ...; bwt at the row of item p is x[p].  Item 0 means the
 * primary row (x[0] = bwt[base]).
 * Sample rate S: a power of two, 1 <= S <= 65 536 (else ARCHON_E_ARG).  Sampled items are p = 0, S, 2S, ... < n.
 *   ISA samples   isa_s[k] = the row of item kS, k = 0 .. ceil(n/S) - 1; isa_s[0] = base
 *   SA samples    one value per sampled row, in row order: sa[r], and n for the primary row; a marks bitvector over the
 *                 rows with a rank directory (one u32 per 256 rows) maps a sampled row to its slot
 *   locate        row r of item s = sa[r]: LF steps until the row is sampled; after t steps sa[r] = sample - t, t the least
 *                 t >= 0 with (s + t) mod S == 0 or s + t == n.  The starts of pattern j are sa[r] - m_j for r in
 *                 [lo_j, hi_j), pattern by pattern, each in row order: exactly the order and values of
 *                 archon_hip_block_fm_locate
 *   extract       x[a .. a+L): from isa_s[a / S], (a mod S) steps, then emit bwt[row] and step, L times.  Requests are cut at
 *                 the sample points into independent walks of at most S - 1 steps; a request of length 0 reads nothing
 *                 (also at a = n)
 * Example: "banana" (BWT nnbaaa, base 2, sa = 2 4 6 1 3 5), S = 2: isa_s = [2, 0, 1], sampled rows 0, 1, 2.  "an" has rows
 * [4, 6): row 4 takes one step to row 1 (sa 4), giving 3 - 2 = 1; row 5 one step to the primary row (sa 6), giving
 * 5 - 2 = 3.  Extracting x[3 .. 5) starts at isa_s[1] = row 0, takes one step to row 4, then emits 'a' and 'n' (cut at item 4,
 * the 'n' comes from its own walk: isa_s[2] = row 1, no step).
 * Memory: the samples of a handle take at most 8 ceil(n/S) + n/8 + n/64 + 4096 device bytes, beside the BWT and the rank
 * table (at S = 32: about 0.38 n).  Handles without samples count exactly as before and refuse locate and extract
 * (ARCHON_E_ARG).  archon_hip_fm_destroy frees the samples with the rest. */
/* samples from the handle's own BWT (the walk route); replaces earlier samples of the handle.  ARCHON_E_CORRUPT when the
 * handle's bytes are no BWT in a7 format (the LF cycle does not close) */
int  archon_hip_fm_sample(archon_hip_fm *f, uint32_t rate);
/* a standalone handle (own BWT copy + rank table + samples) from the resident block's last forward: samples from its SA when
 * that forward kept one, else by the walk route.  The handle outlives later forwards and archon_hip_block_destroy. */
int  archon_hip_block_fm_index(archon_hip_block *b, uint32_t rate, archon_hip_fm **out);
/* the ISA samples (row of item kS, k = 0 .. ceil(n/S)-1) to a host buffer; *count set even when cap is short (ARCHON_E_ARG) */
int  archon_hip_fm_read_samples(archon_hip_fm *f, uint32_t *isa, uint32_t cap, uint32_t *count);
/* like archon_hip_block_fm_locate, same output order and cap rule; ARCHON_E_ARG on a handle without samples */
int  archon_hip_fm_locate(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k,
                          uint32_t *pos, uint64_t cap, uint64_t *total);
/* request j: x[starts[j] .. starts[j] + offsets[j+1] - offsets[j]) into out[offsets[j] ..); offsets nondecreasing,
 * every range inside [0, n] (else ARCHON_E_ARG, nothing written); k = 0 writes nothing */
int  archon_hip_fm_extract(archon_hip_fm *f, const uint32_t *starts, const uint32_t *offsets, uint32_t k, uint8_t *out);
int  archon_hip_fm_extract_dev(archon_hip_fm *f, const uint32_t *d_starts, const uint32_t *d_offsets, uint32_t k,
                               uint8_t *d_out, void *stream);   /* bad ranges found on the device -> ARCHON_E_ARG */
typedef struct archon_hip_fm_walk_stats {
    uint32_t n, rate;            /* of the handle */
    uint32_t route;              /* sample builds: 1 = from an SA, 2 = by the LF walk; 0 for queries */
    uint32_t kernel_launches, host_syncs;
    uint64_t samples;            /* ISA entries of the handle */
    uint64_t sample_bytes;       /* device bytes of ISA + SA samples + marks + rank directory */
    uint64_t walks;              /* locate: occurrences; extract: segments */
    uint64_t lf_steps;           /* LF steps of all walks */
    uint32_t max_walk;           /* the longest walk's steps */
    uint32_t reserved0;
    float ms_build, ms_query;    /* HIP events on the call's stream */
} archon_hip_fm_walk_stats;
int  archon_hip_get_fm_walk_stats(int dev, archon_hip_fm_walk_stats *out);   /* calling thread's last sample/locate/extract call */

/* ---- approximate search: patterns with up to K substituted bytes --------------------------------------------------------
 * Keys, R and occ' are those of the search rule above; a pattern is consumed in TEXT order, P[0] first, and the primary row
 * is excluded from occ'.  A HIT of pattern P (length m) at distance K is a distinct string w of length m that occurs in x
 * with Hamming distance d(w, P) <= K.  Its rows [lo, hi) are exactly what archon_hip_fm_count(w) returns; distinct hits have
 * disjoint ranges; the occurrences of w start at sa[r] - m for r in [lo, hi).
 * The search and its output order are this depth-first procedure, frame(d, t, lo, hi) called first as frame(0, 0, 0, n):
 *   loop:
 *     if t == m: emit hit (lo, hi, d); return
 *     if d < K:                      an EXPANSION: every child at once
 *         child[c] = [R[c], R[c+1])                           if t == 0 (the buckets: no rank step, not counted)
 *                  = [R[c] + occ'(c,lo), R[c] + occ'(c,hi))   if t >= 1 (counted in `expansions`)
 *         for c = 0 .. 255 ascending, c != P[t], child[c] nonempty: frame(d+1, t+1, child[c])
 *         (lo, hi) = child[P[t]]
 *     else:                          d == K: one rank step, as archon_hip_fm_count takes it
 *         (lo, hi) = the bucket of P[0] if t == 0, else the rank step for P[t] (counted in `steps`)
 *     if lo >= hi: return
 *     t += 1
 * So the hits of one pattern are ordered by their mismatch lists (p1, w[p1]), (p2, w[p2]), ... (p1 < p2 < ...), compared
 * element by element, a list that ends coming AFTER every longer list that starts with it: the exact occurrence, if any,
 * comes last.  This is not row order; it is deterministic and what every entry point returns.
 * m = 0 gives the single hit (0, n, 0); m > n gives no hits and does no work; K = 0 gives one hit exactly when
 * archon_hip_fm_count finds the pattern, with its range and its steps.  0 <= K <= 4, else ARCHON_E_ARG.
 * The work counters follow from x, P and K alone (Sub_t(x): the distinct substrings of length t):
 *   expansions = sum over t = 1 .. m-1 of |{u in Sub_t(x) : d(u, P[0 .. t)) <  K}|
 *   steps      = sum over t = 1 .. m-1 of |{u in Sub_t(x) : d(u, P[0 .. t)) == K}|
 * Example: "banana" (BWT nnbaaa, primary row 2, sa = 2 4 6 1 3 5): "bn" at K = 1 gives the hits (4, 6, 1) ("an", starts 1
 * and 3) and then (0, 1, 1) ("ba", start 0), with 1 expansion and 2 steps; "an" at K = 1 gives only (4, 6, 0).
 * Device work: one wave per pattern, at most K suspended frames (a 2 KiB LDS child table each); an expansion costs about
 * as much as a rank step over all 256 symbols at once, a node at d == K one rank step. */
typedef struct archon_hip_fm_hit {
    uint32_t lo, hi;            /* the rows of the hit's string w */
    uint32_t mismatches;        /* d(w, P) */
    uint32_t pattern;           /* j: the pattern it belongs to */
} archon_hip_fm_hit;
/* nhits[k] and nocc[k] (distinct hits, rows summed over them) always written; *total = the sum of nhits.  hits_or_null NULL:
 * counting only (no emit pass).  cap < *total with hits given: ARCHON_E_ARG, counts and *total written, hits untouched.
 * Patterns and offsets as for archon_hip_fm_count; k = 0 writes *total = 0 and nothing else. */
int  archon_hip_fm_approx(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_mismatches,
                          uint32_t *nhits, uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total);
/* device patterns, offsets, nhits, nocc and hits, *total a host pointer; on `stream` (NULL = the context's own), complete on
 * return; decreasing offsets are found on the device (ARCHON_E_ARG, nothing emitted) */
int  archon_hip_fm_approx_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t max_mismatches,
                              uint32_t *d_nhits, uint32_t *d_nocc, archon_hip_fm_hit *d_hits_or_null, uint64_t cap, uint64_t *total,
                              void *stream);
/* the resident block's BWT; its table is built on the first FM call after a forward, as for archon_hip_block_fm_count */
int  archon_hip_block_fm_approx(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_mismatches,
                                uint32_t *nhits, uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total);
/* the starts of every hit's occurrences, hit by hit, each in row order: sa[r] - m for r in [lo, hi), m the length of pattern
 * hit.pattern (patterns' offsets[k + 1] as given to the search).  *total = their number; cap < *total: ARCHON_E_ARG,
 * nothing written.  hit.pattern >= k, lo > hi or hi > n, or nhits >= 2^32: ARCHON_E_ARG.  A sampled handle (else
 * ARCHON_E_ARG) walks LF to the samples; a block needs the suffix array of its last forward (else ARCHON_E_ARG). */
int  archon_hip_fm_locate_hits(archon_hip_fm *f, const uint32_t *offsets, uint32_t k, const archon_hip_fm_hit *hits, uint64_t nhits,
                               uint32_t *pos, uint64_t cap, uint64_t *total);
int  archon_hip_block_fm_locate_hits(archon_hip_block *b, const uint32_t *offsets, uint32_t k, const archon_hip_fm_hit *hits, uint64_t nhits,
                                     uint32_t *pos, uint64_t cap, uint64_t *total);
/* the CALLING THREAD's last approximate call (approx or locate_hits) on `dev`; approximate calls leave archon_hip_fm_stats,
 * archon_hip_fm_walk_stats and the rest alone */
typedef struct archon_hip_fm_approx_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t patterns;          /* k of the call */
    uint32_t max_mismatches;    /* K (0 for locate_hits) */
    uint32_t built;             /* 1 when the call built the block's table */
    uint64_t pattern_bytes;     /* bytes of the patterns */
    uint64_t expansions;        /* expansions at t >= 1 (count pass) */
    uint64_t steps;             /* single rank steps at t >= 1 (count pass) */
    uint64_t hits;              /* hits found (approx) or located (locate_hits) */
    uint64_t occurrences;       /* rows summed over those hits */
    uint64_t lf_steps;          /* locate_hits on a sampled handle: LF steps of all walks */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_build;             /* device time of the table build, 0 without one */
    float ms_count, ms_emit;    /* device time of the count and the emit pass (HIP events) */
    float ms_locate;            /* device time of locate_hits' kernel */
} archon_hip_fm_approx_stats;
int  archon_hip_get_fm_approx_stats(int dev, archon_hip_fm_approx_stats *out);

/* ---- class search: patterns whose positions each accept a set of bytes ----------------------------------------------------
 * Case folding, a wildcard at a known position, IUPAC codes: the pattern says WHERE the text may differ and INTO WHAT.
 * A CLASS TABLE is uint32_t classes[256][8] (8 KiB): bit c of classes[b] is word c >> 5, bit c & 31; when it is set the text
 * byte c is accepted where the pattern holds byte b.  Pattern bytes are class names: the identity table makes the call
 * archon_hip_fm_count; classes['a'] = {a, A} folds case; a byte may name a class that does not hold the byte itself, as IUPAC
 * N = {A, C, G, T} does.  One table serves all patterns of a call.
 * Keys, R and occ' are those of the search rule above.  Sigma(x) is the set of bytes that occur in the block (the nonempty
 * buckets, R[c] < R[c+1]); the EFFECTIVE CLASS of position t is M_t = classes[P[t]] cut to Sigma(x).
 * A HIT of pattern P (length m) is a distinct string w of length m that occurs in x with w[t] in M_t for every t.  Its rows
 * [lo, hi) are exactly what archon_hip_fm_count(w) returns, its `mismatches` the number of t with w[t] != P[t]; the record
 * is archon_hip_fm_hit, and archon_hip_fm_locate_hits / archon_hip_block_fm_locate_hits locate these hits as they stand.
 * The search and its output order are this depth-first procedure, frame(t, lo, hi, d) called first as frame(0, 0, n, 0):
 *   loop:
 *     if t == m: emit hit (lo, hi, d); return
 *     if |M_t| == 1 (its symbol c):  one rank step, as archon_hip_fm_count takes it
 *         (lo, hi) = the bucket of c if t == 0, else the rank step for c (t >= 1: counted in `steps`)
 *         if lo >= hi: return
 *         d += (c != P[t]); t += 1
 *     else:                          an EXPANSION, as archon_hip_fm_approx takes it
 *         child[c] = [R[c], R[c+1])                           if t == 0 (the buckets: no rank step, not counted)
 *                  = [R[c] + occ'(c,lo), R[c] + occ'(c,hi))   if t >= 1 (counted in `expansions`)
 *         for c in M_t ascending, child[c] nonempty: frame(t+1, child[c], d + (c != P[t]))
 *         return
 * So the hits of one pattern come in ascending byte order of their strings w, the patterns in ascending j, and the ranges
 * of one pattern's hits are disjoint.  m = 0 gives the single hit (0, n, 0); m > n, or an empty M_t at any t, gives no hits
 * and does no work.  The work counters follow from x, P and the table alone (Sub_t(x): the distinct substrings of length t):
 *   expansions = sum over t = 1 .. m-1 with |M_t| >= 2 of |{u in Sub_t(x) : u[i] in M_i for all i < t}|
 *   steps      = the same sum over the t with |M_t| == 1
 * The WIDTH of a pattern is W = sum over t of (|M_t| - 1); it bounds the frames that can be pending at once (the frames
 * pushed at position t are at most |M_t| - 1, and the pending ones lie beside one path).  Every call requires W <= 1024 for
 * every pattern that is searched (a pattern that does no work -- m > n, or an empty M_t -- has no width), otherwise
 * ARCHON_E_ARG and nothing written.  Because M_t is cut to Sigma(x), a wildcard costs 3 on DNA and 255 on random bytes.
 * Example: "banana" (BWT nnbaaa, primary row 2, sa = 2 4 6 1 3 5), the identity table with classes['?'] = all bytes, the
 * pattern "?a": Sigma(x) = {a, b, n}, W = 2; the buckets expand into three children at t = 0 (not counted) and each child
 * takes one rank step with 'a': 0 expansions, 3 steps.  The child "a" dies at "aa"; the hits are (0, 1, 1) ("ba", start 0)
 * and then (1, 3, 1) ("na", starts 2 and 4).
 * Device work: one wave per pattern with a stack of 16-byte frames in LDS, sized by the widest pattern of the call; a pass
 * over the patterns before the search finds the widths and the patterns with an empty class. */
/* nhits[k] and nocc[k] (distinct hits, rows summed over them) and *total (the sum of nhits) written by every call that
 * searches.  hits_or_null NULL: counting only (no emit pass).  cap < *total with hits given: ARCHON_E_ARG, counts and *total
 * written, hits untouched.  Patterns and offsets as for archon_hip_fm_count; k = 0 writes *total = 0 and nothing else.
 * NULL classes: ARCHON_E_ARG before the handle is read. */
int  archon_hip_fm_classes(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, const uint32_t *classes,
                           uint32_t *nhits, uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total);
/* device patterns, offsets, table, nhits, nocc and hits, *total a host pointer; on `stream` (NULL = the context's own),
 * complete on return; decreasing offsets are found on the device (ARCHON_E_ARG, nothing written) */
int  archon_hip_fm_classes_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, const uint32_t *d_classes,
                               uint32_t *d_nhits, uint32_t *d_nocc, archon_hip_fm_hit *d_hits_or_null, uint64_t cap, uint64_t *total,
                               void *stream);
/* the resident block's BWT; its table is built on the first FM call after a forward, as for archon_hip_block_fm_approx */
int  archon_hip_block_fm_classes(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, const uint32_t *classes,
                                 uint32_t *nhits, uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total);
/* the CALLING THREAD's last class call on `dev`; class calls leave every other statistics record alone */
typedef struct archon_hip_fm_class_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t patterns;          /* k of the call */
    uint32_t max_width;         /* the largest W of the call's searched patterns, saturating (above 1024: the call was refused) */
    uint32_t built;             /* 1 when the call built the block's table */
    uint64_t pattern_bytes;     /* bytes of the patterns */
    uint64_t expansions;        /* expansions at t >= 1 (count pass) */
    uint64_t steps;             /* single rank steps at t >= 1 (count pass) */
    uint64_t hits;              /* hits found */
    uint64_t occurrences;       /* rows summed over those hits */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_build;             /* device time of the table build, 0 without one */
    float ms_width;             /* device time of the pass that finds the widths (HIP events) */
    float ms_count, ms_emit;    /* device time of the count and the emit pass */
} archon_hip_fm_class_stats;
int  archon_hip_get_fm_class_stats(int dev, archon_hip_fm_class_stats *out);

/* ---- edit-distance search: patterns with up to K substituted, inserted or deleted bytes -----------------------------------
 * x is the block (n bytes), P a pattern of m bytes, K the allowed errors: an error is a substitution, an insertion or a
 * deletion of one byte, ed the Levenshtein distance.  For an end position e in [0, n] let
 *   D(e) = min over 0 <= s <= e of ed(P, x[s .. e)).
 * A MATCH is an e with D(e) <= K; its record is (start, end, distance, pattern), where start is the LARGEST s with
 * ed(P, x[s .. e)) = D(e): the shortest best occurrence that ends at e.  Matches come pattern by pattern, each pattern's
 * matches by ascending end.  Ends next to a good end match too, at a higher distance: that is the definition, as Sellers'
 * algorithm and agrep use it, and a caller who wants one occurrence per place keeps the local minima of the distance.
 * The same as a recurrence over cells (i, j), 0 <= i <= m, 0 <= j <= n, a cell being a pair (d, s):
 *   (0, j) = (0, j);  (i, 0) = (i, 0);  otherwise d is the least of diag.d + [P[i-1] != x[j-1]], up.d + 1 and left.d + 1,
 *   and s the largest s among the candidates that reach it.  The matches are the j with (m, j).d <= K.
 * Example, x = "banana": "bnan" at K = 1 gives (start 0, end 3, 1) and (2, 5, 1); "nab" at K = 1 gives (2, 4, 1), (2, 5, 1)
 * and (4, 6, 1).
 * Limits: 0 <= K <= 8, and every pattern has K < m <= 4096 (at m <= K every position would match; a long text belongs to
 * archon_hip_fm_ms_text).  A call that breaks one is ARCHON_E_ARG and writes nothing; the device form finds a bad pattern on
 * the device and emits nothing.  With n < m - K a pattern has no matches and does no work.  k = 0 writes *total = 0 and
 * nothing else.
 * The search is a filter with a dense check, and its work counters follow from x, P, K and the tile width W (32) alone:
 *   pieces    piece i (0 <= i <= K) is P[o_i .. o_{i+1}), o_i = floor(i m / (K + 1)): nonempty, and a pattern with at most K
 *             errors holds one of them unchanged.  They are searched where they lie in the pattern buffer
 *   seeds     the rows of piece i are its archon_hip_fm_count range; a row r gives the piece's start p = sa[r] - its length,
 *             as locate does, and the diagonal g = p - o_i (signed).  seed_rows = the sum of the ranges
 *   tiles     with u = e - (m - K) for a match end e (0 <= u <= n - m + K), tile t of a pattern owns the ends with
 *             floor(u / W) = t.  A seed marks the tiles of u in [max(g, 0), min(g + 2K, n - m + K)] (none when that is empty):
 *             every match lies in a marked tile, and a marked tile reports ALL of its matches however it came to be marked, so
 *             the output does not depend on the seeds.  tiles = the distinct marked (pattern, tile) pairs, rows = the sum
 *             over them of m, hits = the matches
 * Device work: a wave per marked pair, its lanes the W + 2K diagonals around the tile, a loop over the pattern's bytes. */
typedef struct archon_hip_fm_edit_hit {
    uint32_t start, end;        /* the occurrence x[start .. end) */
    uint32_t distance;          /* ed(P, x[start .. end)) = D(end) */
    uint32_t pattern;           /* j: the pattern it belongs to */
} archon_hip_fm_edit_hit;
/* A handle with samples (archon_hip_fm_sample / archon_hip_block_fm_index; else ARCHON_E_ARG): the seeds are located by the
 * LF walk, the text around the marked tiles is extracted.  nhits[k] and *total (the sum of nhits) always written.
 * hits_or_null NULL: counting only.  cap < *total with hits given: ARCHON_E_ARG, counts and *total written, hits untouched.
 * Patterns and offsets as for archon_hip_fm_count.  ARCHON_E_NOMEM names a single pattern whose seeds exceed the scratch of
 * a batch (256 MiB). */
int  archon_hip_fm_edit(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_errors, uint32_t *nhits,
                        archon_hip_fm_edit_hit *hits_or_null, uint64_t cap, uint64_t *total);
/* device patterns, offsets, nhits and hits, *total a host pointer; on `stream` (NULL = the context's own), complete on return */
int  archon_hip_fm_edit_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t max_errors,
                            uint32_t *d_nhits, archon_hip_fm_edit_hit *d_hits_or_null, uint64_t cap, uint64_t *total, void *stream);
/* the resident block: its text and the suffix array of its last forward (ARCHON_E_ARG when that kept none); its table is
 * built on the first FM call after a forward, as for archon_hip_block_fm_count */
int  archon_hip_block_fm_edit(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_errors,
                              uint32_t *nhits, archon_hip_fm_edit_hit *hits_or_null, uint64_t cap, uint64_t *total);
/* the CALLING THREAD's last edit call on `dev`; edit calls leave every other record alone */
typedef struct archon_hip_fm_edit_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t patterns;          /* k of the call */
    uint32_t max_errors;        /* K */
    uint32_t tile;              /* W */
    uint32_t batches;           /* batches of patterns the scratch budget cut the call into */
    uint32_t built;             /* 1 when the call built the block's table */
    uint64_t pattern_bytes;     /* bytes of the patterns */
    uint64_t seed_rows;         /* rows of all pieces */
    uint64_t tiles;             /* distinct marked (pattern, tile) pairs */
    uint64_t rows;              /* pattern bytes summed over them */
    uint64_t hits;              /* matches */
    uint64_t lf_steps;          /* a handle: LF steps of the seeds' walks and of the extracted text */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_build;             /* device time of the table build, 0 without one */
    float ms_seed;              /* pieces, their count and locate, the marks and the sweep */
    float ms_extract;           /* a handle: the text of the marked tiles */
    float ms_count, ms_emit;    /* the count and the emit pass of the banded check (HIP events) */
} archon_hip_fm_edit_stats;
int  archon_hip_get_fm_edit_stats(int dev, archon_hip_fm_edit_stats *out);

/* ---- super-maximal exact matches: which pieces of a pattern occur, with a mirror index ------------------------------------
 * Keys, R and occ' are those of the search rule above.  An SMEM of a pattern P of length m is a pair (b, e), 0 <= b < e <= m,
 * such that P[b .. e) occurs in x, and b == 0 or P[b-1 .. e) does not occur, and e == m or P[b .. e+1) does not occur: an
 * occurring piece of P that no other occurring piece of P contains.  Ordered by b the SMEMs of a pattern have strictly
 * increasing e, so a pattern has at most m of them.  A position of P whose byte does not occur in x lies in no SMEM.
 * The MIRROR of a handle is the a7 transform (BWT and primary row) of xr = x reversed, with a rank table of its own in the
 * layout above.  A rank step on the primary index extends a match to the right; one on the mirror extends it to the left:
 * P[b' .. e] occurs in x exactly when the search rule finds P[e], P[e-1], ..., P[b'] in the mirror.
 * The search, its output order and its work counters are this procedure:
 *   b = 0
 *   while b < m:
 *     F: the search rule on the primary index from P[b]: the bucket of P[b] (no step), then one rank step per further byte,
 *        until the range is empty or P ends.  l = the bytes matched, [lo, hi) the last range that held rows.
 *        l == 0 (P[b] is not in x): b += 1; continue
 *        fwd_steps += l if b + l < m, else l - 1          (the failing step counts, as in archon_hip_fm_count)
 *        e = b + l; found += 1; if e - b >= min_len: emit (lo, hi, b, e)
 *        if e == m: stop
 *     B: the search rule on the mirror with P[e], P[e-1], ..., at most down to P[b+1] (P[b .. e] is known not to occur).
 *        g = the bytes matched
 *        g == 0 (P[e] is not in x): b = e + 1; continue
 *        b' = e - g + 1; bwd_steps += g if b' > b + 1, else g - 1          (no step is spent on P[b])
 *        b = b'
 * The SMEMs of a pattern are emitted in ascending b, the patterns in ascending j.  The rows [lo, hi) are rows of the PRIMARY
 * index: exactly what archon_hip_fm_count returns for P[b .. e), so every occurrence starts at sa[r] - (e - b).  m = 0 gives
 * no SMEM and no step; a pattern longer than the block is searched like any other.  min_len only filters the output: it
 * changes neither counter nor `found`.
 * Example: "banana" (BWT nnbaaa, primary row 2, sa = 2 4 6 1 3 5; mirror: "ananab", BWT bnnaaa, primary row 3): "nanb" gives
 * F from 0: n, a, n match (rows [5, 6)), b fails: 3 steps, the SMEM (5, 6, 0, 3) ("nan", start sa[5] - 3 = 2).  B with
 * "b", then "n": "nb" does not occur, g = 1, 1 step, b' = 3.  F from 3: the bucket of b, the SMEM (3, 4, 3, 4) (start
 * sa[3] - 1 = 0) and the end of P.  fwd_steps = 3, bwd_steps = 1, found = 2.
 * Memory: the mirror is one more device allocation of the handle, its BWT (n + 64 bytes) and rank table: at most
 * 1.5 n + n / 64 + 4096 bytes at the table's default sizes, freed by archon_hip_fm_destroy.  Handles without a mirror behave
 * exactly as before and refuse the SMEM search (ARCHON_E_ARG).
 * Device work: one wave per pattern, every step one rank step of archon_hip_fm_count; a single long pattern runs on one
 * wave, one dependent step after the other.
 * A handle serves one thread at a time (as above): a mirror build frees the handle's earlier mirror, so archon_hip_fm_mirror,
 * _fm_mirror_dev and archon_hip_block_fm_mirror must not run while another call uses the same handle. */
/* the mirror from the handle's own BWT: its inverse, the reversed text, a forward transform and the table, all in the calling
 * thread's context arena (about 32 n bytes for the nested forward).  Replaces an earlier mirror.  ARCHON_E_CORRUPT when the
 * handle's bytes are no BWT in a7 format. */
int  archon_hip_fm_mirror(archon_hip_fm *f);
/* the same from a device copy of the text x (n bytes, any address), which saves the inverse; on `stream` (NULL = the context's
 * own), complete on return.  A text whose 256 byte counts differ from the handle's is refused with ARCHON_E_ARG: a cheap guard,
 * not a proof -- a different text with the same counts gives a mirror of that text, and SMEMs that mean nothing.  The text is
 * read in aligned 16-byte granules: at an address that is no multiple of 16 the call also reads (and ignores) the up to 15
 * bytes of the granules of d_x[0] and d_x[n-1] that lie outside the text; they share those bytes' 16-byte granule. */
int  archon_hip_fm_mirror_dev(archon_hip_fm *f, const uint8_t *d_x, void *stream);
/* for a handle made by archon_hip_block_fm_index from this block's last forward: the mirror from the resident x.  A handle of
 * another length or primary row is ARCHON_E_ARG. */
int  archon_hip_block_fm_mirror(archon_hip_block *b, archon_hip_fm *f);
/* the mirror's BWT (n bytes) and primary row to the host; *base_id set even when cap < n (ARCHON_E_ARG) */
int  archon_hip_fm_read_mirror(archon_hip_fm *f, uint8_t *bwt, uint32_t cap, uint32_t *base_id);
typedef struct archon_hip_fm_mem {
    uint32_t lo, hi;            /* the rows of P[start .. end) in the primary index */
    uint32_t start, end;        /* b and e: the piece of the pattern */
    uint32_t pattern;           /* j: the pattern it belongs to */
    uint32_t reserved0;
} archon_hip_fm_mem;
/* nmems[k] and nocc[k] (SMEMs of at least min_len bytes, rows summed over them) always written; *total = the sum of nmems.
 * nocc[j] saturates at 2^32 - 1 (a long pattern's pieces can hold more rows than that; the SMEMs carry the exact ranges).
 * mems_or_null NULL: counting only (no emit pass).  cap < *total with mems given: ARCHON_E_ARG, counts and *total written, mems
 * untouched.  Patterns and offsets as for archon_hip_fm_count; k = 0 writes *total = 0 and nothing else. */
int  archon_hip_fm_smems(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t min_len,
                         uint32_t *nmems, uint32_t *nocc, archon_hip_fm_mem *mems_or_null, uint64_t cap, uint64_t *total);
/* device patterns, offsets, nmems, nocc and mems, *total a host pointer; on `stream` (NULL = the context's own), complete on
 * return; decreasing offsets are found on the device (ARCHON_E_ARG, nothing emitted) */
int  archon_hip_fm_smems_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t min_len,
                             uint32_t *d_nmems, uint32_t *d_nocc, archon_hip_fm_mem *d_mems_or_null, uint64_t cap, uint64_t *total,
                             void *stream);
/* the starts of every SMEM's occurrences, SMEM by SMEM, each in row order: sa[r] - (end - start) for r in [lo, hi).  *total =
 * their number; cap < *total: ARCHON_E_ARG, nothing written.  lo > hi, hi > n, end < start or nmems >= 2^32: ARCHON_E_ARG.  A
 * sampled handle (else ARCHON_E_ARG) walks LF to the samples and needs no mirror; a block needs the suffix array of its last
 * forward (else ARCHON_E_ARG), the rows being rows of that block's BWT. */
int  archon_hip_fm_locate_mems(archon_hip_fm *f, const archon_hip_fm_mem *mems, uint64_t nmems, uint32_t *pos, uint64_t cap, uint64_t *total);
int  archon_hip_block_fm_locate_mems(archon_hip_block *b, const archon_hip_fm_mem *mems, uint64_t nmems, uint32_t *pos, uint64_t cap,
                                     uint64_t *total);
/* the CALLING THREAD's last SMEM call (mirror, smems or locate_mems) on `dev`; SMEM calls leave archon_hip_stats,
 * archon_hip_fm_stats, archon_hip_fm_walk_stats, archon_hip_fm_approx_stats and the rest alone */
typedef struct archon_hip_fm_mem_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t patterns;          /* k of the call */
    uint32_t min_len;           /* of the call (0 for mirror and locate_mems) */
    uint32_t built;             /* 1 when the call built a mirror */
    uint64_t pattern_bytes;     /* bytes of the patterns */
    uint64_t fwd_steps;         /* rank steps on the primary index (count pass) */
    uint64_t bwd_steps;         /* rank steps on the mirror (count pass) */
    uint64_t found;             /* SMEMs of any length */
    uint64_t mems;              /* SMEMs of at least min_len bytes (smems) or located (locate_mems) */
    uint64_t occurrences;       /* rows summed over those */
    uint64_t lf_steps;          /* locate_mems on a sampled handle: LF steps of all walks */
    uint64_t mirror_bytes;      /* device bytes of the handle's mirror: BWT and rank table */
    uint32_t kernel_launches;   /* launches issued by the call, those of a mirror's nested transforms included */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_mirror;            /* device time of a mirror build, end to end (HIP events) */
    float ms_count, ms_emit;    /* device time of the count and the emit pass */
    float ms_locate;            /* device time of locate_mems' kernel */
} archon_hip_fm_mem_stats;
int  archon_hip_get_fm_mem_stats(int dev, archon_hip_fm_mem_stats *out);

/* ---- matching statistics: the longest occurring piece that ends at every position of a pattern, with the block's LCP array ----
 * Keys, R, occ', rows and the primary row are those of the search rule above.  lcp is the block's LCP array (archon_hip_lcp);
 * lcp[0] is read as 0 and lcp[n] as 0.  For a pattern P of length m and every end e in 1 .. m, the record of e is (len, lo, hi):
 * len is the largest l <= e such that P[e-l .. e) occurs in x, [lo, hi) exactly what archon_hip_fm_count returns for that piece,
 * and (0, 0, n) when P[e-1] is not in x.
 * A rank step extends a match to the right, so the pattern is read once, forward; the parent LCP interval shortens the match.
 * There is no second transform and no mirror.  The search and its work counters are this procedure (Ohlebusch, Gog and Kuegel
 * 2010), from the state (lo, hi, l) = (0, n, 0):
 *   for t = 0 .. m-1, c = P[t]:
 *     loop:
 *       if l == 0:  [a, b) = [R[c], R[c+1]) (no step);  nonempty: (lo, hi, l) = (a, b, 1), else (0, n, 0);  break
 *       steps += 1;  [a, b) = the rank step of c on [lo, hi)
 *       if a < b:   (lo, hi, l) = (a, b, l + 1);  break
 *       parents += 1
 *       l' = min(max(lcp[lo], lcp[hi]), l - 1)      (the min changes nothing for a true LCP array: it makes any array terminate)
 *       if l' == 0: (lo, hi, l) = (0, n, 0)
 *       else:       lo = the greatest p <= lo with lcp[p] < l';  hi = the least q >= hi with lcp[q] < l', or n;  l = l'
 *     the record of e = t + 1 is (l, lo, hi)
 * Every length in (l', l] has the same rows as l, so skipping them loses nothing.  A parent move lowers l by at least 1 and a
 * byte raises it by at most 1: for ANY data and pattern parents <= m and steps <= 2 m, and both follow from x and P alone.
 * The SMEMs follow from the records: P[e-len .. e) is an SMEM exactly when len > 0 and (e == m or len(e+1) <= len(e)), its rows
 * the record's: the set and the order of archon_hip_fm_smems.
 * Example: "banana" (lcp 0 1 3 0 0 2) and "nanb": the records are (1,4,6) (2,1,3) (3,5,6) (1,3,4).  n is a bucket; a and n are
 * two steps; b fails on [5, 6) and the state moves to l' = 2, rows [4, 6); b fails again and the state moves to l' = 0; b is then
 * a bucket: 4 steps and 2 parents.  The SMEMs from the records are (0, 3) and (3, 4), as in the example above.
 * Each parent move is two nearest-smaller-value searches in a minimum hierarchy over lcp of fan-out F (that of
 * archon_hip_repeats: 16): at most 2 (2 F - 1) entries of lcp and the hierarchy per level.
 * Memory: the attached array is one more device allocation of the handle, the n words (4 n + 64 bytes) and the hierarchy's
 * levels behind them: 4 n + 64 + 4 tree_words bytes, tree_words = the sum over the levels of their entries (about n / (F - 1)):
 * about 4.27 n at F = 16.  archon_hip_fm_destroy frees it.  Handles without one behave exactly as before and refuse
 * archon_hip_fm_ms (ARCHON_E_ARG).
 * Device work: one wave per pattern, every step one rank step of archon_hip_fm_count; a single long pattern runs on one wave
 * (archon_hip_fm_ms_text, further down, spreads one long text over the device).
 * The worst case is a pattern a a ... a b against a block of one repeated byte a: the last byte takes a parent move per a.
 * Example: "aaaa" (lcp 0 3 2 1) and "aaaab": the records are (1,0,4) (2,0,3) (3,0,2) (4,0,1) (0,0,4).  The a's are a bucket and 3
 * steps; b fails at l = 4, 3, 2 and 1 (4 steps, 4 parents) and is then an empty bucket: 7 steps and 4 parents.
 * A handle serves one thread at a time (as above): an attach frees the handle's earlier array. */
/* lcp[n] on the host: copied into the handle, the hierarchy built behind it.  Replaces an earlier attachment.  An entry
 * lcp[i], i >= 1, of n or more (a true one is at most n - 1) is ARCHON_E_CORRUPT and leaves an earlier attachment in place: a
 * cheap guard, not a proof -- any other wrong array returns ARCHON_OK and gives unspecified records, every access inside the
 * buffers and every range inside [0, n]. */
int  archon_hip_fm_attach_lcp(archon_hip_fm *f, const uint32_t *lcp);
/* the same from a device array; on `stream` (NULL = the context's own), complete on return */
int  archon_hip_fm_attach_lcp_dev(archon_hip_fm *f, const uint32_t *d_lcp, void *stream);
/* for a handle made by archon_hip_block_fm_index from this block's last forward, which must have kept its suffix array (else
 * ARCHON_E_ARG): the LCP array is computed on the device (its record in archon_hip_lcp_stats) and attached from there; it never
 * visits the host.  A handle of another length or primary row is ARCHON_E_ARG. */
int  archon_hip_block_fm_attach_lcp(archon_hip_block *b, archon_hip_fm *f);
/* len, lo, hi: arrays of offsets[k] words; the record of end e of pattern j goes to index offsets[j] + e - 1, nothing else is
 * written.  lo_or_null and hi_or_null are both given or both NULL (lengths only); one without the other is ARCHON_E_ARG.
 * Patterns and offsets as for archon_hip_fm_count; k = 0 and m = 0 write nothing; a pattern longer than the block is searched
 * like any other.  A handle without an attached LCP array is ARCHON_E_ARG. */
int  archon_hip_fm_ms(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *len, uint32_t *lo_or_null,
                      uint32_t *hi_or_null);
/* device patterns, offsets and records; on `stream` (NULL = the context's own), complete on return; decreasing offsets are
 * found on the device (ARCHON_E_ARG, nothing promised about the records) */
int  archon_hip_fm_ms_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t *d_len,
                          uint32_t *d_lo_or_null, uint32_t *d_hi_or_null, void *stream);
/* the CALLING THREAD's last attach or matching-statistics call on `dev`; these calls leave every other statistics record alone
 * (archon_hip_block_fm_attach_lcp keeps the LCP step's record in archon_hip_lcp_stats, as archon_hip_block_repeats does) */
typedef struct archon_hip_fm_ms_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t patterns;          /* k of the call (0 for an attach) */
    uint32_t fan;               /* F: fan-out of the hierarchy of the handle's attached array (0 without one) */
    uint32_t levels;            /* its levels above lcp: ceil(log_F n) */
    uint32_t attached;          /* 1 when the call attached an array */
    uint64_t pattern_bytes;     /* bytes of the patterns */
    uint64_t steps;             /* rank steps */
    uint64_t parents;           /* parent moves */
    uint64_t probes;            /* entries of lcp and the hierarchy the parent moves read, counted as the kernel reads them */
    uint64_t matched;           /* the sum of all len */
    uint32_t longest;           /* the largest len */
    uint64_t lcp_bytes;         /* device bytes of the attached array and its hierarchy */
    uint32_t kernel_launches;   /* launches issued by the call (those of the block form's LCP step are in archon_hip_lcp_stats) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_lcp;               /* block form only: device time of the LCP array */
    float ms_attach;            /* device time of the guard and the hierarchy (HIP events) */
    float ms_query;             /* device time of the search */
} archon_hip_fm_ms_stats;
int  archon_hip_get_fm_ms_stats(int dev, archon_hip_fm_ms_stats *out);

/* ---- the repeats of a block: LCP intervals, maximal and supermaximal repeats (no counterpart in the reference) -----------
 * What a caller computes next from the suffix array, its LCP array and the BWT: which strings repeat in the block, how often
 * and where.  Rows, sa, lcp, bwt and the primary row `base` are those above (row r holds item sa[r], bwt[r] = x[sa[r]], the
 * primary row holds item n and stores x[0] as a stand-in); lcp[0] is taken as 0 whatever it holds.
 * LCP interval: a row k in 1 .. n-1 with l = lcp[k] > 0 defines
 *   lo = the greatest p < k with lcp[p] < l (row 0 at the latest), hi = the least q > k with lcp[q] < l, or n if there is none.
 * Row k REPRESENTS the interval when no k' in (lo, k) has lcp[k'] == l: every interval has exactly one representative, and a
 * block has at most n - 1 intervals.  The rows [lo, hi) are exactly the occurrences of the string u = x[s-l .. s), s = sa[r]
 * of any of them: each occurrence starts at sa[r] - l, and [lo, hi) is what archon_hip_fm_count(u) returns.
 *   kind 0  every LCP interval: the repeats u that cannot be extended to the left (their occurrences are not all preceded by
 *           the same byte; an occurrence at the start of the text counts as different from all others)
 *   kind 1  maximal repeats: a kind 0 interval whose occurrences are not all followed by the same byte: bwt[lo .. hi) are not
 *           all equal, or base lies in [lo, hi) (the primary row has no following byte)
 *   kind 2  supermaximal repeats: a kind 1 interval where every lcp[k], lo < k < hi, equals l and the following bytes are
 *           pairwise distinct, the primary row distinct from every byte (hence hi - lo <= 257): a maximal repeat that is a
 *           substring of no other maximal repeat
 * Examples.  "banana" (sa = 2 4 6 1 3 5, lcp = 0 1 3 0 0 2, BWT nnbaaa, base 2): kind 0 gives (lo, hi, len, row) = (0,3,1,1)
 * "a", (1,3,3,2) "ana", (4,6,2,5) "an"; kind 1 the first two; kind 2 (1,3,3,2) only.  "abracadabra": kind 1 gives (0,5,1,1)
 * "a" and (2,4,4,3) "abra", kind 2 (2,4,4,3).
 * Output order: ascending representative row.  Filters: min_len keeps len >= min_len (0 behaves as 1), min_occ keeps
 * hi - lo >= min_occ (0 and 1 behave as 2); they change the output and the `repeats`, `occurrences` and `longest` counters
 * only, never `intervals`.
 * Cap rule (that of archon_hip_fm_smems): *total is a host pointer and always written.  out NULL: counting only, no emit pass.
 * cap < *total with out given: ARCHON_E_ARG, *total written, out untouched.  ARCHON_E_ARG for a null lcp or bwt, n = 0,
 * base_id >= n or kind > 2; n = 1 gives *total = 0.
 * Work: both ends of an interval are nearest-smaller-value searches in a minimum hierarchy over lcp with fan-out F = 16 (level
 * j holds the minimum of each F^j rows, L = ceil(log_F n) levels): a search reads at most F - 1 entries per level on the way up
 * and F on the way down, a row takes at most two searches, so for ANY data
 *   probes <= 2 (2 F - 1) L (n - 1)
 * (a block of one repeated byte, lcp = 0, n-1, n-2, ..., 1, sends every left search to row 0).  The supermaximal check reads
 * at most 257 rows of lcp and bwt per interval, not counted in probes.
 * Bad input: an lcp that is not the LCP array of anything returns ARCHON_OK with unspecified contents; every access stays
 * inside the buffers and every emitted lo < row < hi <= n.
 * Workspace, from the calling thread's context arena: 4 n / (F - 1) bytes of hierarchy, 4 n + 4 bytes of change-flag sums (kind
 * 1 only) and n / 400 bytes of tile words: about 4.3 n bytes.  The host forms stage lcp, bwt and the repeats besides.
 * Locating needs no new call: a repeat (lo, hi, len) is located by archon_hip_block_fm_locate_mems / archon_hip_fm_locate_mems
 * with an archon_hip_fm_mem {lo, hi, start 0, end len}: the starts sa[r] - len, r in [lo, hi).  The rows of a handle made by
 * archon_hip_block_fm_index are the block's rows. */
typedef struct archon_hip_repeat {
    uint32_t lo, hi;            /* the rows of the repeat's occurrences */
    uint32_t len;               /* its length l */
    uint32_t row;               /* its representative row k */
} archon_hip_repeat;
/* device lcp[n], bwt[n] (any address) and out; on `stream` (NULL = the context's own), complete on return */
int  archon_hip_repeats_dev(const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, uint32_t kind, uint32_t min_len,
                            uint32_t min_occ, archon_hip_repeat *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream);
/* host lcp[n], bwt[n] and out */
int  archon_hip_repeats(const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base_id, uint32_t kind, uint32_t min_len,
                        uint32_t min_occ, archon_hip_repeat *out_or_null, uint64_t cap, uint64_t *total, int dev);
/* the resident block of the handle's last forward: its LCP array is computed on the device (as archon_hip_block_lcp does, and
 * with the same record in archon_hip_lcp_stats) and consumed there, it never visits the host: 4 n bytes of staging beside the
 * 8 n bytes of arena the LCP call takes and the repeats call takes over.  out is a host buffer.  ARCHON_E_ARG when that
 * forward kept no suffix array. */
int  archon_hip_block_repeats(archon_hip_block *b, uint32_t kind, uint32_t min_len, uint32_t min_occ, archon_hip_repeat *out_or_null,
                              uint64_t cap, uint64_t *total);
/* the CALLING THREAD's last repeats call on `dev`; repeats calls leave every other record alone (archon_hip_block_repeats
 * also keeps the LCP record of its LCP step) */
typedef struct archon_hip_repeat_stats {
    uint32_t n, kind, min_len, min_occ;     /* of the call, as given */
    uint32_t fan, levels;       /* F and L of the hierarchy */
    uint32_t longest;           /* the longest repeat that passed kind and filters */
    uint32_t kernel_launches;   /* launches issued by the call (block form: without those of its LCP step) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call (block form: the LCP step's included) */
    uint32_t reserved0;
    uint64_t intervals;         /* all LCP intervals: follows from lcp alone */
    uint64_t repeats;           /* those that passed kind and filters: *total */
    uint64_t occurrences;       /* hi - lo summed over them */
    uint64_t sum_lcp;           /* lcp[1] + ... + lcp[n-1] */
    uint64_t distinct_substrings;   /* n (n + 1) / 2 - sum_lcp */
    uint64_t probes;            /* entries of lcp and of the hierarchy the searches of the count pass read */
    float ms_lcp;               /* block form: device time of the LCP step */
    float ms_count, ms_emit;    /* device time of the count pass (hierarchy and flag sums included) and of the emit pass */
    float reserved1;
} archon_hip_repeat_stats;
int  archon_hip_get_repeat_stats(int dev, archon_hip_repeat_stats *out);

/* ---- longest previous factors and the LZ77 parse of a block (no counterpart in the reference) ---------------------------
 * What a caller computes next from the suffix array and its LCP array: how far back every prefix of the block repeats, and the
 * greedy parse into phrases that follows from it -- the phrase count z as a measure of repetitiveness, the phrases for relative
 * compression, LZ-based indexes or the front half of an LZ coder.  Rows, items, sa, lcp and a7 order are those above: row r
 * holds item sa[r] in 1..n, the key of item s is x[s-1], x[s-2], ..., x[0], INF; lcp[0] is taken as 0 whatever it holds.
 * Direction: with dir = 0 (earlier) an item t is admissible for s when t < s, with dir = 1 (later) when t > s.
 * LPF of item s: the largest l such that x[s-l .. s) = x[t-l .. t) for an admissible t.  On the arrays, with r the row of s:
 *   p = the greatest row < r holding an admissible item, L = min lcp[p+1 .. r], or 0 if there is no such p;
 *   q = the least row > r holding an admissible item,    R = min lcp[r+1 .. q], or 0 if there is no such q;
 *   source rule: if L >= R and L > 0 then len = L, src = sa[p]; else if R > 0 then len = R, src = sa[q]; else len = src = 0.
 * The output is one struct archon_hip_lpf {len, src} per item, stored at index s - 1: text order, not row order.
 * Parse: start with e = n; while e > 0 emit the phrase {end, len, src} = (e, len(e), src(e)) and set e -= min(max(1, len(e)), e).
 * A phrase with len 0 is the literal x[e-1]; otherwise x[e-len .. e) = x[src-len .. src).  Output order is chain order, the
 * phrase ending at n first.  The min with e is a guard, taken although a true LPF never exceeds e: the parse is a rule about
 * the len words of ANY array, it stays inside the buffers and emits at most n phrases whatever they hold.  With true LPF
 * records the phrase lengths, a literal read as 1, sum to n.
 * The two directions: dir 0 parses x itself, every phrase copies from strictly earlier text (overlap allowed), so the parse
 * decodes left to right.  For a text z pass x = reverse(z) with dir 1: the chain is then the textbook greedy LZ77 of z, left to
 * right; a phrase (end, len, src) starts at z position n - end and copies from z position n - src.
 * Examples.  "banana" (sa = 2 4 6 1 3 5, lcp = 0 1 3 0 0 2): dir 0 gives (len, src) for items 1..6 = (0,0) (0,0) (0,0) (1,2)
 * (2,3) (3,4) and the phrases (6,3,4) (3,0,0) (2,0,0) (1,0,0); dir 1 gives (0,0) (1,4) (2,5) (3,6) (0,0) (0,0) and the phrases
 * (6,0,0) (5,0,0) (4,3,6) (1,0,0).  "abracadabra" with dir 0 gives the phrases (11,4,4) (7,0,0) (6,1,4) (5,0,0) (4,1,1)
 * (3,0,0) (2,0,0) (1,0,0).
 * Cap rule of the parse (that of archon_hip_repeats): *total is a host pointer and always written.  out NULL: counting only,
 * no emit pass.  cap < *total with out given: ARCHON_E_ARG, *total written, out untouched.  ARCHON_E_ARG for a null sa, lcp or
 * lpf, n = 0 or dir > 1; n = 1 gives one literal.
 * Work of the LPF pass: p and q are nearest-smaller-value searches over sa, L and R range minima over lcp.  Two hierarchies
 * with fan-out F = 16 (level j holds the minimum of each F^j rows of lcp, and the least -- dir 1: the greatest -- item of them;
 * L = ceil(log_F n) levels) answer both in one walk per side: at most F - 1 node pairs per level on the way up and F on the way
 * down, so for ANY data
 *   probes <= 2 (2 F - 1) L n
 * (a block of one repeated byte has sa descending: with dir 0 every left search runs to row 0).
 * Work of the parse: tiles of T = 256 items in K levels, T^K >= n.  F_k[e], the first chain node below e's level-k tile, costs
 * one gather per item and level (k = 1 in LDS, every higher level in T launches); the descent marks the path from n with one
 * walker per tile and level.  `hops` is the longest walk of each level of the descent, summed -- the dependent steps on the
 * call's critical path -- and for ANY data
 *   hops <= ceil(n / T^(K-1)) + (K - 1) T <= K T.
 * Bad input.  An sa value outside 1..n is never used as an index: ARCHON_E_CORRUPT, the output untouched.  A value that occurs
 * twice, or an lcp that is not the LCP array of anything, returns ARCHON_OK with unspecified contents; every access stays inside
 * the buffers.  The parse accepts any len words (above).
 * Workspace, from the calling thread's context arena: the LPF pass 8 n / (F - 1) bytes (0.54 n); the parse 4 (K - 1) n bytes of
 * F arrays, n bytes of marks and n / 60 bytes of entry and tile words: 5 n up to 2^16 items, 9 n up to 2^24, 13 n above.  The
 * host forms stage sa, lcp, the records and the phrases besides. */
struct archon_hip_lpf {         /* (a tag only: the name is also that of the call below) */
    uint32_t len;               /* the longest previous factor that ends at the item */
    uint32_t src;               /* the item where a copy of it ends (0 when len is 0) */
};
typedef struct archon_hip_lpf archon_hip_lpf_rec;
typedef struct archon_hip_phrase {
    uint32_t end;               /* the item the phrase ends at: it covers x[end - max(1, len) .. end) */
    uint32_t len, src;          /* the record of that item: len 0 is the literal x[end-1] */
} archon_hip_phrase;
/* device sa[n], lcp[n] (any address) and lpf[n] (8-byte aligned); on `stream` (NULL = the context's own), complete on return */
int  archon_hip_lpf_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t dir, archon_hip_lpf_rec *d_lpf, int dev, void *stream);
/* host sa[n], lcp[n] and lpf[n] */
int  archon_hip_lpf(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t dir, archon_hip_lpf_rec *lpf, int dev);
/* device lpf[n] (any 4-byte aligned address: only the len words decide the chain, len and src of the chain's items are copied)
 * and out; on `stream`, complete on return */
int  archon_hip_lz_parse_dev(const archon_hip_lpf_rec *d_lpf, uint32_t n, archon_hip_phrase *d_out_or_null, uint64_t cap, uint64_t *total,
                             int dev, void *stream);
/* host lpf[n] and out */
int  archon_hip_lz_parse(const archon_hip_lpf_rec *lpf, uint32_t n, archon_hip_phrase *out_or_null, uint64_t cap, uint64_t *total, int dev);
/* the resident block of the handle's last forward: its LCP array is computed on the device (as archon_hip_block_lcp does, and
 * with the same record in archon_hip_lcp_stats), the LPF pass and the parse run there; neither array visits the host unless
 * asked for: lpf_or_null (host, n records) is written when the LPF pass succeeded, out_or_null (host) under the cap rule.
 * 12 n bytes of staging (the LCP array and the records) beside the arena.  ARCHON_E_ARG when that forward kept no suffix array. */
int  archon_hip_block_lz(archon_hip_block *b, uint32_t dir, archon_hip_lpf_rec *lpf_or_null, archon_hip_phrase *out_or_null, uint64_t cap,
                         uint64_t *total);
/* the CALLING THREAD's last LZ call on `dev` (an LPF call leaves the parse's fields 0, a parse call those of the LPF pass); LZ
 * calls leave every other record alone (archon_hip_block_lz also keeps the LCP record of its LCP step) */
typedef struct archon_hip_lz_stats {
    uint32_t n, dir;            /* of the call, as given (dir: 0 for a parse call) */
    uint32_t fan, levels;       /* F and L of the LPF pass's hierarchies */
    uint32_t tile, parse_levels;    /* T and K of the parse */
    uint32_t longest;           /* the largest len among the phrases */
    uint32_t kernel_launches;   /* launches issued by the call (block form: without those of its LCP step) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call (block form: the LCP step's included) */
    uint32_t reserved0;
    uint64_t phrases;           /* z: *total */
    uint64_t literals;          /* phrases with len 0 */
    uint64_t probes;            /* node pairs the searches of the LPF pass read */
    uint64_t hops;              /* the longest walk of each level of the descent, summed */
    float ms_lcp;               /* block form: device time of the LCP step */
    float ms_lpf;               /* device time of the LPF pass, its hierarchies included */
    float ms_parse;             /* device time of the F arrays, the descent and the count pass */
    float ms_emit;              /* device time of the scan and the emit pass */
} archon_hip_lz_stats;
int  archon_hip_get_lz_stats(int dev, archon_hip_lz_stats *out);

/* ---- the k-mers of a block: their counts, the count at every position, the shortest unique substrings (no counterpart in the
 * reference) ----------------------------------------------------------------------------------------------------------------
 * What a caller asks of a suffix-sorted block first: how often does each k-mer occur?  Which k-mers exist and with what counts
 * (the spectrum), how often the k-mer at each text position occurs (the mappability track of genomics), and which substrings
 * are unique -- seed selection, error thresholds, repeat masking, unique markers.  All of it follows from sa and lcp in a few
 * streaming passes, with no search structure.  Rows, items, sa, lcp and a7 order are those above: row r holds item sa[r] in
 * 1..n, the key of item s is x[s-1], x[s-2], ..., x[0], INF; lcp[0] is taken as 0 whatever it holds, and lcp[n] as 0.
 * k-mer groups, for k >= 1: row i STARTS A GROUP when i == 0 or lcp[i] < k; group g is the rows [starts[g], starts[g+1]), with n
 * after the last group.  A group is a k-mer exactly when sa[lo] >= k: then all its rows hold the string w = x[e-k .. e), e =
 * sa[r]; [lo, hi) is what archon_hip_fm_count(w) returns, and the occurrences start at sa[r] - k.  A group with sa[lo] < k is a
 * single SHORT ROW, whose key ends in INF before k symbols: there are exactly min(k - 1, n) of them.  k > n gives no k-mers;
 * k = 0 is ARCHON_E_ARG.  Output order is ascending row: ascending order of the reversed k-mer, a7 order.
 * Example "banana" (sa = 2 4 6 1 3 5, lcp = 0 1 3 0 0 2), as (lo, hi, item): k = 1 gives (0,3,2) "a", (3,4,1) "b", (4,6,3) "n";
 * k = 2 gives (0,1,2) "ba", (1,3,4) "na", (4,6,3) "an" (a7 order: by the reversed bytes ab, an, na); k = 3 gives (1,3,4) "ana", (4,5,3) "ban", (5,6,5) "nan", rows 0 and 3
 * being short.
 * Filters: min_occ <= hi - lo <= max_occ is kept; min_occ 0 behaves as 1, max_occ 0 means no limit.  They change the output and
 * the `kmers` and `occurrences` counters only.
 * Histogram: hist[c], c in 1 .. bins-1, is the number of distinct k-mers with exactly c occurrences; the last bin holds every
 * k-mer with >= bins-1 occurrences, bin 0 stays 0.  It covers ALL k-mers, not only those the filters keep: the spectrum of the
 * block for that k.  bins is in 2 .. 4096, or 0 with a NULL hist; anything else is ARCHON_E_ARG.
 * Cap rule (that of archon_hip_repeats): *total is a host pointer and always written.  out NULL: counting only, no emit pass.
 * cap < *total with out given: ARCHON_E_ARG, *total and the histogram written, out untouched.
 * Per-position counts: occ[p], p in 0 .. n-k, is the number of occurrences of x[p .. p+k) in x: for a row r of a k-mer group,
 * occ[sa[r] - k] = hi - lo.  n - k + 1 words in text order; with k > n nothing is written.  "banana": k = 1 gives 1 3 2 3 2 3,
 * k = 2 gives 1 2 2 2 2, k = 3 gives 1 2 1 2.
 * Shortest unique substring ending at an item: with r the row of item e and m = max(lcp[r], lcp[r+1]), sus[e-1] = m + 1 if
 * m + 1 <= e, else 0: the whole prefix x[0 .. e) occurs again, so nothing that ends at e is unique.  n words in text order.
 * x[e-L .. e) with L = sus[e-1] > 0 occurs once and every shorter suffix of it at least twice; and occ[p] == 1 exactly when
 * 0 < sus[p+k-1] <= k.  "banana": 1 2 3 4 3 4.  A caller who wants the shortest unique substring STARTING at a position passes
 * the reversed text, as for the textbook LZ77 parse above: item e of reverse(z) is position n - e of z.
 * Invariants of the record: distinct + short_rows == groups; the counts of all k-mers sum to n - k + 1 when k <= n; hist sums
 * to distinct.
 * Work: bounds (reads sa and lcp, 8 n bytes), a one-workgroup scan of the tile words, starts (reads lcp, writes 4 G), then
 *   kmers      the count pass over the G groups (two words of starts and one item each), and with out given a scan and the same
 *              pass again storing 12 bytes per k-mer: 4 launches counting, 6 with the emit pass; 1 host wait, 2 when a
 *              histogram is given or the emit pass runs (out given and *total > 0)
 *   kmer_occ   one pass over the rows (sa and lcp again, two cached words of starts, one scattered 4-byte store per row):
 *              4 launches; 1 host wait, 2 in the host and block forms
 *   sus        a check of sa and one pass (lcp, sa, one scattered store per row): 2 launches; 1 host wait, 2 in the host and
 *              block forms
 * (the block forms add the waits of their LCP step, not its launches).
 * Bad input.  An sa value outside 1..n is never used as an index: ARCHON_E_CORRUPT, the outputs untouched (*total is 0).  A
 * value that occurs twice, or an lcp that is not the LCP array of anything, returns ARCHON_OK with unspecified contents; every
 * access stays inside the buffers and every emitted record has lo < hi <= n.
 * Workspace, from the calling thread's context arena: 4 (n + 1) bytes of starts, n / 256 bytes of tile words and 16 KiB of
 * histogram; sus takes none.  The host forms stage sa, lcp and the result besides.
 * Locating and document frequency need no new call: a k-mer (lo, hi) is located by archon_hip_block_fm_locate_mems /
 * archon_hip_fm_locate_mems with an archon_hip_fm_mem {lo, hi, start 0, end k}, and archon_hip_fm_docs_ranges over lo and hi
 * lists the documents of every k-mer. */
typedef struct archon_hip_kmer {
    uint32_t lo, hi;            /* the rows of the k-mer's occurrences */
    uint32_t item;              /* sa[lo], the end of one of them: the bytes are x[item-k .. item) */
} archon_hip_kmer;
/* device sa[n], lcp[n], out and hist (any 4-byte aligned address); on `stream` (NULL = the context's own), complete on return */
int  archon_hip_kmers_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ,
                          archon_hip_kmer *d_out_or_null, uint64_t cap, uint64_t *total, uint32_t *d_hist_or_null, uint32_t bins, int dev,
                          void *stream);
/* host sa[n], lcp[n], out and hist */
int  archon_hip_kmers(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ,
                      archon_hip_kmer *out_or_null, uint64_t cap, uint64_t *total, uint32_t *hist_or_null, uint32_t bins, int dev);
/* the resident block of the handle's last forward and its suffix array (ARCHON_E_ARG when that forward kept none): its LCP array
 * is computed on the device (as archon_hip_block_lcp does, and with the same record in archon_hip_lcp_stats) and consumed there,
 * it never visits the host.  out and hist are host buffers. */
int  archon_hip_block_kmers(archon_hip_block *b, uint32_t k, uint32_t min_occ, uint32_t max_occ, archon_hip_kmer *out_or_null, uint64_t cap,
                            uint64_t *total, uint32_t *hist_or_null, uint32_t bins);
/* occ[n - k + 1] on the device, on the host, of the resident block (host occ) */
int  archon_hip_kmer_occ_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t k, uint32_t *d_occ, int dev, void *stream);
int  archon_hip_kmer_occ(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t k, uint32_t *occ, int dev);
int  archon_hip_block_kmer_occ(archon_hip_block *b, uint32_t k, uint32_t *occ);
/* sus[n] on the device, on the host, of the resident block (host sus) */
int  archon_hip_sus_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t *d_sus, int dev, void *stream);
int  archon_hip_sus(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t *sus, int dev);
int  archon_hip_block_sus(archon_hip_block *b, uint32_t *sus);
/* the CALLING THREAD's last call of this family on `dev`; these calls leave every other record alone (the block forms also keep
 * the LCP record of their LCP step).  A kmer_occ call fills `groups` and leaves the other work counters 0, a sus call all of them */
typedef struct archon_hip_kmer_stats {
    uint32_t n, k, min_occ, max_occ;        /* of the call, as given (k 0 for sus) */
    uint32_t bins;              /* of the call, as given */
    uint32_t tile;              /* rows of a tile of the passes */
    uint32_t what;              /* 0 kmers, 1 kmer_occ, 2 sus */
    uint32_t kernel_launches;   /* launches issued by the call (block form: without those of its LCP step) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call (block form: the LCP step's included) */
    uint32_t most;              /* the largest count of a k-mer */
    uint64_t groups;            /* G: rows that start a group */
    uint64_t short_rows;        /* groups that are a short row */
    uint64_t distinct;          /* groups that are a k-mer: all k-mers of the block */
    uint64_t kmers;             /* those that passed the filters: *total */
    uint64_t occurrences;       /* hi - lo summed over them */
    uint64_t unique;            /* k-mers with one occurrence */
    float ms_lcp;               /* block form: device time of the LCP step */
    float ms_count;             /* device time of bounds, scan and starts, and of the count pass of kmers */
    float ms_emit;              /* device time of the scan of the group tiles and the emit pass */
    float ms_scatter;           /* device time of the occ pass; of the check and the pass of sus */
} archon_hip_kmer_stats;
int  archon_hip_get_kmer_stats(int dev, archon_hip_kmer_stats *out);

/* ---- the minimal absent words of a block (no counterpart in the reference) ----------------------------------------------------
 * The calls above say what occurs in a block, how often and where; this one gives the complement.  A MINIMAL ABSENT WORD (MAW)
 * of x is a string that does not occur in x while every proper substring of it does: the nullomers of a genome, a negative
 * dictionary, the basis of alignment-free comparison.  Rows, items, sa, lcp, bwt, the primary row `base` and a7 order are those
 * of the repeats section; lcp[0] reads as 0.
 * Definition.  A MAW of x of length at least 2 is a.w.b (bytes a, b, a string w, possibly empty) such that a.w occurs in x, w.b
 * occurs in x and a.w.b does not.  Bytes that do not occur in x at all (the absent words of length 1) are not reported: they are
 * the empty buckets, and the record counts them (absent_bytes).
 * The same in rows.  A NODE is the root -- l = 0, rows [0, n), ordered as row 0 -- or an LCP interval (lo, hi, l, k) exactly as
 * archon_hip_repeats kind 0 defines it, k its representative row.  The CHILDREN of a node are the pieces of [lo, hi) cut at every
 * row q in (lo, hi) with lcp[q] == l.  All rows of a child [clo, chi) hold the same symbol at depth l of their key: the byte
 * a = x[sa[clo] - l - 1], and then [clo, chi) is what archon_hip_fm_count(a.w) returns; or INF, when sa[clo] == l: a single row,
 * the occurrence of w at the start of the text, which names no a and yields no word.  B([p, q)) is the set of bwt[r] for r in
 * [p, q) with r != base; for the root only, B(node) also takes bwt[base] = x[0], which follows no item, so that B(root) is the
 * set of bytes that occur in x.  The words of a node are, for each child with a byte a, the words a.w.b for every b in
 * B(node) \ B(child).  Only the root and the nodes that are maximal repeats (kind 1: bwt[lo .. hi) not all equal, or base
 * inside) can yield a word: a right-uniform node has B(child) == B(node) for every child.
 * Output order: nodes in ascending representative row, the root first; within a node the children in ascending row; within a
 * child b ascending.  The order is the same on every run.
 * Examples.  "banana" (sa 2 4 6 1 3 5, lcp 0 1 3 0 0 2, BWT nnbaaa, base 2) gives seven words, as (lo, hi, len, item, last):
 * (0,3,2,2,'a') "aa", (0,3,2,2,'b') "ab", (3,4,2,1,'b') "bb", (3,4,2,1,'n') "bn", (4,6,2,3,'b') "nb", (4,6,2,3,'n') "nn" from
 * the root, and (2,3,5,6,'n') "nanan" from the node (1,3,3,2) "ana".  "abracadabra" gives 25: 18 of length 2; cab, cac, dac,
 * dad, rab, rad from the node (0,5,1,1) "a", whose fourth child is the INF row of item 1; dabrac from the node (2,4,4,3) "abra".
 * A block of n equal bytes c gives exactly one word, c repeated n + 1 times (n = 1 included).
 * Filters: min_len <= len <= max_len is kept; min_len 0 or 1 behaves as 2, max_len 0 means no limit; min_len > max_len with
 * max_len != 0 is ARCHON_E_ARG.  A node with l + 2 outside the filter does no set work (the root counts as l = 0): words up to
 * a small length is the common use, and cheap.
 * Cap rule (that of archon_hip_repeats): *total is a host pointer and always written.  out NULL: counting only.  cap < *total
 * with out given: ARCHON_E_ARG, out untouched.  (More than 2^32 - 1 words are counted but not emitted: ARCHON_E_ARG.)
 * Bad input.  An sa value outside 1..n: ARCHON_E_CORRUPT, the outputs untouched (*total is 0).  Arrays that are not the SA, LCP
 * array or BWT of anything return ARCHON_OK with unspecified contents; every access stays inside the buffers, and a node is
 * left after 257 children.  Null pointers, n = 0, base_id >= n or the filter above: ARCHON_E_ARG with *total = 0.
 * Method (csrc/maw.hiph).  The check of sa; the minimum hierarchy over lcp and the flag sums S of a repeats call of kind 1, so
 * that right-uniform is S[hi] == S[lo + 1]; a rank table over the BWT (the FM index's; the host and device forms build one over
 * a copy of bwt for the call, the block form uses and keeps the block's own).  Then one pass, run twice (count, and emit behind
 * a scan of the tile words): every lane settles one row as the repeats pass does, and the wave then takes the rows that are
 * nodes one after the other: B(node), then child by child (one right search for the next cut) B(child) and
 * popc(B(node) & ~B(child)) words.  A set over at most direct_rows (64) rows is read from bwt, a row per lane; a longer one is
 * ONE expansion of the rank table (all 256 children of the range at once; the ones that are nonempty are the set).
 * Bounds, for any arrays: the children of all nodes together are at most 2n; per row one left search, per node and per child
 * one right search, each within the repeats bound of 2F - 1 entries per level; a set costs at most 64 row reads or one
 * expansion.  A block of one byte has n - 1 nested intervals of which all but [0, n) are right-uniform: they are dropped after
 * the left search and one comparison of S, and [0, n) gives the one word.
 * Launches: 1 (check) + levels + 3 (flag sums) + 1 counting, 2 more with the emit pass; the host and device forms add the 3 of
 * the table, the block form only when it builds the block's.  Host waits: 1 counting, 2 with the emit pass; 1 more for a table
 * that is built; the block form adds those of its LCP step.
 * Workspace, from the calling thread's context arena: that of a repeats call of kind 1 (4 (n + 1) bytes of S, about 4 n / (F-1)
 * of hierarchy) and n / 64 bytes of tile words; the host and device forms hold a copy of the BWT and its table (about 1.5 n
 * bytes) for the duration of the call. */
typedef struct archon_hip_maw {
    uint32_t lo, hi;            /* the rows of a.w: the occurrences of the word without its last byte */
    uint32_t len;               /* the length of the word, l + 2 */
    uint32_t item;              /* sa[lo]: a.w = x[item-len+1 .. item) */
    uint32_t last;              /* b (0..255) */
} archon_hip_maw;               /* 20 bytes; the word is x[item-len+1 .. item) followed by `last` */
/* device sa[n], lcp[n], bwt[n] and out (any 4-byte aligned address); on `stream` (NULL = the context's own), complete on return */
int  archon_hip_maws_dev(const uint32_t *d_sa, const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, uint32_t min_len,
                         uint32_t max_len, archon_hip_maw *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream);
/* host sa[n], lcp[n], bwt[n] and out */
int  archon_hip_maws(const uint32_t *sa, const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base_id, uint32_t min_len, uint32_t max_len,
                     archon_hip_maw *out_or_null, uint64_t cap, uint64_t *total, int dev);
/* the resident block of the handle's last forward and its suffix array (ARCHON_E_ARG when that forward kept none): its LCP array
 * is computed on the device as archon_hip_block_repeats does; the rank table is the block's own, built on the first FM call
 * after a forward and kept -- this call builds it when it is missing and says so (`built`).  out is a host buffer. */
int  archon_hip_block_maws(archon_hip_block *b, uint32_t min_len, uint32_t max_len, archon_hip_maw *out_or_null, uint64_t cap, uint64_t *total);
/* the CALLING THREAD's last call of this family on `dev`; these calls leave every other record alone (the block form also keeps
 * the LCP record of its LCP step).  Every counter but the two sets_* and probes follows from x and the filters alone; sets_*
 * from x, the filters and direct_rows; probes also from the fan-out */
typedef struct archon_hip_maw_stats {
    uint32_t n, min_len, max_len;   /* of the call, as given */
    uint32_t fan, levels;       /* fan-out and levels of the minimum hierarchy over lcp */
    uint32_t direct_rows;       /* a set over at most this many rows is read from bwt, a longer one from the rank table */
    uint32_t built;             /* 1 when this call built a rank table */
    uint32_t kernel_launches;   /* launches issued by the call (block form: without those of its LCP step) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call (block form: the LCP step's included) */
    uint32_t absent_bytes;      /* 256 less the bytes that occur in x: the absent words of length 1 */
    uint32_t shortest, longest; /* of the words that passed; 0 when there is none */
    uint64_t intervals;         /* all LCP intervals, as a repeats call reports them */
    uint64_t nodes;             /* the root and the maximal repeats, of those whose l + 2 passes the filter */
    uint64_t children;          /* children visited over those nodes, the INF ones included */
    uint64_t sets_direct;       /* byte sets read from bwt: one per node and one per child with a byte */
    uint64_t sets_table;        /* ... taken from the rank table */
    uint64_t words;             /* *total */
    uint64_t probes;            /* entries of the hierarchy the searches read */
    float ms_lcp;               /* block form: device time of the LCP step */
    float ms_build;             /* device time of the table build, when built */
    float ms_count;             /* device time of the check, the hierarchy, the flag sums and the count pass */
    float ms_emit;              /* device time of the scan of the tile words and the emit pass */
} archon_hip_maw_stats;
/* (not named archon_hip_get_*_stats: it behaves as those do) */
int  archon_hip_maw_last_stats(int dev, archon_hip_maw_stats *out);

/* ---- order-k entropy, substring complexity and BWT runs of a block (no counterpart in the reference) ----------------------------
 * How compressible is this block, and at which context order?  Block-sorting coders are judged against the empirical entropy H_k;
 * the usual measures of repetitiveness are z (LZ77 phrases: archon_hip_block_lz), r (the runs of the BWT) and delta (the substring
 * complexity).  Rows, items, sa, lcp, bwt, the primary row `base` and a7 order are those of the repeats and k-mer sections;
 * lcp[0] reads as 0.
 * 1. Order-k statistics, k >= 0.  By the text: for every string w of length k let F_w be the multiset of the bytes x[p] with
 * k <= p < n and x[p-k .. p) = w (an occurrence of w at the very end of x is followed by nothing and adds nothing).  contexts =
 * the w with F_w not empty; deterministic = the w with exactly one distinct byte in F_w; pairs = the sum over w of the distinct
 * bytes of F_w, which is the number of distinct (k+1)-mers of x; symbols = the sum of |F_w| = max(n - k, 0); bits = the sum over
 * w and c of n_wc log2(|F_w| / n_wc) = n H_k(x).  By rows, k >= 1: the groups are those of archon_hip_kmers; a group with
 * sa[lo] < k is a short row and adds nothing; for a k-mer group [lo, hi), F is bwt[r] for r in [lo, hi), r != base; a group left
 * empty by that (the single row base) is no context.  k = 0: one group [0, n), and bwt[base] = x[0] counts, so that bits is
 * n H_0(x).  k > n: the record is all zero but for k.
 * Examples.  "banana" (BWT nnbaaa, base 2): k = 0 gives contexts 1, deterministic 0, pairs 3, symbols 6, bits 8.754887502163468;
 * k = 1, 2, 3 give (3, 3, 3, 6 - k, 0.0).  "abracadabra": k = 0 (1, 0, 5, 11, 22.44410733057346), k = 1 (5, 4, 7, 10, 6.0),
 * k = 2 (7, 7, 7, 9, 0.0).  pairs at k equals `distinct` of an archon_hip_kmers call at k + 1; bits never grows with k.
 * 2. Substring complexity.  d_l, the number of distinct substrings of length l, is n - l + 1 - #{i >= 1 : lcp[i] >= l}: each of the
 * n - l + 1 items of length at least l starts a new l-mer unless it shares l symbols with the row before it.  counts[l-1] = d_l for
 * l = 1 .. max_len; max_len 0 behaves as min(n, 4095), a value above n as n.  substrings = n (n + 1) / 2 - lcp_sum is the number
 * of all distinct substrings.  delta = max over l of d_l / l is reported as (delta_len, delta_count), compared exactly by 64-bit
 * cross-multiplication, ties to the smallest l, over l <= max_len; delta_exact = 1 when max_len == n or
 * delta_count (max_len + 1) >= (n - max_len) delta_len: no longer l can beat it, since d_l <= n - l + 1.
 * 3. BWT runs.  runs = 1 + #{i >= 1 : bwt[i] != bwt[i-1]} over the n stored bytes, the one at base included: what the -m stage
 * sees.  longest_run is the length of the longest one.  Without a bwt both are 0.
 * Examples.  "banana": d = 3 3 3 3 2 1, substrings 15, lcp_sum 6, lcp_max 3, delta (1, 3), runs 3, longest_run 3.
 * "abracadabra": d = 5 7 7 7 7 6 5 4 3 2 1, substrings 54, lcp_sum 12, lcp_max 4, delta (1, 5), runs 7, longest_run 4.
 * Arguments.  ks[nk] and out[nk] are host arrays, 1 <= nk <= 64; the records come in the order of ks.  rec is a host pointer.
 * Bad input.  Null pointers (counts and, for complexity, bwt may be null), n = 0, nk outside 1..64 and base_id >= n:
 * ARCHON_E_ARG, with the records zeroed.  An sa value outside 1..n: ARCHON_E_CORRUPT, the outputs untouched.  Arrays that are
 * not the SA, LCP array or BWT of anything return ARCHON_OK with unspecified contents; every access stays inside the buffers.  No
 * GPU: ARCHON_E_NODEVICE; there is no CPU fallback.
 * Method (csrc/entropy.hiph).  Per order k >= 1 the bounds, scan and starts passes of a k-mer call, then the follower pass over
 * tiles of rows (the tile is that of the k-mer passes) and a reduction.  The 64 rows a wave holds in one step are its window.  A
 * group inside the window is settled by the wave without a loop over rows: each lane holds (group, byte), and the classes of
 * equal pairs are peeled by a ballot and a popcount, the first lane of a class adding c log2(m / c); a group of one row costs
 * nothing (groups_in_wave).  A group of at most direct_rows (64) rows that ends past the window belongs to the wave that holds
 * its first row, which reads bwt[lo .. hi), a row per lane (groups_direct).  A longer group is ONE expansion of the FM index's
 * rank table: the 256 child sizes are the follower counts, the primary row left out (groups_table), so a block of one byte at
 * k = 5 is one expansion, not n row reads.  No group is read by two waves.  Order 0 is one expansion of [0, n) and x[0].  bits is
 * summed in doubles without floating-point atomics -- lanes, wave, tile slot, then a fixed-order reduction --, so the same call
 * with the same tile gives the same 64 bits on every run.  The host and device forms build a rank table over a copy of bwt for
 * the call, the block form uses and keeps the block's own.  Complexity: a histogram of lcp (bins below 4096 in LDS per workgroup,
 * higher ones by global atomics, values of max_len and above in the last bin), one streaming pass over bwt for the runs, and one
 * workgroup for the suffix sums, the arg-max and the longest run.
 * Launches: entropy 5 per order in 1..n, 1 for order 0, none for an order above n; the host and device forms add the 3 of the
 * table, the block form only when it builds the block's.  Complexity 2, 3 with a bwt.  Host waits: ONE per call, however many
 * orders it takes -- the words of the orders stay on the device until the end; the host and device forms of entropy add 1 for the
 * table they build, the block forms those of their LCP step (and 1 for a table that is built).
 * Workspace, from the calling thread's context arena: entropy that of a k-mer call, 8 bytes per tile and 4 KiB of records;
 * complexity 8 max_len bytes and 12 bytes per tile of rows. */
/* (the two records share their names with the host forms below, as struct stat does with stat(): they have no typedef and are
 * written `struct archon_hip_entropy`, `struct archon_hip_complexity`) */
struct archon_hip_entropy {               /* 48 bytes */
    uint32_t k, reserved;
    uint64_t contexts;          /* the k-mers that are followed by a byte somewhere */
    uint64_t deterministic;     /* ... always by the same one */
    uint64_t pairs;             /* distinct (context, byte) pairs: the distinct (k+1)-mers */
    uint64_t symbols;           /* max(n - k, 0) */
    double   bits;              /* n * H_k */
};
struct archon_hip_complexity {            /* 56 bytes */
    uint32_t n, max_len;        /* max_len as the call used it */
    uint32_t lcp_max;
    uint32_t delta_len, delta_count;    /* the l <= max_len with the largest d_l / l (the smallest such l), and d_l */
    uint32_t delta_exact;       /* 1: no l above max_len can beat it */
    uint32_t longest_run, reserved;
    uint64_t lcp_sum, substrings;
    uint64_t runs;              /* runs, longest_run 0 without a bwt */
};
/* device sa[n], lcp[n], bwt[n]; ks and out on the host; on `stream` (NULL = the context's own), complete on return */
int  archon_hip_entropy_dev(const uint32_t *d_sa, const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, const uint32_t *ks,
                            uint32_t nk, struct archon_hip_entropy *out, int dev, void *stream);
/* host sa[n], lcp[n], bwt[n] */
int  archon_hip_entropy(const uint32_t *sa, const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base_id, const uint32_t *ks, uint32_t nk,
                        struct archon_hip_entropy *out, int dev);
/* the resident block of the handle's last forward and its suffix array (ARCHON_E_ARG when that forward kept none): its LCP array
 * is computed on the device as archon_hip_block_kmers does; the rank table is the block's own, built on the first FM call after
 * a forward and kept -- this call builds it when it is missing and says so (`built`) */
int  archon_hip_block_entropy(archon_hip_block *b, const uint32_t *ks, uint32_t nk, struct archon_hip_entropy *out);
/* device lcp[n], bwt[n] or NULL, counts[max_len as used] or NULL (any 4-byte aligned address); rec on the host */
int  archon_hip_complexity_dev(const uint32_t *d_lcp, const uint8_t *d_bwt_or_null, uint32_t n, uint32_t max_len, uint32_t *d_counts_or_null,
                               struct archon_hip_complexity *rec, int dev, void *stream);
/* host lcp[n], bwt[n] or NULL, counts or NULL */
int  archon_hip_complexity(const uint32_t *lcp, const uint8_t *bwt_or_null, uint32_t n, uint32_t max_len, uint32_t *counts_or_null,
                           struct archon_hip_complexity *rec, int dev);
/* the resident block, its suffix array and its BWT; counts is a host buffer */
int  archon_hip_block_complexity(archon_hip_block *b, uint32_t max_len, uint32_t *counts_or_null, struct archon_hip_complexity *rec);
/* the CALLING THREAD's last call of this family on `dev`; these calls leave every other record alone (the block forms also keep
 * the LCP record of their LCP step).  The three groups_* follow from x, the orders, the tile and direct_rows */
typedef struct archon_hip_entropy_stats {
    uint32_t n, nk;             /* of the call (nk 0 for complexity) */
    uint32_t what;              /* 0 entropy, 1 complexity */
    uint32_t tile;              /* rows of a tile of the passes (test route KMER_TILE) */
    uint32_t direct_rows;       /* a group of at most this many rows is read from bwt, a longer one from the rank table */
    uint32_t built;             /* 1 when this call built a rank table */
    uint32_t kernel_launches;   /* launches issued by the call (block forms: without those of the LCP step) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call (block forms: the LCP step's included) */
    uint64_t groups_direct;     /* summed over the orders: k-mer groups of 2 .. direct_rows rows that end past their wave's window */
    uint64_t groups_table;      /* ... of more rows: one expansion each; order 0 counts one */
    uint64_t groups_in_wave;    /* ... inside their wave's window, those of one row included */
    float ms_lcp;               /* block forms: device time of the LCP step */
    float ms_build;             /* device time of the table build, when built */
    float ms_count;             /* device time of the passes */
} archon_hip_entropy_stats;
int  archon_hip_entropy_last_stats(int dev, archon_hip_entropy_stats *out);

/* ---- the runs (maximal repetitions, tandem repeats) of a block, and longest-common-extension queries -----------------------------
 * (no counterpart in the reference)  archon_hip_repeats lists WHICH strings recur; these calls list where a string recurs back to
 * back: `anana` in `banana`, a microsatellite in DNA, a repeated record in a log.  Rows, items, sa, lcp and a7 order are those of
 * the repeats section; lcp[0] reads as 0.
 * LCE.  For items s, t in 0..n, lce(s, t) is the number of leading symbols in which the a7 keys of s and t agree: the length of
 * the longest common suffix of x[0..s) and x[0..t).  lce(s, s) = s; lce(0, .) = 0; for s != t, both >= 1, it is
 * min lcp[min(r_s, r_t) + 1 .. max(r_s, r_t)] with r = isa[.], the row of the item.
 * Run.  (start, end, period) is a run of x when x[start..end) has smallest period p = period, end - start >= 2p, and it can be
 * extended neither way: start == 0 or x[start-1] != x[start-1+p], and end == n or x[end] != x[end-p].  A block has fewer than n
 * runs.
 * The rule.  It fixes the output order and the work counters, and needs only LCEs in the key direction and one second sort.
 * rank0[s] is the row of item s in the a7 suffix array of x, rank1[s] its row in the a7 suffix array of the complemented block
 * xc[i] = 255 - x[i]; every LCE is that of x.  For s = 1..n ascending, and for l = 0 then l = 1:
 *   1. t is the greatest item in 1..s-1 with rank_l[t] > rank_l[s]; none: no candidate.  p = s - t; a period filter that
 *      excludes p: no candidate.  Count `candidates`.
 *   2. R = lce(s, t).  R == 0: stop.
 *   3. If s + p <= n and lce(s + p, s) >= p: stop (this root is not the outermost one).  Otherwise count `roots`.
 *   4. L is the greatest l' in 0..min(p-1, n-s) with lce(s + l', t + l') >= l' (monotone in l'), found by
 *      lo = 0, hi = min(p-1, n-s); while lo < hi: m = (lo+hi+1)>>1; lce(s+m, t+m) >= m ? lo = m : hi = m-1.  R + L < p: stop.
 *   5. start = t - R, end = s + L.  The run is kept when start == 0 and l == 0; or start >= 1, l == 0 and
 *      rank0[start] > rank0[start+p]; or start >= 1, l == 1 and rank0[start] < rank0[start+p].  (The keys' first bytes
 *      x[start-1] and x[start-1+p] differ, so rank0 orders them.)  Count `runs`.
 *   6. The filters; emit (start, end, period, root = s).
 * Behind it is the runs theorem of Bannai et al.: descending rank0 is the suffix order of the reversed block under reversed byte
 * order with the end smallest, descending rank1 the same under plain byte order; step 1 is the longest Lyndon word that ends at
 * s; step 3 keeps one root per run, step 5 one order per run.  Every run is emitted exactly once, in ascending root.
 * lce_queries counts one per step 2, one per step 3 that is evaluated (s + p <= n), one per iteration of the loop of step 4.
 * Examples, as records (start, end, period, root), then candidates / roots / lce_queries:
 *   "banana"       (1,6,2,6)                                        7 / 1 / 8
 *   "mississippi"  (2,4,1,4) (5,7,1,7) (1,8,3,8) (8,10,1,10)       16 / 6 / 24
 *   "aaaa"         (0,4,1,4)                                        6 / 2 / 10
 *   "abracadabra"  none                                            18 / 5 / 26
 * Filters: min_period <= period, period <= max_period (0: no upper bound), end - start >= min_copies * period
 * (min_copies >= 2) and end - start >= min_len.  min_copies < 2, or min_period > max_period with max_period != 0:
 * ARCHON_E_ARG with *total = 0.
 * Cap rule (that of archon_hip_repeats): *total is a host pointer and always written.  out NULL: counting only.  cap < *total
 * with out given: ARCHON_E_ARG, *total written, out untouched.
 * Bad input.  sa or sa_c not a permutation of 1..n: ARCHON_E_CORRUPT, the outputs untouched (*total is 0).  A permutation that
 * is not the right suffix array, or an lcp that is no LCP array, returns ARCHON_OK with unspecified records; every access stays
 * inside the buffers.  An LCE item above n: ARCHON_E_ARG with nothing written (the device form finds it on the device); k = 0
 * writes nothing.  Null pointers, n = 0: ARCHON_E_ARG.  No GPU: ARCHON_E_NODEVICE; there is no CPU fallback.
 * Method (csrc/runs.hiph).  The inverse arrays rank0 and rank1 by a scatter that flags values outside 1..n and, in a second
 * kernel, leftovers; one minimum hierarchy over ~rank_l in item order per order (fan-out: test route LZ_FAN, default 16), so that
 * step 1 is one nearest-smaller-value walk to the left; the minimum hierarchy over lcp of a repeats call (test route REP_FAN),
 * so that an LCE is one range minimum.  Then one pass over tiles of 2048 items, run twice (count, and emit behind a scan of the
 * tile words): a lane takes an item and both orders.  The emit pass runs the rule again.  No atomics on the output.
 * Work, for any data: per item and order one left search of at most 31 ceil(log16 n) probes (2F - 1 per level) and at most
 * 2 + ceil(log2 p) LCEs, each one range minimum of at most 2(F - 1) entries per level.  A block of one byte drops every
 * candidate but the last at step 3.
 * Launches: 1 + 1 (scatter, leftovers) per array, the levels of the three hierarchies, 1 counting; 2 more with the emit pass.
 * The block form adds the complement kernel; the launches of its second forward transform and of its LCP step stay out of the
 * record.  Host waits: 1 counting, 2 with the emit pass
 * (the host form's copy back rides on the second); the block form adds those of its forward and LCP steps.  An LCE call: the
 * scatter, the leftovers, the lcp hierarchy, the check of the items and the query kernel; one wait, two in the host and block forms.
 * Workspace, from the calling thread's context arena: 8 (n + 1) bytes of inverse arrays, about 12 n / (F-1) of hierarchies,
 * n / 512 bytes of tile words (an LCE call: 4 (n + 1) and one hierarchy).  The host form stages sa, lcp and sa_c (12 n bytes). */
typedef struct archon_hip_run {
    uint32_t start, end;        /* x[start .. end) */
    uint32_t period;            /* its smallest period */
    uint32_t root;              /* the item s of the rule that found it, start + period <= root <= end; the output ascends in it */
} archon_hip_run;               /* 16 bytes */
/* host sa[n], lcp[n], items s[k], t[k] and out[k] */
int  archon_hip_lce(const uint32_t *sa, const uint32_t *lcp, uint32_t n, const uint32_t *s, const uint32_t *t, uint32_t k, uint32_t *out, int dev);
/* device arrays (any 4-byte aligned address); on `stream` (NULL = the context's own), complete on return */
int  archon_hip_lce_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, const uint32_t *d_s, const uint32_t *d_t, uint32_t k, uint32_t *d_out,
                        int dev, void *stream);
/* the resident block of the handle's last forward and its suffix array (ARCHON_E_ARG when that forward kept none); s, t and out
 * are host buffers */
int  archon_hip_block_lce(archon_hip_block *b, const uint32_t *s, const uint32_t *t, uint32_t k, uint32_t *out);
/* host sa[n], lcp[n], sa_c[n] (the a7 suffix array of the complemented block) and out */
int  archon_hip_runs(const uint32_t *sa, const uint32_t *lcp, const uint32_t *sa_c, uint32_t n, uint32_t min_period, uint32_t max_period,
                     uint32_t min_copies, uint32_t min_len, archon_hip_run *out_or_null, uint64_t cap, uint64_t *total, int dev);
/* device arrays and out (any 4-byte aligned address); on `stream`, complete on return */
int  archon_hip_runs_dev(const uint32_t *d_sa, const uint32_t *d_lcp, const uint32_t *d_sa_c, uint32_t n, uint32_t min_period, uint32_t max_period,
                         uint32_t min_copies, uint32_t min_len, archon_hip_run *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream);
/* The resident block and its suffix array.  The call complements the resident text into memory of its own (outside the arena),
 * runs a forward transform on that copy in the block's context -- archon_hip_get_stats and the resident block are left as they
 * were -- and keeps only rank1 of it; then the LCP step of archon_hip_block_repeats and the passes.  out is a host buffer. */
int  archon_hip_block_runs(archon_hip_block *b, uint32_t min_period, uint32_t max_period, uint32_t min_copies, uint32_t min_len,
                           archon_hip_run *out_or_null, uint64_t cap, uint64_t *total);
/* the CALLING THREAD's last runs or LCE call on `dev`; these calls leave every other record alone (the block forms also keep the
 * LCP record of their LCP step).  candidates, roots, lce_queries, runs, emitted and longest_period follow from x and the filters
 * alone; probes also from the fan-out */
typedef struct archon_hip_run_stats {
    uint32_t n;                 /* of the call */
    uint32_t min_period, max_period, min_copies, min_len;   /* the filters, as given (an LCE call: 0) */
    uint32_t what;              /* 0 runs, 1 LCE */
    uint32_t fan, lcp_fan;      /* fan-out of the rank hierarchies and of the hierarchy over lcp */
    uint32_t levels;            /* levels of the hierarchy over lcp */
    uint32_t longest_period;    /* of the records that passed every filter */
    uint32_t kernel_launches;   /* launches issued by the call (block forms: without those of the second sort and the LCP step) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call (block forms: the second sort's and the LCP step's included) */
    uint64_t candidates;        /* step 1 */
    uint64_t roots;             /* step 3 */
    uint64_t lce_queries;       /* steps 2, 3 and 4 (an LCE call: k) */
    uint64_t probes;            /* entries of the rank hierarchies the left searches read */
    uint64_t runs;              /* step 5: the runs whose period passes, before the copies and length filters */
    uint64_t emitted;           /* *total */
    float ms_forward;           /* block form: device time of the second sort */
    float ms_lcp;               /* block forms: device time of the LCP step */
    float ms_build;             /* device time of the inverse arrays and the hierarchies */
    float ms_count;             /* device time of the count pass (an LCE call: of the query kernel) */
    float ms_emit;              /* device time of the scan of the tile words and the emit pass */
} archon_hip_run_stats;
int  archon_hip_runs_last_stats(int dev, archon_hip_run_stats *out);

/* ---- matching statistics of a long text, and its relative LZ parse against the block ------------------------------------------
 * archon_hip_fm_ms runs one wave per pattern, so one long pattern runs on one wave.  These calls take ONE text P of m bytes --
 * another version of a file, a read set, the next block of a container -- and spread it over the device.  The result is defined
 * by the text and the block alone: for every end e in 1 .. m the record (len, lo, hi) is exactly the record archon_hip_fm_ms
 * defines for P as one pattern (len the largest l <= e with P[e-l .. e) in x, [lo, hi) what archon_hip_fm_count returns for that
 * piece, (0, 0, n) when P[e-1] is not in x).  No record shows where the text was cut.
 * Method.  P is cut into chunks of C bytes (1024); chunk c covers the ends in (cC, min(m, (c+1)C)] and s_c = cC.
 *   walk   the procedure above over the chunks as ceil(m / C) patterns, one wave each.  Chunk c starts from the empty match at
 *          s_c, so its record at e is that of the longest suffix of P[s_c .. e) in x: its len is min(ms(e), e - s_c).  A record
 *          is SATURATED when its len == e - s_c; every other record is already exact, and so is all of chunk 0.  Saturation is
 *          prefix-closed within a chunk.  A chunk is FULL when its last record is saturated.
 *   sweep  start[c], the exact record at end s_c, for every c >= 1: the walk's record at index s_c - 1 when c = 1 or chunk c - 1
 *          is not full, else join(start[c-1], C, the rows of chunk c-1's last record).  A run of full chunks is a chain of
 *          dependent joins: one lane per run, the runs in parallel.
 *   fix    one lane per end: a saturated record of a chunk c >= 1 becomes join(start[c], e - s_c, its own rows).  It reads
 *          start[] and its own record only, so no lane waits for another.
 * The join.  join((L, lo_s, hi_s), y, [lo, hi)) takes the exact state at s and the rows of Y = P[s .. e), |Y| = y, and needs the
 * suffix array and its inverse beside the LCP array.  For a row r in [lo, hi) let q(r) = isa[sa[r] - y], and q(r) = n when
 * sa[r] <= y (item 0, whose key is INF alone).  The rows of Y share reverse(Y) and then order by the key of the item before Y, so q
 * is strictly increasing over them.
 *   if L == 0: the result is (y, lo, hi)
 *   a = the first r with q(r) >= lo_s, b = the first r with q(r) >= hi_s (binary searches)
 *   if a < b:  the result is (y + L, a, b)
 *   else:      lp = min lcp[q(a-1)+1 .. lo_s] when a > lo, else 0;  ls = min lcp[hi_s .. q(a)] when a < hi, else 0 (lcp[n] is 0)
 *              l = max(lp, ls);  if l == 0 the result is (y, lo, hi)
 *              u = the greatest p <= lo_s with lcp[p] < l;  v = the least p >= hi_s with lcp[p] < l, or n   (the parent move above)
 *              the result is (y + l, the first r with q(r) >= u, the first r with q(r) >= v)
 * The two range minima use the hierarchy of the attached LCP array: at most 2 (F - 1) entries per level each, and the two
 * searches at most 2 (2 F - 1) per level as above.
 * Example: "banana" (sa 2 4 6 1 3 5, isa[1..6] = 3 0 4 1 5 2, lcp 0 1 3 0 0 2), the text "nanan" and C = 2.  The walk gives
 * (1,4,6) (2,1,3) | (1,4,6) (2,1,3) | (1,4,6): every record saturated, three full chunks.  start[1] = (2,1,3).  start[2] =
 * join((2,1,3), 2, [1,3)): q = 0 1, a = 2 < b = 3: (4,2,3), "nana".  The fix: e = 3 is join((2,1,3), 1, [4,6)): q = 0 1, a = 5 <
 * b = 6: (3,5,6); e = 4 is start[2]; e = 5 is join((4,2,3), 1, [4,6)): q = 0 1, a = b = 6; lp = min lcp[2 .. 2] = 3, ls = 0, l = 3;
 * u = 1, v = 3; the rows with q in [1, 3) are [5, 6): (4,5,6), "anan".  The records are (1,4,6) (2,1,3) (3,5,6) (4,2,3) (4,5,6).
 * Worst case: a text that occurs entire in the block (the block itself) makes every chunk full: the sweep is one chain of
 * ceil(m / C) - 2 dependent joins on one lane, and the fix joins every end after the first chunk.
 * Memory: the suffix array is one more device allocation of the handle, sa[n] and isa[n + 1]: 4 n + 4 (n + 1) bytes.  isa is preset
 * to n and scattered from sa by one kernel.  archon_hip_fm_destroy frees it; handles without it behave exactly as before.  A call
 * takes 12 m bytes of records plus the chunks' words from the calling thread's context arena, the host forms the text besides.
 * A handle serves one thread at a time (as above). */
/* sa[n] on the host: copied into the handle, isa made behind it.  Replaces an earlier attachment.  A value outside 1 .. n is
 * ARCHON_E_CORRUPT and leaves an earlier attachment in place.  A value that occurs twice returns ARCHON_OK and gives
 * unspecified records, every access inside the buffers. */
int  archon_hip_fm_attach_sa(archon_hip_fm *f, const uint32_t *sa);
/* the same from a device array; on `stream` (NULL = the context's own), complete on return */
int  archon_hip_fm_attach_sa_dev(archon_hip_fm *f, const uint32_t *d_sa, void *stream);
/* device to device from the resident block; preconditions and ARCHON_E_ARG cases are those of archon_hip_block_fm_attach_lcp.
 * The block's LCP step reads the resident suffix array and leaves it as it is: the two attachments may come in either order. */
int  archon_hip_block_fm_attach_sa(archon_hip_block *b, archon_hip_fm *f);
/* host text[m] and len[m], lo[m], hi[m]: the record of end e at index e - 1.  lo_or_null and hi_or_null are both given or both
 * NULL (lengths only); one without the other is ARCHON_E_ARG.  m = 0 writes nothing; a text longer than the block is searched
 * like any other.  A handle without an LCP array or without a suffix array is ARCHON_E_ARG.  Four launches and one host wait. */
int  archon_hip_fm_ms_text(archon_hip_fm *f, const uint8_t *text, uint32_t m, uint32_t *len, uint32_t *lo_or_null, uint32_t *hi_or_null);
/* device text and records; on `stream` (NULL = the context's own), complete on return: one host wait */
int  archon_hip_fm_ms_text_dev(archon_hip_fm *f, const uint8_t *d_text, uint32_t m, uint32_t *d_len, uint32_t *d_lo_or_null,
                               uint32_t *d_hi_or_null, void *stream);
/* The relative Lempel-Ziv parse of the text against the block.  One kernel turns the records into archon_hip_lpf_rec {len,
 * src = sa[lo], or 0 when len is 0} and the parse of archon_hip_lz_parse makes the phrases over the m items: a phrase (end, len,
 * src) says P[end-len .. end) = x[src-len .. src), len 0 is the literal P[end-1].  Output order is chain order from m; the cap
 * rule is that of archon_hip_lz_parse (*total always written; out NULL: counting only; cap < *total: ARCHON_E_ARG, out untouched).
 * The parse is greedy from the RIGHT: the longest phrase that ends at m, then the longest that ends where it starts.  Reversing
 * both texts gives the greedy parse from the left, as the LZ77 parse above does with dir 1.  m = 0 gives *total = 0. */
int  archon_hip_fm_rlz(archon_hip_fm *f, const uint8_t *text, uint32_t m, archon_hip_phrase *out_or_null, uint64_t cap, uint64_t *total);
/* device text and phrases; on `stream`, complete on return */
int  archon_hip_fm_rlz_dev(archon_hip_fm *f, const uint8_t *d_text, uint32_t m, archon_hip_phrase *d_out_or_null, uint64_t cap, uint64_t *total,
                           void *stream);
/* the CALLING THREAD's last attach_sa, ms_text or rlz call on `dev`; these calls leave every other statistics record alone
 * (archon_hip_fm_ms_stats and archon_hip_lz_stats included).  saturated, full_chunks, runs and longest_run follow from x, P and C
 * alone. */
typedef struct archon_hip_fm_text_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t m;                 /* bytes of the text (0 for an attach) */
    uint32_t chunk;             /* C */
    uint32_t chunks;            /* ceil(m / C) */
    uint32_t fan;               /* F of the hierarchy of the handle's attached LCP array (0 without one) */
    uint32_t levels;            /* its levels */
    uint64_t saturated;         /* records the fix rewrote: the saturated records of chunks 1 .. */
    uint32_t full_chunks;       /* chunks whose last record is saturated */
    uint32_t runs;              /* runs of full chunks the sweep joined along */
    uint32_t longest_run;       /* the dependent joins of the sweep's longest chain */
    uint64_t sa_probes;         /* evaluations of q */
    uint64_t lcp_probes;        /* entries of lcp and the hierarchy the joins read */
    uint64_t matched;           /* the sum of all len */
    uint32_t longest;           /* the largest len */
    uint64_t phrases;           /* rlz: *total */
    uint64_t sa_bytes;          /* device bytes of the attached sa and isa */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_walk;              /* device time of the offsets and the walk (HIP events) */
    float ms_sweep;             /* of the sweep */
    float ms_fix;               /* of the fix */
    float ms_parse;             /* rlz: of the record kernel and the parse */
} archon_hip_fm_text_stats;
int  archon_hip_get_fm_text_stats(int dev, archon_hip_fm_text_stats *out);

/* ---- document listing: which documents of a block hold each pattern, and how often ------------------------------------------------
 * A block is often a collection: the files of an archive, a read set, the versions of a record.  Every other query above answers
 * with rows or block offsets; these calls answer with documents.
 * Documents.  bounds[0 .. D] with bounds[0] = 0 < bounds[1] < ... < bounds[D] = n and 1 <= D <= n; document d is
 * x[bounds[d] .. bounds[d+1]).  Anything else is ARCHON_E_ARG: a decreasing or equal pair, bounds[0] != 0, bounds[D] != n, D = 0,
 * D > n.  A refused attach leaves an earlier attachment in place.
 * Document of an item.  Item s in 1 .. n belongs to the d with bounds[d] < s <= bounds[d+1]: the document that holds byte x[s-1].
 * Document of a row.  Row r belongs to the document of sa[r].
 * Document of an occurrence.  An occurrence of a pattern of m bytes at row r is x[sa[r]-m .. sa[r]).  It belongs to the document
 * that holds its LAST byte -- also when it starts before that document's first byte.  A caller who wants no occurrence across a
 * boundary ends every document with a byte the patterns do not hold (a newline, a 0), as collections are commonly stored; these
 * calls do not filter such occurrences out.
 * Listing of a row range [lo, hi), valid when lo <= hi <= n (else ARCHON_E_ARG): every distinct document among its rows gives one
 * record with its term frequency tf (the rows of the range in that document) and its first row (the least row of the range in that
 * document).  Records come range by range, by ascending j, and within a range by ascending row.  The tf of a range sum to
 * hi - lo.  An empty range lists nothing.  SMEMs, approximate hits and repeats are row ranges too: their lo and hi list the same way.
 * Example: "banana", sa = 2 4 6 1 3 5, bounds = 0 3 6: the documents are "ban" and "ana", the rows' documents 0 1 1 0 0 1.
 *   "an"  rows [4, 6)  records (doc, tf, row) = (0, 1, 4) (1, 1, 5)
 *   "a"   rows [0, 3)  (0, 1, 0) (1, 2, 1)
 *   "na"  rows [1, 3)  (1, 2, 1): the occurrence x[2 .. 4) starts in document 0 and ends in document 1, so it counts for 1.
 * Memory: the documents are one more device allocation of the handle, bounds (D + 1 words) | pv[n] | pos[n] | L[n]:
 * 12 n + 4 (D + 1) bytes plus padding.  L holds the rows sorted by (document, row), so document d's rows are
 * L[bounds[d] .. bounds[d+1]), ascending; pos[r] is the index of row r in L; pv[r] is 1 + the greatest row < r of the same
 * document, 0 when there is none.  One kernel makes the pairs (document of sa[r], r), a stable LSB radix sort orders them on the
 * bytes of D - 1 that can differ (none at D = 1), one kernel writes L, pos and pv.  The scratch, 24 n bytes, is the calling
 * thread's context arena.  archon_hip_fm_destroy frees the allocation; handles without documents behave exactly as before and
 * refuse these calls.
 * Method of a listing.  Row r starts a document of [lo, hi) exactly when pv[r] <= lo.  Every nonempty range is cut into tiles of T
 * rows (4096) counted from its own lo, one wave per tile; the count pass reads pv alone; a scan gives every tile its place; the emit
 * pass, run only when records are asked for and fit, walks the same tiles 64 rows at a time.  Only a first row does more: it reads
 * p = pos[r], finds d = upper_bound(bounds, p) - 1 and tf = lower_bound(L[p .. bounds[d+1]), hi) - p.  A call lists at most
 * 2^32 - 1 rows (ARCHON_E_ARG above that), and its tile words fit 256 MiB of arena (ARCHON_E_NOMEM above that).
 * A handle serves one thread at a time (as above). */
typedef struct archon_hip_fm_doc {
    uint32_t doc;      /* the document */
    uint32_t tf;       /* rows of the range in it */
    uint32_t row;      /* the first of them: sa[row] - m is one start (archon_hip_fm_locate_mems gives all) */
    uint32_t range;    /* j: the pattern or range it belongs to */
} archon_hip_fm_doc;
/* bounds[ndocs + 1] on the host: copied into the handle, L, pos and pv made behind it from the handle's attached suffix array
 * (archon_hip_fm_attach_sa; a handle without one is ARCHON_E_ARG).  Replaces an earlier attachment; the suffix array may be
 * attached again or not afterwards, the documents keep what they made. */
int  archon_hip_fm_attach_docs(archon_hip_fm *f, const uint32_t *bounds, uint32_t ndocs);
/* the same from a device array, whose entries a kernel checks; on `stream` (NULL = the context's own), complete on return */
int  archon_hip_fm_attach_docs_dev(archon_hip_fm *f, const uint32_t *d_bounds, uint32_t ndocs, void *stream);
/* f a handle from archon_hip_block_fm_index of this block's last forward, which kept its suffix array: reads the resident array
 * device to device and needs no archon_hip_fm_attach_sa; preconditions and ARCHON_E_ARG cases of archon_hip_block_fm_attach_sa */
int  archon_hip_block_fm_attach_docs(archon_hip_block *b, archon_hip_fm *f, const uint32_t *bounds, uint32_t ndocs);
/* Host patterns (offsets[k + 1] as archon_hip_fm_count): the count, then the listing of its ranges; `range` of a record is the
 * pattern.  The cap rule is that of archon_hip_fm_smems: ndocs[k] (the distinct documents of every pattern) and *total (their sum)
 * are always written; docs_or_null NULL: document frequencies only, no emit pass; cap < *total with docs_or_null given is
 * ARCHON_E_ARG with docs untouched; k = 0 writes *total = 0 and nothing else.  *total is 0 after any other refusal.  A handle
 * without documents is ARCHON_E_ARG. */
int  archon_hip_fm_docs(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *ndocs,
                        archon_hip_fm_doc *docs_or_null, uint64_t cap, uint64_t *total);
/* device patterns, offsets, counts and records, *total on the host; on `stream`, complete on return */
int  archon_hip_fm_docs_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t *d_ndocs,
                            archon_hip_fm_doc *d_docs_or_null, uint64_t cap, uint64_t *total, void *stream);
/* the listing of k row ranges [lo[j], hi[j]) on the host; a range that is not lo <= hi <= n is ARCHON_E_ARG */
int  archon_hip_fm_docs_ranges(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, uint32_t k, uint32_t *ndocs,
                               archon_hip_fm_doc *docs_or_null, uint64_t cap, uint64_t *total);
/* device ranges, counts and records; a bad range is found on the device: ARCHON_E_ARG, nothing emitted */
int  archon_hip_fm_docs_ranges_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, uint32_t k, uint32_t *d_ndocs,
                                   archon_hip_fm_doc *d_docs_or_null, uint64_t cap, uint64_t *total, void *stream);
/* The document of items.  Item s in 1 .. n -- what a locate returns plus m, or a start p passed as p + 1 -- gives doc[i] and, when
 * off_or_null is given, its offset s - 1 - bounds[doc] in it.  An item outside 1 .. n is ARCHON_E_ARG, nothing written. */
int  archon_hip_fm_doc_of(archon_hip_fm *f, const uint32_t *items, uint64_t count, uint32_t *doc, uint32_t *off_or_null);
/* device arrays; on `stream`, complete on return */
int  archon_hip_fm_doc_of_dev(archon_hip_fm *f, const uint32_t *d_items, uint64_t count, uint32_t *d_doc, uint32_t *d_off_or_null, void *stream);
/* the CALLING THREAD's last documents call (attach, listing or doc_of) on `dev`; these calls leave every other statistics record
 * alone.  rows, tiles and listed follow from x, bounds, the ranges and T alone. */
typedef struct archon_hip_fm_doc_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t docs;              /* D */
    uint32_t ranges;            /* k */
    uint32_t tile;              /* T */
    uint32_t attached;          /* 1 when the call attached documents */
    uint32_t sort_passes;       /* radix passes the attach ran: at most ceil(bits(D - 1) / 8) */
    uint32_t longest_tf;        /* the largest tf emitted */
    uint32_t reserved0;
    uint64_t pattern_bytes;     /* bytes of the patterns (0 for ranges) */
    uint64_t rows;              /* the sum of hi - lo */
    uint64_t tiles;             /* the sum of ceil((hi - lo) / T) over the nonempty ranges */
    uint64_t listed;            /* *total */
    uint64_t probes;            /* entries of bounds and L the emit pass's two searches read: at most listed (ceil(log2(D+1)) + ceil(log2(n+1))) */
    uint64_t doc_bytes;         /* device bytes of the attachment */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_attach;            /* device time of the attach (HIP events) */
    float ms_search;            /* of the count of the patterns and the tiling of the ranges */
    float ms_count;             /* of the count pass, its scan and the per-range counts */
    float ms_emit;              /* of the emit pass */
} archon_hip_fm_doc_stats;
int  archon_hip_get_fm_doc_stats(int dev, archon_hip_fm_doc_stats *out);

/* ---- windows: count, select and list a row range's occurrences in text order ----------------------------------------------------
 * Every search above ends in a row range [lo, hi) of the suffix array, and a locate lists it in row order.  These calls answer
 * in TEXT order without listing the range: how many of its occurrences end inside a window of the block, which is the first one
 * at or after a position, the next, the last, the first ten.  The cost of an answer is ceil(log2(n+1)) rank steps however many
 * rows the range has.
 * Rows and items.  Rows are 0 .. n-1.  Items sa[r] are 1 .. n.
 * Query.  A row range [lo, hi) with lo <= hi <= n and an item window [a, b) with a <= b <= n + 1.  Anything else is ARCHON_E_ARG.
 * a and b both NULL mean the whole block (a = 0, b = n + 1); one of them NULL alone is ARCHON_E_ARG.
 * Window of a query: the multiset { sa[r] : lo <= r < hi, a <= sa[r] < b }, in ascending item order.
 * Occurrences.  An occurrence of an m-byte pattern at row r is x[sa[r]-m .. sa[r]), as everywhere else: the item is its END.
 * Starts in [p, q) are items in [p + m, q + m).  Document d is items [bounds[d] + 1, bounds[d+1] + 1).
 * count:  count[j] is the size of the window.
 * select: item[j] is the idx[j]-th smallest item of the window (0-based), and 0 when the window has idx[j] items or fewer: 0 is no
 *         item, so it is the sentinel.  idx = 0 gives the first occurrence at or after a, idx = count - 1 the last one before b.
 * list:   range j emits its min(count[j], most) smallest items (most = 0: all of them) as records {item, range}, range by range
 *         and ascending within a range.  count[j] is always the full window size; *total is the number of records.
 * Examples: "banana", sa = 2 4 6 1 3 5.
 *   rows [0, 3) ("a"), no window: count 3, list 2 4 6
 *   rows [0, 3), window [3, 7): count 2, select 0 -> 4, select 1 -> 6, select 2 -> 0
 *   rows [4, 6) ("an"), window [1, 4): count 1, list 3
 *   rows [0, 6), window [2, 6), most 3: count 4, list 2 3 4
 *   rows [2, 2), window [0, 7): count 0, list nothing, select 0 -> 0
 * Structure: a wavelet matrix over the suffix array, one more device allocation of the handle.  L = ceil(log2(n+1)) levels (the
 * bit length of n, at least 1), most significant bit first: level l holds bit L-1-l of every value in the level's order, and the
 * order of level l+1 is the stable partition of level l, zeros first.  With B = ceil(n / 256) a level is 8 B words of bits and
 * B + 1 directory words -- entry i the ones before bit 256 i, the last entry all ones of the level -- padded to 256 bytes:
 *   wm_bytes = L * 256 * ceil(4 (9 B + 1) / 256)
 * about L (n/8 + n/64) bytes: 4.1 n at n = 2^28, 3.5 n at 16 MiB.  It is built on the device, level by level, from two n-word
 * buffers in the calling thread's context arena (a ballot per 64 values, a scan of the 256-bit blocks' popcounts, a stable scatter).
 * archon_hip_fm_destroy frees it; handles without one behave exactly as before and refuse these calls with ARCHON_E_ARG.
 * Method.  less(lo, hi, v), the items below v among the rows, walks the levels with two ranks each: a one bit of v adds the zeros
 * of the range and maps it to z + rank1, a zero bit maps it to rank0.  v = 0 is 0 and v >= 2^L is hi - lo, both with no walk (at
 * n = 2^k - 1 the bound n + 1 has L + 1 bits).  count = less(b) - less(a).  select walks once more with idx + less(a), taking the
 * zero side while the index is below the zeros of the range; it is refused (item 0) when idx + less(a) >= less(b).  One lane
 * answers one query; a list counts, scans min(count, most) and emits with one lane per record.
 * walks (statistics) counts root-to-leaf walks: an empty range makes none; in a nonempty range a bound of 0 or >= 2^L makes none
 * and every other bound makes one; every select and every emitted record makes one more, a refused select (item 0) none: it
 * is settled by the two bounds.  So the walks of the bounds follow from n and the queries alone, while those of the selects and
 * of the records, like in_window and listed, depend on the suffix array as the answers do.
 * A handle serves one thread at a time (as above). */
typedef struct archon_hip_fm_win {
    uint32_t item;     /* sa[r] of a row of the range inside the window: the occurrence is x[item-m .. item) */
    uint32_t range;    /* j: the range it belongs to */
} archon_hip_fm_win;
/* Builds the matrix from the handle's attached suffix array (archon_hip_fm_attach_sa; a handle without one is ARCHON_E_ARG).
 * Replaces an earlier matrix; a refused attach leaves it in place.  The suffix array may be attached again or not afterwards,
 * the matrix keeps what it made. */
int  archon_hip_fm_attach_wm(archon_hip_fm *f);
/* f a handle from archon_hip_block_fm_index of this block's last forward, which kept its suffix array: reads the resident array
 * device to device and needs no archon_hip_fm_attach_sa; preconditions and ARCHON_E_ARG cases of archon_hip_block_fm_attach_docs */
int  archon_hip_block_fm_attach_wm(archon_hip_block *b, archon_hip_fm *f);
/* k queries on the host: lo[k], hi[k], a_or_null[k], b_or_null[k] -> count[k].  k = 0 does nothing. */
int  archon_hip_fm_win_count(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, const uint32_t *a_or_null, const uint32_t *b_or_null,
                             uint32_t k, uint32_t *count);
/* device arrays; on `stream` (NULL = the context's own), complete on return.  A bad query is found on the device: ARCHON_E_ARG,
 * and what d_count holds then is unspecified */
int  archon_hip_fm_win_count_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_a_or_null,
                                 const uint32_t *d_b_or_null, uint32_t k, uint32_t *d_count, void *stream);
/* k queries and idx[k] on the host -> item[k] */
int  archon_hip_fm_win_select(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, const uint32_t *a_or_null, const uint32_t *b_or_null,
                              const uint32_t *idx, uint32_t k, uint32_t *item);
/* device arrays; on `stream`, complete on return; a bad query as in archon_hip_fm_win_count_dev */
int  archon_hip_fm_win_select_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_a_or_null,
                                  const uint32_t *d_b_or_null, const uint32_t *d_idx, uint32_t k, uint32_t *d_item, void *stream);
/* The list of k queries on the host.  The cap rule is that of archon_hip_fm_docs: count[k] and *total (the number of records) are
 * always written; out_or_null NULL: counts only, no emit pass; cap < *total with out_or_null given is ARCHON_E_ARG with out
 * untouched; k = 0 writes *total = 0 and nothing else.  *total is 0 after any other refusal.  More than 2^32 - 1 records is
 * ARCHON_E_ARG. */
int  archon_hip_fm_win_list(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, const uint32_t *a_or_null, const uint32_t *b_or_null,
                            uint32_t k, uint32_t most, uint32_t *count, archon_hip_fm_win *out_or_null, uint64_t cap, uint64_t *total);
/* device queries, counts and records, *total on the host; on `stream`, complete on return.  A bad query is found on the device:
 * ARCHON_E_ARG, nothing emitted */
int  archon_hip_fm_win_list_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_a_or_null,
                                const uint32_t *d_b_or_null, uint32_t k, uint32_t most, uint32_t *d_count, archon_hip_fm_win *d_out_or_null,
                                uint64_t cap, uint64_t *total, void *stream);
/* the CALLING THREAD's last window call (attach, count, select or list) on `dev`; these calls leave every other statistics record
 * alone.  n, levels, ranges, most, rows and wm_bytes follow from n and the queries alone; in_window, listed and walks also from the
 * suffix array (the rule above); none but the times from anything else. */
typedef struct archon_hip_fm_win_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t levels;            /* L */
    uint32_t ranges;            /* k */
    uint32_t most;              /* of a list */
    uint32_t attached;          /* 1 when the call built the matrix */
    uint32_t reserved0;
    uint64_t rows;              /* the sum of hi - lo */
    uint64_t in_window;         /* the sum of the counts */
    uint64_t listed;            /* records emitted */
    uint64_t walks;             /* root-to-leaf walks made (the rule above) */
    uint64_t wm_bytes;          /* bytes of the matrix (the formula above) */
    uint32_t kernel_launches;   /* launches issued by the call */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_attach;            /* device time of the build (HIP events) */
    float ms_count;             /* of the count or select kernel, and of a list's scan */
    float ms_emit;              /* of the emit pass */
} archon_hip_fm_win_stats;
int  archon_hip_fm_win_last_stats(int dev, archon_hip_fm_win_stats *out);

/* ---- overlaps: which documents of a block end with a beginning of a pattern, and how long the shared piece is -------------------
 * The suffix-prefix overlap, the edge of an overlap or string graph: the first step of an overlap-based assembler, of joining reads
 * to contigs, of stitching fragments of logs or records.  archon_hip_fm_count gives the rows of a whole pattern, not of each of its
 * prefixes, and the document listing names documents that hold an occurrence anywhere, not ones that END with it.
 * Keys, R, occ', rows and the primary row are those of the search rule of archon_hip_fm_count.
 * Ends.  The handle gets ends[0 .. D), items with 1 <= ends[0] < ends[1] < ... < ends[D-1] <= n; anything else is ARCHON_E_ARG.
 * Document d ENDS AT item ends[d]: its last byte is x[ends[d]-1].  ends[D-1] = n is allowed; its end row is the primary row and is
 * found like any other.  Where documents finish with a separator the caller passes the item before the separator
 * (bounds[d+1] - 1), otherwise bounds[d+1].
 * Overlap.  For a query Q of m bytes and a length l with min_len <= l <= min(m, n), document d overlaps Q by l when l <= ends[d]
 * and x[ends[d]-l .. ends[d]) = Q[0..l).  As in the document listing, the piece may begin before the document does: a document
 * shorter than l whose predecessors end the right way overlaps too.  Collections whose documents end with a byte the queries do
 * not hold (a newline, a 0) have no such pieces.  l = m means the whole query is a suffix of the document; it is reported like
 * any other overlap.
 * Walk.  Q is walked as archon_hip_fm_count walks it, P[0] first, and the walk stops when the range empties: after l bytes the
 * range [lo, hi) holds exactly the rows r with x[sa[r]-l .. sa[r]) = Q[0..l), and document d overlaps Q by l exactly when its END
 * ROW, the row r with sa[r] = ends[d], lies in that range.  A query longer than n is walked as its first n bytes (unlike the
 * count it is not refused a walk).  m = 0 gives no overlap.  min_len = 0 is ARCHON_E_ARG.
 * Records.  {query, doc, len, row}, 16 bytes; row is the end row, so sa[row] = ends[doc].  The order is query by query, within a
 * query by ascending len, within a length by ascending row.  It is the same on every run: it comes from a count pass and an emit
 * pass over the identical search, and no atomics decide a position.
 * Counts.  novl[k], the overlaps of every query, and *total, their sum, are always written.  A query whose count does not fit 32
 * bits is ARCHON_E_ARG, and so are records asked for when *total does not.
 * Example: "banana" (sa = 2 4 6 1 3 5), ends = {3, 6} ("ban", "ana"), min_len 1.
 *   Q = "ana": l = 1 rows [0, 3), end row 2 (item 6): (doc 1, len 1, row 2); l = 2 rows [4, 6), end row 4 (item 3): (doc 0, len 2,
 *              row 4); l = 3 rows [1, 3), end row 2: (doc 1, len 3, row 2).  3 overlaps, 2 rank steps, 3 lengths tested, 3 hit.
 *   Q = "nab": l = 1 rows [4, 6): (doc 0, len 1, row 4); l = 2 rows [1, 3): (doc 1, len 2, row 2); l = 3 empty.  2 overlaps.
 * Structure: the ends, one more device allocation of the handle: ends[D] | erow[D] | edoc[D] | one bit vector over the rows.  erow
 * holds the end rows ascending, edoc[j] the document of erow[j]; the bit vector marks the end rows in the layout of a level of the
 * wavelet matrix above (8 B words of bits, B + 1 directory words, B = ceil(n / 256), padded to 256 bytes):
 *   end_bytes = 256 ceil(12 D / 256) + 256 ceil(4 (9 B + 1) / 256)
 * about 0.14 n + 12 D bytes.  It is built on the device from the suffix array: a bitmap over the items from ends, one pass over sa
 * that ballots isend[sa[r]] into the row words, a scan of the blocks' popcounts, a compaction.  An sa value outside 1 .. n is never
 * used as an index; a suffix array whose end rows do not number D is ARCHON_E_CORRUPT.  archon_hip_fm_destroy frees
 * it; handles without ends behave exactly as before and refuse archon_hip_fm_overlaps with ARCHON_E_ARG.
 * Method.  One wave per query.  Every step is the rank step of archon_hip_fm_count; after the step that completes a length
 * l >= min_len with rows in the range, c = rank1(hi) - rank1(lo) on the bit vector: one directory word and one 32-byte block each.
 * The count pass sums c; the emit pass writes the c records of that length, 64 at a time, lane i from erow and edoc at
 * rank1(lo) + i, at the exclusive sum of novl before the query plus the records of its shorter lengths.
 * Launches and waits (kernel_launches, host_syncs of the statistics): an attach is 6 launches and 1 wait.  A search with
 * ovl_or_null NULL is 1 launch and 1 wait.  With records asked for it is 4 launches (the count pass and the 3 of the scan) and 1
 * wait when *total is 0 or the call is refused, and one launch and one wait more otherwise; a host form whose context arena has to
 * grow for the records runs the count pass and the scan once more (4 launches more), which a repeated call does not.
 * A handle serves one thread at a time (as above). */
typedef struct archon_hip_fm_ovl {
    uint32_t query;    /* j: the query it belongs to */
    uint32_t doc;      /* d: the document that ends with Q[0..len) */
    uint32_t len;      /* l */
    uint32_t row;      /* the end row of the document: sa[row] = ends[doc] */
} archon_hip_fm_ovl;
/* ends[ndocs] on the host, checked on the host.  Needs the handle's attached suffix array (archon_hip_fm_attach_sa; else
 * ARCHON_E_ARG), as archon_hip_fm_attach_docs does.  Replaces earlier ends; a refused attach leaves the handle exactly as it was,
 * and the earlier ends still answer. */
int  archon_hip_fm_attach_ends(archon_hip_fm *f, const uint32_t *ends, uint32_t ndocs);
/* ends on the device; on `stream` (NULL = the context's own), complete on return.  A kernel checks the entries: ARCHON_E_ARG */
int  archon_hip_fm_attach_ends_dev(archon_hip_fm *f, const uint32_t *d_ends, uint32_t ndocs, void *stream);
/* f a handle from archon_hip_block_fm_index of this block's last forward, which kept its suffix array: reads the resident array
 * device to device and needs no archon_hip_fm_attach_sa; preconditions and ARCHON_E_ARG cases of archon_hip_block_fm_attach_docs */
int  archon_hip_block_fm_attach_ends(archon_hip_block *b, archon_hip_fm *f, const uint32_t *ends, uint32_t ndocs);
/* novl[k] and *total (the sum of novl) always written.  ovl_or_null NULL: counting only (no emit pass).  cap < *total with ovl
 * given: ARCHON_E_ARG, counts and *total written, ovl untouched.  Patterns and offsets as for archon_hip_fm_count; k = 0 writes
 * *total = 0 and nothing else.  *total is 0 after any other refusal. */
int  archon_hip_fm_overlaps(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t min_len, uint32_t *novl,
                            archon_hip_fm_ovl *ovl_or_null, uint64_t cap, uint64_t *total);
/* device patterns, offsets, novl and ovl, *total a host pointer; on `stream` (NULL = the context's own), complete on return;
 * decreasing offsets are found on the device (ARCHON_E_ARG, nothing emitted) */
int  archon_hip_fm_overlaps_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t min_len,
                                uint32_t *d_novl, archon_hip_fm_ovl *d_ovl_or_null, uint64_t cap, uint64_t *total, void *stream);
/* the CALLING THREAD's last overlap call (attach or search) on `dev`; these calls leave every other statistics record alone.
 * All but the times follow from the block, the ends and the queries alone. */
typedef struct archon_hip_fm_ovl_stats {
    uint32_t n;                 /* block size of the index */
    uint32_t docs;              /* D */
    uint32_t queries;           /* k */
    uint32_t min_len;           /* of the call (0 for an attach) */
    uint32_t attached;          /* 1 when the call attached ends */
    uint32_t longest;           /* the longest overlap */
    uint64_t pattern_bytes;     /* bytes of the patterns */
    uint64_t steps;             /* rank steps (count pass) */
    uint64_t tested;            /* lengths l >= min_len reached with rows in the range: two rank1 each */
    uint64_t hit;               /* of them, lengths with at least one overlap */
    uint64_t overlaps;          /* the sum of novl */
    uint64_t emitted;           /* records written */
    uint64_t end_bytes;         /* bytes of the ends (the formula above) */
    uint32_t kernel_launches;   /* launches issued by the call (the statement above) */
    uint32_t host_syncs;        /* times the host waited for the stream inside the call */
    float ms_attach;            /* device time of the build (HIP events) */
    float ms_count;             /* of the count pass, and of the scan when records are asked for */
    float ms_emit;              /* of the emit pass */
    uint32_t reserved0;
} archon_hip_fm_ovl_stats;
int  archon_hip_fm_ovl_last_stats(int dev, archon_hip_fm_ovl_stats *out);

/* ---- measurement ------------------------------------------------------------- */

/* Per-stage device times (HIP events on the stream the kernels ran on) and
 * work counters of the CALLING THREAD's most recent forward/inverse call on `dev`. */
typedef struct archon_hip_stats {
    uint32_t n;                  /* block size of the call */
    uint32_t radix_passes;       /* LSB radix passes executed by the first-stage sort */
    uint32_t doubling_rounds;    /* prefix-doubling rounds executed */
    uint64_t unresolved_initial; /* items left tied by the first stage */
    uint64_t unresolved_total;   /* sum over rounds of items entering a round */
    float ms_total;              /* whole device pipeline */
    float ms_hist;               /* hist256 / bucket setup */
    float ms_sort;               /* first-stage radix bucketing */
    float ms_doubling;           /* prefix-doubling refinement */
    float ms_bwt;                /* sa_to_bwt */
    float ms_lf_build;           /* inverse: LF table */
    float ms_lf_walk;            /* inverse: chain walk */
    uint64_t walk_chains;        /* inverse: number of sub-chains walked in parallel */
    uint32_t kernel_launches;    /* launches issued by the call */
    uint32_t radix_pass_timed;   /* first-stage radix passes bracketed by their own HIP events */
    float ms_radix_pass_sum;     /* device time inside those passes (pass kernels only) */
    float ms_local_sort;         /* streaming path: in-LDS bucket sorts (k_local_sort) */
    float ms_resolve;            /* streaming path: k_resolve_ties */
    uint32_t path;               /* 1 = streaming first stage (2 passes + local sort), 0 = 7-pass LSB */
    uint32_t tie_groups;         /* groups still tied after 5 key bytes */
    uint32_t tie_items;          /* rows flagged as tied by k_local_sort */
    float ms_pass_text;          /* streaming path: LSB pass A (k_pass_text), its own HIP events */
    float ms_pass_rec;           /* streaming path: LSB pass B (k_pass_rec), its own HIP events */
    uint32_t alphabet_bits;      /* 7-pass path: bits per symbol when the alphabet was compacted (0 = bytes) */
    uint32_t period;             /* long-repeat defence: the neighbour gap p it ran with (0 = not run) */
    uint32_t chain_items;        /* rows it settled without doubling */
    uint32_t text_rounds;        /* refinement rounds keyed on the next 4 text bytes (before any doubling round) */
    uint64_t seg_big_items;      /* sum over rounds of entries in groups too long for the in-workgroup sort (sent through the global sort) */
    uint64_t chain_pairs;        /* pairs of rows settled passage by passage (long duplicates) instead of by further doubling rounds */
    uint32_t break_rounds;       /* rounds keyed on the distance to the last defect of the period (groups that straddle defects) */
    uint32_t break_settled;      /* rows such a round settled */
    uint64_t mid_items;          /* sum over rounds of entries in groups of 1025 .. 16384 rows, each sorted by one workgroup in LDS */
    uint64_t arena_bytes;        /* device workspace the call used (bump-allocated from the context's arenas; forward calls) */
    uint32_t host_syncs;         /* times the host waited for the stream inside the call (forward calls: one for a block the streaming stage settles) */
    uint32_t reserved0;
} archon_hip_stats;

int archon_hip_get_stats(int dev, archon_hip_stats *out);

#ifdef __cplusplus
}
#endif
#endif
