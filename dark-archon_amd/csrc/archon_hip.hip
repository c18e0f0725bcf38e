// archon_hip.hip -- the translation unit of libarchon_hip.so and its C ABI (include/archon_hip.h, include/archon_hip_test.h).
// The rule of this file: an entry point checks its arguments, takes a context (with_ctx, context.hiph), stages host buffers
// and keeps the call's record; everything that launches a kernel lives in a .hiph file, beside the kernels it launches.
// gfx950 only.
#include "common.hiph"
#include "util.hiph"
#include "context.hiph"
#include "radix_sort.hiph"
#include "bucket_sort.hiph"
#include "forward.hiph"
#include "periodic.hiph"
#include "rounds.hiph"
#include "rank_writer.hiph"
#include "mid_rounds.hiph"
#include "forward_driver.hiph"
#include "inverse.hiph"
#include "post.hiph"
#include "lcp.hiph"
#include "fm.hiph"
#include "fm_walk.hiph"
#include "fm_approx.hiph"
#include "fm_class.hiph"
#include "fm_mem.hiph"
#include "fm_ms.hiph"
#include "fm_text.hiph"
#include "fm_doc.hiph"
#include "fm_win.hiph"
#include "fm_ovl.hiph"
#include "fm_host.hiph"
#include "analysis.hiph"
#include "repeats.hiph"
#include "lz.hiph"
#include "kmers.hiph"
#include "maw.hiph"
#include "entropy.hiph"
#include "runs.hiph"

#include <limits.h>
#include <stdlib.h>
#include <thread>
#include <vector>

using namespace archon;

// =====================================================================
// What the entry points share: argument checks, staging, the resident block, the batch workers (file-local, C++ linkage)
// =====================================================================
static int check_n(uint32_t n)
{
    if (n < 1 || n > ARCHON_HIP_MAX_N) {
        set_error("block size %u out of range [1, %u]", n, ARCHON_HIP_MAX_N);
        return ARCHON_E_ARG;
    }
    return ARCHON_OK;
}

// ---- repeats, LZ, k-mers
static int rep_check(const void *lcp, const void *bwt, const void *total, uint32_t n, uint32_t base_id, uint32_t kind)
{
    if (!lcp || !bwt || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("primary row %u out of range [0, %u)", base_id, n); return ARCHON_E_ARG; }
    return rep_check_kind(kind);
}

static int lpf_check(const void *sa, const void *lcp, const void *lpf, uint32_t n, uint32_t dir)
{
    if (!sa || !lcp || !lpf) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return lz_check_dir(dir);
}

// *total is written whenever it is given: 0 before any refusal (the cap rule's "always written")
static int parse_check(const void *lpf, uint64_t *total, uint32_t n)
{
    if (total) *total = 0;
    if (!lpf || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    return check_n(n);
}

static int kmers_check(const void *sa, const void *lcp, uint64_t *total, uint32_t n, uint32_t k, const void *hist, uint32_t bins)
{
    if (total) *total = 0;
    if (!sa || !lcp || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return kmer_check_args(k, hist, bins);
}

// sa and lcp of host buffers through staging buffers 0 and 1 (k-mers, minimal absent words, entropy, runs, LCE)
static int stage_sa_lcp(Ctx *c, hipStream_t s, const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t **d_sa, uint32_t **d_lcp)
{
    ARCHON_TRY(ctx_io(c, 0, (size_t)n * 4 + 64, (void **)d_sa));
    ARCHON_TRY(ctx_io(c, 1, (size_t)n * 4 + 64, (void **)d_lcp));
    ARCHON_HIP_TRY(hipMemcpyAsync(*d_sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, s));
    ARCHON_HIP_TRY(hipMemcpyAsync(*d_lcp, lcp, (size_t)n * 4, hipMemcpyHostToDevice, s));
    return ARCHON_OK;
}

static int kmer_occ_check(const void *sa, const void *lcp, const void *occ, uint32_t n, uint32_t k)
{
    if (!sa || !lcp || !occ) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return kmer_check_args(k, nullptr, 0);
}

static int sus_check(const void *sa, const void *lcp, const void *sus, uint32_t n)
{
    if (!sa || !lcp || !sus) { set_error("null pointer"); return ARCHON_E_ARG; }
    return check_n(n);
}

// *total is written whenever it is given: 0 before any refusal
static int maws_check(const void *sa, const void *lcp, const void *bwt, uint64_t *total, uint32_t n, uint32_t base_id, uint32_t min_len, uint32_t max_len)
{
    if (total) *total = 0;
    if (!sa || !lcp || !bwt || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("primary row %u out of range [0, %u)", base_id, n); return ARCHON_E_ARG; }
    return maw_check_filters(min_len, max_len);
}

// the records are zeroed by any refusal of the arguments
static int entropy_args(const void *sa, const void *lcp, const void *bwt, uint32_t n, uint32_t base_id, const uint32_t *ks, uint32_t nk, const void *out)
{
    ARCHON_TRY(ent_check_orders(ks, nk, out));
    if (!sa || !lcp || !bwt) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("primary row %u out of range [0, %u)", base_id, n); return ARCHON_E_ARG; }
    return ARCHON_OK;
}
static int entropy_check(const void *sa, const void *lcp, const void *bwt, uint32_t n, uint32_t base_id, const uint32_t *ks, uint32_t nk, struct archon_hip_entropy *out)
{
    return ent_refused(entropy_args(sa, lcp, bwt, n, base_id, ks, nk, out), out, nk);
}

static int complexity_args(const void *lcp, uint32_t n, const void *rec)
{
    if (!lcp || !rec) { set_error("null pointer"); return ARCHON_E_ARG; }
    return check_n(n);
}
static int complexity_check(const void *lcp, uint32_t n, struct archon_hip_complexity *rec)
{
    const int rc = complexity_args(lcp, n, rec);
    if (rc != ARCHON_OK && rec) memset(rec, 0, sizeof *rec);
    return rc;
}

// *total is written whenever it is given: 0 before any refusal
static int runs_check(const void *sa, const void *lcp, const void *sa_c, uint64_t *total, uint32_t n, uint32_t min_period, uint32_t max_period,
                      uint32_t min_copies)
{
    if (total) *total = 0;
    if (!sa || !lcp || !sa_c || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return run_check_filters(min_period, max_period, min_copies);
}

static int lce_check(const void *sa, const void *lcp, uint32_t n, const void *s, const void *t, uint32_t k, const void *out)
{
    if (!sa || !lcp || (k && (!s || !t || !out))) { set_error("null pointer"); return ARCHON_E_ARG; }
    return check_n(n);
}

// host items: one above n refuses the call before anything runs
static int lce_check_items(const uint32_t *s, const uint32_t *t, uint32_t k, uint32_t n)
{
    for (uint32_t i = 0; i < k; ++i)
        if (s[i] > n || t[i] > n) { set_error("lce: pair %u is (%u, %u), an item above %u", i, s[i], t[i], n); return ARCHON_E_ARG; }
    return ARCHON_OK;
}

// host queries through staging buffer 2: s, t and the answers, k words each
static int lce_stage(Ctx *c, hipStream_t st, const uint32_t *s, const uint32_t *t, uint32_t k, uint32_t **d_q)
{
    ARCHON_TRY(ctx_io(c, 2, (size_t)k * 12 + 64, (void **)d_q));
    ARCHON_HIP_TRY(hipMemcpyAsync(*d_q, s, (size_t)k * 4, hipMemcpyHostToDevice, st));
    ARCHON_HIP_TRY(hipMemcpyAsync(*d_q + k, t, (size_t)k * 4, hipMemcpyHostToDevice, st));
    return ARCHON_OK;
}

// ---- the FM index: text calls, documents
static int fmt_check(const archon_hip_fm *f, const void *text, const void *len, const void *lo, const void *hi)
{
    if (!f || !text || !len) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!lo != !hi) { set_error("FM ms text: lo and hi are both given or both null"); return ARCHON_E_ARG; }
    return fmt_check_attached(f);
}

// *total is written whenever it is given: 0 before any refusal
static int rlz_check(const archon_hip_fm *f, const void *text, uint64_t *total)
{
    if (total) *total = 0;
    if (!f || !text || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    return fmt_check_attached(f);
}

// what an attach asks of host bounds before the handle is read, then with it
static int fmd_attach_check(const archon_hip_fm *f, const uint32_t *bounds, uint32_t ndocs)
{
    ARCHON_TRY(fmd_check_bounds(bounds, ndocs));
    if (!f->sa.mem) { set_error("FM attach docs: the handle has no suffix array (archon_hip_fm_attach_sa)"); return ARCHON_E_ARG; }
    return fmd_check_fit(f->n, bounds, ndocs);
}

// *total is written whenever it is given: 0 before any refusal
static int fmd_check(const archon_hip_fm *f, const void *a, const void *b, const void *ndocs, uint64_t *total)
{
    if (total) *total = 0;
    if (!f || !a || !b || !ndocs || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    return ARCHON_OK;
}

static int fmd_doc_of_check(const archon_hip_fm *f, const void *items, uint64_t count, const void *doc)
{
    if (!f || (!items && count) || (!doc && count)) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (count >> 32) { set_error("FM doc of: %llu items in one call", (unsigned long long)count); return ARCHON_E_ARG; }
    return fmd_check_attached(f);
}

// a window call's pointers: lo, hi and the answer whenever there are queries, a and b both given or both null
static int fmwin_check(const archon_hip_fm *f, const void *lo, const void *hi, const void *a, const void *b, const void *answer, uint32_t k)
{
    if (!f || (k && (!lo || !hi || !answer))) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!a != !b) { set_error("FM window: a and b are both given or both null"); return ARCHON_E_ARG; }
    return ARCHON_OK;
}

// ---- resident blocks
// What a block-coder object keeps on the device between enCompute, validate and enWrite (bwt/a7/src/main.cpp:39-46): the
// block, its suffix array and its BWT, in buffers of its own.  The state belongs to the HANDLE -- any number of objects on
// any number of threads; the compute arena is the calling thread's context, held only for the duration of a call.
struct FmRelease {
    void operator()(archon_hip_fm *f) const { fm_release(f); }
};
struct ARCHON_LOCAL archon_hip_block {
    int dev = 0;
    std::mutex mu;
    DevBuf x, bwt, sa;                  // n + 64 bytes each (x and bwt: both or neither), 4 n + 64; freed by archon_hip_block_destroy
    uint8_t *d_x() const { return reinterpret_cast<uint8_t *>(x.p); }
    uint8_t *d_bwt() const { return reinterpret_cast<uint8_t *>(bwt.p); }
    uint32_t *d_sa() const { return reinterpret_cast<uint32_t *>(sa.p); }
    uint32_t n = 0, base = 0;
    bool valid = false, has_sa = false;
    archon_hip_stats stats;
    std::unique_ptr<archon_hip_fm, FmRelease> fm;   // the FM index over d_bwt, built by the first FM call after a forward
};

// what a call that reads the resident block (with_sa: and its suffix array) asks first, under the block's lock
static int block_check(const archon_hip_block *b, bool with_sa)
{
    if (with_sa && !(b->valid && b->has_sa)) { set_error("no resident block with its suffix array"); return ARCHON_E_ARG; }
    if (!b->valid) { set_error("no resident block"); return ARCHON_E_ARG; }
    return ARCHON_OK;
}

static int block_reserve(archon_hip_block *b, uint32_t n, bool want_sa)
{
    // the old ones go before the new ones are made: at 1 GiB blocks the peak matters
    const size_t need = (size_t)n + 64, need_sa = (size_t)n * 4 + 64;
    if (need > b->x.bytes) {
        (void)b->x.release();
        (void)b->bwt.release();
        if (b->x.alloc(need, "resident block") != ARCHON_OK || b->bwt.alloc(need, "resident block") != ARCHON_OK) {
            (void)b->x.release();       // both or neither
            return ARCHON_E_NOMEM;
        }
    }
    if (want_sa && need_sa > b->sa.bytes) {
        (void)b->sa.release();
        ARCHON_TRY(b->sa.alloc(need_sa, "resident block"));
    }
    return ARCHON_OK;
}

// The resident LCP array into staging buffer 1, its record kept for the thread whether or not the run succeeded, its time
// into *ms_lcp_or_null when it did
static int block_lcp_step(Ctx *c, hipStream_t s, const archon_hip_block *b, uint32_t **d_lcp, float *ms_lcp_or_null)
{
    ARCHON_TRY(ctx_io(c, 1, (size_t)b->n * 4 + 64, (void **)d_lcp));
    archon_hip_lcp_stats st = {};
    const uint32_t launches0 = t_launch_count;
    const int rc = lcp_run(c, s, b->d_x(), b->n, b->d_sa(), b->d_bwt(), *d_lcp, &st);
    t_launch_count = launches0;         // the step's launches are in its own record, not in the calling form's: that one goes on from here
    t_lcp_stats.keep(b->dev, st);
    if (rc == ARCHON_OK && ms_lcp_or_null) *ms_lcp_or_null = st.ms_total;
    return rc;
}

// The block's FM handle over its own BWT, built by the first FM call after a forward: its build into *st, which then says built
static int block_fm_table(Ctx *c, hipStream_t s, archon_hip_block *b, archon_hip_fm_stats *st)
{
    if (b->fm) return ARCHON_OK;
    archon_hip_fm *f = nullptr;
    ARCHON_TRY(fm_build(c, s, nullptr, b->d_bwt(), false, b->n, b->base, &f, st));
    b->fm.reset(f);
    return ARCHON_OK;
}

// the same for a call that keeps another record: a table built here is this call's work, into its own record, while fm_stats
// stays as it was
template <class Stats>
static int block_fm_table_own(Ctx *c, hipStream_t s, archon_hip_block *b, Stats *st)
{
    archon_hip_fm_stats fst = {};
    ARCHON_TRY(block_fm_table(c, s, b, &fst));
    st->built = fst.built;
    st->ms_build = fst.ms_build;
    return ARCHON_OK;
}

// a handle given beside a block is one of that block's BWT, on its device
static int block_check_handle(const archon_hip_block *b, const archon_hip_fm *f, const char *what)
{
    if (f->dev != b->dev || f->n != b->n || f->base != b->base) {
        set_error("%s: the handle (%u bytes, primary row %u) is not of this block (%u bytes, primary row %u)", what, f->n, f->base, b->n, b->base);
        return ARCHON_E_ARG;
    }
    return ARCHON_OK;
}

// The (dev)-keyed form of the same: the calling thread's own default block on that device (so two threads never see each
// other's BWT, whatever context they compute on).
struct DefaultBlocks {
    archon_hip_block *blk[kMaxDev] = {};
    ~DefaultBlocks() { for (auto *b : blk) archon_hip_block_destroy(b); }
};
static thread_local DefaultBlocks t_blocks;

static int default_block(int dev, archon_hip_block **out)
{
    if (dev < 0 || dev >= kMaxDev) { set_error("device %d out of range", dev); return ARCHON_E_NODEVICE; }
    if (!t_blocks.blk[dev]) ARCHON_TRY(archon_hip_block_create(dev, &t_blocks.blk[dev]));
    *out = t_blocks.blk[dev];
    return ARCHON_OK;
}

// ---- several small blocks per call: the workers of a batch
static int batch_workers(const uint32_t *n, uint32_t count, int workers)
{
    uint32_t mx = 0;
    for (uint32_t i = 0; i < count; ++i) mx = n[i] > mx ? n[i] : mx;
    int w = workers > 0 ? workers : (mx <= (4u << 20) ? 8 : mx <= (16u << 20) ? 4 : 2);
    if (w > kCtxPerDev) w = kCtxPerDev;
    if ((uint32_t)w > count) w = (int)count;
    return w < 1 ? 1 : w;
}

template <class Fn>
static int run_batch(uint32_t count, int w, int dev, Fn fn)
{
    std::atomic<int> rc{ARCHON_OK};
    std::atomic<uint32_t> next{0};
    std::mutex emu;
    char emsg[sizeof t_err] = "";
    std::vector<std::thread> th;
    for (int t = 0; t < w; ++t)
        th.emplace_back([&, t] {
            (void)archon_hip_bind_context(dev, t);
            for (;;) {
                const uint32_t i = next.fetch_add(1u);
                if (i >= count || rc.load() != ARCHON_OK) return;
                const int r = fn(i);
                if (r != ARCHON_OK) {
                    std::lock_guard<std::mutex> lk(emu);
                    if (rc.load() == ARCHON_OK) { rc.store(r); snprintf(emsg, sizeof emsg, "block %u: %s", i, t_err); }
                    return;
                }
            }
        });
    for (auto &t : th) t.join();
    if (rc.load() != ARCHON_OK) set_error("%s", emsg);
    return rc.load();
}

// ---- the test routes (archon_hip_test_route): one row per route -- its name, how its value is checked, where it is stored,
// the bounds.  Every kind has one check and one message
enum class RouteKind {
    kFlag,      // nonzero switches it on: stored as 1 / 0
    kValue,     // stored as given
    kClamp,     // below lo: lo, above hi: `over`
    kPow2,      // a power of two in [lo, hi], or 0
    kRange,     // a value in [lo, hi]; one that is not positive is stored as 0
    kMul64,     // a multiple of 64 in [lo, hi], or 0
};
struct RouteRow {
    const char *name;
    RouteKind kind;
    void (*store)(long);
    long lo, hi, over;
    const char *refusal;        // kRange, kMul64: what the message says behind "NAME=value"
};
#define ROUTE_FLAG(bit) [](long v) { if (v) g_route.flags |= (bit); else g_route.flags &= ~(uint32_t)(bit); }
#define ROUTE_FIELD(f) [](long v) { g_route.f = (decltype(g_route.f))v; }
static_assert(bs::kMaxRanges == 1024 && fmd::kMinTile == 64 && fmd::kMaxTile == 1u << 20, "the bounds the messages of PASS_RANGES and DOC_TILE name");
static const RouteRow kRoutes[] = {
    {"NO_ALIGNED", RouteKind::kFlag, ROUTE_FLAG(kRtNoAligned)},
    {"NO_CHAINS", RouteKind::kFlag, ROUTE_FLAG(kRtNoChains)},
    {"NO_PACK", RouteKind::kFlag, ROUTE_FLAG(kRtNoPack)},
    {"NO_PAIR_CHAINS", RouteKind::kFlag, ROUTE_FLAG(kRtNoPairChains)},
    {"NO_PERIOD_HINT", RouteKind::kFlag, ROUTE_FLAG(kRtNoPeriodHint)},
    {"NO_BREAK_ROUND", RouteKind::kFlag, ROUTE_FLAG(kRtNoBreakRound)},
    {"NO_PERIOD_STREAM", RouteKind::kFlag, ROUTE_FLAG(kRtNoPeriodStream)},
    {"NO_RANK_WRITER", RouteKind::kFlag, ROUTE_FLAG(kRtNoRankWriter)},
    {"NO_TEXT_ROUNDS", RouteKind::kFlag, ROUTE_FLAG(kRtNoTextRounds)},
    {"NO_MID", RouteKind::kFlag, ROUTE_FLAG(kRtNoMid)},
    {"NO_SHALLOW", RouteKind::kFlag, ROUTE_FLAG(kRtNoShallow)},
    {"NO_CLOSED_FORM", RouteKind::kFlag, ROUTE_FLAG(kRtNoClosedForm)},
    {"NO_REL_RECORDS", RouteKind::kFlag, ROUTE_FLAG(kRtNoRelRecords)},
    {"FM_SAMPLE_WALK", RouteKind::kFlag, ROUTE_FIELD(fm_sample_walk)},
    {"SMALL_BLOCK", RouteKind::kValue, ROUTE_FIELD(small_block)},
    {"ALIGNED_MIN", RouteKind::kValue, ROUTE_FIELD(aligned_min)},
    {"REL_MIN_SEG", RouteKind::kValue, ROUTE_FIELD(rel_min_seg)},
    {"KEY_BYTES", RouteKind::kValue, ROUTE_FIELD(key_bytes)},
    {"INV_SBITS", RouteKind::kValue, ROUTE_FIELD(inv_sbits)},
    {"INV_WALK_WGS", RouteKind::kValue, ROUTE_FIELD(inv_walk_wgs)},
    {"FORCE_PATH", RouteKind::kClamp, ROUTE_FIELD(force_path), -1, 1, 1},
    {"INV_ROWS", RouteKind::kClamp, ROUTE_FIELD(inv_rows), -1, 2, 1},                   // (anything above 2 asks for rows: 1)
    {"INV_SLAB", RouteKind::kClamp, ROUTE_FIELD(inv_slab), 0, LONG_MAX, 0},
    {"FM_SUB_ROWS", RouteKind::kPow2, ROUTE_FIELD(fm_sub_rows), 16, 1024},
    {"FM_SUPER_ROWS", RouteKind::kPow2, ROUTE_FIELD(fm_super_rows), 16, 65536},
    {"REP_FAN", RouteKind::kPow2, ROUTE_FIELD(rep_fan), 2, 64},
    {"LZ_FAN", RouteKind::kPow2, ROUTE_FIELD(lz_fan), 2, 64},
    {"LZ_TILE", RouteKind::kPow2, ROUTE_FIELD(lz_tile), 2, (long)lz::kMaxTile},
    {"KMER_TILE", RouteKind::kPow2, ROUTE_FIELD(kmer_tile), (long)kmer::kMinTile, (long)kmer::kDefaultTile},
    {"PASS_RANGES", RouteKind::kRange, ROUTE_FIELD(pass_ranges), 0, bs::kMaxRanges, 0, " out of range [1, 1024]"},
    {"LCP_CAP", RouteKind::kRange, ROUTE_FIELD(lcp_cap), LONG_MIN, 4096, 0, " out of range [1, 4096]"},           // (no lower bound: below 1 is the default)
    {"LCP_WINDOW", RouteKind::kRange, ROUTE_FIELD(lcp_window), LONG_MIN, 1l << 30, 0, " out of range [1, 2^30]"},
    {"MS_CHUNK", RouteKind::kRange, ROUTE_FIELD(ms_chunk), 0, 0xFFFFFFFFl, 0, ": not a chunk of 1 .. 2^32 - 1 bytes (0: the default)"},
    {"EDIT_TILE", RouteKind::kRange, ROUTE_FIELD(edit_tile), 0, 64, 0, ": not a tile of 1 .. 64 ends (0: the default)"},
    {"EDIT_BATCH", RouteKind::kRange, ROUTE_FIELD(edit_batch), 0, 0x7FFFFFFFl, 0, ": not a batch of 1 .. 2^31 - 1 patterns (0: the budget's own)"},
    {"STRIDE_GRID", RouteKind::kRange, ROUTE_FIELD(stride_grid), 0, 2048, 0, ": not a grid of 1 .. 2048 workgroups (0: the default)"},
    {"DOC_TILE", RouteKind::kMul64, ROUTE_FIELD(doc_tile), (long)fmd::kMinTile, (long)fmd::kMaxTile, 0, ": not a tile of 64 .. 2^20 rows, a multiple of 64 (0: the default)"},
};
#undef ROUTE_FLAG
#undef ROUTE_FIELD

// =====================================================================
// C ABI
// =====================================================================
extern "C" {

int archon_hip_device_count(void) { return device_count(); }

const char *archon_hip_last_error(void) { return t_err; }

int archon_hip_forward_dev(const uint8_t *d_x, uint32_t n, uint32_t *d_sa_or_null, uint8_t *d_bwt,
                           uint32_t *d_base_id, int dev, void *stream)
{
    if (!d_x || !d_bwt || !d_base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return keep_stats(c, forward_run(c, s, d_x, n, d_sa_or_null, d_bwt, d_base_id)); });
}

int archon_hip_forward(const uint8_t *x, uint32_t n, uint32_t *sa_or_null, uint8_t *bwt, uint32_t *base_id, int dev)
{
    if (!x || !bwt || !base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_x = nullptr, *d_bwt = nullptr;
        uint32_t *d_sa = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_x));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n + 64, (void **)&d_bwt));
        if (sa_or_null) ARCHON_TRY(ctx_io(c, 2, (size_t)n * 4, (void **)&d_sa));
        uint32_t *d_base = c->d_mail() + mail::kDevBase.at;
        ARCHON_HIP_TRY(hipMemcpyAsync(d_x, x, n, hipMemcpyHostToDevice, s));
        ARCHON_TRY(keep_stats(c, forward_run(c, s, d_x, n, d_sa, d_bwt, d_base)));
        // BWT first (the block coder's enWrite can start on it), then the 4N bytes of the suffix array
        ARCHON_HIP_TRY(hipMemcpyAsync(bwt, d_bwt, n, hipMemcpyDeviceToHost, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(base_id, d_base, 4, hipMemcpyDeviceToHost, s));
        if (sa_or_null) ARCHON_HIP_TRY(hipMemcpyAsync(sa_or_null, d_sa, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_get_stats(int dev, archon_hip_stats *out) { return t_stats.get(dev, out, "transform"); }

// ---- the LCP array (lcp.hiph)
int archon_hip_lcp_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, uint32_t *d_lcp, int dev, void *stream)
{
    if (!d_x || !d_sa || !d_lcp) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        archon_hip_lcp_stats st = {};
        const int rc = lcp_run(c, s, d_x, n, d_sa, nullptr, d_lcp, &st);
        t_lcp_stats.keep(dev, st);
        return rc;
    });
}

// host buffers: block, suffix array and result through the context's staging buffers
int archon_hip_lcp(const uint8_t *x, uint32_t n, const uint32_t *sa, uint32_t *lcp, int dev)
{
    if (!x || !sa || !lcp) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_x = nullptr;
        uint32_t *d_lcp = nullptr, *d_sa = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_x));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n * 4 + 64, (void **)&d_lcp));
        ARCHON_TRY(ctx_io(c, 2, (size_t)n * 4 + 64, (void **)&d_sa));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_x, x, n, hipMemcpyHostToDevice, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, s));
        archon_hip_lcp_stats st = {};
        const int rc = lcp_run(c, s, d_x, n, d_sa, nullptr, d_lcp, &st);
        t_lcp_stats.keep(dev, st);
        ARCHON_TRY(rc);
        ARCHON_HIP_TRY(hipMemcpyAsync(lcp, d_lcp, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_get_lcp_stats(int dev, archon_hip_lcp_stats *out) { return t_lcp_stats.get(dev, out, "LCP call"); }

// ---- the repeats of a block (repeats.hiph: the kernels and their drivers; here the argument checks and the statistics)
int archon_hip_repeats_dev(const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, uint32_t kind, uint32_t min_len, uint32_t min_occ,
                           archon_hip_repeat *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream)
{
    ARCHON_TRY(rep_check(d_lcp, d_bwt, total, n, base_id, kind));
    *total = 0;
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_repeat_stats> keep(t_rep_stats, dev);
        rep_call_stats(&keep.st, n, kind, min_len, min_occ);
        RepCall q = {d_lcp, d_bwt, n, base_id, kind, min_len, min_occ};
        return rep_list(c, s, q, d_out_or_null, cap, total, false, &keep.st);
    });
}

// host buffers: the BWT and the LCP array through the context's staging buffers
int archon_hip_repeats(const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base_id, uint32_t kind, uint32_t min_len, uint32_t min_occ,
                       archon_hip_repeat *out_or_null, uint64_t cap, uint64_t *total, int dev)
{
    ARCHON_TRY(rep_check(lcp, bwt, total, n, base_id, kind));
    *total = 0;
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_repeat_stats> keep(t_rep_stats, dev);
        rep_call_stats(&keep.st, n, kind, min_len, min_occ);
        uint8_t *d_bwt = nullptr;
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_bwt));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n * 4 + 64, (void **)&d_lcp));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_bwt, bwt, n, hipMemcpyHostToDevice, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)n * 4, hipMemcpyHostToDevice, s));
        RepCall q = {d_lcp, d_bwt, n, base_id, kind, min_len, min_occ};
        return rep_list(c, s, q, out_or_null, cap, total, true, &keep.st);
    });
}

int archon_hip_get_repeat_stats(int dev, archon_hip_repeat_stats *out) { return t_rep_stats.get(dev, out, "repeats call"); }

// ---- longest previous factors and the LZ77 parse (lz.hiph: the kernels and their drivers; here the argument checks and the statistics)
int archon_hip_lpf_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t dir, archon_hip_lpf_rec *d_lpf, int dev, void *stream)
{
    ARCHON_TRY(lpf_check(d_sa, d_lcp, d_lpf, n, dir));
    if ((uintptr_t)d_lpf & 7u) { set_error("lpf: the records are not 8-byte aligned"); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_lz_stats> keep(t_lz_stats, dev);
        lz_call_stats(&keep.st, n, dir);
        StageTimer tm(c, 96, s);
        return lpf_run(c, s, tm, d_sa, d_lcp, n, dir, d_lpf, &keep.st);
    });
}

// host buffers: sa, lcp and the records through the context's staging buffers
int archon_hip_lpf(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t dir, archon_hip_lpf_rec *lpf, int dev)
{
    ARCHON_TRY(lpf_check(sa, lcp, lpf, n, dir));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_lz_stats> keep(t_lz_stats, dev);
        lz_call_stats(&keep.st, n, dir);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        archon_hip_lpf_rec *d_lpf = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n * 4 + 64, (void **)&d_sa));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n * 4 + 64, (void **)&d_lcp));
        ARCHON_TRY(ctx_io(c, 2, (size_t)n * 8 + 64, (void **)&d_lpf));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)n * 4, hipMemcpyHostToDevice, s));
        StageTimer tm(c, 96, s);
        ARCHON_TRY(lpf_run(c, s, tm, d_sa, d_lcp, n, dir, d_lpf, &keep.st));
        ARCHON_HIP_TRY(hipMemcpyAsync(lpf, d_lpf, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_lz_parse_dev(const archon_hip_lpf_rec *d_lpf, uint32_t n, archon_hip_phrase *d_out_or_null, uint64_t cap, uint64_t *total, int dev,
                            void *stream)
{
    ARCHON_TRY(parse_check(d_lpf, total, n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_lz_stats> keep(t_lz_stats, dev);
        lz_call_stats(&keep.st, n, 0);
        StageTimer tm(c, 96, s);
        ParseCall q = {reinterpret_cast<const uint32_t *>(d_lpf), n};
        return parse_list(c, s, tm, q, d_out_or_null, cap, total, false, &keep.st);
    });
}

// host buffers: the records through staging buffer 0, the phrases through 2
int archon_hip_lz_parse(const archon_hip_lpf_rec *lpf, uint32_t n, archon_hip_phrase *out_or_null, uint64_t cap, uint64_t *total, int dev)
{
    ARCHON_TRY(parse_check(lpf, total, n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_lz_stats> keep(t_lz_stats, dev);
        lz_call_stats(&keep.st, n, 0);
        uint32_t *d_lpf = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n * 8 + 64, (void **)&d_lpf));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_lpf, lpf, (size_t)n * 8, hipMemcpyHostToDevice, s));
        StageTimer tm(c, 96, s);
        ParseCall q = {d_lpf, n};
        return parse_list(c, s, tm, q, out_or_null, cap, total, true, &keep.st);
    });
}

int archon_hip_get_lz_stats(int dev, archon_hip_lz_stats *out) { return t_lz_stats.get(dev, out, "LZ call"); }

// ---- k-mers, per-position counts and shortest unique substrings (kmers.hiph: the kernels and their drivers; here the argument
// checks and the statistics).  *total is written whenever it is given: 0 before any refusal
int archon_hip_kmers_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ,
                         archon_hip_kmer *d_out_or_null, uint64_t cap, uint64_t *total, uint32_t *d_hist_or_null, uint32_t bins, int dev, void *stream)
{
    ARCHON_TRY(kmers_check(d_sa, d_lcp, total, n, k, d_hist_or_null, bins));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, k, min_occ, max_occ, bins, 0);
        KmerCall q = {d_sa, d_lcp, n, k, min_occ, max_occ, bins};
        return kmer_list(c, s, q, d_out_or_null, cap, total, d_hist_or_null, false, &keep.st);
    });
}

int archon_hip_kmers(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ, archon_hip_kmer *out_or_null,
                     uint64_t cap, uint64_t *total, uint32_t *hist_or_null, uint32_t bins, int dev)
{
    ARCHON_TRY(kmers_check(sa, lcp, total, n, k, hist_or_null, bins));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, k, min_occ, max_occ, bins, 0);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, s, sa, lcp, n, &d_sa, &d_lcp));
        KmerCall q = {d_sa, d_lcp, n, k, min_occ, max_occ, bins};
        return kmer_list(c, s, q, out_or_null, cap, total, hist_or_null, true, &keep.st);
    });
}

int archon_hip_kmer_occ_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t k, uint32_t *d_occ, int dev, void *stream)
{
    ARCHON_TRY(kmer_occ_check(d_sa, d_lcp, d_occ, n, k));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, k, 0, 0, 0, 1);
        KmerCall q = {d_sa, d_lcp, n, k};
        return kmer_occ_run(c, s, q, d_occ, false, &keep.st);
    });
}

int archon_hip_kmer_occ(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t k, uint32_t *occ, int dev)
{
    ARCHON_TRY(kmer_occ_check(sa, lcp, occ, n, k));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, k, 0, 0, 0, 1);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, s, sa, lcp, n, &d_sa, &d_lcp));
        KmerCall q = {d_sa, d_lcp, n, k};
        return kmer_occ_run(c, s, q, occ, true, &keep.st);
    });
}

int archon_hip_sus_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, uint32_t *d_sus, int dev, void *stream)
{
    ARCHON_TRY(sus_check(d_sa, d_lcp, d_sus, n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, 0, 0, 0, 0, 2);
        return kmer_sus_run(c, s, d_sa, d_lcp, n, d_sus, false, &keep.st);
    });
}

int archon_hip_sus(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t *sus, int dev)
{
    ARCHON_TRY(sus_check(sa, lcp, sus, n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, 0, 0, 0, 0, 2);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, s, sa, lcp, n, &d_sa, &d_lcp));
        return kmer_sus_run(c, s, d_sa, d_lcp, n, sus, true, &keep.st);
    });
}

int archon_hip_get_kmer_stats(int dev, archon_hip_kmer_stats *out) { return t_kmer_stats.get(dev, out, "k-mer call"); }

// ---- minimal absent words (maw.hiph: the kernel and its drivers; here the argument checks and the statistics)
int archon_hip_maws_dev(const uint32_t *d_sa, const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, uint32_t min_len,
                        uint32_t max_len, archon_hip_maw *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream)
{
    ARCHON_TRY(maws_check(d_sa, d_lcp, d_bwt, total, n, base_id, min_len, max_len));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_maw_stats> keep(t_maw_stats, dev);
        maw_call_stats(&keep.st, n, min_len, max_len);
        return maw_over_copy(c, s, d_sa, d_lcp, nullptr, d_bwt, n, base_id, min_len, max_len, d_out_or_null, cap, total, false, &keep.st);
    });
}

// host buffers: sa and lcp through staging buffers 0 and 1, the BWT straight into the call's table, the words through buffer 2
int archon_hip_maws(const uint32_t *sa, const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base_id, uint32_t min_len, uint32_t max_len,
                    archon_hip_maw *out_or_null, uint64_t cap, uint64_t *total, int dev)
{
    ARCHON_TRY(maws_check(sa, lcp, bwt, total, n, base_id, min_len, max_len));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_maw_stats> keep(t_maw_stats, dev);
        maw_call_stats(&keep.st, n, min_len, max_len);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, s, sa, lcp, n, &d_sa, &d_lcp));
        return maw_over_copy(c, s, d_sa, d_lcp, bwt, nullptr, n, base_id, min_len, max_len, out_or_null, cap, total, true, &keep.st);
    });
}

int archon_hip_maw_last_stats(int dev, archon_hip_maw_stats *out) { return t_maw_stats.get(dev, out, "minimal-absent-words call"); }

// ---- order-k entropy, substring complexity and BWT runs (entropy.hiph: the kernels and their drivers; here the argument checks
// and the statistics)
int archon_hip_entropy_dev(const uint32_t *d_sa, const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, const uint32_t *ks,
                           uint32_t nk, struct archon_hip_entropy *out, int dev, void *stream)
{
    ARCHON_TRY(entropy_check(d_sa, d_lcp, d_bwt, n, base_id, ks, nk, out));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_entropy_stats> keep(t_ent_stats, dev);
        ent_call_stats(&keep.st, n, nk, 0);
        return ent_over_copy(c, s, d_sa, d_lcp, nullptr, d_bwt, n, base_id, ks, nk, out, &keep.st);
    });
}

// host buffers: sa and lcp through staging buffers 0 and 1, the BWT straight into the call's table
int archon_hip_entropy(const uint32_t *sa, const uint32_t *lcp, const uint8_t *bwt, uint32_t n, uint32_t base_id, const uint32_t *ks, uint32_t nk,
                       struct archon_hip_entropy *out, int dev)
{
    ARCHON_TRY(entropy_check(sa, lcp, bwt, n, base_id, ks, nk, out));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_entropy_stats> keep(t_ent_stats, dev);
        ent_call_stats(&keep.st, n, nk, 0);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, s, sa, lcp, n, &d_sa, &d_lcp));
        return ent_over_copy(c, s, d_sa, d_lcp, bwt, nullptr, n, base_id, ks, nk, out, &keep.st);
    });
}

int archon_hip_complexity_dev(const uint32_t *d_lcp, const uint8_t *d_bwt_or_null, uint32_t n, uint32_t max_len, uint32_t *d_counts_or_null,
                              struct archon_hip_complexity *rec, int dev, void *stream)
{
    ARCHON_TRY(complexity_check(d_lcp, n, rec));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_entropy_stats> keep(t_ent_stats, dev);
        ent_call_stats(&keep.st, n, 0, 1);
        return cx_run(c, s, d_lcp, d_bwt_or_null, n, max_len, d_counts_or_null, false, rec, &keep.st);
    });
}

// host buffers: lcp through staging buffer 1, the BWT through buffer 0
int archon_hip_complexity(const uint32_t *lcp, const uint8_t *bwt_or_null, uint32_t n, uint32_t max_len, uint32_t *counts_or_null,
                          struct archon_hip_complexity *rec, int dev)
{
    ARCHON_TRY(complexity_check(lcp, n, rec));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_entropy_stats> keep(t_ent_stats, dev);
        ent_call_stats(&keep.st, n, 0, 1);
        uint32_t *d_lcp = nullptr;
        uint8_t *d_bwt = nullptr;
        ARCHON_TRY(ctx_io(c, 1, (size_t)n * 4 + 64, (void **)&d_lcp));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)n * 4, hipMemcpyHostToDevice, s));
        if (bwt_or_null) {
            ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_bwt));
            ARCHON_HIP_TRY(hipMemcpyAsync(d_bwt, bwt_or_null, n, hipMemcpyHostToDevice, s));
        }
        return cx_run(c, s, d_lcp, d_bwt, n, max_len, counts_or_null, true, rec, &keep.st);
    });
}

int archon_hip_entropy_last_stats(int dev, archon_hip_entropy_stats *out) { return t_ent_stats.get(dev, out, "entropy call"); }

// ---- runs and longest common extensions (runs.hiph: the kernels and their drivers; here the argument checks and the statistics)
int archon_hip_lce_dev(const uint32_t *d_sa, const uint32_t *d_lcp, uint32_t n, const uint32_t *d_s, const uint32_t *d_t, uint32_t k, uint32_t *d_out,
                       int dev, void *stream)
{
    ARCHON_TRY(lce_check(d_sa, d_lcp, n, d_s, d_t, k, d_out));
    if (!k) return ARCHON_OK;
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_run_stats> keep(t_run_stats, dev);
        run_call_stats(&keep.st, n, 0, 0, 0, 0, 1);
        return lce_run(c, s, d_sa, d_lcp, n, d_s, d_t, k, d_out, &keep.st);
    });
}

// host buffers: sa and lcp through staging buffers 0 and 1, the queries and their answers through buffer 2
int archon_hip_lce(const uint32_t *sa, const uint32_t *lcp, uint32_t n, const uint32_t *s, const uint32_t *t, uint32_t k, uint32_t *out, int dev)
{
    ARCHON_TRY(lce_check(sa, lcp, n, s, t, k, out));
    if (!k) return ARCHON_OK;
    ARCHON_TRY(lce_check_items(s, t, k, n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t st) -> int {
        KeepStats<archon_hip_run_stats> keep(t_run_stats, dev);
        run_call_stats(&keep.st, n, 0, 0, 0, 0, 1);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr, *d_q = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, st, sa, lcp, n, &d_sa, &d_lcp));
        ARCHON_TRY(lce_stage(c, st, s, t, k, &d_q));
        ARCHON_TRY(lce_run(c, st, d_sa, d_lcp, n, d_q, d_q + k, k, d_q + 2 * (size_t)k, &keep.st));
        ARCHON_HIP_TRY(hipMemcpyAsync(out, d_q + 2 * (size_t)k, (size_t)k * 4, hipMemcpyDeviceToHost, st));
        ARCHON_SYNC(st);
        return ARCHON_OK;
    });
}

int archon_hip_runs_dev(const uint32_t *d_sa, const uint32_t *d_lcp, const uint32_t *d_sa_c, uint32_t n, uint32_t min_period, uint32_t max_period,
                        uint32_t min_copies, uint32_t min_len, archon_hip_run *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream)
{
    ARCHON_TRY(runs_check(d_sa, d_lcp, d_sa_c, total, n, min_period, max_period, min_copies));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_run_stats> keep(t_run_stats, dev);
        run_call_stats(&keep.st, n, min_period, max_period, min_copies, min_len, 0);
        ARCHON_TRY(run_begin(c, s));
        RunCall q = {d_sa, d_lcp, d_sa_c, nullptr, n, {min_period, max_period, min_copies, min_len}};
        return run_list(c, s, q, d_out_or_null, cap, total, false, 0, &keep.st);
    });
}

// host buffers: sa, lcp and sa_c through staging buffers 0, 1 and 2; the records through buffer 0, which sa has left by then
int archon_hip_runs(const uint32_t *sa, const uint32_t *lcp, const uint32_t *sa_c, uint32_t n, uint32_t min_period, uint32_t max_period,
                    uint32_t min_copies, uint32_t min_len, archon_hip_run *out_or_null, uint64_t cap, uint64_t *total, int dev)
{
    ARCHON_TRY(runs_check(sa, lcp, sa_c, total, n, min_period, max_period, min_copies));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_run_stats> keep(t_run_stats, dev);
        run_call_stats(&keep.st, n, min_period, max_period, min_copies, min_len, 0);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr, *d_sa_c = nullptr;
        ARCHON_TRY(stage_sa_lcp(c, s, sa, lcp, n, &d_sa, &d_lcp));
        ARCHON_TRY(ctx_io(c, 2, (size_t)n * 4 + 64, (void **)&d_sa_c));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_sa_c, sa_c, (size_t)n * 4, hipMemcpyHostToDevice, s));
        ARCHON_TRY(run_begin(c, s));
        RunCall q = {d_sa, d_lcp, d_sa_c, nullptr, n, {min_period, max_period, min_copies, min_len}};
        return run_list(c, s, q, out_or_null, cap, total, true, 0, &keep.st);
    });
}

int archon_hip_runs_last_stats(int dev, archon_hip_run_stats *out) { return t_run_stats.get(dev, out, "runs or LCE call"); }

// ---- the FM index (fm_host.hiph: the handle and every driver; here the argument checks and the statistics)
int archon_hip_fm_create(const uint8_t *bwt, uint32_t n, uint32_t base_id, int dev, archon_hip_fm **out)
{
    if (!bwt || !out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("primary row %u out of range [0, %u)", base_id, n); return ARCHON_E_ARG; }
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, dev);
        return fm_build(c, s, bwt, nullptr, true, n, base_id, out, &keep.st);
    });
}

int archon_hip_fm_create_dev(const uint8_t *d_bwt, uint32_t n, uint32_t base_id, int dev, void *stream, archon_hip_fm **out)
{
    if (!d_bwt || !out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("primary row %u out of range [0, %u)", base_id, n); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, dev);
        return fm_build(c, s, nullptr, d_bwt, true, n, base_id, out, &keep.st);
    });
}

void archon_hip_fm_destroy(archon_hip_fm *f) { fm_release(f); }

int archon_hip_fm_count(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *lo, uint32_t *hi)
{
    if (!f || !patterns || !offsets || !lo || !hi) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!k) return ARCHON_OK;
    ARCHON_TRY(fm_check_offsets(offsets, k));
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, f->dev);
        return fm_count_host(c, s, f, patterns, offsets, k, lo, hi, &keep.st);
    });
}

int archon_hip_fm_count_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t *d_lo, uint32_t *d_hi,
                            void *stream)
{
    if (!f || !d_patterns || !d_offsets || !d_lo || !d_hi) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, f->dev);
        return fm_count_dev(c, s, f, d_patterns, d_offsets, k, d_lo, d_hi, &keep.st);
    });
}

int archon_hip_get_fm_stats(int dev, archon_hip_fm_stats *out) { return t_fm_stats.get(dev, out, "FM call"); }

// ---- the sampled FM index
int archon_hip_fm_sample(archon_hip_fm *f, uint32_t rate)
{
    if (!f) { set_error("null pointer"); return ARCHON_E_ARG; }
    uint32_t rbits;
    ARCHON_TRY(fmw_rate_bits(rate, &rbits));
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_walk_stats> keep(t_fmw_stats, f->dev);
        return fm_sample_run(c, s, f, rbits, nullptr, &keep.st);
    });
}

int archon_hip_fm_read_samples(archon_hip_fm *f, uint32_t *isa, uint32_t cap, uint32_t *count)
{
    if (!f || !isa || !count) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_sampled(f));
    *count = f->smp.ns;
    if (cap < f->smp.ns) { set_error("FM samples: %u ISA entries, room for %u", f->smp.ns, cap); return ARCHON_E_ARG; }
    ARCHON_HIP_TRY(hipSetDevice(f->dev));
    ARCHON_HIP_TRY(hipMemcpy(isa, f->smp.isa, (size_t)f->smp.ns * 4, hipMemcpyDeviceToHost));
    return ARCHON_OK;
}

int archon_hip_fm_locate(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *pos, uint64_t cap, uint64_t *total)
{
    if (!f || !patterns || !offsets || !pos || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_sampled(f));
    *total = 0;
    if (!k) return ARCHON_OK;
    ARCHON_TRY(fm_check_offsets(offsets, k));
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, f->dev);
        KeepStats<archon_hip_fm_walk_stats> walk(t_fmw_stats, f->dev, false);      // (the locate's launches, not the count's: fm_locate_rows)
        fmw_handle_stats(f, &walk.st);
        return fm_locate_host(c, s, f, nullptr, patterns, offsets, k, pos, cap, total, &keep.st, &walk.st);
    });
}

int archon_hip_fm_extract(archon_hip_fm *f, const uint32_t *starts, const uint32_t *offsets, uint32_t k, uint8_t *out)
{
    if (!f || !starts || !offsets || !out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_sampled(f));
    if (!k) return ARCHON_OK;
    for (uint32_t j = 0; j < k; ++j) {
        if (offsets[j + 1] < offsets[j]) { set_error("FM extract: offsets[%u] < offsets[%u]", j + 1, j); return ARCHON_E_ARG; }
        if ((uint64_t)starts[j] + (offsets[j + 1] - offsets[j]) > f->n) {
            set_error("FM extract: request %u [%u, %llu) outside [0, %u]", j, starts[j], (unsigned long long)starts[j] + (offsets[j + 1] - offsets[j]), f->n);
            return ARCHON_E_ARG;
        }
    }
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_walk_stats> keep(t_fmw_stats, f->dev);
        fmw_handle_stats(f, &keep.st);
        return fm_extract_host(c, s, f, starts, offsets, k, out, &keep.st);
    });
}

int archon_hip_fm_extract_dev(archon_hip_fm *f, const uint32_t *d_starts, const uint32_t *d_offsets, uint32_t k, uint8_t *d_out, void *stream)
{
    if (!f || !d_starts || !d_offsets || !d_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_sampled(f));
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_walk_stats> keep(t_fmw_stats, f->dev);
        fmw_handle_stats(f, &keep.st);
        return fm_extract_dev(c, s, f, d_starts, d_offsets, k, d_out, &keep.st);
    });
}

int archon_hip_get_fm_walk_stats(int dev, archon_hip_fm_walk_stats *out) { return t_fmw_stats.get(dev, out, "sampled FM call"); }

// ---- approximate search
int archon_hip_fm_approx(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_mismatches, uint32_t *nhits,
                         uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total)
{
    if (!f || !patterns || !offsets || !nhits || !nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fma_check_k(max_mismatches));
    ARCHON_TRY(fm_check_offsets(offsets, k));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_approx_stats> keep(t_fma_stats, f->dev);
        fma_call_stats(&keep.st, f->n, k, max_mismatches);
        return fm_search_host(c, s, FmaSearch{max_mismatches}, f, patterns, offsets, k, nhits, nocc, hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_approx_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t max_mismatches,
                             uint32_t *d_nhits, uint32_t *d_nocc, archon_hip_fm_hit *d_hits_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    if (!f || !d_patterns || !d_offsets || !d_nhits || !d_nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fma_check_k(max_mismatches));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_approx_stats> keep(t_fma_stats, f->dev);
        fma_call_stats(&keep.st, f->n, k, max_mismatches);
        return fm_search_dev(c, s, FmaSearch{max_mismatches}, f, d_patterns, d_offsets, k, d_nhits, d_nocc, d_hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_locate_hits(archon_hip_fm *f, const uint32_t *offsets, uint32_t k, const archon_hip_fm_hit *hits, uint64_t nhits, uint32_t *pos,
                              uint64_t cap, uint64_t *total)
{
    if (!f || !offsets || (!hits && nhits) || !pos || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_sampled(f));
    ARCHON_TRY(fma_check_hits(offsets, k, hits, nhits, f->n));
    *total = 0;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_approx_stats> keep(t_fma_stats, f->dev);
        fma_call_stats(&keep.st, f->n, k, 0);
        return fma_locate(c, s, f, nullptr, offsets, k, hits, nhits, pos, cap, total, &keep.st);
    });
}

int archon_hip_get_fm_approx_stats(int dev, archon_hip_fm_approx_stats *out) { return t_fma_stats.get(dev, out, "approximate FM call"); }

// ---- class search
int archon_hip_fm_classes(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, const uint32_t *classes, uint32_t *nhits,
                          uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total)
{
    if (!f || !patterns || !offsets || !classes || !nhits || !nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_offsets(offsets, k));
    if (!k) { *total = 0; return ARCHON_OK; }
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_class_stats> keep(t_fmc_stats, f->dev);
        fmc_call_stats(&keep.st, f->n, k);
        return fm_search_host(c, s, FmcSearch{classes, nullptr}, f, patterns, offsets, k, nhits, nocc, hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_classes_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, const uint32_t *d_classes,
                              uint32_t *d_nhits, uint32_t *d_nocc, archon_hip_fm_hit *d_hits_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    if (!f || !d_patterns || !d_offsets || !d_classes || !d_nhits || !d_nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!k) { *total = 0; return ARCHON_OK; }
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_class_stats> keep(t_fmc_stats, f->dev);
        fmc_call_stats(&keep.st, f->n, k);
        return fm_search_dev(c, s, FmcSearch{nullptr, d_classes}, f, d_patterns, d_offsets, k, d_nhits, d_nocc, d_hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_get_fm_class_stats(int dev, archon_hip_fm_class_stats *out) { return t_fmc_stats.get(dev, out, "class FM call"); }

// ---- edit-distance search
int archon_hip_fm_edit(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_errors, uint32_t *nhits,
                       archon_hip_fm_edit_hit *hits_or_null, uint64_t cap, uint64_t *total)
{
    if (!f || !patterns || !offsets || !nhits || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fme_check_k(max_errors));
    ARCHON_TRY(fme_check_patterns(offsets, k, max_errors));
    ARCHON_TRY(fm_check_sampled(f));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_edit_stats> keep(t_fme_stats, f->dev);
        fme_call_stats(&keep.st, f->n, k, max_errors);
        return fme_host(c, s, f, nullptr, nullptr, patterns, offsets, k, max_errors, nhits, hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_edit_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t max_errors, uint32_t *d_nhits,
                           archon_hip_fm_edit_hit *d_hits_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    if (!f || !d_patterns || !d_offsets || !d_nhits || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fme_check_k(max_errors));
    ARCHON_TRY(fme_check_count(k));
    ARCHON_TRY(fm_check_sampled(f));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_edit_stats> keep(t_fme_stats, f->dev);
        fme_call_stats(&keep.st, f->n, k, max_errors);
        return fme_dev(c, s, f, d_patterns, d_offsets, k, max_errors, d_nhits, d_hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_get_fm_edit_stats(int dev, archon_hip_fm_edit_stats *out) { return t_fme_stats.get(dev, out, "edit-distance FM call"); }

// ---- the mirror and the SMEM search
int archon_hip_fm_mirror(archon_hip_fm *f)
{
    if (!f) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, f->dev);
        fmm_call_stats(&keep.st, f, f->n, 0, 0);
        return fmm_mirror_run(c, s, f, nullptr, false, &keep.st);
    });
}

int archon_hip_fm_mirror_dev(archon_hip_fm *f, const uint8_t *d_x, void *stream)
{
    if (!f || !d_x) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, f->dev);
        fmm_call_stats(&keep.st, f, f->n, 0, 0);
        return fmm_mirror_run(c, s, f, d_x, true, &keep.st);
    });
}

int archon_hip_fm_read_mirror(archon_hip_fm *f, uint8_t *bwt, uint32_t cap, uint32_t *base_id)
{
    if (!f || !bwt || !base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmm_check_mirror(f));
    *base_id = f->mirror->base;
    if (cap < f->n) { set_error("FM mirror: %u bytes, room for %u", f->n, cap); return ARCHON_E_ARG; }
    ARCHON_HIP_TRY(hipSetDevice(f->dev));
    ARCHON_HIP_TRY(hipMemcpy(bwt, f->mirror->tab.bwt, f->n, hipMemcpyDeviceToHost));
    return ARCHON_OK;
}

int archon_hip_fm_smems(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t min_len, uint32_t *nmems,
                        uint32_t *nocc, archon_hip_fm_mem *mems_or_null, uint64_t cap, uint64_t *total)
{
    if (!f || !patterns || !offsets || !nmems || !nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_offsets(offsets, k));
    ARCHON_TRY(fmm_check_mirror(f));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, f->dev);
        fmm_call_stats(&keep.st, f, f->n, k, min_len);
        return fm_search_host(c, s, FmmSearch{min_len}, f, patterns, offsets, k, nmems, nocc, mems_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_smems_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t min_len, uint32_t *d_nmems,
                            uint32_t *d_nocc, archon_hip_fm_mem *d_mems_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    if (!f || !d_patterns || !d_offsets || !d_nmems || !d_nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmm_check_mirror(f));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, f->dev);
        fmm_call_stats(&keep.st, f, f->n, k, min_len);
        return fm_search_dev(c, s, FmmSearch{min_len}, f, d_patterns, d_offsets, k, d_nmems, d_nocc, d_mems_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_locate_mems(archon_hip_fm *f, const archon_hip_fm_mem *mems, uint64_t nmems, uint32_t *pos, uint64_t cap, uint64_t *total)
{
    if (!f || (!mems && nmems) || !pos || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_sampled(f));
    ARCHON_TRY(fmm_check_mems(mems, nmems, f->n));
    *total = 0;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, f->dev);
        fmm_call_stats(&keep.st, f, f->n, 0, 0);
        return fmm_locate(c, s, f, nullptr, mems, nmems, pos, cap, total, &keep.st);
    });
}

int archon_hip_get_fm_mem_stats(int dev, archon_hip_fm_mem_stats *out) { return t_fmm_stats.get(dev, out, "SMEM call"); }

// ---- the attached LCP array and the matching statistics
int archon_hip_fm_attach_lcp(archon_hip_fm *f, const uint32_t *lcp)
{
    if (!f || !lcp) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ms_stats> keep(t_fms_stats, f->dev);
        fms_call_stats(&keep.st, f, 0);
        return fms_attach_run(c, s, f, lcp, nullptr, &keep.st);
    });
}

int archon_hip_fm_attach_lcp_dev(archon_hip_fm *f, const uint32_t *d_lcp, void *stream)
{
    if (!f || !d_lcp) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ms_stats> keep(t_fms_stats, f->dev);
        fms_call_stats(&keep.st, f, 0);
        return fms_attach_run(c, s, f, nullptr, d_lcp, &keep.st);
    });
}

int archon_hip_fm_ms(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *len, uint32_t *lo_or_null,
                     uint32_t *hi_or_null)
{
    if (!f || !patterns || !offsets || !len) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!lo_or_null != !hi_or_null) { set_error("FM ms: lo and hi are both given or both null"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_offsets(offsets, k));
    ARCHON_TRY(fms_check_attached(f));
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ms_stats> keep(t_fms_stats, f->dev);
        fms_call_stats(&keep.st, f, k);
        return fms_host(c, s, f, patterns, offsets, k, len, lo_or_null, hi_or_null, &keep.st);
    });
}

int archon_hip_fm_ms_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t *d_len, uint32_t *d_lo_or_null,
                         uint32_t *d_hi_or_null, void *stream)
{
    if (!f || !d_patterns || !d_offsets || !d_len) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!d_lo_or_null != !d_hi_or_null) { set_error("FM ms: lo and hi are both given or both null"); return ARCHON_E_ARG; }
    ARCHON_TRY(fms_check_attached(f));
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ms_stats> keep(t_fms_stats, f->dev);
        fms_call_stats(&keep.st, f, k);
        return fms_dev(c, s, f, d_patterns, d_offsets, k, d_len, d_lo_or_null, d_hi_or_null, &keep.st);
    });
}

int archon_hip_get_fm_ms_stats(int dev, archon_hip_fm_ms_stats *out) { return t_fms_stats.get(dev, out, "matching-statistics call"); }

// ---- the attached suffix array, the matching statistics of a long text and its relative LZ parse
int archon_hip_fm_attach_sa(archon_hip_fm *f, const uint32_t *sa)
{
    if (!f || !sa) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, f->dev);
        fmt_call_stats(&keep.st, f, 0);
        return fmt_attach_run(c, s, f, sa, nullptr, &keep.st);
    });
}

int archon_hip_fm_attach_sa_dev(archon_hip_fm *f, const uint32_t *d_sa, void *stream)
{
    if (!f || !d_sa) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, f->dev);
        fmt_call_stats(&keep.st, f, 0);
        return fmt_attach_run(c, s, f, nullptr, d_sa, &keep.st);
    });
}

int archon_hip_fm_ms_text(archon_hip_fm *f, const uint8_t *text, uint32_t m, uint32_t *len, uint32_t *lo_or_null, uint32_t *hi_or_null)
{
    ARCHON_TRY(fmt_check(f, text, len, lo_or_null, hi_or_null));
    if (!m) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, f->dev);
        fmt_call_stats(&keep.st, f, m);
        return fmt_host(c, s, f, text, m, len, lo_or_null, hi_or_null, &keep.st);
    });
}

int archon_hip_fm_ms_text_dev(archon_hip_fm *f, const uint8_t *d_text, uint32_t m, uint32_t *d_len, uint32_t *d_lo_or_null, uint32_t *d_hi_or_null,
                              void *stream)
{
    ARCHON_TRY(fmt_check(f, d_text, d_len, d_lo_or_null, d_hi_or_null));
    if (!m) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, f->dev);
        fmt_call_stats(&keep.st, f, m);
        return fmt_dev(c, s, f, d_text, m, d_len, d_lo_or_null, d_hi_or_null, &keep.st);
    });
}

int archon_hip_fm_rlz(archon_hip_fm *f, const uint8_t *text, uint32_t m, archon_hip_phrase *out_or_null, uint64_t cap, uint64_t *total)
{
    ARCHON_TRY(rlz_check(f, text, total));
    if (!m) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, f->dev);
        fmt_call_stats(&keep.st, f, m);
        return fmt_rlz(c, s, f, text, nullptr, m, out_or_null, nullptr, cap, total, &keep.st);
    });
}

int archon_hip_fm_rlz_dev(archon_hip_fm *f, const uint8_t *d_text, uint32_t m, archon_hip_phrase *d_out_or_null, uint64_t cap, uint64_t *total,
                          void *stream)
{
    ARCHON_TRY(rlz_check(f, d_text, total));
    if (!m) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, f->dev);
        fmt_call_stats(&keep.st, f, m);
        return fmt_rlz(c, s, f, nullptr, d_text, m, nullptr, d_out_or_null, cap, total, &keep.st);
    });
}

int archon_hip_get_fm_text_stats(int dev, archon_hip_fm_text_stats *out) { return t_fmt_stats.get(dev, out, "text call"); }

// ---- documents
int archon_hip_fm_attach_docs(archon_hip_fm *f, const uint32_t *bounds, uint32_t ndocs)
{
    if (!f || !bounds) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmd_attach_check(f, bounds, ndocs));
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, 0);
        return fmd_attach_run(c, s, f, f->sa.sa, bounds, nullptr, ndocs, &keep.st);
    });
}

int archon_hip_fm_attach_docs_dev(archon_hip_fm *f, const uint32_t *d_bounds, uint32_t ndocs, void *stream)
{
    if (!f || !d_bounds) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!ndocs) { set_error("FM attach docs: no documents"); return ARCHON_E_ARG; }
    if (!f->sa.mem) { set_error("FM attach docs: the handle has no suffix array (archon_hip_fm_attach_sa)"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmd_check_fit(f->n, nullptr, ndocs));
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, 0);
        return fmd_attach_run(c, s, f, f->sa.sa, nullptr, d_bounds, ndocs, &keep.st);
    });
}

int archon_hip_fm_docs(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *ndocs, archon_hip_fm_doc *docs_or_null,
                       uint64_t cap, uint64_t *total)
{
    ARCHON_TRY(fmd_check(f, patterns, offsets, ndocs, total));
    ARCHON_TRY(fm_check_offsets(offsets, k));
    ARCHON_TRY(fmd_check_attached(f));
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, k);
        return fmd_host(c, s, f, patterns, offsets, k, ndocs, docs_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_docs_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t *d_ndocs,
                           archon_hip_fm_doc *d_docs_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    ARCHON_TRY(fmd_check(f, d_patterns, d_offsets, d_ndocs, total));
    ARCHON_TRY(fmd_check_attached(f));
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, k);
        return fmd_dev(c, s, f, d_patterns, d_offsets, k, d_ndocs, d_docs_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_docs_ranges(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, uint32_t k, uint32_t *ndocs, archon_hip_fm_doc *docs_or_null,
                              uint64_t cap, uint64_t *total)
{
    ARCHON_TRY(fmd_check(f, lo, hi, ndocs, total));
    ARCHON_TRY(fmd_check_attached(f));
    for (uint32_t j = 0; j < k; ++j)
        if (lo[j] > hi[j] || hi[j] > f->n) { set_error("FM docs: range %u, rows [%u, %u), is not lo <= hi <= %u", j, lo[j], hi[j], f->n); return ARCHON_E_ARG; }
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, k);
        return fmd_ranges_host<true>(c, s, f, lo, hi, k, ndocs, docs_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_docs_ranges_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, uint32_t k, uint32_t *d_ndocs,
                                  archon_hip_fm_doc *d_docs_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    ARCHON_TRY(fmd_check(f, d_lo, d_hi, d_ndocs, total));
    ARCHON_TRY(fmd_check_attached(f));
    if (!k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, k);
        return fmd_ranges_dev(c, s, f, d_lo, d_hi, k, d_ndocs, d_docs_or_null, cap, total, &keep.st);
    });
}

int archon_hip_fm_doc_of(archon_hip_fm *f, const uint32_t *items, uint64_t count, uint32_t *doc, uint32_t *off_or_null)
{
    ARCHON_TRY(fmd_doc_of_check(f, items, count, doc));
    for (uint64_t i = 0; i < count; ++i)
        if (items[i] - 1 >= f->n) { set_error("FM doc of: item %llu is %u, outside 1 .. %u", (unsigned long long)i, items[i], f->n); return ARCHON_E_ARG; }
    if (!count) return ARCHON_OK;
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, 0);
        return fmd_doc_of(c, s, f, items, nullptr, count, doc, off_or_null, &keep.st);
    });
}

int archon_hip_fm_doc_of_dev(archon_hip_fm *f, const uint32_t *d_items, uint64_t count, uint32_t *d_doc, uint32_t *d_off_or_null, void *stream)
{
    ARCHON_TRY(fmd_doc_of_check(f, d_items, count, d_doc));
    if (!count) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, f->dev);
        fmd_call_stats(&keep.st, f, 0);
        return fmd_doc_of(c, s, f, nullptr, d_items, count, d_doc, d_off_or_null, &keep.st);
    });
}

int archon_hip_get_fm_doc_stats(int dev, archon_hip_fm_doc_stats *out) { return t_fmd_stats.get(dev, out, "documents call"); }

// ---- windows
int archon_hip_fm_attach_wm(archon_hip_fm *f)
{
    if (!f) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!f->sa.mem) { set_error("FM attach wm: the handle has no suffix array (archon_hip_fm_attach_sa)"); return ARCHON_E_ARG; }
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_win_stats> keep(t_fmwin_stats, f->dev);
        fmwin_call_stats(&keep.st, f, 0, 0);
        return fmwin_attach_run(c, s, f, f->sa.sa, &keep.st);
    });
}

// one window call of either kind, host or device arrays: the checks every form shares, the context, the record
static int fmwin_call(archon_hip_fm *f, FmWinCall q, void *stream, uint64_t *total)
{
    q.f = f;
    ARCHON_TRY(fmwin_check_attached(f));
    if (q.host) ARCHON_TRY(fmwin_check_queries(f->n, q.lo, q.hi, q.a, q.b, q.k));
    if (!q.k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_win_stats> keep(t_fmwin_stats, f->dev);
        fmwin_call_stats(&keep.st, f, q.k, q.most);
        return fmwin_run(c, s, q, total, &keep.st);
    });
}

int archon_hip_fm_win_count(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, const uint32_t *a_or_null, const uint32_t *b_or_null, uint32_t k,
                            uint32_t *count)
{
    ARCHON_TRY(fmwin_check(f, lo, hi, a_or_null, b_or_null, count, k));
    return fmwin_call(f, FmWinCall{f, k, 0, lo, hi, a_or_null, b_or_null, nullptr, true, false, false, count, nullptr, nullptr, 0}, nullptr, nullptr);
}

int archon_hip_fm_win_count_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_a_or_null, const uint32_t *d_b_or_null,
                                uint32_t k, uint32_t *d_count, void *stream)
{
    ARCHON_TRY(fmwin_check(f, d_lo, d_hi, d_a_or_null, d_b_or_null, d_count, k));
    return fmwin_call(f, FmWinCall{f, k, 0, d_lo, d_hi, d_a_or_null, d_b_or_null, nullptr, false, false, false, d_count, nullptr, nullptr, 0}, stream, nullptr);
}

int archon_hip_fm_win_select(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, const uint32_t *a_or_null, const uint32_t *b_or_null,
                             const uint32_t *idx, uint32_t k, uint32_t *item)
{
    ARCHON_TRY(fmwin_check(f, lo, hi, a_or_null, b_or_null, item, k));
    if (k && !idx) { set_error("null pointer"); return ARCHON_E_ARG; }
    return fmwin_call(f, FmWinCall{f, k, 0, lo, hi, a_or_null, b_or_null, idx, true, true, false, nullptr, item, nullptr, 0}, nullptr, nullptr);
}

int archon_hip_fm_win_select_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_a_or_null, const uint32_t *d_b_or_null,
                                 const uint32_t *d_idx, uint32_t k, uint32_t *d_item, void *stream)
{
    ARCHON_TRY(fmwin_check(f, d_lo, d_hi, d_a_or_null, d_b_or_null, d_item, k));
    if (k && !d_idx) { set_error("null pointer"); return ARCHON_E_ARG; }
    return fmwin_call(f, FmWinCall{f, k, 0, d_lo, d_hi, d_a_or_null, d_b_or_null, d_idx, false, true, false, nullptr, d_item, nullptr, 0}, stream, nullptr);
}

int archon_hip_fm_win_list(archon_hip_fm *f, const uint32_t *lo, const uint32_t *hi, const uint32_t *a_or_null, const uint32_t *b_or_null, uint32_t k,
                           uint32_t most, uint32_t *count, archon_hip_fm_win *out_or_null, uint64_t cap, uint64_t *total)
{
    if (total) *total = 0;
    if (!total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmwin_check(f, lo, hi, a_or_null, b_or_null, count, k));
    return fmwin_call(f, FmWinCall{f, k, most, lo, hi, a_or_null, b_or_null, nullptr, true, false, true, count, nullptr,
                                   reinterpret_cast<fmwin::FmWin *>(out_or_null), cap}, nullptr, total);
}

int archon_hip_fm_win_list_dev(archon_hip_fm *f, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_a_or_null, const uint32_t *d_b_or_null,
                               uint32_t k, uint32_t most, uint32_t *d_count, archon_hip_fm_win *d_out_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    if (total) *total = 0;
    if (!total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmwin_check(f, d_lo, d_hi, d_a_or_null, d_b_or_null, d_count, k));
    return fmwin_call(f, FmWinCall{f, k, most, d_lo, d_hi, d_a_or_null, d_b_or_null, nullptr, false, false, true, d_count, nullptr,
                                   reinterpret_cast<fmwin::FmWin *>(d_out_or_null), cap}, stream, total);
}

int archon_hip_fm_win_last_stats(int dev, archon_hip_fm_win_stats *out) { return t_fmwin_stats.get(dev, out, "window call"); }

// ---- overlaps
int archon_hip_fm_attach_ends(archon_hip_fm *f, const uint32_t *ends, uint32_t ndocs)
{
    if (!f || !ends) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmo_check_ends(ends, ndocs));
    if (!f->sa.mem) { set_error("FM attach ends: the handle has no suffix array (archon_hip_fm_attach_sa)"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmo_check_fit(f->n, ends, ndocs));
    return with_ctx(f->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ovl_stats> keep(t_fmo_stats, f->dev);
        fmo_call_stats(&keep.st, f, 0, 0);
        return fmo_attach_run(c, s, f, f->sa.sa, ends, nullptr, ndocs, &keep.st);
    });
}

int archon_hip_fm_attach_ends_dev(archon_hip_fm *f, const uint32_t *d_ends, uint32_t ndocs, void *stream)
{
    if (!f || !d_ends) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!ndocs) { set_error("FM attach ends: no documents"); return ARCHON_E_ARG; }
    if (!f->sa.mem) { set_error("FM attach ends: the handle has no suffix array (archon_hip_fm_attach_sa)"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmo_check_fit(f->n, nullptr, ndocs));
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ovl_stats> keep(t_fmo_stats, f->dev);
        fmo_call_stats(&keep.st, f, 0, 0);
        return fmo_attach_run(c, s, f, f->sa.sa, nullptr, d_ends, ndocs, &keep.st);
    });
}

// one overlaps call, host or device arrays: the checks both forms share, the context, the record.  *total is written whenever it
// is given: 0 before any refusal
static int fmo_call(archon_hip_fm *f, FmoCall q, void *stream, uint64_t *total)
{
    if (total) *total = 0;
    if (!f || !q.pat || !q.off || !q.novl || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!q.min_len) { set_error("FM overlaps: min_len = 0"); return ARCHON_E_ARG; }
    if (q.host) ARCHON_TRY(fm_check_offsets(q.off, q.k));
    ARCHON_TRY(fmo_check_attached(f));
    if (!q.k) return ARCHON_OK;
    return with_ctx(f->dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ovl_stats> keep(t_fmo_stats, f->dev);
        fmo_call_stats(&keep.st, f, q.k, q.min_len);
        return fmo_run(c, s, q, total, &keep.st);
    });
}

int archon_hip_fm_overlaps(archon_hip_fm *f, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t min_len, uint32_t *novl,
                           archon_hip_fm_ovl *ovl_or_null, uint64_t cap, uint64_t *total)
{
    return fmo_call(f, FmoCall{f, k, min_len, patterns, offsets, true, novl, reinterpret_cast<fmo::FmOvl *>(ovl_or_null), cap}, nullptr, total);
}

int archon_hip_fm_overlaps_dev(archon_hip_fm *f, const uint8_t *d_patterns, const uint32_t *d_offsets, uint32_t k, uint32_t min_len, uint32_t *d_novl,
                               archon_hip_fm_ovl *d_ovl_or_null, uint64_t cap, uint64_t *total, void *stream)
{
    return fmo_call(f, FmoCall{f, k, min_len, d_patterns, d_offsets, false, d_novl, reinterpret_cast<fmo::FmOvl *>(d_ovl_or_null), cap}, stream, total);
}

int archon_hip_fm_ovl_last_stats(int dev, archon_hip_fm_ovl_stats *out) { return t_fmo_stats.get(dev, out, "overlap call"); }

// ---- resident blocks ---------------------------------------------------------------------------------------------------
int archon_hip_block_create(int dev, archon_hip_block **out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_device(dev));
    archon_hip_block *b = new archon_hip_block();
    b->dev = dev;
    memset(&b->stats, 0, sizeof b->stats);
    *out = b;
    return ARCHON_OK;
}

void archon_hip_block_destroy(archon_hip_block *b)
{
    if (!b) return;
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->fm.reset();
        // an empty block (a thread's default block at thread exit) touches no device; bwt is there exactly when x is
        if (b->x || b->sa) {
            (void)hipSetDevice(b->dev);
            (void)b->x.release();
            (void)b->bwt.release();
            (void)b->sa.release();
        }
    }
    delete b;
}

int archon_hip_block_forward(archon_hip_block *b, const uint8_t *x, uint32_t n, uint32_t *sa_or_null, uint32_t *base_id)
{
    if (!b || !x || !base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    std::lock_guard<std::mutex> lkb(b->mu);
    b->valid = false;
    b->fm.reset();
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        ARCHON_TRY(block_reserve(b, n, sa_or_null != nullptr));
        uint32_t *d_sa = sa_or_null ? b->d_sa() : nullptr;
        uint32_t *d_base = c->d_mail() + mail::kDevBase.at;
        ARCHON_HIP_TRY(hipMemcpyAsync(b->d_x(), x, n, hipMemcpyHostToDevice, s));
        ARCHON_TRY(forward_run(c, s, b->d_x(), n, d_sa, b->d_bwt(), d_base));
        ARCHON_HIP_TRY(hipMemcpyAsync(base_id, d_base, 4, hipMemcpyDeviceToHost, s));
        if (sa_or_null) ARCHON_HIP_TRY(hipMemcpyAsync(sa_or_null, d_sa, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        b->n = n;
        b->base = *base_id;
        b->has_sa = sa_or_null != nullptr;
        b->valid = true;
        b->stats = c->stats;
        t_stats.keep(b->dev, c->stats);
        return ARCHON_OK;
    });
}

int archon_hip_block_read_bwt(archon_hip_block *b, uint32_t offset, uint32_t len, uint8_t *dst)
{
    if (!b || !dst) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    if (!b->valid || (uint64_t)offset + len > b->n) { set_error("no resident BWT for that range"); return ARCHON_E_ARG; }
    ARCHON_HIP_TRY(hipSetDevice(b->dev));
    ARCHON_HIP_TRY(hipMemcpy(dst, b->d_bwt() + offset, len, hipMemcpyDeviceToHost));
    return ARCHON_OK;
}

int archon_hip_block_validate(archon_hip_block *b)
{
    if (!b) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int { return validate_resident_run(c, s, b->d_x(), b->n, b->d_sa(), b->d_bwt(), b->base); });
}

// the result through a staging buffer
int archon_hip_block_lcp(archon_hip_block *b, uint32_t *lcp)
{
    if (!b || !lcp) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, nullptr));
        ARCHON_HIP_TRY(hipMemcpyAsync(lcp, d_lcp, (size_t)b->n * 4, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

// the LCP array into staging buffer 1, as archon_hip_block_lcp makes it, and from there into the repeats' count pass
int archon_hip_block_repeats(archon_hip_block *b, uint32_t kind, uint32_t min_len, uint32_t min_occ, archon_hip_repeat *out_or_null, uint64_t cap,
                             uint64_t *total)
{
    if (!b || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(rep_check_kind(kind));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    *total = 0;
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_repeat_stats> keep(t_rep_stats, b->dev);
        rep_call_stats(&keep.st, b->n, kind, min_len, min_occ);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        RepCall q = {d_lcp, b->d_bwt(), b->n, b->base, kind, min_len, min_occ};
        return rep_list(c, s, q, out_or_null, cap, total, true, &keep.st);
    });
}

// the LCP array into staging buffer 1, the LPF records into staging buffer 0, the phrases through 2: neither array visits the
// host unless the caller asks for it
int archon_hip_block_lz(archon_hip_block *b, uint32_t dir, archon_hip_lpf_rec *lpf_or_null, archon_hip_phrase *out_or_null, uint64_t cap, uint64_t *total)
{
    if (total) *total = 0;          // (written before any refusal, as in parse_check)
    if (!b || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(lz_check_dir(dir));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_lz_stats> keep(t_lz_stats, b->dev);
        lz_call_stats(&keep.st, b->n, dir);
        uint32_t *d_lcp = nullptr;
        archon_hip_lpf_rec *d_lpf = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)b->n * 8 + 64, (void **)&d_lpf));       // (before the LCP runs: a refusal leaves no record of it)
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        StageTimer tm(c, 96, s);
        ARCHON_TRY(lpf_run(c, s, tm, b->d_sa(), d_lcp, b->n, dir, d_lpf, &keep.st));
        if (lpf_or_null) ARCHON_HIP_TRY(hipMemcpyAsync(lpf_or_null, d_lpf, (size_t)b->n * 8, hipMemcpyDeviceToHost, s));
        ParseCall q = {reinterpret_cast<const uint32_t *>(d_lpf), b->n};
        return parse_list(c, s, tm, q, out_or_null, cap, total, true, &keep.st);     // (its count waits for the stream: the records have arrived)
    });
}

// the LCP array into staging buffer 1 and, with the resident suffix array, into the k-mer passes; the results through buffer 2
int archon_hip_block_kmers(archon_hip_block *b, uint32_t k, uint32_t min_occ, uint32_t max_occ, archon_hip_kmer *out_or_null, uint64_t cap, uint64_t *total,
                           uint32_t *hist_or_null, uint32_t bins)
{
    if (total) *total = 0;
    if (!b || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(kmer_check_args(k, hist_or_null, bins));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, b->dev);
        kmer_call_stats(&keep.st, b->n, k, min_occ, max_occ, bins, 0);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        KmerCall q = {b->d_sa(), d_lcp, b->n, k, min_occ, max_occ, bins};
        return kmer_list(c, s, q, out_or_null, cap, total, hist_or_null, true, &keep.st);
    });
}

int archon_hip_block_kmer_occ(archon_hip_block *b, uint32_t k, uint32_t *occ)
{
    if (!b || !occ) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(kmer_check_args(k, nullptr, 0));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, b->dev);
        kmer_call_stats(&keep.st, b->n, k, 0, 0, 0, 1);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        KmerCall q = {b->d_sa(), d_lcp, b->n, k};
        return kmer_occ_run(c, s, q, occ, true, &keep.st);
    });
}

int archon_hip_block_sus(archon_hip_block *b, uint32_t *sus)
{
    if (!b || !sus) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, b->dev);
        kmer_call_stats(&keep.st, b->n, 0, 0, 0, 0, 2);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        return kmer_sus_run(c, s, b->d_sa(), d_lcp, b->n, sus, true, &keep.st);
    });
}

// the LCP array into staging buffer 1, the block's own rank table (built here when no FM call has), the words through buffer 2
int archon_hip_block_maws(archon_hip_block *b, uint32_t min_len, uint32_t max_len, archon_hip_maw *out_or_null, uint64_t cap, uint64_t *total)
{
    if (total) *total = 0;
    if (!b || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(maw_check_filters(min_len, max_len));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_maw_stats> keep(t_maw_stats, b->dev);
        maw_call_stats(&keep.st, b->n, min_len, max_len);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        ARCHON_TRY(block_fm_table_own(c, s, b, &keep.st));
        const MawCall q = {b->d_sa(), d_lcp, b->fm->table(), min_len, max_len};
        return maw_run(c, s, q, out_or_null, cap, total, true, &keep.st);
    });
}

// the LCP array into staging buffer 1, the block's own rank table (built here when no FM call has); one wait for all orders
int archon_hip_block_entropy(archon_hip_block *b, const uint32_t *ks, uint32_t nk, struct archon_hip_entropy *out)
{
    ARCHON_TRY(ent_refused(ent_check_orders(ks, nk, out), out, nk));
    if (!b) { set_error("null pointer"); return ent_refused(ARCHON_E_ARG, out, nk); }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(ent_refused(block_check(b, true), out, nk));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_entropy_stats> keep(t_ent_stats, b->dev);
        ent_call_stats(&keep.st, b->n, nk, 0);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        ARCHON_TRY(block_fm_table_own(c, s, b, &keep.st));
        return ent_run(c, s, b->d_sa(), d_lcp, b->fm->table(), ks, nk, out, &keep.st);
    });
}

// the LCP array into staging buffer 1; the runs are those of the resident BWT
int archon_hip_block_complexity(archon_hip_block *b, uint32_t max_len, uint32_t *counts_or_null, struct archon_hip_complexity *rec)
{
    if (!b || !rec) {
        if (rec) memset(rec, 0, sizeof *rec);
        set_error("null pointer");
        return ARCHON_E_ARG;
    }
    std::lock_guard<std::mutex> lkb(b->mu);
    if (block_check(b, true) != ARCHON_OK) {
        memset(rec, 0, sizeof *rec);
        return ARCHON_E_ARG;
    }
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_entropy_stats> keep(t_ent_stats, b->dev);
        ent_call_stats(&keep.st, b->n, 0, 1);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        return cx_run(c, s, d_lcp, b->d_bwt(), b->n, max_len, counts_or_null, true, rec, &keep.st);
    });
}

// the LCP array into staging buffer 1, the queries and their answers through buffer 2
int archon_hip_block_lce(archon_hip_block *b, const uint32_t *s, const uint32_t *t, uint32_t k, uint32_t *out)
{
    if (!b || (k && (!s || !t || !out))) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    if (!k) return ARCHON_OK;
    ARCHON_TRY(lce_check_items(s, t, k, b->n));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t st) -> int {
        KeepStats<archon_hip_run_stats> keep(t_run_stats, b->dev);
        run_call_stats(&keep.st, b->n, 0, 0, 0, 0, 1);
        uint32_t *d_lcp = nullptr, *d_q = nullptr;
        ARCHON_TRY(block_lcp_step(c, st, b, &d_lcp, &keep.st.ms_lcp));
        ARCHON_TRY(lce_stage(c, st, s, t, k, &d_q));
        ARCHON_TRY(lce_run(c, st, b->d_sa(), d_lcp, b->n, d_q, d_q + k, k, d_q + 2 * (size_t)k, &keep.st));
        ARCHON_HIP_TRY(hipMemcpyAsync(out, d_q + 2 * (size_t)k, (size_t)k * 4, hipMemcpyDeviceToHost, st));
        ARCHON_SYNC(st);
        return ARCHON_OK;
    });
}

// The second sort first -- the complemented text, a forward transform on it, rank1 into memory of the call's own, the three
// buffers of the sort freed --, so that its arena and buffers are not live beside the LCP step's; then the LCP array into staging
// buffer 1 and the passes; the records through buffer 2
int archon_hip_block_runs(archon_hip_block *b, uint32_t min_period, uint32_t max_period, uint32_t min_copies, uint32_t min_len,
                          archon_hip_run *out_or_null, uint64_t cap, uint64_t *total)
{
    if (total) *total = 0;
    if (!b || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(run_check_filters(min_period, max_period, min_copies));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_run_stats> keep(t_run_stats, b->dev);
        run_call_stats(&keep.st, b->n, min_period, max_period, min_copies, min_len, 0);
        DevBuf rank1;
        ARCHON_TRY(rank1.alloc(((size_t)b->n + 1) * 4 + 64, "runs: rank of the complemented block"));
        ARCHON_TRY(run_begin(c, s));
        ARCHON_TRY(run_second_sort(c, s, b->d_x(), b->n, reinterpret_cast<uint32_t *>(rank1.p), &keep.st));
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        RunCall q = {b->d_sa(), d_lcp, nullptr, reinterpret_cast<const uint32_t *>(rank1.p), b->n, {min_period, max_period, min_copies, min_len}};
        return run_list(c, s, q, out_or_null, cap, total, true, 2, &keep.st);
    });
}

int archon_hip_block_fm_count(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *lo, uint32_t *hi)
{
    if (!b || !patterns || !offsets || !lo || !hi) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, false));
    if (!k) return ARCHON_OK;
    ARCHON_TRY(fm_check_offsets(offsets, k));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, b->dev);
        ARCHON_TRY(block_fm_table(c, s, b, &keep.st));
        return fm_count_host(c, s, b->fm.get(), patterns, offsets, k, lo, hi, &keep.st);
    });
}

int archon_hip_block_fm_locate(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t *pos, uint64_t cap,
                               uint64_t *total)
{
    if (!b || !patterns || !offsets || !pos || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    *total = 0;
    if (!k) return ARCHON_OK;
    ARCHON_TRY(fm_check_offsets(offsets, k));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_stats> keep(t_fm_stats, b->dev);
        ARCHON_TRY(block_fm_table(c, s, b, &keep.st));
        return fm_locate_host(c, s, b->fm.get(), b->d_sa(), patterns, offsets, k, pos, cap, total, &keep.st, nullptr);
    });
}

int archon_hip_block_fm_index(archon_hip_block *b, uint32_t rate, archon_hip_fm **out)
{
    if (!b || !out) { set_error("null pointer"); return ARCHON_E_ARG; }
    uint32_t rbits;
    ARCHON_TRY(fmw_rate_bits(rate, &rbits));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, false));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        archon_hip_fm *f = nullptr;
        {
            KeepStats<archon_hip_fm_stats> keep(t_fm_stats, b->dev);
            ARCHON_TRY(fm_build(c, s, nullptr, b->d_bwt(), true, b->n, b->base, &f, &keep.st));
        }
        // the samples' record is kept once there is a table to sample
        KeepStats<archon_hip_fm_walk_stats> keep(t_fmw_stats, b->dev);
        const bool from_sa = b->has_sa && !g_route.fm_sample_walk;
        const int rc = fm_sample_run(c, s, f, rbits, from_sa ? b->d_sa() : nullptr, &keep.st);
        if (rc != ARCHON_OK) fm_release(f);
        else *out = f;
        return rc;
    });
}

int archon_hip_block_fm_approx(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_mismatches,
                               uint32_t *nhits, uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total)
{
    if (!b || !patterns || !offsets || !nhits || !nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fma_check_k(max_mismatches));
    ARCHON_TRY(fm_check_offsets(offsets, k));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, false));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_approx_stats> keep(t_fma_stats, b->dev);
        fma_call_stats(&keep.st, b->n, k, max_mismatches);
        ARCHON_TRY(block_fm_table_own(c, s, b, &keep.st));
        return fm_search_host(c, s, FmaSearch{max_mismatches}, b->fm.get(), patterns, offsets, k, nhits, nocc, hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_block_fm_classes(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, const uint32_t *classes,
                                uint32_t *nhits, uint32_t *nocc, archon_hip_fm_hit *hits_or_null, uint64_t cap, uint64_t *total)
{
    if (!b || !patterns || !offsets || !classes || !nhits || !nocc || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fm_check_offsets(offsets, k));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, false));
    if (!k) { *total = 0; return ARCHON_OK; }
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_class_stats> keep(t_fmc_stats, b->dev);
        fmc_call_stats(&keep.st, b->n, k);
        ARCHON_TRY(block_fm_table_own(c, s, b, &keep.st));
        return fm_search_host(c, s, FmcSearch{classes, nullptr}, b->fm.get(), patterns, offsets, k, nhits, nocc, hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_block_fm_locate_hits(archon_hip_block *b, const uint32_t *offsets, uint32_t k, const archon_hip_fm_hit *hits, uint64_t nhits,
                                    uint32_t *pos, uint64_t cap, uint64_t *total)
{
    if (!b || !offsets || (!hits && nhits) || !pos || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(fma_check_hits(offsets, k, hits, nhits, b->n));
    *total = 0;
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_approx_stats> keep(t_fma_stats, b->dev);
        fma_call_stats(&keep.st, b->n, k, 0);
        return fma_locate(c, s, nullptr, b->d_sa(), offsets, k, hits, nhits, pos, cap, total, &keep.st);
    });
}

int archon_hip_block_fm_edit(archon_hip_block *b, const uint8_t *patterns, const uint32_t *offsets, uint32_t k, uint32_t max_errors, uint32_t *nhits,
                             archon_hip_fm_edit_hit *hits_or_null, uint64_t cap, uint64_t *total)
{
    if (!b || !patterns || !offsets || !nhits || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fme_check_k(max_errors));
    ARCHON_TRY(fme_check_patterns(offsets, k, max_errors));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    *total = 0;
    if (!k) return ARCHON_OK;
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_edit_stats> keep(t_fme_stats, b->dev);
        fme_call_stats(&keep.st, b->n, k, max_errors);
        ARCHON_TRY(block_fm_table_own(c, s, b, &keep.st));
        return fme_host(c, s, b->fm.get(), b->d_sa(), b->d_x(), patterns, offsets, k, max_errors, nhits, hits_or_null, cap, total, &keep.st);
    });
}

int archon_hip_block_fm_mirror(archon_hip_block *b, archon_hip_fm *f)
{
    if (!b || !f) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, false));
    ARCHON_TRY(block_check_handle(b, f, "FM mirror"));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, b->dev);
        fmm_call_stats(&keep.st, f, f->n, 0, 0);
        return fmm_mirror_run(c, s, f, b->d_x(), false, &keep.st);
    });
}

// the LCP array into staging buffer 1, as archon_hip_block_lcp makes it, and from there into the handle: it never visits the host
int archon_hip_block_fm_attach_lcp(archon_hip_block *b, archon_hip_fm *f)
{
    if (!b || !f) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(block_check_handle(b, f, "FM attach lcp"));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ms_stats> keep(t_fms_stats, b->dev);
        fms_call_stats(&keep.st, f, 0);
        uint32_t *d_lcp = nullptr;
        ARCHON_TRY(block_lcp_step(c, s, b, &d_lcp, &keep.st.ms_lcp));
        return fms_attach_run(c, s, f, nullptr, d_lcp, &keep.st);
    });
}

// the resident suffix array into the handle, device to device (the LCP step reads b->d_sa() and leaves it as it is)
int archon_hip_block_fm_attach_sa(archon_hip_block *b, archon_hip_fm *f)
{
    if (!b || !f) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(block_check_handle(b, f, "FM attach sa"));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_text_stats> keep(t_fmt_stats, b->dev);
        fmt_call_stats(&keep.st, f, 0);
        return fmt_attach_run(c, s, f, nullptr, b->d_sa(), &keep.st);
    });
}

// the resident suffix array read where it is, device to device: the handle needs no attached suffix array of its own
int archon_hip_block_fm_attach_docs(archon_hip_block *b, archon_hip_fm *f, const uint32_t *bounds, uint32_t ndocs)
{
    if (!b || !f || !bounds) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmd_check_bounds(bounds, ndocs));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(block_check_handle(b, f, "FM attach docs"));
    ARCHON_TRY(fmd_check_fit(f->n, bounds, ndocs));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_doc_stats> keep(t_fmd_stats, b->dev);
        fmd_call_stats(&keep.st, f, 0);
        return fmd_attach_run(c, s, f, b->d_sa(), bounds, nullptr, ndocs, &keep.st);
    });
}

// the resident suffix array read where it is, device to device, as the documents' block form reads it
int archon_hip_block_fm_attach_wm(archon_hip_block *b, archon_hip_fm *f)
{
    if (!b || !f) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(block_check_handle(b, f, "FM attach wm"));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_win_stats> keep(t_fmwin_stats, b->dev);
        fmwin_call_stats(&keep.st, f, 0, 0);
        return fmwin_attach_run(c, s, f, b->d_sa(), &keep.st);
    });
}

// the resident suffix array read where it is, device to device, as the documents' block form reads it
int archon_hip_block_fm_attach_ends(archon_hip_block *b, archon_hip_fm *f, const uint32_t *ends, uint32_t ndocs)
{
    if (!b || !f || !ends) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(fmo_check_ends(ends, ndocs));
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(block_check_handle(b, f, "FM attach ends"));
    ARCHON_TRY(fmo_check_fit(f->n, ends, ndocs));
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_ovl_stats> keep(t_fmo_stats, b->dev);
        fmo_call_stats(&keep.st, f, 0, 0);
        return fmo_attach_run(c, s, f, b->d_sa(), ends, nullptr, ndocs, &keep.st);
    });
}

int archon_hip_block_fm_locate_mems(archon_hip_block *b, const archon_hip_fm_mem *mems, uint64_t nmems, uint32_t *pos, uint64_t cap, uint64_t *total)
{
    if (!b || (!mems && nmems) || !pos || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    ARCHON_TRY(block_check(b, true));
    ARCHON_TRY(fmm_check_mems(mems, nmems, b->n));
    *total = 0;
    return with_ctx(b->dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_fm_mem_stats> keep(t_fmm_stats, b->dev);
        fmm_call_stats(&keep.st, nullptr, b->n, 0, 0);
        return fmm_locate(c, s, nullptr, b->d_sa(), mems, nmems, pos, cap, total, &keep.st);
    });
}

int archon_hip_block_stats(archon_hip_block *b, archon_hip_stats *out)
{
    if (!b || !out) { set_error("null pointer"); return ARCHON_E_ARG; }
    std::lock_guard<std::mutex> lkb(b->mu);
    *out = b->stats;
    return ARCHON_OK;
}

int archon_hip_forward_keep(const uint8_t *x, uint32_t n, uint32_t *sa_or_null, uint32_t *base_id, int dev)
{
    archon_hip_block *b;
    ARCHON_TRY(default_block(dev, &b));
    return archon_hip_block_forward(b, x, n, sa_or_null, base_id);
}

int archon_hip_read_bwt(int dev, uint32_t offset, uint32_t len, uint8_t *dst)
{
    archon_hip_block *b;
    ARCHON_TRY(default_block(dev, &b));
    return archon_hip_block_read_bwt(b, offset, len, dst);
}

int archon_hip_validate_keep(int dev)
{
    archon_hip_block *b;
    ARCHON_TRY(default_block(dev, &b));
    return archon_hip_block_validate(b);
}

int archon_hip_lcp_keep(int dev, uint32_t *lcp)
{
    if (!lcp) { set_error("null pointer"); return ARCHON_E_ARG; }
    archon_hip_block *b;
    ARCHON_TRY(default_block(dev, &b));
    return archon_hip_block_lcp(b, lcp);
}

int archon_hip_bind_context(int dev, int slot)
{
    if (dev < 0 || dev >= kMaxDev || slot < 0 || slot >= kCtxPerDev) { set_error("bind_context: device %d / context %d out of range", dev, slot); return ARCHON_E_ARG; }
    t_slot[dev] = (signed char)(slot + 1);
    return ARCHON_OK;
}

int archon_hip_context_of_thread(int dev)
{
    if (dev < 0 || dev >= kMaxDev) { set_error("device %d out of range", dev); return ARCHON_E_ARG; }
    return thread_slot(dev);
}

int archon_hip_set_option(int dev, const char *name, long value)
{
    if (!name) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (dev < 0 || dev >= kMaxDev) { set_error("device %d out of range", dev); return ARCHON_E_ARG; }
    if (!strcmp(name, "pass_ranges")) {
        if (value < 0 || value > bs::kMaxRanges) { set_error("pass_ranges=%ld out of range [0, %d]", value, bs::kMaxRanges); return ARCHON_E_ARG; }
        g_opt[dev].pass_ranges.store((uint32_t)value);
        return ARCHON_OK;
    }
    if (!strcmp(name, "pass_b_buckets")) { g_opt[dev].pass_b_buckets.store(value ? 1u : 0u); return ARCHON_OK; }
    set_error("unknown option '%s'", name);
    return ARCHON_E_ARG;
}

int archon_hip_get_option(int dev, const char *name, long *value)
{
    if (!name || !value) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (dev < 0 || dev >= kMaxDev) { set_error("device %d out of range", dev); return ARCHON_E_ARG; }
    if (!strcmp(name, "pass_ranges")) { *value = (long)g_opt[dev].pass_ranges.load(); return ARCHON_OK; }
    if (!strcmp(name, "pass_b_buckets")) { *value = (long)g_opt[dev].pass_b_buckets.load(); return ARCHON_OK; }
    set_error("unknown option '%s'", name);
    return ARCHON_E_ARG;
}

void *archon_hip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (device_count() > 0 && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) return p;
    (void)hipGetLastError();
    return nullptr;
}

void archon_hip_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int archon_hip_inverse_dev(const uint8_t *d_bwt, uint32_t n, uint32_t base_id, uint8_t *d_x_out, int dev, void *stream)
{
    if (!d_bwt || !d_x_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("base_id %u >= n %u", base_id, n); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return keep_stats(c, inverse_run(c, s, d_bwt, n, base_id, d_x_out)); });
}

int archon_hip_inverse(const uint8_t *bwt, uint32_t n, uint32_t base_id, uint8_t *x_out, int dev)
{
    if (!bwt || !x_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("base_id %u >= n %u", base_id, n); return ARCHON_E_ARG; }
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_in = nullptr, *d_out = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_in));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n + 64, (void **)&d_out));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_in, bwt, n, hipMemcpyHostToDevice, s));
        ARCHON_TRY(keep_stats(c, inverse_run(c, s, d_in, n, base_id, d_out)));
        ARCHON_HIP_TRY(hipMemcpyAsync(x_out, d_out, n, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_hist256_dev(const uint8_t *d_x, size_t n, uint32_t *d_out256, int dev, void *stream)
{
    if (!d_x || !d_out256) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *, hipStream_t s) -> int {
        ARCHON_TRY(launch_hist256(s, d_x, n, d_out256, n));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_hist256(const uint8_t *x, size_t n, uint32_t out[256], int dev)
{
    if (!x || !out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        DevBuf buf;         // freed when the stream has been waited for (a step that fails leaves it to hipFree, which waits)
        ARCHON_TRY(buf.alloc(n + 64, "hist256"));
        uint32_t *d_counts = c->d_mail() + mail::kDevCounts.at;
        ARCHON_HIP_TRY(hipMemcpyAsync(buf.p, x, n, hipMemcpyHostToDevice, s));
        ARCHON_TRY(launch_hist256(s, reinterpret_cast<const uint8_t *>(buf.p), n, d_counts, n));
        ARCHON_HIP_TRY(hipMemcpyAsync(out, d_counts, 256 * 4, hipMemcpyDeviceToHost, s));
        ARCHON_HIP_TRY(hipStreamSynchronize(s));
        return ARCHON_OK;
    });
}

int archon_hip_validate_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, int dev, void *stream)
{
    if (!d_x || !d_sa) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return validate_run(c, s, d_x, n, d_sa); });
}

int archon_hip_validate_resident_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, const uint8_t *d_bwt, uint32_t base_id, int dev, void *stream)
{
    if (!d_x || !d_sa || !d_bwt) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return validate_resident_run(c, s, d_x, n, d_sa, d_bwt, base_id); });
}

int archon_hip_validate(const uint8_t *x, uint32_t n, const uint32_t *sa, int dev)
{
    if (!x || !sa) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_x = nullptr;
        uint32_t *d_sa = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_x));
        ARCHON_TRY(ctx_io(c, 2, (size_t)n * 4, (void **)&d_sa));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_x, x, n, hipMemcpyHostToDevice, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, s));
        return validate_run(c, s, d_x, n, d_sa);
    });
}

int archon_hip_sa_to_bwt_dev(const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, uint8_t *d_bwt, uint32_t *d_base_id,
                             int dev, void *stream)
{
    if (!d_x || !d_sa || !d_bwt || !d_base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return sa_to_bwt_run(c, s, d_x, n, d_sa, d_bwt, d_base_id); });
}

int archon_hip_sa_to_bwt(const uint8_t *x, uint32_t n, const uint32_t *sa, uint8_t *bwt, uint32_t *base_id, int dev)
{
    if (!x || !sa || !bwt || !base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_x = nullptr, *d_bwt = nullptr;
        uint32_t *d_sa = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_x));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n + 64, (void **)&d_bwt));
        ARCHON_TRY(ctx_io(c, 2, (size_t)n * 4 + 64, (void **)&d_sa));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_x, x, n, hipMemcpyHostToDevice, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, s));
        ARCHON_TRY(sa_to_bwt_run(c, s, d_x, n, d_sa, d_bwt, c->d_mail() + mail::kDevSaBase.at));
        ARCHON_HIP_TRY(hipMemcpyAsync(bwt, d_bwt, n, hipMemcpyDeviceToHost, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(base_id, c->d_mail() + mail::kDevSaBase.at, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

// ---- SURVEY 8(f) N4 on the device (post.hiph; parity unpinned -- the host stage host/archon_post.cpp states the format)
int archon_hip_post_decode_dev(const uint8_t *d_in, size_t in_bytes, uint8_t *d_bwt, uint32_t cap, uint32_t *n_out, int dev, void *stream)
{
    if (!d_in || !d_bwt || !n_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return post_decode_run(c, s, d_in, in_bytes, d_bwt, cap, n_out); });
}

int archon_hip_inverse_post(const uint8_t *in, size_t in_bytes, uint32_t base_id, uint8_t *x_out, uint32_t cap, uint32_t *n_out, int dev)
{
    if (!in || !x_out || !n_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (cap > ARCHON_HIP_MAX_N) { set_error("block size %u out of range", cap); return ARCHON_E_ARG; }
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_in = nullptr, *d_bwt = nullptr, *d_out = nullptr;
        ARCHON_TRY(ctx_io(c, 0, in_bytes + 64, (void **)&d_in));
        ARCHON_TRY(ctx_io(c, 1, (size_t)cap + 64, (void **)&d_bwt));
        ARCHON_TRY(ctx_io(c, 2, (size_t)cap + 64, (void **)&d_out));
        // only the packed stream crosses the link on the way in
        ARCHON_HIP_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, s));
        ARCHON_TRY(post_decode_run(c, s, d_in, in_bytes, d_bwt, cap, n_out));
        const uint32_t n = *n_out;
        if (n == 0) return ARCHON_OK;
        if (base_id >= n) { set_error("base_id %u >= n %u", base_id, n); return ARCHON_E_ARG; }
        ARCHON_TRY(keep_stats(c, inverse_run(c, s, d_bwt, n, base_id, d_out)));
        ARCHON_HIP_TRY(hipMemcpyAsync(x_out, d_out, n, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

size_t archon_hip_post_bound(uint32_t n) { return post::block_bound(n); }

int archon_hip_post_encode_dev(const uint8_t *d_bwt, uint32_t n, uint8_t *d_out, size_t cap, size_t *out_bytes, int dev, void *stream)
{
    if ((!d_bwt && n) || !d_out || !out_bytes) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (n > ARCHON_HIP_MAX_N) { set_error("block size %u out of range [0, %u]", n, ARCHON_HIP_MAX_N); return ARCHON_E_ARG; }
    if (cap < post::block_bound(n)) { set_error("post stage: output buffer of %zu bytes, %zu needed (archon_hip_post_bound)", cap, post::block_bound(n)); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return post_run(c, s, d_bwt, n, d_out, out_bytes); });
}

int archon_hip_forward_post(const uint8_t *x, uint32_t n, uint8_t *out, size_t cap, size_t *out_bytes, uint32_t *base_id, int dev)
{
    if (!x || !out || !out_bytes || !base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    // (cap may be smaller than archon_hip_post_bound(n), the format's worst case of 20 bits per symbol: the stream is built on the
    //  device at full size and a stream longer than cap is an error of this call -- nothing is truncated)
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_x = nullptr, *d_bwt = nullptr, *d_pk = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_x));
        ARCHON_TRY(ctx_io(c, 1, (size_t)n + 64, (void **)&d_bwt));
        ARCHON_TRY(ctx_io(c, 2, post::block_bound(n) + 64, (void **)&d_pk));
        uint32_t *d_base = c->d_mail() + mail::kDevBase.at;
        ARCHON_HIP_TRY(hipMemcpyAsync(d_x, x, n, hipMemcpyHostToDevice, s));
        ARCHON_TRY(keep_stats(c, forward_run(c, s, d_x, n, nullptr, d_bwt, d_base)));
        ARCHON_TRY(post_run(c, s, d_bwt, n, d_pk, out_bytes));
        if (*out_bytes > cap) { set_error("post stage: stream of %zu bytes, output buffer of %zu (archon_hip_post_bound gives the worst case)", *out_bytes, cap); return ARCHON_E_ARG; }
        // only the packed stream crosses the link
        ARCHON_HIP_TRY(hipMemcpyAsync(out, d_pk, *out_bytes, hipMemcpyDeviceToHost, s));
        ARCHON_HIP_TRY(hipMemcpyAsync(base_id, d_base, 4, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_lms_select_dev(const uint8_t *d_x, uint32_t n, uint32_t *d_count256, uint32_t *d_items, uint32_t *n1, int dev, void *stream)
{
    if (!d_x || !d_count256 || !d_items || !n1) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return lms_select_run(c, s, d_x, n, d_count256, d_items, n1); });
}

int archon_hip_lms_select(const uint8_t *x, uint32_t n, uint32_t count[256], uint32_t *items, uint32_t *n1, int dev)
{
    if (!x || !count || !items || !n1) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        uint8_t *d_x = nullptr;
        uint32_t *d_items = nullptr;
        ARCHON_TRY(ctx_io(c, 0, (size_t)n + 64, (void **)&d_x));
        ARCHON_TRY(ctx_io(c, 2, ((size_t)n / 2 + 8) * 4, (void **)&d_items));
        ARCHON_HIP_TRY(hipMemcpyAsync(d_x, x, n, hipMemcpyHostToDevice, s));
        ARCHON_TRY(lms_select_run(c, s, d_x, n, c->d_mail() + mail::kDevLmsCount.at, d_items, n1));
        ARCHON_HIP_TRY(hipMemcpyAsync(count, c->d_mail() + mail::kDevLmsCount.at, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (*n1) ARCHON_HIP_TRY(hipMemcpyAsync(items, d_items, (size_t)*n1 * 4, hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_radix_scatter_dev(const uint8_t *d_src, size_t n, uint8_t *d_dst, int dev, void *stream)
{
    if (!d_src || !d_dst) { set_error("null pointer"); return ARCHON_E_ARG; }
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int { return radix_scatter_run(c, s, d_src, n, d_dst); });
}

int archon_hip_radix_scatter(const uint8_t *src, size_t n, uint8_t *dst, int dev)
{
    if (!src || !dst) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (n >= 0xFFFFFFFFull) { set_error("n too large"); return ARCHON_E_ARG; }
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        DevBuf a, b;        // (freed on the context's device, when the run has waited for its stream)
        ARCHON_TRY(a.alloc(n + 64, "radix scatter"));
        ARCHON_TRY(b.alloc(n + 64, "radix scatter"));
        ARCHON_HIP_TRY(hipMemcpy(a.p, src, n, hipMemcpyHostToDevice));
        ARCHON_TRY(radix_scatter_run(c, s, reinterpret_cast<const uint8_t *>(a.p), n, reinterpret_cast<uint8_t *>(b.p)));
        ARCHON_HIP_TRY(hipMemcpy(dst, b.p, n, hipMemcpyDeviceToHost));
        return ARCHON_OK;
    });
}

// ---- several small blocks per call ---------------------------------------------------------------------------------------
// x3's default block is 4 MiB (bwt/final/x3/archon.c:100,108).  One such block is thirty launches of a few microseconds and
// one or two host round trips: alone on the device it runs at a tenth of the rate of a 256 MiB block.  A batch call deals its
// blocks to `workers` host threads, each bound to a compute context of its own (stream, arena, staging buffers): the
// blocks' kernels, copies and launch gaps overlap.  workers <= 0: chosen from the largest block (8 up to 4 MiB, 4 up to
// 16 MiB, 2 beyond).  Blocks are independent; the first error stops the rest and is returned.
int archon_hip_forward_batch(const uint8_t *const *x, const uint32_t *n, uint32_t count, uint8_t *const *bwt, uint32_t *base_id, int dev, int workers)
{
    if (!x || !n || !bwt || !base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (count == 0) return ARCHON_OK;
    return run_batch(count, batch_workers(n, count, workers), dev, [&](uint32_t i) { return archon_hip_forward(x[i], n[i], nullptr, bwt[i], base_id + i, dev); });
}

int archon_hip_inverse_batch(const uint8_t *const *bwt, const uint32_t *n, const uint32_t *base_id, uint32_t count, uint8_t *const *x_out, int dev, int workers)
{
    if (!bwt || !n || !base_id || !x_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (count == 0) return ARCHON_OK;
    return run_batch(count, batch_workers(n, count, workers), dev, [&](uint32_t i) { return archon_hip_inverse(bwt[i], n[i], base_id[i], x_out[i], dev); });
}

int archon_hip_forward_batch_dev(const uint8_t *const *d_x, const uint32_t *n, uint32_t count, uint32_t *const *d_sa_or_null, uint8_t *const *d_bwt,
                                 uint32_t *const *d_base_id, int dev, int workers)
{
    if (!d_x || !n || !d_bwt || !d_base_id) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (count == 0) return ARCHON_OK;
    return run_batch(count, batch_workers(n, count, workers), dev,
                     [&](uint32_t i) { return archon_hip_forward_dev(d_x[i], n[i], d_sa_or_null ? d_sa_or_null[i] : nullptr, d_bwt[i], d_base_id[i], dev, nullptr); });
}

int archon_hip_inverse_batch_dev(const uint8_t *const *d_bwt, const uint32_t *n, const uint32_t *base_id, uint32_t count, uint8_t *const *d_x_out, int dev, int workers)
{
    if (!d_bwt || !n || !base_id || !d_x_out) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (count == 0) return ARCHON_OK;
    return run_batch(count, batch_workers(n, count, workers), dev, [&](uint32_t i) { return archon_hip_inverse_dev(d_bwt[i], n[i], base_id[i], d_x_out[i], dev, nullptr); });
}

int archon_hip_reserve(uint32_t n, int dev, size_t *bytes_or_null)
{
    ARCHON_TRY(check_n(n));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t) -> int {
        // (reserving means: no allocation inside a later call, whatever the block) -- the layouts counted, not carved
        FwdBuf B{};
        InvArena L;
        Carve f1, f2, i1;
        size_t need = fwd_tier1(f1, B, n, dev, true);
        const size_t inv = inv_layout(i1, L, n);
        if (inv > need) need = inv;
        ARCHON_TRY(ctx_ensure_arena(c, need));
        ARCHON_TRY(ctx_ensure_arena2(c, fwd_tier2(f2, B, n)));
        if (bytes_or_null) *bytes_or_null = c->arena.bytes + c->arena2.bytes;
        return ARCHON_OK;
    });
}

int archon_hip_release(int dev)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (dev < 0 || dev >= kMaxDev) return ARCHON_OK;
    for (int slot = 0; slot < kCtxPerDev; ++slot) {
        Ctx *c = g_ctx[dev][slot];
        if (!c) continue;
        {
            std::lock_guard<std::mutex> lk2(c->mu);
            (void)hipSetDevice(dev);
            (void)hipDeviceSynchronize();
        }
        delete c;       // (~Ctx and its DevBufs, on the device set above; its lock is free again: a locked mutex is not destroyed)
        g_ctx[dev][slot] = nullptr;
    }
    return ARCHON_OK;
}

#ifdef ARCHON_EXPERIMENTS
/* experiments library only (tools/): phase stamps of the last pass A ([0..31]) and pass B ([32..63]) launch */
int archon_hip_exp_stamps(unsigned long long out[64])
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bs::g_pass_stamps), 64 * sizeof(unsigned long long)) == hipSuccess ? ARCHON_OK : ARCHON_E_HIP;
}
/* phase stamps of bucket 30000's workgroup in the last k_local_sort launch */
int archon_hip_exp_ls_stamps(unsigned long long out[16])
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bs::g_ls_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? ARCHON_OK : ARCHON_E_HIP;
}

/* cycle stamps of the middle workgroup of the last k_post_piece launch */
int archon_hip_exp_post_stamps(unsigned long long out[16])
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(post::g_post_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? ARCHON_OK : ARCHON_E_HIP;
}

/* phase stamps of the middle workgroup of the last k_round_fused launch */
int archon_hip_exp_fu_stamps(unsigned long long out[24])
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fwd::g_fu_stamps), 24 * sizeof(unsigned long long)) == hipSuccess ? ARCHON_OK : ARCHON_E_HIP;
}
#endif

/* include/archon_hip_test.h: test-only routing (every route yields the same a7 order; see common.hiph, struct Route) */
int archon_hip_test_route(const char *name, long value)
{
    if (!name) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!strcmp(name, "RESET")) { g_route = Route(); return ARCHON_OK; }
    for (const RouteRow &r : kRoutes) {
        if (strcmp(name, r.name)) continue;
        const bool inside = value >= r.lo && value <= r.hi;
        switch (r.kind) {
        case RouteKind::kFlag: value = value ? 1 : 0; break;
        case RouteKind::kValue: break;
        case RouteKind::kClamp: value = value < r.lo ? r.lo : value > r.hi ? r.over : value; break;
        case RouteKind::kPow2:
            if (value && (!inside || (value & (value - 1)))) { set_error("%s=%ld: not a power of two in [%ld, %ld]", name, value, r.lo, r.hi); return ARCHON_E_ARG; }
            break;
        case RouteKind::kRange:
            if (!inside) { set_error("%s=%ld%s", name, value, r.refusal); return ARCHON_E_ARG; }
            if (value < 0) value = 0;
            break;
        case RouteKind::kMul64:
            if (value && (!inside || value % 64)) { set_error("%s=%ld%s", name, value, r.refusal); return ARCHON_E_ARG; }
            break;
        }
        r.store(value);
        return ARCHON_OK;
    }
    set_error("unknown route '%s'", name);
    return ARCHON_E_ARG;
}

}  // extern "C"
