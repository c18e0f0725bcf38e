// archon_hip.hip -- C ABI of libarchon_hip.so (include/archon_hip.h): contexts,
// the forward / inverse drivers and the host-buffer wrappers.  gfx950 only.
#include "common.hiph"
#include "util.hiph"
#include "radix_sort.hiph"
#include "bucket_sort.hiph"
#include "forward.hiph"
#include "periodic.hiph"
#include "rounds.hiph"
#include "rank_writer.hiph"
#include "mid_rounds.hiph"
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
#include "fm_host.hiph"
#include "repeats.hiph"
#include "lz.hiph"
#include "kmers.hiph"

#include <stdarg.h>
#include <atomic>
#include <chrono>
#include <stdlib.h>
#include <thread>
#include <type_traits>
#include <vector>

namespace archon {

// ------------------------------------------------------------------ errors
static thread_local char t_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof t_err, fmt, ap);
    va_end(ap);
}

Route g_route;
thread_local uint32_t t_sync_count = 0, t_launch_count = 0;

// ------------------------------------------------------------------ contexts
// Compute contexts of a device (arena, staging buffers, stream, mailbox each), created when first used: a host thread is
// bound to one of the first two at its first call on the device and stays there, so one thread sees exactly the
// single-context behaviour, while two threads feeding one GPU -- the container's workers (host/archon_container.cpp) --
// overlap: block k's device-to-host copy runs beside block k+1's host-to-device copy and kernels instead of the three
// standing in series behind one mutex.  Contexts 2 .. 7 exist for callers that name them (archon_hip_bind_context): the
// batch entry points and the container run up to eight small blocks side by side -- a 4 MiB block is thirty launches of
// a few microseconds each and cannot fill the chip or hide its own launch gaps.
static constexpr int kMaxDev = 64, kCtxPerDev = 8, kCtxDefault = 2;      // contexts a device can have / that threads are dealt to by themselves
static constexpr uint32_t kTieListCap = 1u << 20;
static constexpr uint32_t kSmallBlock = 8u << 20;       // blocks below this take the byte count + LSB passes instead of the streaming stage
static Ctx *g_ctx[kMaxDev][kCtxPerDev];
static std::mutex g_ctx_mu;
// The binding is per (thread, device): the k-th thread that comes to device d takes context k mod 2 OF THAT DEVICE (one
// process-wide counter would hand the two workers of a GPU the same context on every node with an even number of GPUs),
// or the context it asked for by name (archon_hip_bind_context: the container's worker w of GPU d asks for context w / G).
static std::atomic<unsigned> g_next_slot[kMaxDev];
static thread_local signed char t_slot[kMaxDev];      // 0: not bound yet; else slot + 1
// The statistics of the calling thread's last call of one kind on a device: kept per thread, so that no other thread's
// call on the same context can replace them.
template <class T>
struct LastStats {
    T v[kMaxDev];
    bool set[kMaxDev];
    void keep(int dev, const T &st)
    {
        v[dev] = st;
        set[dev] = true;
    }
    int get(int dev, T *out, const char *what) const
    {
        if (dev < 0 || dev >= kMaxDev || !set[dev]) { set_error("the calling thread has run no %s on device %d", what, dev); return ARCHON_E_ARG; }
        *out = v[dev];
        return ARCHON_OK;
    }
};
static thread_local LastStats<archon_hip_stats> t_stats;                // transforms (archon_hip_get_stats)
static thread_local LastStats<archon_hip_lcp_stats> t_lcp_stats;        // LCP calls: they leave archon_hip_stats alone
static thread_local LastStats<archon_hip_fm_stats> t_fm_stats;          // FM calls: they leave both of the others alone
static thread_local LastStats<archon_hip_fm_walk_stats> t_fmw_stats;    // sampled-index calls: sample, block_fm_index, locate, extract
static thread_local LastStats<archon_hip_fm_approx_stats> t_fma_stats;  // approximate calls: approx, locate_hits
static thread_local LastStats<archon_hip_fm_class_stats> t_fmc_stats;   // class calls: classes, classes_dev, block_fm_classes
static thread_local LastStats<archon_hip_fm_edit_stats> t_fme_stats;    // edit-distance calls: edit, edit_dev, block_fm_edit
static thread_local LastStats<archon_hip_fm_mem_stats> t_fmm_stats;     // SMEM calls: mirror, smems, locate_mems
static thread_local LastStats<archon_hip_fm_ms_stats> t_fms_stats;      // matching-statistics calls: attach_lcp, ms
static thread_local LastStats<archon_hip_fm_text_stats> t_fmt_stats;    // text calls: attach_sa, ms_text, rlz
static thread_local LastStats<archon_hip_fm_doc_stats> t_fmd_stats;     // documents calls: attach_docs, docs, docs_ranges, doc_of
static thread_local LastStats<archon_hip_repeat_stats> t_rep_stats;     // repeats calls
static thread_local LastStats<archon_hip_lz_stats> t_lz_stats;          // LZ calls: lpf, lz_parse, block_lz
static thread_local LastStats<archon_hip_kmer_stats> t_kmer_stats;      // k-mer calls: kmers, kmer_occ, sus

// The record of one FM call: kept for the calling thread when the scope ends, on whichever path the call leaves it, with the
// host waits and the kernel launches since the scope began.  A record that covers less than its call takes its launches
// where that part runs (`whole_call` false).
template <class T>
struct KeepStats {
    LastStats<T> &last;
    int dev;
    bool whole_call;
    uint32_t syncs0 = t_sync_count, launches0 = t_launch_count;
    T st = {};
    KeepStats(LastStats<T> &l, int d, bool whole = true) : last(l), dev(d), whole_call(whole) {}
    ~KeepStats()
    {
        st.host_syncs = t_sync_count - syncs0;
        if (whole_call) st.kernel_launches = t_launch_count - launches0;
        last.keep(dev, st);
    }
};

static inline int keep_stats(Ctx *c, int rc)
{
    t_stats.keep(c->dev, c->stats);
    return rc;
}

static int thread_slot(int dev)
{
    if (!t_slot[dev]) t_slot[dev] = (signed char)(1 + g_next_slot[dev].fetch_add(1u) % (unsigned)kCtxDefault);
    return t_slot[dev] - 1;
}

// Product options (archon_hip_set_option), per device: read by every transform on that device when it starts.
struct DevOpt {
    std::atomic<uint32_t> pass_ranges{0};       // ranges the streaming passes are cut into; 0 = one per CU
    std::atomic<uint32_t> pass_b_buckets{1};    // pass B deals whole second-byte buckets when the block is balanced
};
static DevOpt g_opt[kMaxDev];

static int device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

static int check_device(int dev)
{
    const int ndev = device_count();
    if (ndev <= 0) {
        set_error("no HIP device available (libarchon_hip has no CPU fallback)");
        return ARCHON_E_NODEVICE;
    }
    if (dev < 0 || dev >= ndev || dev >= kMaxDev) {
        set_error("device %d out of range (have %d)", dev, ndev);
        return ARCHON_E_NODEVICE;
    }
    return ARCHON_OK;
}

int ctx_get(int dev, Ctx **out)
{
    ARCHON_TRY(check_device(dev));
    const int slot = thread_slot(dev);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    ARCHON_HIP_TRY(hipSetDevice(dev));
    if (!g_ctx[dev][slot]) {
        // published after its last allocation: one that fails frees what was made, on this device
        std::unique_ptr<Ctx> c(new Ctx());
        c->dev = dev;
        memset(&c->stats, 0, sizeof c->stats);
        ARCHON_HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        ARCHON_HIP_TRY(hipHostMalloc((void **)&c->h_mail, mail::kWords * sizeof(uint32_t), hipHostMallocDefault));
        memset(c->h_mail, 0, mail::kWords * sizeof(uint32_t));
        ARCHON_HIP_TRY(hipHostGetDevicePointer((void **)&c->h_mail_dev, c->h_mail, 0));      // (coherent: bs::k_mail writes the block's summary there)
        ARCHON_TRY(c->mail_dev.alloc(mail::kDevWords * sizeof(uint32_t), "context mailbox"));
        g_ctx[dev][slot] = c.release();
    }
    *out = g_ctx[dev][slot];
    return ARCHON_OK;
}

// what the DevBufs of a context do not own; the caller has set the device (ctx_get, archon_hip_release)
Ctx::~Ctx()
{
    if (h_mail) (void)hipHostFree(h_mail);
    for (hipEvent_t e : ev_pool)
        if (e) (void)hipEventDestroy(e);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

// Grows a buffer of a context to `want` bytes when it holds fewer than `need`: the device is idle before the old buffer
// goes.  `fail` is the message of a failed allocation, given the bytes asked for.
static int regrow(DevBuf &b, size_t need, size_t want, const char *fail)
{
    if (need <= b.bytes) return ARCHON_OK;
    ARCHON_HIP_TRY(hipDeviceSynchronize());
    ARCHON_HIP_TRY(b.release());
    if (b.alloc(want, "context") != ARCHON_OK) {
        set_error(fail, want);
        return ARCHON_E_NOMEM;
    }
    return ARCHON_OK;
}

int ctx_ensure_arena(Ctx *c, size_t bytes)
{
    return regrow(c->arena, bytes, bytes + (bytes >> 4) + (1u << 20), "device arena allocation of %zu bytes failed");
}

// the second tier grows like the first; growing it never touches the first (a forward call asks for it in mid-flight)
static int ctx_ensure_arena2(Ctx *c, size_t bytes)
{
    return regrow(c->arena2, bytes, bytes + (bytes >> 4) + (1u << 20), "device arena allocation of %zu bytes (general stage) failed");
}

int ctx_io(Ctx *c, int slot, size_t bytes, void **out)
{
    ARCHON_TRY(regrow(c->io[slot], bytes, bytes + 256, "device staging allocation of %zu bytes failed"));
    *out = c->io[slot].p;
    return ARCHON_OK;
}

// Every entry point that computes runs `body` on the calling thread's context of `dev`, under the context's lock, with the
// device set, on the caller's stream when it gave one and on the context's own otherwise.
template <class Body>
static int with_ctx(int dev, void *stream, Body &&body)
{
    Ctx *c;
    ARCHON_TRY(ctx_get(dev, &c));
    std::lock_guard<std::mutex> lk(c->mu);
    ARCHON_HIP_TRY(hipSetDevice(dev));
    return body(c, stream ? (hipStream_t)stream : c->own_stream);
}

// ------------------------------------------------------------------ forward driver
// Device arena of one forward call (one hipMalloc per context, carved by fwd_tier1 / fwd_tier2 below).  Lifetimes decide what shares memory:
//   keyA / keyB (8N each), the value block (8N)   first stage (pass records, or the (key, item) pairs of the 7-pass sort);
//        then the B rounds' (group | key, item) pairs, k_b_finish's rank log in the key buffer the sort left free, and --
//        between rounds, when all of that is dead -- the rank writer's two record regions and the pair chains' sort buffers
//   rlog (8N)   the S rounds' rank log; before the rounds: scratch of the run shortcut / the scans (B.dst)
//   keep (4N)   scratch of the run shortcut and the recount; in the rounds: the pair list
static size_t key_words(uint32_t n)          // u64 words of a key buffer (+ 512: k_local_sort's last round reads, and ignores, rows past the block)
{
    const size_t r = rw::region_records(n);
    return (r > (size_t)n ? r : (size_t)n) + 520;
}
// partial tables of the two-byte count: one per workgroup, at most 256 of them unless a test asks for more pass ranges
// (a test's route wins over the device's option)
static uint32_t eff_pass_ranges(int dev) { return g_route.pass_ranges ? g_route.pass_ranges : g_opt[dev].pass_ranges.load(); }
static uint32_t h16_parts(int dev) { return eff_pass_ranges(dev) > 256u ? (uint32_t)bs::kMaxRanges : 256u; }
// groups the B list / a mid directory can hold: a group of the B list is longer than the S list's limit or straddles a
// tile of the sweep that made it (at most one per tile)
static size_t mid_dir_cap(uint32_t n) { return (size_t)n / 512 + 64; }
// The last kClosedTail bytes of the first-tier arena lie outside every forward call's cursor: the closed form of a clean periodic
// block (periodic.hiph) keeps the nested transform's results there -- suffix array, BWT and row offsets of the 2p-byte block,
// p <= 65 536 -- while the nested call carves the arena from its bottom.
static constexpr size_t kClosedTail = 2u << 20;

// The forward call's 1024 scratch words (FwdBuf::small), cleared by bs::k_prep, which sets the period probe's result word to "none".
namespace fwd_small {
constexpr uint32_t kCounts = 0;     // [256] byte counts of a small block (launch_hist256)
constexpr uint32_t kTotal = 600;    // scan totals; the entries of the first B list (k_first_groups)
constexpr uint32_t kTicket = 601;   // look-back ticket of the sorts and the list kernels (rs::Scratch)
constexpr uint32_t kErr = 602;      // consistency flag (rs::Scratch)
constexpr uint32_t kBase = 603;     // the primary index
constexpr uint32_t kSettled = 604;  // rows the run shortcut settled
constexpr uint32_t kLastBrk = 606;  // [2] the period's last real break, how many breaks
constexpr uint32_t kProbe = 610;    // [pf::kCleanWords] the period probe: period, votes, breaks, whole text compared
constexpr uint32_t kCtl = 640;      // bs::TieCtl
constexpr uint32_t kFu = 700;       // [6] counters of the rounds (general_stage), the words of Cnt
enum Cnt : uint32_t { kCntS = 0, kCntLog = 1, kCntB = 2, kCntGroups = 3, kCntPairs = 4, kCntSeen = 5, kCntWords = 6 };      // entries appended to the next S list, rank log
                                    // entries, entries of the next B list, its groups, pairs listed, pairs seen
constexpr uint32_t kLut = 900;      // [64] the packed keys' recode table (256 bytes)
constexpr uint32_t kWords = 1024;
static_assert(kCounts + 256 <= kTotal && kLastBrk + 2 <= kProbe && kProbe + pf::kCleanWords <= kCtl &&
              kCtl + sizeof(bs::TieCtl) / 4 <= kFu && kFu + kCntWords <= kLut && kLut + 64 <= kWords, "forward scratch words overlap");
}

struct FwdBuf {
    uint8_t *xa;
    uint64_t *keyA, *keyB;
    uint32_t *valA, *valB, *rank, *brk, *sa_own, *v, *keep, *dst;
    uint32_t *upos[2], *ug[2], *uitem[2], *rhist, *pairw;
    uint8_t *y;
    rw::Buffers rwb;           // rank_writer.hiph (r1 / r2 are set per use: they live in the key / value buffers)
    uint2 *slist[2], *rlog;    // rounds.hiph: entries of short groups {row, item | head}, the round's rank updates {item, rank}
    uint32_t *scan_tmp, *hist16, *small;
    bs::Prep *prep;
    uint2 *tie_list;
    uint32_t *h16part;         // packed partial two-byte counts, one 128 KiB table per workgroup of k_hist16
    uint4 *trash;              // write-only trash lines of the pass workgroups (passes.hiph, emit_rec)
    rs::Scratch sc;
    // mid_rounds.hiph: directory of the B list, the class directories of the mid lists (double-buffered), the counters
    uint32_t *gdir_off, *gdir_row, *gcls, *gbig, *mc, *tile_g0, *tile_big;
    uint4 *dirS[2], *dirL[2];
};

// Tier 1: what every block needs (the first stage and its tables).  Returns the bytes to ask for: these, the closed-form tail
// and slack.
static size_t fwd_tier1(Carve &a, FwdBuf &B, uint32_t n, int dev, bool own_sa)
{
    B.xa = a.take<uint8_t>((size_t)n + 64);                     // aligned copy of x (when needed)
    B.y = a.take<uint8_t>((size_t)n + 64);                      // packed key text y (compacted alphabets)
    B.keyA = a.take<uint64_t>(key_words(n));
    B.keyB = a.take<uint64_t>(key_words(n));
    B.valA = reinterpret_cast<uint32_t *>(a.take<uint64_t>(key_words(n)));      // valA | valB
    B.valB = B.valA ? B.valA + ((size_t)n + 16) : nullptr;
    B.sa_own = own_sa ? a.take<uint32_t>(n) : nullptr;          // sa (when the caller wants none)
    B.sc.d_status = a.take<uint32_t>(rs::status_words(n));
    B.sc.d_ghist = a.take<uint32_t>(8 * 256);
    B.sc.d_gstart = a.take<uint32_t>(8 * 256);
    B.hist16 = a.take<uint32_t>(65536);                         // } contiguous: zeroed by ONE memset per count
    B.rhist = a.take<uint32_t>((size_t)bs::kMaxRanges * 256);   // } (hist16, range table of the passes, the counters that
    B.prep = a.take<bs::Prep>(1);                               // }  open Prep)
    B.tie_list = a.take<uint2>(kTieListCap);
    B.trash = a.take<uint4>((size_t)bs::kMaxRanges * bs::kTrashWords);
    B.h16part = a.take<uint32_t>((size_t)h16_parts(dev) * 32768u);   // partial two-byte counts, one table per workgroup of the count
    B.small = a.take<uint32_t>(fwd_small::kWords);
    return a.off + kClosedTail + (1u << 16);
}

// what a caller that keeps buffers of its own above a nested forward call has to leave free (fm_host.hiph: the mirror build)
static size_t fwd_tier1_need(uint32_t n, int dev)
{
    Carve count;
    FwdBuf B{};
    return fwd_tier1(count, B, n, dev, true);
}
static size_t fwd_closed_tail() { return kClosedTail; }

// Tier 2: what only the general stage needs.  Returns the bytes to ask for.
static size_t fwd_tier2(Carve &a, FwdBuf &B, uint32_t n)
{
    const size_t dir = mid_dir_cap(n) + 8;
    B.rank = a.take<uint32_t>((size_t)n + 1);
    B.brk = a.take<uint32_t>(n);                                // the run shortcut's break table, kept for the break-distance round
    B.v = a.take<uint32_t>(n);                                  // first row of the group of every row
    B.keep = a.take<uint32_t>(n);
    for (int i = 0; i < 2; ++i) {                               // the B list (double-buffered)
        B.upos[i] = a.take<uint32_t>(n);
        B.ug[i] = a.take<uint32_t>(n);
        B.uitem[i] = a.take<uint32_t>(n);
    }
    B.pairw = a.take<uint32_t>((size_t)n / 2 + 8);              // the pair list's {row, flag} words
    B.scan_tmp = a.take<uint32_t>(scan_temp_words(n));
    B.slist[0] = a.take<uint2>((size_t)n + 8);                  // the S lists of the refinement rounds (double-buffered)
    B.slist[1] = a.take<uint2>((size_t)n + 8);
    B.rlog = a.take<uint2>((size_t)n + 8);                      // the rank log
    B.dst = reinterpret_cast<uint32_t *>(B.rlog);               // (scratch of the run shortcut / the scans before the rounds)
    B.rwb.cnt1 = a.take<uint32_t>(rw::kMaxCoarse + rw::fine_buckets(n) + 64);
    B.rwb.cnt2 = B.rwb.cnt1 ? B.rwb.cnt1 + rw::kMaxCoarse : nullptr;
    B.gdir_off = a.take<uint32_t>(dir);                         // directory of the B list: first entry, first row, place in the
    B.gdir_row = a.take<uint32_t>(dir);                         // big list, number among the big groups
    B.gcls = a.take<uint32_t>(dir);
    B.gbig = a.take<uint32_t>(dir);
    for (int i = 0; i < 2; ++i) {                               // directories of the two mid classes, double-buffered
        B.dirS[i] = a.take<uint4>(dir);
        B.dirL[i] = a.take<uint4>(dir);
    }
    B.mc = a.take<uint32_t>(fwd::kMcWords);
    B.tile_g0 = a.take<uint32_t>((size_t)n / fwd::kBfTile + 8);         // per tile of the B list: groups before it,
    B.tile_big = a.take<uint32_t>((size_t)n / fwd::kBfTile / 32 + 8);   // "holds big entries"
    return a.off + (1u << 16);
}

static_assert(fwd::kMcWords <= mail::kRounds.len && fwd::kMcWords <= mail::kRoundsInit.len, "the mid lists' counters in the mailbox");
static_assert(2 * fwd::kGapSlots <= mail::kGapTable.len, "the gap table in the mailbox");
static_assert(pf::kCleanWords <= mail::kProbe.len, "the period probe in the mailbox");

// ---- one forward call (forward_run): its buffers, and what each step of the driver decides and leaves for the next

// The route a block takes; the values are those of archon_hip_stats::path.
enum class Path : uint32_t { kSevenPass = 0, kStream = 1, kClosed = 2 };

struct Fwd {
    Ctx *c;
    hipStream_t s;
    uint32_t n;
    int depth;                   // 0 = a caller's block, 1 = the 2p-byte block of a clean periodic block's closed form
    const uint8_t *d_x;          // the text, 16-byte aligned: the caller's, or its copy in B.xa
    uint32_t *d_sa_user;         // the caller's suffix array, or null
    uint8_t *d_bwt;
    uint32_t *d_base_out;        // the caller's primary index
    uint32_t *sa = nullptr, *d_base = nullptr;      // where the suffix array goes; the call's own primary index (fwd_small::kBase)
    bs::TieCtl *d_ctl = nullptr;
    uint32_t *pres = nullptr;    // [pf::kCleanWords] the period probe: [0] period, [1] votes, [2] the text breaks it, [3] the whole text was compared
    FwdBuf B{};
    size_t tail_at = 0, tier1_bytes = 0, arena_bytes = 0, count_zero_bytes = 0;     // the closed-form tail; the arena's tiers; the count's tables
    bool count_tables_clear = true;
    uint32_t R = 0, tpr = 0, allow_aligned = 0;     // the passes' ranges and tiles per range; pass B may deal whole buckets
    bool rel_ok = false;         // ... and take range-relative records
    int forced = -1;             // (tests): 0 = 7-pass route, 1 = streaming stage, -1 = the block decides
    bool closed_ok = false, probe = false, small_block = false;
    bool probe_queued = false, probe_clean = false, probe_fetched = false;      // the period probe: queued, with the whole-text comparison, on its way up
    bool closed = false;         // the probe's verdict: a clean periodic block, written down in closed form
    bs::TieCtl ctl{};            // the streaming stage's tie summary (big_items: its count of items in oversized buckets)
    uint32_t big_items = 0;
    uint32_t hist[256] = {};     // the exact byte histogram x[0 .. n-1], when have_hist
    bool have_hist = false, tail_fetched = false;
    uint32_t sigma = 0, bits = 8;
    uint8_t lut[256];            // the order-preserving recode of the alphabet (have_lut: taken from the presence map)
    bool have_lut = false, presence_done = false;
    Path path = Path::kSevenPass;
    int Q = 1;                   // symbols per key byte on the streaming path
    uint32_t key_bytes = fwd::kKeyBytes, period_hint = 0, period_breaks = 0, closed_period = 0;
    bool brk_ready = false;      // B.brk holds the break table of period_hint, which has period_breaks breaks
    uint32_t h0 = fwd::kKeyBytes, alphabet_bits = 0, radix_passes = 0;      // symbols the first stage sorted on
    bool ws_ready = true, deep_ties = false, stream_done = false;
    // the stages; the 7-pass route's passes (rs::sort_pairs); the streaming stage's passes A and B (their own event banks)
    StageTimer tm{c, 72 * depth, s}, pt{c, 72 * depth + 24, s}, ps{c, 72 * depth + 48, s};
    int e_start = -1, e_count = -1, e_sorted = -1, e_local = -1, e_first = -1, e_general = -1, e_end = -1;
    int iA0 = -1, iA1 = -1, iB0 = -1, iB1 = -1;
    bool trace_host = false;     // (experiments library, ARCHON_TRACE_HOST)
    uint32_t launches0 = 0, syncs0 = 0;             // the thread's counters when the call started (setup): finish subtracts

    // the steps of forward_run, in its order, and what they share
    int setup(), first_look(), closed_form(), alphabet(), period(), recode(), first_stage(), tied_rows(), general_stage(), finish();
    int general_buffers(), fetch_probe(uint32_t words = pf::kCleanWords), fetch_byte_counts(const uint32_t *d_counts), presence();
    int count16(int form, const uint8_t *src, bool force_stream, bool alpha_probe), streaming(int form, const uint8_t *key_text);
    int seven_pass(), first_groups(int mode, const uint64_t *keys, const uint32_t *items, uint32_t shift);
    void queue_probe(bool clean), probe_arrived(), take_byte_hist(bool exact), stamp(int i);
    // what the steps of the general stage (General, Rounds) share: the readback words (mail::GeneralRead), the rounds' counters
    // (fwd_small::Cnt), the look-back words of the list kernels, and the launches that more than one step makes
    uint32_t *rd() const { return c->h_mail + mail::kRead.at; }
    uint32_t *cnt() const { return B.small + fwd_small::kFu; }
    unsigned long long *fg_status() const { return reinterpret_cast<unsigned long long *>(B.sc.d_status); }
    int reset_lookback(uint32_t tiles), recount_tied(), writer_regions(uint64_t *r1);
};

// Calls fn(std::integral_constant<int, V>{}) for the first V of the list that equals v, for the last one when none does: the
// driver's runtime choices (symbols per key byte, a mode, a flag) as the template arguments of the kernel that matches.
template <int V, int... Vs, class Fn>
static void with_const(int v, Fn &&fn)
{
    if constexpr (sizeof...(Vs) == 0) fn(std::integral_constant<int, V>{});
    else if (v == V) fn(std::integral_constant<int, V>{});
    else with_const<Vs...>(v, fn);
}

// ---- the general stage (Fwd::general_stage): its tracer, the refinement rounds (Rounds), its steps (General)

// What more than one step queues.  The look-back words of a list kernel that sweeps `tiles` tiles:
int Fwd::reset_lookback(uint32_t tiles)
{
    ARCHON_HIP_TRY(hipMemsetAsync(fg_status(), 0, (size_t)tiles * sizeof(unsigned long long), s));
    ARCHON_HIP_TRY(hipMemsetAsync(B.sc.d_ticket, 0, sizeof(uint32_t), s));
    return ARCHON_OK;
}

// the tied set as it is now: flags in B.keep, their places in B.dst, their number in fwd_small::kTotal
int Fwd::recount_tied()
{
    ARCHON_LAUNCH(fwd::k_keep_flags, dim3(div_up(n, 256)), dim3(256), 0, s, B.v, n, B.keep);
    ARCHON_TRY(launch_scan<0>(s, B.keep, B.dst, n, B.scan_tmp, B.small + fwd_small::kTotal));
    launches_miscounted(-1);        // four launches, k_keep_flags and the scan's three, were counted as three
    return ARCHON_OK;
}

// the rank writer's record regions (rank_writer.hiph): r1 in a key buffer that is idle, r2 in the value block, the counts cleared
int Fwd::writer_regions(uint64_t *r1)
{
    B.rwb.r1 = reinterpret_cast<uint2 *>(r1);
    B.rwb.r2 = reinterpret_cast<uint2 *>(B.valA);
    ARCHON_HIP_TRY(hipMemsetAsync(B.rwb.cnt1, 0, (rw::kMaxCoarse + rw::fine_buckets(n)) * sizeof(uint32_t), s));
    return ARCHON_OK;
}

struct Rounds;
// Times of the steps and of the rounds, for the experiments library alone (ARCHON_TRACE_ROUNDS; with ARCHON_TRACE_STAMPS the
// stamps of the S kernel's slowest workgroup): the product compiles every call to nothing.
struct RoundTrace {
#ifdef ARCHON_EXPERIMENTS
    using Clock = std::chrono::steady_clock;
    hipStream_t s;
    bool on = getenv("ARCHON_TRACE_ROUNDS") != nullptr;
    Clock::time_point t_last = Clock::now(), t0;
    uint32_t ms0 = 0, mb0 = 0, mm0 = 0;          // the lists when the round began
    explicit RoundTrace(hipStream_t stream) : s(stream) {}
    static double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }
    void step(const char *what)
    {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        fprintf(stderr, "  general_stage: %-28s %.3f ms\n", what, ms_since(t_last));
        t_last = Clock::now();
    }
    int begin(const Rounds &R);
    void break_round(bool distance, uint32_t p, uint32_t h, const Rounds &R) const;
    void doubling_round(uint32_t h, const Rounds &R) const;
#else
    explicit RoundTrace(hipStream_t) {}
    void step(const char *) {}
    int begin(const Rounds &) { return ARCHON_OK; }
    void break_round(bool, uint32_t, uint32_t, const Rounds &) const {}
    void doubling_round(uint32_t, const Rounds &) const {}
#endif
};

// The lists of the refinement rounds and one round over them (rounds.hiph, mid_rounds.hiph).
struct Rounds {
    Fwd &f;
    int cur = 0, cs = 0;                         // the buffers that hold the B list and the S list
    uint32_t ms = 0, mb = 0, bgroups = 1;        // entries of the S list and of the B list, groups of the B list
    uint32_t mm = 0, mdS = 0, mdL = 0;           // the mid lists (mid_rounds.hiph): entries / groups of the two classes in the CURRENT list (buffer `cur`)
    uint64_t *kT = f.B.keyA, *kS = f.B.keyB;     // the B sort's (group | key, item) pairs and the buffers it sorts them into
    uint32_t *vT = f.B.valA, *vS = f.B.valB;
    // pair chains (rounds.hiph, k_pair_*): {smaller item, distance} records, their {row, flag} words, sort buffers, run heads
    // (the list itself lives through the round; the chain pass behind the round's rank updates borrows the key / value
    //  buffers of the B sort, which are idle by then)
    uint64_t *pk = reinterpret_cast<uint64_t *>(f.B.keep), *pk2 = f.B.keyA;       // n/2 records of 8 bytes each
    uint32_t *pv = f.B.pairw, *pv2 = f.B.valA, *pair_v = f.B.valA + (f.n / 2 + 8), *pair_code = f.B.valA + 2 * ((size_t)f.n / 2 + 8);
    // (deep_ties: the streaming stage compared every tied group 64 symbols deep and they still agree -- long duplicates: no
    //  text rounds, and the first doubling round already lists its pairs)
    bool chain_next = f.deep_ties;               // list the pairs of the coming round and settle them by passage
    uint32_t chain_cool = 0;
    const bool chain_ok = f.n >= 4 && !route_off(kRtNoPairChains);
    const bool writer_ok = f.n >= (1u << 22) && !route_off(kRtNoRankWriter);
    const uint32_t kWriterMinLog = f.n >= (1u << 26) ? (24u << 20) : f.n / 4;       // (small blocks keep exercising the writer in the tests)

    // one round: what it was asked for, and what each step decides for the steps behind it
    struct Plan {
        int mode;
        uint32_t hh;
        bool b_only;
        const uint8_t *cert;
        const uint32_t *okey;
        uint32_t chain;                          // the S kernel lists the round's pairs
        uint2 *s_next;                           // the S list the round appends to
        bool mid;                                // the round deals the B list out by group length
        int nxt;                                 // the buffer of the next B list
        uint32_t nS, nL, nbig, nbig_groups;      // groups of the two mid classes; entries / groups that take the global sort
        uint32_t mid_from_b = 0;
        bool split = false;                      // the B list was dealt out: its big groups go to the global sort compacted
        bool writer = false;                     // k_b_finish logs its rank updates by position for the rank writer
        uint32_t shift = 32, nbytes = 0;         // bits of a key, bytes of a (group | key) word
        uint2 *b_log = nullptr;
        uint32_t nlog = 0;                       // entries of the rank log
    };

    explicit Rounds(Fwd &fwd) : f(fwd) {}
    uint32_t tied() const { return ms + mb + mm; }
    int round(int mode, uint32_t hh, bool b_only = false, const uint8_t *cert = nullptr, const uint32_t *okey = nullptr);
    int plan_b(Plan &r), b_keys(const Plan &r), mid_class(const Plan &r, int lanes, const uint4 *dir, uint32_t groups), s_round(const Plan &r), b_sort(Plan &r);
    int fetch_counters(Plan &r), apply_ranks(const Plan &r), next_lists(const Plan &r), pair_chain(uint32_t np);
};

#ifdef ARCHON_EXPERIMENTS
int RoundTrace::begin(const Rounds &R)
{
    ARCHON_SYNC(s);
    t0 = Clock::now();
    ms0 = R.ms, mb0 = R.mb, mm0 = R.mm;
    return ARCHON_OK;
}

void RoundTrace::break_round(bool distance, uint32_t p, uint32_t h, const Rounds &R) const
{
    if (!getenv("ARCHON_TRACE_ROUNDS")) return;
    fprintf(stderr, "break round (%s) p=%u (h=%u) S=%u B=%u %.3f ms -> S=%u B=%u\n", distance ? "distance" : "continuation", p, h, ms0, mb0, ms_since(t0), R.ms, R.mb);
}

void RoundTrace::doubling_round(uint32_t h, const Rounds &R) const
{
    if (!getenv("ARCHON_TRACE_ROUNDS")) return;
    fprintf(stderr, "round h=%u S=%u B=%u M=%u %.3f ms -> S=%u B=%u M=%u (%u + %u groups)\n", h, ms0, mb0, mm0, ms_since(t0), R.ms, R.mb, R.mm, R.mdS, R.mdL);
    unsigned long long v[24];
    if (!ms0 || !getenv("ARCHON_TRACE_STAMPS") || hipMemcpyFromSymbol(v, HIP_SYMBOL(fwd::g_fu_stamps), sizeof v) != hipSuccess) return;
    fprintf(stderr, "   fused wg: longest %llu owned %llu surv/log 0x%llx cycles:", v[11], v[12], v[13]);
    for (int i = 2; i <= 10; ++i) fprintf(stderr, " %llu", v[i] - v[i - 1]);
    fprintf(stderr, " (load, own, gather-issue, heads, ends, sort, newgroups, counts+atomic, stores)\n");
}
#endif

// One round over both lists: mode 0 keys on rank[s-h], mode 1 on the next four text bytes, modes 2 and 3 (hh = the period)
// on the distance to the last period defect and on the rank of the item the key continues as behind it (rounds.hiph,
// break_key / cont_key; rank table kept as in mode 0).
// The rank table is read by every key gather of the round (S: k_round_fused, B: k_b_keys) before anything writes it
// (S: the log, applied at the end; B: k_b_finish): the steps below are ordered accordingly.
// b_only (modes 2, 3 with certified groups, `cert` = the marks of k_zone_certify): the S list sits the round out;
// groups of the B list that have become short are appended to it where it is.
int Rounds::round(int mode, uint32_t hh, bool b_only, const uint8_t *cert, const uint32_t *okey)
{
    Plan r{mode, hh, b_only, cert, okey};
    const uint32_t ms_kept = b_only ? ms : 0u;
    if (b_only) ms = 0;
    r.chain = (chain_next && chain_ok && mode == 0 && ms) ? 1u : 0u;
    const uint32_t m_before = tied();
    // the round's counters start at zero; the kept entries are written behind that clear: k_b_finish appends behind them
    ARCHON_HIP_TRY(hipMemsetAsync(f.cnt(), 0, fwd_small::kCntWords * sizeof(uint32_t), f.s));
    if (ms_kept) ARCHON_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(f.cnt() + fwd_small::kCntS), (int)ms_kept, 1, f.s));
    r.s_next = b_only ? f.B.slist[cs] : f.B.slist[cs ^ 1];
    // Mid groups (mid_rounds.hiph): the B list is dealt out by group length -- groups of at most 16 Ki entries are sorted by
    // ONE workgroup each, in LDS (with the groups the mid kernels made last round); only the longer ones take the global
    // sort.  (Text rounds keep round 3's path: they run on small sets.)
    r.mid = mode != 1 && !route_off(kRtNoMid);
    r.nxt = cur ^ 1;
    ARCHON_TRY(plan_b(r));
    // B: keys (the gather) now, global sort on (group, key) behind the S kernel -- which so runs while the host waits for
    // the sort's digit counts
    ARCHON_TRY(b_keys(r));
    if (r.mid && r.nL) ARCHON_TRY(mid_class(r, fwd::kMidLargeLanes, f.B.dirL[cur], r.nL));
    if (r.mid && r.nS) ARCHON_TRY(mid_class(r, fwd::kMidSmallLanes, f.B.dirS[cur], r.nS));
    ARCHON_TRY(s_round(r));
    ARCHON_TRY(b_sort(r));
    // The round's counters come to the host BEFORE its rank updates are applied: how the S and mid lists' updates (the log) are
    // written depends on how many there are, and the host has to wait for these counters anyway.
    ARCHON_TRY(fetch_counters(r));
    ARCHON_TRY(apply_ranks(r));
    ARCHON_TRY(next_lists(r));
    const uint32_t *rd = f.rd() + mail::kRdCnt;
    const uint32_t np = r.chain ? rd[fwd_small::kCntPairs] : 0u;
    const uint32_t pairs_seen = r.chain ? np : rd[fwd_small::kCntSeen];
    if (np) ARCHON_TRY(pair_chain(np));
    // 9. The next round lists its pairs when this one got nowhere and pairs are most of what is left.
    if (chain_cool) --chain_cool;
    chain_next = chain_ok && !chain_cool && (uint64_t)tied() * 4 >= (uint64_t)m_before * 3 && (uint64_t)pairs_seen * 4 >= ms && ms;
    return ARCHON_OK;
}

// 1. What of the B list takes the global sort: all of it, or -- dealt out (k_b_dir, k_b_plan, one wait) -- its big groups; the
// width of the sort's words.
int Rounds::plan_b(Plan &r)
{
    FwdBuf &B = f.B;
    const uint32_t n = f.n;
    const uint32_t *h_mc = f.c->h_mail + mail::kRounds.at;       // the mid lists' counters (fwd::kMc*)
    r.nS = mdS, r.nL = mdL, r.nbig = mb, r.nbig_groups = bgroups;
    if (r.mid) {
        // the next list starts empty: no groups, its items from the top of the buffer downwards
        // (fills, not copies out of the mailbox: mail::kRounds receives this round's counters further down)
        ARCHON_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(B.mc + fwd::kMcSmall + r.nxt), 0, 1, f.s));
        ARCHON_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(B.mc + fwd::kMcLarge + r.nxt), 0, 1, f.s));
        ARCHON_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(B.mc + fwd::kMcTop + r.nxt), (int)n, 1, f.s));
        // (a B list whose groups average twice the largest mid group -- a periodic block with defects: one group per phase of
        //  the period -- goes to the global sort as it is: the two sweeps that would deal it out find nothing to hand over)
        if (mb && (uint64_t)bgroups * (2u * fwd::kMidLargeCap) > mb) {
            const uint32_t tiles = div_up(mb, fwd::kBfTile);
            ARCHON_TRY(f.reset_lookback(tiles));
            r.split = true;
            ARCHON_LAUNCH(fwd::k_b_dir, dim3(tiles), dim3(256), 0, f.s, B.upos[cur], B.ug[cur], mb, B.gdir_off, B.gdir_row, f.fg_status(), B.sc.d_ticket, B.sc.d_err, B.mc, (uint32_t)mid_dir_cap(n), B.tile_g0);
            ARCHON_LAUNCH(fwd::k_b_plan, dim3(1), dim3(1024), 0, f.s, B.gdir_off, B.gdir_row, mb, B.gcls, B.gbig, B.dirS[cur], B.dirL[cur], B.mc, (uint32_t)cur,
                           (uint32_t)fwd::kMidSmallCap, (uint32_t)fwd::kMidLargeCap, (uint32_t)mid_dir_cap(n), B.sc.d_err, B.tile_big);
            ARCHON_HIP_TRY(hipGetLastError());
            ARCHON_HIP_TRY(hipMemcpyAsync(f.c->h_mail + mail::kRounds.at, B.mc, fwd::kMcWords * sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
            ARCHON_SYNC(f.s);
            if (h_mc[fwd::kMcGroups] > mid_dir_cap(n)) { set_error("B list of %u entries holds %u groups (directory: %zu)", mb, h_mc[fwd::kMcGroups], mid_dir_cap(n)); return ARCHON_E_INTERNAL; }
            r.nS = h_mc[fwd::kMcSmall + cur];
            r.nL = h_mc[fwd::kMcLarge + cur];
            r.nbig = h_mc[fwd::kMcBigEntries];
            r.nbig_groups = h_mc[fwd::kMcBigGroups];
            r.mid_from_b = h_mc[fwd::kMcMidEntries];
            if (r.nbig + r.mid_from_b != mb) { set_error("plan of the B list lost entries (%u + %u of %u)", r.nbig, r.mid_from_b, mb); return ARCHON_E_INTERNAL; }
        }
    }
    f.c->stats.mid_items += r.mid ? mm + r.mid_from_b : 0u;
    // a long B list logs its rank updates by position for the rank writer (apply_ranks) instead of storing them one by one
    r.writer = r.mode != 1 && writer_ok && r.nbig >= (8u << 20);
    uint32_t gbits = 1;
    if (r.mode != 1) { r.shift = 1; while ((2ull * n + (r.mode == 2 ? 2u : 0u)) >> r.shift) ++r.shift; }    // bits of a key k < 2n (mode 2: 2n + 2)
    while ((uint64_t)r.nbig_groups >> gbits) ++gbits;                           // bits of a group number of the (big) B list
    r.nbytes = (r.shift + gbits + 7) / 8;
    return ARCHON_OK;
}

// 2. The keys of the B list's big groups, as (group | key, item) pairs for the global sort, and the sort's first digit counts.
int Rounds::b_keys(const Plan &r)
{
    if (!r.nbig) return ARCHON_OK;
    FwdBuf &B = f.B;
    f.c->stats.seg_big_items += r.nbig;
    const uint32_t tiles = div_up(mb, fwd::kBfTile);
    ARCHON_TRY(f.reset_lookback(tiles));
    ARCHON_HIP_TRY(hipMemsetAsync(B.sc.d_ghist, 0, 8 * 256 * sizeof(uint32_t), f.s));
    if (r.split)
        with_const<0, 2, 3>(r.mode, [&](auto M) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(fwd::k_b_keys_split<decltype(M)::value>), dim3(tiles), dim3(256), 0, f.s, B.upos[cur], B.ug[cur], B.uitem[cur], B.rank, f.d_x, r.hh, f.n,
                           r.shift, mb, kT, vT, f.fg_status(), B.sc.d_ticket, B.sc.d_err, B.sc.d_ghist, r.nbytes, B.brk, r.cert, r.okey,
                           B.gdir_off, B.gcls, B.gbig, B.upos[r.nxt], B.ug[r.nxt], B.tile_g0, B.tile_big);
        });
    else
        with_const<0, 1, 2, 3>(r.mode, [&](auto M) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(fwd::k_b_keys<decltype(M)::value>), dim3(tiles), dim3(256), 0, f.s, B.upos[cur], B.ug[cur], B.uitem[cur], B.rank, f.d_x, r.hh, f.n,
                           r.shift, mb, kT, vT, f.fg_status(), B.sc.d_ticket, B.sc.d_err, B.sc.d_ghist, r.nbytes, B.brk, r.cert, r.okey);
        });
    return ARCHON_OK;
}

// 3. The groups of one mid class (the large one first, then the small one), one workgroup each.
int Rounds::mid_class(const Plan &r, int lanes, const uint4 *dir, uint32_t groups)
{
    FwdBuf &B = f.B;
    with_const<0, 2, 3>(r.mode, [&](auto M) {
        with_const<(int)fwd::kMidLargeLanes, (int)fwd::kMidSmallLanes>(lanes, [&](auto LN) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(fwd::k_mid_round<decltype(M)::value, decltype(LN)::value>), dim3(groups), dim3(decltype(LN)::value), 0, f.s, dir, B.uitem[cur], B.rank, f.d_x, r.hh, f.n,
                           f.sa, r.s_next, B.rlog, f.cnt(), B.uitem[r.nxt], B.dirS[r.nxt], B.dirL[r.nxt], (uint32_t)mid_dir_cap(f.n), B.mc, (uint32_t)r.nxt, f.d_bwt, f.d_base, B.brk, r.cert,
                           r.okey, B.sc.d_err);
        });
    });
    ARCHON_HIP_TRY(hipGetLastError());
    return ARCHON_OK;
}

// 4. The S list, in one kernel: behind the B keys (both read the rank table the round found) and before the B sort, whose
// host waits it fills.
int Rounds::s_round(const Plan &r)
{
    if (!ms) return ARCHON_OK;
    FwdBuf &B = f.B;
    with_const<0, 1, 2, 3>(r.mode, [&](auto M) {
        ARCHON_LAUNCH(HIP_KERNEL_NAME(fwd::k_round_fused<decltype(M)::value>), dim3(div_up(ms, fwd::kFuT)), dim3(fwd::kFuLanes), 0, f.s, B.slist[cs], ms, B.rank, f.d_x, r.hh, f.sa, B.v,
                       B.slist[cs ^ 1], B.rlog, f.cnt(), B.sc.d_err, f.d_bwt, f.d_base, f.n, r.chain, pk, pv, B.brk);
    });
    ARCHON_HIP_TRY(hipGetLastError());
    return ARCHON_OK;
}

// 5. The global sort of the big groups' pairs, and k_b_finish: new groups, ranks (stored, or logged for the writer), the next lists.
int Rounds::b_sort(Plan &r)
{
    if (!r.nbig) return ARCHON_OK;
    FwdBuf &B = f.B;
    uint32_t passes = 0;
    bool b_in_b = false;
    ARCHON_TRY(rs::sort_pairs(f.s, B.sc, kT, vT, kS, vS, r.nbig, (1u << r.nbytes) - 1u, &b_in_b, &passes, nullptr, nullptr, nullptr, true));
    const uint32_t tiles = div_up(r.nbig, fwd::kBfTile);
    ARCHON_TRY(f.reset_lookback(tiles));
    const uint64_t *ks = b_in_b ? kS : kT;
    const uint32_t *vs = b_in_b ? vS : vT;
    r.b_log = r.writer ? reinterpret_cast<uint2 *>(b_in_b ? kT : kS) : nullptr;        // the sort's other key buffer is free now
    // (split: the big groups' rows and old group starts lie compacted in the NEXT list's buffers, which k_b_finish then
    //  overwrites in place -- a tile writes at or below its own positions, and only once every tile before it has
    //  published its totals, which it does after loading its entries)
    const int src = r.split ? r.nxt : cur;
    // (a text round has no rank table yet: its new group starts go to B.v)
    with_const<0, 1>(r.mode == 1, [&](auto T) {
        ARCHON_LAUNCH(HIP_KERNEL_NAME(fwd::k_b_finish<decltype(T)::value>), dim3(tiles), dim3(256), 0, f.s, ks, vs, B.upos[src], B.ug[src], r.nbig, f.sa, decltype(T)::value ? B.v : B.rank, r.s_next,
                       f.cnt(), B.upos[r.nxt], B.ug[r.nxt], B.uitem[r.nxt], f.fg_status(), B.sc.d_ticket, B.sc.d_err, f.d_x, f.d_bwt, f.d_base, f.n, r.b_log);
    });
    ARCHON_HIP_TRY(hipGetLastError());
    return ARCHON_OK;
}

// 6. The round's counters (and the mid lists'), with the round's one unconditional wait.
int Rounds::fetch_counters(Plan &r)
{
    if (r.mid) ARCHON_HIP_TRY(hipMemcpyAsync(f.c->h_mail + mail::kRounds.at, f.B.mc, fwd::kMcWords * sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
    ARCHON_HIP_TRY(hipMemcpyAsync(f.rd() + mail::kRdCnt, f.cnt(), fwd_small::kCntWords * sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
    ARCHON_SYNC(f.s);
    r.nlog = r.mode != 1 ? f.rd()[mail::kRdCnt + fwd_small::kCntLog] : 0u;
    return ARCHON_OK;
}

// 7. Rank updates, now that every key of the round has been read.  Dealt by item into windows of the table (rank_writer.hiph:
// two partition sweeps + one window write, 0.6 ms whatever the number + 11 ps per update) they beat one random store each
// (32 ps) from about 28 M updates on; the B list's updates are logged by position whenever that list is long (b_log).
int Rounds::apply_ranks(const Plan &r)
{
    FwdBuf &B = f.B;
    if (r.b_log || (writer_ok && r.mode != 1 && r.nlog >= kWriterMinLog)) {
        ARCHON_TRY(f.writer_regions(r.b_log == reinterpret_cast<uint2 *>(kT) ? kS : kT));       // the key buffer that is not the B log
        if (r.nlog) ARCHON_LAUNCH(HIP_KERNEL_NAME(rw::k_part<1, 0>), dim3(div_up(r.nlog, rw::kTile)), dim3(rw::kLanes), 0, f.s, B.rlog, nullptr, r.nlog, nullptr, nullptr, nullptr, B.rwb.r1, B.rwb.cnt1);
        if (r.b_log) ARCHON_LAUNCH(HIP_KERNEL_NAME(rw::k_part<1, 0>), dim3(div_up(r.nbig, rw::kTile)), dim3(rw::kLanes), 0, f.s, r.b_log, nullptr, r.nbig, nullptr, nullptr, nullptr, B.rwb.r1, B.rwb.cnt1);
        ARCHON_TRY(rw::write_back(f.s, B.rwb, f.n, B.rank));
        if (!(r.nlog && r.b_log)) launches_miscounted(1);       // rw::k_part<1, 0> was counted for both logs, also when one of them was empty
    } else if (r.nlog) {
        ARCHON_LAUNCH(fwd::k_rank_apply, dim3(div_up(r.nlog, 256)), dim3(256), 0, f.s, B.rlog, f.cnt() + fwd_small::kCntLog, B.rank);
    }
    return ARCHON_OK;
}

// the lists the round left, from its counters
int Rounds::next_lists(const Plan &r)
{
    const uint32_t *rd = f.rd() + mail::kRdCnt, *h_mc = f.c->h_mail + mail::kRounds.at;
    const bool flip = r.mid || mb != 0;         // (short groups that straddle a tile of k_b_finish's sweep stay in B for another round)
    ms = rd[fwd_small::kCntS];
    mb = r.nbig ? rd[fwd_small::kCntB] : 0u;
    bgroups = rd[fwd_small::kCntGroups];
    if (r.mid) {
        mdS = h_mc[fwd::kMcSmall + r.nxt];
        mdL = h_mc[fwd::kMcLarge + r.nxt];
        mm = f.n - h_mc[fwd::kMcTop + r.nxt];
        if (mdS > mid_dir_cap(f.n) || mdL > mid_dir_cap(f.n)) { set_error("mid directory overflow (%u / %u groups)", mdS, mdL); return ARCHON_E_INTERNAL; }
    }
    if (flip) cur ^= 1;
    if (!r.b_only) cs ^= 1;
    return ARCHON_OK;
}

// 8. The round's pairs by passage: sort the records by their smaller item, one look-up per run, spread, apply; one wait for
// the entries the pass hands back to the S list.
int Rounds::pair_chain(uint32_t np)
{
    FwdBuf &B = f.B;
    bool in2 = false;
    uint32_t passes = 0;
    ARCHON_TRY(rs::sort_pairs(f.s, B.sc, pk, pv, pk2, pv2, np, 0xF0u, &in2, &passes));
    const uint64_t *k2 = in2 ? pk2 : pk;
    const uint32_t *v2 = in2 ? pv2 : pv;
    ARCHON_LAUNCH(fwd::k_pair_heads, dim3(div_up(np, 256)), dim3(256), 0, f.s, k2, np, B.rank, pair_v, pair_code);
    ARCHON_TRY(launch_scan<1>(f.s, pair_v, pair_v, np, B.scan_tmp, nullptr));
    ARCHON_LAUNCH(fwd::k_pair_apply, dim3(div_up(np, 256)), dim3(256), 0, f.s, k2, v2, pair_v, pair_code, np, f.sa, B.rank, f.d_x, f.d_bwt, f.d_base, f.n,
                   B.slist[cs], f.cnt());
    ARCHON_HIP_TRY(hipGetLastError());
    launches_miscounted(-1);        // five launches, k_pair_heads, the scan's three and k_pair_apply, were counted as four
    uint32_t *rd = f.rd() + mail::kRdCnt;
    ARCHON_HIP_TRY(hipMemcpyAsync(rd, f.cnt(), sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
    ARCHON_SYNC(f.s);
    const uint32_t back = rd[fwd_small::kCntS] - ms;         // entries the pass could not settle (two per pair)
    ms = rd[fwd_small::kCntS];
    f.c->stats.chain_pairs += np - back / 2u;
    if ((uint64_t)back > np) chain_cool = 3;         // fewer than half of the pairs settled: give the rounds some time
    return ARCHON_OK;
}

// The period-defect rounds (modes 2 and 3 of Rounds::round) and what they go by.
struct PeriodDefects {
    uint32_t period = 0;         // period of the break table in B.brk while its rounds can still settle something
    uint32_t fail = 0;           // continuation rounds in a row that settled nothing
    uint32_t breaks = 0;         // positions where the text stops repeating at that distance
    bool first = true;           // the next of its rounds is the distance round
};

// A5 + A7 for whatever the first stage left tied.  On entry (k_first_groups): sa[] holds the items in first-stage order,
// B.v[i] = first row of the group of row i, and -- ws_ready -- the two lists of the refinement rounds (rounds.hiph): S =
// entries of groups of at most fwd::kFuMax rows in B.slist[0] (fwd_small::kFu counts them), B = the longer groups as
// (row, group start, item) triples in buffer 0 (fwd_small::kTotal counts them, fwd_small::kFu + 3 their groups).  Runs the run
// shortcut for periodic blocks, text rounds, the rank table, doubling rounds with the pair chains.  Rows take their
// BWT symbol when they become final.
struct General {
    Fwd &f;
    archon_hip_stats &st = f.c->stats;
    RoundTrace tr{f.s};
    Rounds R{f};
    PeriodDefects z;
    uint32_t m = 0, h = f.h0;                    // tied rows; symbols every tied group agrees on
    uint32_t ms_first = 0, mb_first = 0, groups_first = 0;      // the lists of k_first_groups
    bool lists_ready = f.ws_ready;               // the lists of k_first_groups still describe the tied set
    bool keep_ready = false;                     // B.keep / B.dst describe the current tied set

    explicit General(Fwd &fwd) : f(fwd) {}
    int entry_counts(), run_shortcut(), settle_runs(uint32_t p), build_lists(), text_rounds(), fill_rank_table(), certified_break_rounds(), break_rounds(), rounds_to_the_end();
};

int Fwd::general_stage()
{
    General g(*this);
    ARCHON_TRY(g.entry_counts());
    ARCHON_TRY(g.run_shortcut());
    ARCHON_TRY(g.build_lists());
    ARCHON_TRY(g.text_rounds());
    ARCHON_TRY(g.fill_rank_table());
    ARCHON_TRY(g.certified_break_rounds());
    ARCHON_TRY(g.rounds_to_the_end());
    g.tr.step("rounds done");
    return ARCHON_OK;
}

// How many rows the first stage left tied, and in which lists.
int General::entry_counts()
{
    tr.step("enter");
    uint32_t *rd = f.rd();
    ARCHON_HIP_TRY(hipMemcpyAsync(rd + mail::kRdTotal, f.B.small + fwd_small::kTotal, sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
    ARCHON_HIP_TRY(hipMemcpyAsync(rd + mail::kRdEntryCnt, f.cnt(), 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
    ARCHON_SYNC(f.s);
    ms_first = f.ws_ready ? rd[mail::kRdEntryCnt + fwd_small::kCntS] : 0u;
    mb_first = rd[mail::kRdTotal];
    groups_first = rd[mail::kRdEntryCnt + fwd_small::kCntGroups];
    m = ms_first + mb_first;
    st.unresolved_initial = m;
    return ARCHON_OK;
}

// Long-repeat defence: when much of the block is tied and one neighbour gap dominates the tied groups,
// settle the periodic runs directly (forward.hiph, k_chain_*) before any doubling round
// (long duplicates without a period -- deep_ties and no period probe -- are pairs: the pair chains of the rounds settle
//  them with less per-group work than this shortcut spends on millions of two-row groups)
int General::run_shortcut()
{
    const uint32_t p_hint = f.period_hint, p_breaks = f.period_breaks;
    if (f.brk_ready && p_breaks && m) {
        // the period is known and the text breaks it somewhere: the tied groups straddle the defects, none of them is one clean
        // run -- the run shortcut would look at every row and settle nothing; the period-defect rounds take all of it
        z.period = p_hint;
        z.breaks = p_breaks;
        st.period = p_hint;
        return ARCHON_OK;
    }
    if (!(m >= f.n / 16 && !(f.deep_ties && p_hint == 0) && !route_off(kRtNoChains))) return ARCHON_OK;
    uint32_t p = p_hint;
    bool dominant = p_hint != 0;        // the driver's period probe already named the period (and the groups may be unordered)
    if (!dominant) {
        // ... or a sample of the neighbour gaps inside the tied groups does: the most frequent gap, when it is a quarter of the sample
        uint32_t *tab = f.B.hist16;                     // 2 * kGapSlots words (32 KiB) of the two-byte count's table, idle by now (256 KiB whatever n is:
                                                        // a list buffer of a small block is shorter than the table)
        ARCHON_HIP_TRY(hipMemsetAsync(tab, 0, 2 * fwd::kGapSlots * sizeof(uint32_t), f.s));
        ARCHON_LAUNCH(fwd::k_gap_sample, dim3(div_up(div_up(f.n, fwd::kGapStride), 256)), dim3(256), 0, f.s, f.sa, f.B.v, f.n, tab);
        const uint32_t *h_tab = f.c->h_mail + mail::kGapTable.at;
        ARCHON_HIP_TRY(hipMemcpyAsync(f.c->h_mail + mail::kGapTable.at, tab, 2 * fwd::kGapSlots * sizeof(uint32_t), hipMemcpyDeviceToHost, f.s));
        ARCHON_SYNC(f.s);
        uint64_t total = 0;
        uint32_t best = 0;
        for (uint32_t i = 0; i < fwd::kGapSlots; ++i) {
            total += h_tab[i];
            if (h_tab[i] > h_tab[best]) best = i;
        }
        p = h_tab[fwd::kGapSlots + best];
        dominant = (uint64_t)h_tab[best] * 4 >= total;
    }
    if (p >= 1 && p < f.n && dominant) ARCHON_TRY(settle_runs(p));
    return ARCHON_OK;
}

// The runs of period p settled directly: the break table (unless the period stage left it), the chain kernels, and -- when
// they settled some rows but not all -- the tied set counted again.
int General::settle_runs(uint32_t p)
{
    FwdBuf &B = f.B;
    hipStream_t s = f.s;
    const uint32_t n = f.n;
    uint32_t *rd = f.rd();
    uint32_t *brk = B.brk, *ginfo = B.dst, *gend = B.keep, *settled = B.small + fwd_small::kSettled;
    uint32_t *gmin = B.ug[1], *gmax = B.uitem[1];       // the second triple buffers are idle
    uint32_t *d_lastbrk = B.small + fwd_small::kLastBrk;
    if (!(f.brk_ready && p == f.period_hint)) {
        ARCHON_HIP_TRY(hipMemsetAsync(d_lastbrk, 0, 2 * sizeof(uint32_t), s));  // [0] last real break, [1] how many
        ARCHON_LAUNCH(fwd::k_period_breaks, dim3(div_up(div_up(n, 4), 256)), dim3(256), 0, s, f.d_x, n, p, brk, d_lastbrk);
        ARCHON_TRY(launch_scan<1>(s, brk, brk, n, B.scan_tmp, nullptr));
    }
    ARCHON_LAUNCH(fwd::k_chain_init, dim3(div_up(n, 256)), dim3(256), 0, s, B.v, n, gmin, gmax, ginfo);
    ARCHON_HIP_TRY(hipMemsetAsync(settled, 0, sizeof(uint32_t), s));
    tr.step("breaks + scan + memsets");
    ARCHON_LAUNCH(fwd::k_chain_minmax, dim3(div_up(n, fwd::kChainRows)), dim3(256), 0, s, f.sa, B.v, n, gmin, gmax);
    tr.step("chain_minmax");
    ARCHON_LAUNCH(fwd::k_chain_probe, dim3(div_up(n, fwd::kChainRows)), dim3(256), 0, s, f.d_x, f.sa, B.v, brk, n, p, gmin, gmax, d_lastbrk, ginfo, gend);
    tr.step("chain_probe");
    ARCHON_LAUNCH(fwd::k_chain_apply, dim3(div_up(n, fwd::kChainRows)), dim3(256), 0, s, f.sa, B.v, ginfo, gend, gmin, gmax, brk, d_lastbrk, f.d_x, n, p, f.d_bwt, f.d_base, settled);
    tr.step("chain_apply");
    ARCHON_HIP_TRY(hipMemcpyAsync(rd + mail::kRdSettled, settled, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_HIP_TRY(hipMemcpyAsync(rd + mail::kRdBreaks, d_lastbrk + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    z.breaks = rd[mail::kRdBreaks];
    if (f.brk_ready && p == f.period_hint) launches_miscounted(4);     // k_period_breaks and its scan, launched and counted by Fwd::period, were counted here again
    const uint32_t done = rd[mail::kRdSettled];
    if (done >= m) {
        m = 0;                          // every tied row was settled: nothing to count or compact
    } else if (done != 0 || !lists_ready) {
        lists_ready = false;
        keep_ready = true;
        // the tied set again, without the settled groups
        ARCHON_TRY(f.recount_tied());
        ARCHON_HIP_TRY(hipMemcpyAsync(rd + mail::kRdTotal, B.small + fwd_small::kTotal, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        ARCHON_SYNC(s);
        m = rd[mail::kRdTotal];
    }
    tr.step("keep + scan again");
    st.period = p;
    st.chain_items = done;
    if (m) z.period = p;                // what is left straddles defects of the period: one break-distance round once h >= p
    return ARCHON_OK;
}

// The lists of the rounds: those of k_first_groups while they still describe the tied set; otherwise -- the run shortcut
// changed the set, or the set was only counted -- all of it as triples, then split into the lists (k_classify: short groups
// to S, the others stay in row order).
int General::build_lists()
{
    FwdBuf &B = f.B;
    hipStream_t s = f.s;
    uint32_t init[fwd::kMcWords] = {};          // the mid lists start empty, their items from the top of the buffers downwards
    init[fwd::kMcTop] = init[fwd::kMcTop + 1] = f.n;
    memcpy(f.c->h_mail + mail::kRoundsInit.at, init, sizeof init);     // (words of their own: mail::kRounds takes the rounds' counters)
    ARCHON_HIP_TRY(hipMemcpyAsync(B.mc, f.c->h_mail + mail::kRoundsInit.at, sizeof init, hipMemcpyHostToDevice, s));
    if (!m) return ARCHON_OK;
    if (lists_ready) {
        R.ms = ms_first;
        R.mb = mb_first;
        R.bgroups = groups_first;
        return ARCHON_OK;
    }
    if (!keep_ready) ARCHON_TRY(f.recount_tied());
    ARCHON_LAUNCH(fwd::k_compact_first, dim3(div_up(f.n, 256)), dim3(256), 0, s, B.keep, B.dst, B.v, f.sa, f.n, B.upos[0], B.ug[0], B.uitem[0]);
    const uint32_t tiles = div_up(m, fwd::kClT);
    uint32_t *d_cnt = f.cnt(), *rd = f.rd() + mail::kRdCnt;
    ARCHON_HIP_TRY(hipMemsetAsync(d_cnt, 0, 4 * sizeof(uint32_t), s));
    ARCHON_TRY(f.reset_lookback(tiles));
    ARCHON_LAUNCH(fwd::k_classify, dim3(tiles), dim3(fwd::kFuLanes), 0, s, B.upos[0], B.ug[0], B.uitem[0], m, B.slist[R.cs], d_cnt + fwd_small::kCntS,
                   B.upos[1], B.ug[1], B.uitem[1], d_cnt + fwd_small::kCntB, f.fg_status(), B.sc.d_ticket, B.sc.d_err);
    ARCHON_HIP_TRY(hipGetLastError());
    ARCHON_HIP_TRY(hipMemcpyAsync(rd, d_cnt, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    R.ms = rd[fwd_small::kCntS];
    R.mb = rd[fwd_small::kCntB];
    R.bgroups = R.mb / (fwd::kFuMax + 1u) + 2u;          // every group left in B is longer than kFuMax
    R.cur = 1;
    if (R.ms + R.mb != m) { set_error("classification lost entries (%u + %u of %u)", R.ms, R.mb, m); return ARCHON_E_INTERNAL; }
    tr.step("classify");
    return ARCHON_OK;
}

// Text rounds: while few items are tied, key them on the next four bytes of the text instead of on ranks -- no
// inverse suffix array yet (filling it costs more than a whole round on a small set).  They stop as soon as a round
// fails to halve the set (long repeats: doubling is what resolves those).
int General::text_rounds()
{
    while (m && !route_off(kRtNoTextRounds) && !f.deep_ties && (uint64_t)m * 4 <= f.n && st.text_rounds < 4 && h < f.n) {
        st.unresolved_total += m;
        ++st.text_rounds;
        tr.step("before text round");
        ARCHON_TRY(R.round(1, h));
        tr.step("text round");
        h += 4;
        const uint32_t m2 = R.tied();
        const bool productive = (uint64_t)m2 * 2 <= m;
        m = m2;
        if (!productive) break;
    }
    return ARCHON_OK;
}

// Ranks are needed only now: rank[sa[i]] = first row of the group of row i, for every row -- dealt by item into windows of
// the table (rank_writer.hiph) instead of n random stores when the block is large enough for the writer.
int General::fill_rank_table()
{
    if (!m) return ARCHON_OK;
    FwdBuf &B = f.B;
    tr.step("before scatter_rank");
    if (R.writer_ok) {
        ARCHON_TRY(f.writer_regions(B.keyA));           // (the first stage's pairs / records are dead)
        ARCHON_LAUNCH(HIP_KERNEL_NAME(rw::k_part<1, 1>), dim3(div_up(f.n, rw::kTile)), dim3(rw::kLanes), 0, f.s, nullptr, nullptr, f.n, f.sa, B.v, nullptr, B.rwb.r1, B.rwb.cnt1);
        ARCHON_TRY(rw::write_back(f.s, B.rwb, f.n, B.rank));
    } else {
        ARCHON_LAUNCH(fwd::k_scatter_rank, dim3(div_up(f.n, 256)), dim3(256), 0, f.s, f.sa, B.v, f.n, B.rank);
    }
    tr.step("scatter_rank");
    return ARCHON_OK;
}

// Period defects, long groups, before the groups are tied over a whole period (a periodic block enters with h = 3):
// certify the groups whose members share a whole period (k_zone_certify) and run the break rounds on those alone --
// unless the defects are so many that the byte-by-byte comparisons of the certification would cost more than the rounds.
int General::certified_break_rounds()
{
    if (!(m && R.mb && z.period && h < z.period && (uint64_t)z.breaks * z.period * z.period <= 8ull * f.n && !route_off(kRtNoBreakRound))) return ARCHON_OK;
    FwdBuf &B = f.B;
    uint8_t *cert = reinterpret_cast<uint8_t *>(B.pairw);                // (2n bytes, idle until a doubling round lists pairs; the rank log takes the mid kernels' updates)
    uint32_t *okey = B.keep;                                             // (idle until a doubling round lists pairs)
    ARCHON_HIP_TRY(hipMemsetAsync(cert, 0, f.n, f.s));
    ARCHON_HIP_TRY(hipMemsetAsync(okey, 0, (size_t)f.n * sizeof(uint32_t), f.s));
    ARCHON_LAUNCH(fwd::k_zone_certify, dim3(div_up(f.n, 256)), dim3(256), 0, f.s, B.rank, f.sa, B.brk, f.d_x, f.n, z.period, cert, okey);
    ARCHON_HIP_TRY(hipGetLastError());
    tr.step("zone certify");
    for (bool distance = true;; distance = false) {
        st.unresolved_total += R.mb + R.mm;
        ++st.break_rounds;
        const uint32_t before = R.tied();
        ARCHON_TRY(R.round(distance ? 2 : 3, z.period, true, cert, okey));
        const uint32_t settled = before - R.tied();
        st.break_settled += settled;
        m = R.tied();
        tr.step(distance ? "break round on certified groups (distance)" : "break round on certified groups (continuation)");
        if (!(R.mb + R.mm) || (!distance && !settled)) break;
    }
    return ARCHON_OK;
}

// Groups that straddle defects of the period: once every group is tied over a whole period, one round keyed on the
// distance to the last defect settles them, bar the items that share that distance and the side they leave on; those
// follow from the rank of the item their key continues as -- a round that is repeated while it settles something
// (the continuation items may have been settled by the round before) and tried again behind every doubling round
// until it has failed twice in a row.  h stays: what these rounds leave tied is still tied over h symbols.
int General::break_rounds()
{
    for (;;) {
        st.unresolved_total += m;
        ++st.break_rounds;
        const bool distance = z.first;
        ARCHON_TRY(tr.begin(R));
        ARCHON_TRY(R.round(distance ? 2 : 3, z.period));
        tr.break_round(distance, z.period, h, R);
        const uint32_t settled = m - R.tied();
        st.break_settled += settled;
        m = R.tied();
        z.first = false;
        if (!m) break;
        if (!distance) {
            if (settled) z.fail = 0;
            else { ++z.fail; break; }
        }
    }
    return ARCHON_OK;
}

// Doubling rounds until nothing is tied, the period-defect rounds in front of each while they are worth trying.
int General::rounds_to_the_end()
{
    while (m) {
        if (z.period && h >= z.period && z.fail < 2 && !route_off(kRtNoBreakRound)) {
            ARCHON_TRY(break_rounds());
            if (!m) break;
        }
        st.unresolved_total += m;
        ++st.doubling_rounds;
        ARCHON_TRY(tr.begin(R));
        ARCHON_TRY(R.round(0, h));
        tr.doubling_round(h, R);
        m = R.tied();
        if (h > f.n && m) {   // h >= n resolves everything; reaching here means an internal fault
            set_error("doubling did not converge (m=%u at h=%u)", m, h);
            return ARCHON_E_INTERNAL;
        }
        h = h > 0x40000000u ? 0x80000000u : h * 2;
    }
    return ARCHON_OK;
}

// ---- the forward driver: its steps (Fwd), then forward_run, which takes them in order

#ifdef ARCHON_EXPERIMENTS
// host-side phases of a call (experiments library, ARCHON_TRACE_HOST): entry, first launch issued, everything queued, wait over, statistics read
static thread_local std::chrono::steady_clock::time_point t_host[5];
void Fwd::stamp(int i) { if (trace_host) t_host[i] = std::chrono::steady_clock::now(); }
#else
void Fwd::stamp(int) {}
#endif

// The key forms of the streaming stage: Q symbols per key byte (1 = plain bytes; 2 / 4 / 8 = a compacted alphabet), or
// kHotForm -- plain bytes, ranked wave-aggregated for periodic blocks (measured on a^N: passes 0.98 + 1.12 ms against 1.48 + 1.46).
constexpr int kHotForm = 0;
static constexpr int key_q(int form) { return form == kHotForm ? 1 : form; }
// Pass geometry: 1024 lanes x 12 items = tiles of 12 288 items, one workgroup per CU (passes.hiph).
constexpr uint32_t kTileItems = bs::kPassTile;
constexpr uint32_t kPackSigma = 32;          // alphabets up to this many distinct bytes sort on packed keys

// Tier 2, when the block first needs it (a periodic block's break table, the entry sweep of the general stage): rank table,
// lists, logs, directories -- 70 N that a block the streaming stage settles never touches.
int Fwd::general_buffers()
{
    if (B.rank) return ARCHON_OK;
    { Carve count; ARCHON_TRY(ctx_ensure_arena2(c, fwd_tier2(count, B, n))); }
    Carve a2{c->arena2.p, 0, c->arena2.bytes};
    fwd_tier2(a2, B, n);
    if (!a2.ok()) { set_error("arena exhausted (general stage)"); return ARCHON_E_NOMEM; }
    B.rwb.r1 = B.rwb.r2 = nullptr;
    arena_bytes = tier1_bytes + a2.off;
    return ARCHON_OK;
}

// 1. Arena tier 1, the block's prologue (k_prep), the aligned copy of the text, the pass geometry and what the block may try.
int Fwd::setup()
{
#ifdef ARCHON_EXPERIMENTS
    trace_host = depth == 0 && getenv("ARCHON_TRACE_HOST") != nullptr;
#endif
    stamp(0);
    { Carve count; ARCHON_TRY(ctx_ensure_arena(c, fwd_tier1(count, B, n, c->dev, d_sa_user == nullptr))); }
    launches0 = t_launch_count;
    syncs0 = t_sync_count;
    memset(&c->stats, 0, sizeof c->stats);
    c->stats.n = n;

    // tier 1 from the arena's bottom up to the closed-form tail, which lies at a fixed distance from the arena's end
    tail_at = (c->arena.bytes - kClosedTail) & ~size_t(255);
    Carve a1{c->arena.p, 0, tail_at};
    fwd_tier1(a1, B, n, c->dev, d_sa_user == nullptr);
    if (!a1.ok()) { set_error("arena exhausted (tier 1 of a %u-byte block reaches the closed-form tail)", n); return ARCHON_E_NOMEM; }
    tier1_bytes = arena_bytes = a1.off;
    B.sc.d_ticket = B.small + fwd_small::kTicket;
    B.sc.d_err = B.small + fwd_small::kErr;
    B.sc.h_mail = c->h_mail;
    d_base = B.small + fwd_small::kBase;
    d_ctl = reinterpret_cast<bs::TieCtl *>(B.small + fwd_small::kCtl);
    pres = B.small + fwd_small::kProbe;
    // (one launch clears the scratch words, arms the period probe's result word and clears the two-byte count's tables)
    count_zero_bytes = (size_t)(reinterpret_cast<char *>(&B.prep->rowtot[0]) - reinterpret_cast<char *>(B.hist16));
    ARCHON_LAUNCH(bs::k_prep, dim3(256), dim3(256), 0, s, B.small, fwd_small::kWords, fwd_small::kProbe, reinterpret_cast<uint4 *>(B.hist16), (uint32_t)(count_zero_bytes / 16));
    launches_miscounted(-1);        // k_prep was not counted here, where every block launches it, but with each streaming stage (Fwd::streaming)
    static_assert(offsetof(bs::Prep, rowtot) % 16 == 0, "the count's tables end on a 16-byte boundary");
    stamp(1);

    if ((uintptr_t)d_x & 15) {   // kernels want 16-byte aligned text
        ARCHON_HIP_TRY(hipMemcpyAsync(B.xa, d_x, n, hipMemcpyDeviceToDevice, s));
        d_x = B.xa;
    }
    sa = d_sa_user ? d_sa_user : B.sa_own;
    e_start = tm.mark();

    // A2 / bucket setup: the two-byte count (a4 compute(), archon.c:146-161) and its scans.  The count
    // runs over the tile ranges of LSB pass A (R contiguous ranges, one persistent workgroup each), so
    // the same sweep also delivers that pass's per-range digit table.
    const uint32_t ntiles = div_up(n, kTileItems);
    // option "pass_ranges" (archon_hip_set_option): ranges the passes are cut into (default: one per CU).  bench.py asks for 1024 at N > 1
    // (shorter tails while RCCL's kernels hold CUs); tests use odd counts.  Whatever is asked for, a range never
    // exceeds 2^24 items (pass A stages positions relative to its range start in 24 bits).
    R = (uint32_t)kNumCU;
    if (const uint32_t asked = eff_pass_ranges(c->dev)) {
        if (asked > (uint32_t)bs::kMaxRanges) { set_error("pass ranges %u out of range [1, %d]", asked, bs::kMaxRanges); return ARCHON_E_ARG; }
        R = asked;
    }
    if (R > ntiles) R = ntiles;
    tpr = div_up(ntiles, R);
    const uint32_t tpr_max = bs::kRangeMaxItems / kTileItems;
    if (tpr > tpr_max) tpr = tpr_max;
    R = div_up(ntiles, tpr);
    if (R > (uint32_t)bs::kMaxRanges) { set_error("block of %u bytes needs %u pass ranges (max %d)", n, R, bs::kMaxRanges); return ARCHON_E_INTERNAL; }
    // The two-byte count decides the route.  The host does not wait for it: the count leaves a `skip` flag on the
    // device, the whole streaming stage is queued behind it, and its kernels return at once when the flag says
    // "skewed".  One host round trip per block (after k_resolve_ties) instead of two.
    // bucket-per-workgroup pass B (Prep::aligned) needs 256 workgroups and enough tiles per bucket to matter
    const uint32_t aligned_min = g_route.aligned_min >= 0 ? (uint32_t)g_route.aligned_min : (1u << 24);      // (tests lower it to run bucket mode on small blocks)
    allow_aligned = (n >= aligned_min && !route_off(kRtNoAligned) && g_opt[c->dev].pass_b_buckets.load()) ? 1u : 0u;
    // bucket mode moves range-relative records between the passes (passes.hiph: no byte stream beside them)
    // -- where a bucket's segments (one per pass-A range: n / (256 R) places on average) are long enough that a wave's 1024 places
    // nearly always lie inside one: from 4096 places on, i.e. 256 MiB with one range per CU.  Shorter segments make pass B look its
    // records' ranges up one by one: 16 / 64 / 128 MiB blocks measured 0.36 / 0.46 / 0.62 ms in pass B against 0.08 / 0.25 / 0.52.
    const uint32_t rel_min_seg = g_route.rel_min_seg >= 0 ? (uint32_t)g_route.rel_min_seg : 4096u;
    rel_ok = allow_aligned && !route_off(kRtNoRelRecords) && (uint64_t)n >= (uint64_t)R * 256u * rel_min_seg;
    // Clean periodic blocks (periodic.hiph): the period probe and the comparison of the whole text with itself p further down are
    // queued in FRONT of the count -- device-conditional, a block without a voted period pays three empty launches -- and their
    // verdict comes to the host with the block's first round trip; k_rows_scan reads it too and lets the streaming kernels return.
    forced = g_route.force_path;
    closed_ok = depth == 0 && forced < 0 && n >= (1u << 16) && !route_off(kRtNoPeriodProbe) && !route_off(kRtNoChains) && !route_off(kRtNoClosedForm);
    probe = forced < 0 && !route_off(kRtNoProbe);
    // Small blocks (the container's default is 4 MiB, bwt/final/x3/archon.c:100): the streaming stage is built for blocks that fill
    // the chip -- its two-byte count keeps 128 KiB of counters per workgroup on all 256 CUs, its bucket sort launches 65 536
    // workgroups -- and costs 0.7 ms whatever the block holds.  Below kSmallBlock a block takes a plain byte count and the LSB
    // passes, whose cost follows its size.
    const uint32_t small_limit = g_route.small_block >= 0 ? (uint32_t)g_route.small_block : kSmallBlock;
    small_block = forced < 0 && n >= 8 && n < small_limit;
    return ARCHON_OK;
}

// The period probe (k_period_find, k_period_vote) and -- `clean` -- the comparison of the whole text with itself p further down
// (pf::k_period_clean).  The result word was set to "none" and the votes and flags behind it cleared by k_prep.
void Fwd::queue_probe(bool clean)
{
    ARCHON_LAUNCH(fwd::k_period_find, dim3(fwd::kPeriodSearch / 256), dim3(256), 0, s, d_x, n, pres);
    ARCHON_LAUNCH(fwd::k_period_vote, dim3(fwd::kPeriodVotes / 256), dim3(256), 0, s, d_x, n, pres);
    if (clean) ARCHON_LAUNCH(pf::k_period_clean, dim3(kNumCU * 8), dim3(256), 0, s, d_x, n, pres);
    probe_queued = true;
    probe_clean = clean;
}

// the probe's verdict into the mailbox (mail::kProbe), with the round trip that follows
int Fwd::fetch_probe(uint32_t words)
{
    if (probe_queued) ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kProbe.at, pres, words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    probe_fetched = probe_queued;
    return ARCHON_OK;
}

// The verdict has arrived (the wait behind fetch_probe or k_mail is over).  A clean periodic block (periodic.hiph): x[i] == x[i-p]
// for every i >= p (k_period_clean compared all of it), p minimal (the smallest distance at which the block's middle window
// recurs: a smaller period would recur there too), n >= 16 p -- it is written down in closed form.
void Fwd::probe_arrived()
{
    const uint32_t *h_probe = c->h_mail + mail::kProbe.at;
    if (closed_ok && probe_fetched && h_probe[0] != 0xFFFFFFFFu && h_probe[3] == 1u && h_probe[2] == 0u) closed = true;
}

// The block's byte counts (a small block's exact ones, or the two-byte count's column sums) and x[n-1] into the mailbox
int Fwd::fetch_byte_counts(const uint32_t *d_counts)
{
    uint32_t *h_last = c->h_mail + mail::kLastByte.at;
    *h_last = 0;
    ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kByteCounts.at, d_counts, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_HIP_TRY(hipMemcpyAsync(h_last, d_x + (n - 1), 1, hipMemcpyDeviceToHost, s));
    return ARCHON_OK;
}

// The block's byte histogram x[0 .. n-1] out of the mailbox, right after the wait that brought it (mail::kByteCounts lies inside
// the staging rs::sort_pairs overwrites).  The two-byte count's second-byte column sums are the bytes x[0 .. n-2] plus the 0xFF
// in front of x[0]: x[n-1] is added and the pad removed.
void Fwd::take_byte_hist(bool exact)
{
    const uint32_t *h_counts = c->h_mail + mail::kByteCounts.at, last_byte = c->h_mail[mail::kLastByte.at] & 0xFFu;
    for (uint32_t v = 0; v < 256; ++v) hist[v] = exact ? h_counts[v] : h_counts[v] - (v == 0xFFu ? 1u : 0u) + (v == last_byte ? 1u : 0u);
    have_hist = true;
}

// the exact alphabet: 256 presence bits -> sigma, lut (the order-preserving recode)
int Fwd::presence()
{
    ARCHON_LAUNCH(bs::k_presence, dim3(kNumCU * 8), dim3(256), 0, s, d_x, n, B.prep->present);
    const uint32_t *h_present = c->h_mail + mail::kPresence.at;
    ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kPresence.at, B.prep->present, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (!probe_fetched) ARCHON_TRY(fetch_probe());         // (hinted: the period probe's verdict has not travelled yet)
    ARCHON_SYNC(s);
    probe_arrived();
    sigma = 0;
    for (uint32_t v = 0; v < 256; ++v) {
        lut[v] = (uint8_t)sigma;
        if ((h_present[v >> 5] >> (v & 31u)) & 1u) ++sigma;
    }
    presence_done = true;
    return ARCHON_OK;
}

// The two-byte count of src in key form `form` and its scans; k_rows_scan leaves the route's verdict on the device.
// alpha_probe: a workgroup that sees at most 4 distinct bytes gives the count up (Prep::suspect).
int Fwd::count16(int form, const uint8_t *src, bool force_stream, bool alpha_probe)
{
    uint32_t *d_suspect = alpha_probe ? &B.prep->suspect : nullptr;
    if (!count_tables_clear) ARCHON_HIP_TRY(hipMemsetAsync(B.hist16, 0, count_zero_bytes, s));      // (the block's first count finds them cleared by k_prep)
    count_tables_clear = false;
    // the count runs with at most 256 workgroups per half: with more pass ranges each workgroup covers several of
    // them and reads the column sums off between two (more workgroups would only flush their 32 768 bins more often)
    const uint32_t sub = (R > 256u && R % 256u == 0u) ? R / 256u : 1u;
    const uint32_t nparts = div_up(R, sub);
    // B.hist16 (zeroed above) first serves as the spill table of the count, then receives the totals (k_rows_total)
    with_const<kHotForm, 1, 2, 4, 8>(form, [&](auto k) {
        constexpr int F = decltype(k)::value;
        ARCHON_LAUNCH(HIP_KERNEL_NAME(bs::k_hist16<key_q(F), F == kHotForm>), dim3(nparts), dim3(bs::kH16Block), 0, s, src, n, B.h16part, B.hist16,
                       tpr * kTileItems, B.rhist, d_suspect, sub);
    });
    static_assert(bs::kMaxRanges <= 1024, "four ranges per lane in the column half of k_rows_sum_total");
    ARCHON_LAUNCH(bs::k_rows_sum_total, dim3(512), dim3(256), 0, s, B.hist16, B.h16part, nparts, B.prep, (uint32_t)bs::kLsCap, B.rhist, R);
    ARCHON_LAUNCH(bs::k_rows_scan, dim3(256), dim3(256), 0, s, B.hist16, B.prep, force_stream ? 1u : 0u, allow_aligned, d_ctl, (uint32_t)kTieListCap, n,
                   probe_clean ? pres : nullptr);
    ARCHON_HIP_TRY(hipGetLastError());
    e_count = tm.mark();
    return ARCHON_OK;
}

// ---- streaming first stage: two LSB passes + in-LDS bucket sorts; ends with the block's host round trip ----
// (the tie summary was initialised on the device by k_rows_scan, which also left the count summary in it)
int Fwd::streaming(int form, const uint8_t *key_text)
{
    const int q = key_q(form);
    const bool hot = form == kHotForm;      // a periodic block: a few digits per tile, its oversized buckets deferred (k_unpack_big)
    const uint32_t *d_skip = &B.prep->skip;
    uint2 *A_R = reinterpret_cast<uint2 *>(B.keyA);     // pass A out: {K, I} records + the first-key-byte stream
    uint8_t *A_B1 = reinterpret_cast<uint8_t *>(B.valA);
    uint2 *B_R = reinterpret_cast<uint2 *>(B.keyB);     // pass B out
    iA0 = ps.mark();
    // Both record formats of the passes are queued (passes.hiph): the plain one and -- where bucket mode is possible at all -- the
    // range-relative one; which of the two a block takes is the count's choice of pass-B mode (Prep::aligned), known on the device
    // only, and the instantiation that does not match returns at once.
    const uint32_t twin = rel_ok ? 1u : 0u;
    with_const<kHotForm, 1, 2, 4, 8>(form, [&](auto k) {
        constexpr int F = decltype(k)::value;
        auto pass_a = [&](auto rel) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(bs::k_pass_text<bs::kPassBlock, bs::kPassIPT, key_q(F), F == kHotForm, decltype(rel)::value>), dim3(R), dim3(bs::kPassBlock),
                           0, s, d_x, n, tpr, A_R, A_B1, B.prep->startA, B.rhist, key_text, d_skip, B.trash, &d_ctl->base_bucket, twin);
        };
        pass_a(std::false_type{});
        if (rel_ok) pass_a(std::true_type{});
    });
    iA1 = ps.mark();
    // pass B walks the same tile grid in the same ranges; in bucket mode (Prep::aligned) workgroup c takes bucket c
    const uint32_t gridB = (allow_aligned && R < 256u) ? 256u : R;      // bucket mode needs 256; surplus workgroups return at once
    ARCHON_LAUNCH(bs::k_range_hist_text, dim3(R), dim3(bs::kRhBlock), 0, s, A_B1, n, tpr, B.rhist, 0u, kTileItems, d_skip);
    ARCHON_LAUNCH(bs::k_col_prefix, dim3(256), dim3(1024), 0, s, B.rhist, R, d_skip, twin);    // (bucket mode with range-relative records: pass A's table stays)
    iB0 = ps.mark();
    with_const<0, 1>(hot, [&](auto h) {
        auto pass_b = [&](auto rel) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(bs::k_pass_rec<bs::kPassBBlock, bs::kPassBIPT, decltype(h)::value != 0, decltype(rel)::value>), dim3(gridB), dim3(bs::kPassBBlock),
                           0, s, A_R, A_B1, n, tpr, B_R, B.prep->startB, B.rhist, B.prep->startA, d_skip, B.prep->start16, B.trash, twin, B.rhist, R, tpr * kTileItems);
        };
        pass_b(std::false_type{});
        if (rel_ok) pass_b(std::true_type{});
    });
    iB1 = ps.mark();
    e_sorted = tm.mark();
    // (a block of few rows per bucket: the short instance of the bucket sort in front of the general one -- whichever matches the
    //  count's largest bucket runs, the other returns at once)
    const uint32_t avg_rows = n >> 16;
    const uint32_t short_rounds = hot ? 0u : avg_rows <= 400u ? 1u : avg_rows <= 1350u ? 3u : 0u;
    if (short_rounds) {
        with_const<1, 3>((int)short_rounds, [&](auto r) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(bs::k_local_sort<decltype(r)::value>), dim3(65536), dim3(bs::kLsBlock), 0, s, B_R, B.prep->start16, n, sa, d_bwt, d_ctl,
                           B.tie_list, d_skip, 0u, 0u);
        });
    }
    ARCHON_LAUNCH(HIP_KERNEL_NAME(bs::k_local_sort<bs::kLsIPT>), dim3(65536), dim3(bs::kLsBlock), 0, s, B_R, B.prep->start16, n, sa,
                   d_bwt, d_ctl, B.tie_list, d_skip, hot ? 1u : 0u, short_rounds * (uint32_t)bs::kLsBlock);
    if (hot) ARCHON_LAUNCH(bs::k_unpack_big, dim3(div_up(n, bs::kUnpackChunk)), dim3(256), 0, s, B_R, B.prep->start16, n, sa, d_bwt, d_ctl, d_skip);
    e_local = tm.mark();
    ARCHON_LAUNCH(bs::k_resolve_ties, dim3(div_up(kTieListCap, 256)), dim3(256), 0, s, d_x, n, B.tie_list, d_ctl,
                   sa, d_bwt, 5u * (uint32_t)q, 64u * (uint32_t)q, d_skip);
    ARCHON_HIP_TRY(hipGetLastError());
    launches_miscounted(1);         // k_prep of Fwd::setup was counted here: once per streaming stage of the block, never on the other routes
    // (on the chance that this is all the block needs -- the graded case -- the primary index goes to the caller and the
    //  consistency flag to the host with the same round trip: the call then ends without a second one.  Everything the host
    //  reads -- summary, flag, byte counts for skewed blocks, the period probe -- is written into the pinned mailbox by k_mail.)
    e_first = tm.mark();
    ARCHON_LAUNCH(bs::k_mail, dim3(1), dim3(256), 0, s, d_ctl, B.sc.d_err, q == 1 ? B.prep->cntA : nullptr, d_x + (n - 1),
                   probe_clean ? pres : nullptr, c->h_mail_dev, d_base_out, ++c->mail_seq);
    ARCHON_HIP_TRY(hipGetLastError());
    probe_fetched = probe_clean;
    stamp(2);
    // the host's one wait of the block: spin on the sequence word k_mail writes last (pinned, coherent memory); should it not
    // turn up within 50 ms the ordinary wait takes over (and reports whatever went wrong on the stream)
    {
        ++t_sync_count;
        volatile uint32_t *seqw = c->h_mail + bs::kMailSeq;         // (clear of every region of the mailbox: common.hiph)
        const uint32_t want = c->mail_seq;
        const auto t_spin = std::chrono::steady_clock::now();
        for (uint32_t spins = 0; *seqw != want; ++spins) {
            __builtin_ia32_pause();
            if ((spins & 0xFFFu) == 0xFFFu && std::chrono::steady_clock::now() - t_spin > std::chrono::milliseconds(50)) {
                ARCHON_HIP_TRY(hipStreamSynchronize(s));
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    stamp(3);
    memcpy(&ctl, c->h_mail + mail::kSummary.at, sizeof ctl);
    big_items = ctl.big_items;
    if (ctl.fault) { set_error("tie list names rows outside the block (device flag 0x%x)", ctl.fault); return ARCHON_E_INTERNAL; }
    if (q == 1) take_byte_hist(false);          // (used only by skewed blocks)
    probe_arrived();
    return ARCHON_OK;
}

// 2. The first look at the block: a small block's byte count; a big block's probe, two-byte count and streaming stage -- or
// its alphabet first, when the context's last block suggests it.
int Fwd::first_look()
{
    if (small_block) {
        uint32_t *d_counts = B.small + fwd_small::kCounts;
        ARCHON_TRY(launch_hist256(s, d_x, n, d_counts, n));
        e_count = tm.mark();
        ARCHON_TRY(fetch_byte_counts(d_counts));
        // (a small block's time is its host round trips: the period probe and the block's last bytes -- what the LSB passes' digit
        //  counts need -- travel with the byte count instead of taking one each further down)
        ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kTail.at, d_x + (n - 8), 8, hipMemcpyDeviceToHost, s));
        tail_fetched = true;
        if (n >= (1u << 16) && !route_off(kRtNoPeriodProbe)) {
            queue_probe(closed_ok);
            ARCHON_TRY(fetch_probe());
        }
        ARCHON_SYNC(s);
        take_byte_hist(true);
        probe_arrived();
        return ARCHON_OK;
    }
    if (closed_ok) queue_probe(true);
    if (probe && c->hint_poor_alphabet) {
        // The last block of this context had at most 4 distinct bytes (DNA after DNA: BASELINE.json configs[3]), and its first
        // attempt -- a count that gives up at once, the streaming stage queued behind it returning kernel by kernel, a round
        // trip -- cost 160 us for nothing.  This one shows its alphabet first; with more than 4 distinct bytes it takes the
        // ordinary first attempt after all, with 4 or fewer it goes where the count's probe would have sent it.
        ARCHON_TRY(presence());
        if (closed) return ARCHON_OK;
        if (sigma <= 4) {
            ctl.suspect = 1;
            return ARCHON_OK;
        }
    }
    // a big block's first attempt: two-byte count (with the alphabet probe) and the streaming stage behind it
    ARCHON_TRY(count16(1, d_x, forced == 1, probe));
    if (forced == 0) {          // (tests: the 7-pass route needs the count on the host before going on)
        ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kBigItems.at, &B.prep->big_items, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        ARCHON_TRY(fetch_byte_counts(B.prep->cntA));
        ARCHON_SYNC(s);
        big_items = c->h_mail[mail::kBigItems.at];
        take_byte_hist(false);
        return ARCHON_OK;
    }
    ARCHON_TRY(streaming(1, d_x));
    path = (forced == 1 || (uint64_t)big_items * 2 <= n) ? Path::kStream : Path::kSevenPass;
    return ARCHON_OK;
}

static int forward_run(Ctx *c, hipStream_t s, const uint8_t *d_x_in, uint32_t n, uint32_t *d_sa_user, uint8_t *d_bwt, uint32_t *d_base_out, int depth);

// 3. A clean periodic block: sort its first 2p bytes -- the ordinary transform, nested -- and expand their suffix array.
int Fwd::closed_form()
{
    const uint32_t p = c->h_mail[mail::kProbe.at], m2 = 2u * p;
    Carve t{c->arena.p + tail_at, 0, kClosedTail};
    uint32_t *sa2 = t.take<uint32_t>(m2);
    uint32_t *off = t.take<uint32_t>(m2 + 1);
    uint8_t *bwt2 = t.take<uint8_t>(m2);
    uint32_t *base2 = t.take<uint32_t>(64);
    if (!base2 || (uint64_t)p * pf::kMinPeriods + 64u > n) {
        set_error("closed form: period %u of a block of %u bytes does not fit its scratch", p, n);
        return ARCHON_E_INTERNAL;
    }
    // the nested call asks for no more than the arena holds: it neither grows nor frees it, and its tier 1 ends below the tail
    FwdBuf nb{};
    Carve count;
    if (fwd_tier1(count, nb, m2, c->dev, false) > c->arena.bytes) {
        set_error("closed form: tier 1 of the %u-byte block of period %u does not fit below the tail", m2, p);
        return ARCHON_E_INTERNAL;
    }
    const bool x_in_arena = d_x == B.xa;
    ARCHON_TRY(forward_run(c, s, d_x, m2, sa2, bwt2, base2, depth + 1));      // (c->stats, tier 1: the nested call's from here on)
    const uint64_t arena1 = c->stats.arena_bytes;
    // Tier 1 again, for the expansion.  The nested call carved it from the bottom: of the aligned copy of the text (B.xa) only
    // the slot is kept, so that tile_lo lands behind it -- its first 2p + 64 bytes are still the text (the nested block read them
    // in place), the rest was overwritten, and k_expand reads nothing of x but x[0].
    Carve a{c->arena.p, 0, tail_at};
    if (x_in_arena) (void)a.take<uint8_t>((size_t)n + 64);
    const uint32_t ntiles = div_up(n, pf::kTile);
    uint32_t *tile_lo = a.take<uint32_t>((size_t)ntiles + 2);
    if (!tile_lo) { set_error("arena exhausted (closed form)"); return ARCHON_E_NOMEM; }
    ARCHON_LAUNCH(pf::k_offsets, dim3(1), dim3(1024), 0, s, sa2, m2, p, n, off);
    ARCHON_LAUNCH(pf::k_tiles, dim3(div_up(ntiles + 1, 256)), dim3(256), 0, s, off, m2, ntiles, tile_lo);
    ARCHON_LAUNCH(pf::k_expand, dim3(ntiles), dim3(256), 0, s, off, sa2, bwt2, tile_lo, m2, p, n, d_x, d_sa_user, d_bwt, d_base_out);
    ARCHON_HIP_TRY(hipGetLastError());
    e_sorted = e_end = tm.mark();
    uint32_t *rd = c->h_mail + mail::kRead.at;
    ARCHON_HIP_TRY(hipMemcpyAsync(rd, off + m2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    if (rd[0] != n) { set_error("closed form: the classes of period %u hold %u rows of %u", p, rd[0], n); return ARCHON_E_INTERNAL; }
    path = Path::kClosed;
    closed_period = p;
    arena_bytes = arena1 > a.off ? arena1 : a.off;
    if (depth == 0) c->hint_poor_alphabet = true;      // (periodic after periodic: the probe's verdict before any count)
    return ARCHON_OK;
}

// 4. A workgroup of the count saw at most 4 distinct bytes and the count was abandoned (k_hist16): get the exact
// alphabet from a presence map; a block that only LOOKED poor is counted again without the probe
int Fwd::alphabet()
{
    if (probe && ctl.suspect) {
        if (!presence_done) ARCHON_TRY(presence());
        if (sigma <= 16 && !route_off(kRtNoPack)) {
            have_lut = true;
            path = Path::kSevenPass;
        } else {
            sigma = 0;
            ctl.suspect = 0;
            ARCHON_TRY(count16(1, d_x, false, false));
            ARCHON_TRY(streaming(1, d_x));
            path = ((uint64_t)big_items * 2 <= n) ? Path::kStream : Path::kSevenPass;
        }
    } else {
        sigma = 0;
    }
    if (probe && !small_block) c->hint_poor_alphabet = have_lut && sigma <= 4;      // (what the next block of this context looks at first)
    return ARCHON_OK;
}

// 4. A periodic block (aaa..., abab..., a motif repeated: BASELINE.json configs[2]) needs no deep first stage: the run
// shortcut of general_stage settles its chains whatever depth the first stage reached.  So it takes the streaming
// passes after all -- two key bytes, its oversized buckets handed on as groups tied at depth 2 (k_unpack_big) --
// or, with that route switched off, three key bytes of the 7-pass sort.
int Fwd::period()
{
    if (path == Path::kSevenPass && n >= (1u << 16) && !route_off(kRtNoPeriodProbe)) {
        if (!probe_queued) {        // (k_prep armed the result word, and no kernel has been handed it since)
            queue_probe(false);
            ARCHON_TRY(fetch_probe(2));              // the period and its votes
            ARCHON_SYNC(s);
        }
        const uint32_t *h_probe = c->h_mail + mail::kProbe.at;
        if (h_probe[0] != 0xFFFFFFFFu && h_probe[1] * 10 >= fwd::kPeriodVotes * 9) {
            key_bytes = 3;
            // ... provided every two-byte bucket is ONE run of the period: a bucket that joins two phases of the period (the same
            // two bytes at two places of the motif) is no run, and sorting it out at depth 2 costs more than a third key
            // byte.  The two-byte count tells: a single run holds n / p items.  (Periods 1 and 2 cannot collide.)
            const uint32_t pp = h_probe[0];
            if (!route_off(kRtNoPeriodHint)) period_hint = pp;     // the run shortcut need not sample neighbour gaps for it
            const bool count_ok = forced < 0 && !ctl.suspect;
            const bool single_runs = pp <= 2 || (count_ok && (uint64_t)ctl.max_bucket * 2 * pp <= (uint64_t)n * 3);
            if (forced < 0 && single_runs && !small_block && !route_off(kRtNoPeriodStream)) {
                period_hint = pp;               // (the streaming passes keep no order inside a bucket: gap sampling would not work)
                ARCHON_TRY(count16(kHotForm, d_x, true, false));
                ARCHON_TRY(streaming(kHotForm, d_x));
                path = Path::kStream;
            }
        }
    }
    // A block with a period: where does the text break it?  (The table serves the run shortcut; a block WITH breaks skips the
    // shortcut -- its groups straddle the defects -- gets its tied rows listed by the entry sweep and goes to the
    // period-defect rounds.)
    if (!period_hint || route_off(kRtNoChains)) return ARCHON_OK;
    ARCHON_TRY(general_buffers());
    uint32_t *d_lastbrk = B.small + fwd_small::kLastBrk;
    ARCHON_HIP_TRY(hipMemsetAsync(d_lastbrk, 0, 2 * sizeof(uint32_t), s));          // [0] last real break, [1] how many
    ARCHON_LAUNCH(fwd::k_period_breaks, dim3(div_up(div_up(n, 4), 256)), dim3(256), 0, s, d_x, n, period_hint, B.brk, d_lastbrk);
    ARCHON_TRY(launch_scan<1>(s, B.brk, B.brk, n, B.scan_tmp, nullptr));
    uint32_t *rd = c->h_mail + mail::kRead.at;
    ARCHON_HIP_TRY(hipMemcpyAsync(rd + 2, d_lastbrk + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    brk_ready = true;
    period_breaks = route_off(kRtNoBreakRound) ? 0u : rd[2];
    return ARCHON_OK;
}

// 5. Heavily skewed at two bytes.  Alphabet compaction: with <= 16 distinct bytes a key
// byte holds 2, 4 or 8 symbols; if the two-byte buckets of THAT text are small enough the block still
// takes the streaming stage (DNA: 8 symbols deep after two passes), else the 7-pass sort on packed keys.
int Fwd::recode()
{
    if (path != Path::kSevenPass) return ARCHON_OK;
    if (!have_lut) {
        for (uint32_t v = 0; v < 256; ++v) {
            lut[v] = (uint8_t)sigma;
            if (hist[v]) ++sigma;
        }
    }
    bits = 1;
    while ((1u << bits) < sigma) ++bits;
    // (17 ... 32 distinct bytes -- lower-case prose -- still pack: five bits per symbol, eleven symbols in the seven key bytes instead of
    //  seven; the streaming stage's key text holds whole symbols per byte and stops at 16)
    if (sigma > kPackSigma || route_off(kRtNoPack)) return ARCHON_OK;
    uint8_t *d_lut = reinterpret_cast<uint8_t *>(B.small + fwd_small::kLut);
    static_assert(mail::kLut.len * 4 == sizeof lut, "the recode table's staging");
    memcpy(c->h_mail + mail::kLut.at, lut, 256);
    ARCHON_HIP_TRY(hipMemcpyAsync(d_lut, c->h_mail + mail::kLut.at, 256, hipMemcpyHostToDevice, s));
    if (sigma >= 2 && sigma <= 16 && forced < 0 && !small_block && !route_off(kRtNoPackStream)) {
        const int q = bits == 1 ? 8 : bits == 2 ? 4 : 2;
        with_const<8, 4, 2>(q, [&](auto k) {
            ARCHON_LAUNCH(HIP_KERNEL_NAME(bs::k_build_y<decltype(k)::value>), dim3(div_up(div_up(n, 16), 256)), dim3(256), 0, s, d_x, n, d_lut, B.y);
        });
        ARCHON_TRY(count16(q, B.y, false, false));
        ARCHON_TRY(streaming(q, B.y));
        if ((uint64_t)big_items * 2 <= n) {
            path = Path::kStream;
            Q = q;
            alphabet_bits = 8 / q;
        }
    }
    ARCHON_SYNC(s);          // the table upload has left mail::kLut, which the sorts below overwrite
    return ARCHON_OK;
}

// entry of the general stage (k_first_groups): clean SA, group starts and the compacted working set in one sweep
int Fwd::first_groups(int mode, const uint64_t *keys, const uint32_t *items, uint32_t shift)
{
    ARCHON_TRY(general_buffers());
    unsigned long long *fg_status = reinterpret_cast<unsigned long long *>(B.sc.d_status);
    const uint32_t tiles = div_up(n, fwd::kFgTile);
    ARCHON_HIP_TRY(hipMemsetAsync(fg_status, 0, (size_t)tiles * sizeof(unsigned long long), s));
    ARCHON_HIP_TRY(hipMemsetAsync(B.sc.d_ticket, 0, sizeof(uint32_t), s));
    ARCHON_HIP_TRY(hipMemsetAsync(B.small + fwd_small::kFu, 0, 4 * sizeof(uint32_t), s));
    const uint32_t ws_mode = ws_ready ? 2u : 0u;      // 2: the S / B lists of rounds.hiph
    with_const<0, 1>(mode, [&](auto m) {
        ARCHON_LAUNCH(HIP_KERNEL_NAME(fwd::k_first_groups<decltype(m)::value>), dim3(tiles), dim3(256), 0, s, keys, items, shift, n, sa, d_bwt, d_base, B.v,
                       B.upos[0], B.ug[0], B.uitem[0], B.small + fwd_small::kTotal, fg_status, B.sc.d_ticket, B.sc.d_err, ws_mode, B.slist[0],
                       B.small + fwd_small::kFu, (uint32_t)fwd::kFuMax);
    });
    ARCHON_HIP_TRY(hipGetLastError());
    return ARCHON_OK;
}

// ---- first stage for heavily skewed blocks: LSB passes on packed 7-byte keys ----
// alphabet compaction: with <= 16 distinct bytes the key holds 56/bits symbols
int Fwd::seven_pass()
{
    const bool packed = sigma <= kPackSigma && !route_off(kRtNoPack);
    static thread_local uint32_t hist_given[8 * 256];
    bool use_given = false, shallow = false;
    if (packed) {
        h0 = 56 / bits;
        ARCHON_HIP_TRY(hipMemsetAsync(B.sc.d_ghist, 0, 8 * 256 * sizeof(uint32_t), s));
        const uint32_t want = div_up(div_up(n, 4), 256), cap = (uint32_t)kNumCU * 8;
        ARCHON_LAUNCH(fwd::k_init_keys_packed, dim3(want < cap ? want : cap), dim3(256), 0, s, d_x, n, reinterpret_cast<const uint8_t *>(B.small + fwd_small::kLut),
                       bits, h0, B.keyA, B.valA, B.sc.d_ghist);        // (... and the digit counts of the passes)
        alphabet_bits = bits;
        h0 = (8 * key_bytes) / bits;            // symbols the sorted key bytes hold
    } else {
        h0 = key_bytes;
        if (have_hist && n >= 8) {
            // Digit histograms without a sweep over the keys: key byte q (q = 1 is the top byte) of item s is x[s-q], or
            // 0xFF where s < q; over s = 1..n that is the byte histogram of x[0 .. n-q] plus q-1 pads.  The byte histogram
            // of x came with the first look (take_byte_hist); the last bytes of x are fetched here.
            // How many key bytes?  Were the bytes independent, an item would share its first d bytes with n * (sum p^2)^d others: a
            // block whose byte counts say "fewer than one in 32" at d < 7 (incompressible data: 4 bytes for 4 MiB) sorts on d bytes --
            // 38 us per pass saved on a 4 MiB block -- and what stays tied goes to the rounds at depth d like any other tie.  Text
            // (sum p^2 about 1/15) keeps its seven bytes -- its bytes are far from independent, so anything above 1/128 does.  An
            // estimate only: the order never depends on it.
            if (key_bytes == fwd::kKeyBytes && period_hint == 0 && !route_off(kRtNoShallow)) {
                double s2 = 0.0;
                for (uint32_t v = 0; v < 256; ++v) s2 += ((double)hist[v] / n) * ((double)hist[v] / n);
                double e = (double)n;
                for (uint32_t d = 1; d < fwd::kKeyBytes && s2 * 128.0 <= 1.0; ++d) {     // (nearly flat counts only: text is far from independent)
                    e *= s2;
                    if (d >= 3 && e * 32.0 <= 1.0) { key_bytes = d; shallow = true; break; }
                }
                h0 = key_bytes;
            }
            if (g_route.key_bytes >= 3 && g_route.key_bytes < (int)fwd::kKeyBytes && key_bytes == fwd::kKeyBytes && period_hint == 0) {
                key_bytes = (uint32_t)g_route.key_bytes;       // (tests / experiments: the order never depends on the depth)
                shallow = true;
                h0 = key_bytes;
            }
            if (!tail_fetched) {
                ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kTail.at, d_x + (n - 8), 8, hipMemcpyDeviceToHost, s));
                ARCHON_SYNC(s);
            }
            const uint8_t *tail = reinterpret_cast<const uint8_t *>(c->h_mail + mail::kTail.at);      // x[n-8 .. n-1]
            for (uint32_t q = 1; q <= 7; ++q) {
                uint32_t *hq = hist_given + (8 - q) * 256;                               // pass p = 8 - q sorts on key byte q
                memcpy(hq, hist, sizeof hist);
                for (uint32_t j = n - q + 1; j < n; ++j) --hq[tail[j - (n - 8)]];        // bytes past x[n-q] are no digit of depth q
                hq[0xFF] += q - 1;
            }
            use_given = true;
        }
    }
    ARCHON_HIP_TRY(hipGetLastError());
    bool in_b = false;
    const uint32_t pass_mask = (0xFFu << (8 - key_bytes)) & 0xFEu;          // the top key_bytes bytes; byte 0 is payload
    // (plain bytes with the histograms in hand: the first pass that runs makes the pairs from the text itself)
    const bool from_text = !packed && use_given;
    if (!packed && !from_text)
        ARCHON_LAUNCH(fwd::k_init_keys, dim3(div_up(div_up(n, 4), 256)), dim3(256), 0, s, d_x, n, B.keyA, B.valA);
    ARCHON_TRY(rs::sort_pairs(s, B.sc, B.keyA, B.valA, B.keyB, B.valB, n, pass_mask, &in_b, &radix_passes, &pt,
                              use_given ? hist_given : nullptr, from_text ? d_x : nullptr, packed));
    if (from_text && radix_passes == 0)          // every digit constant: no pass ran, the pairs still have to exist
        ARCHON_LAUNCH(fwd::k_init_keys, dim3(div_up(div_up(n, 4), 256)), dim3(256), 0, s, d_x, n, B.keyA, B.valA);
    // the kernel that makes the keys, k_init_keys or k_init_keys_packed, was counted twice -- also where the first pass makes them
    // from the text and neither runs
    launches_miscounted(from_text && radix_passes != 0 ? 2 : 1);
    e_sorted = e_first = tm.mark();
    ws_ready = key_bytes == fwd::kKeyBytes || period_breaks != 0 || shallow;     // a clean periodic block: the run shortcut will empty the working set
    return first_groups(0, in_b ? B.keyB : B.keyA, in_b ? B.valB : B.valA, 8u * (8u - key_bytes));
}

// 6. The first stage: the 7-pass sort, or what the streaming stage left -- nothing, or tied rows for the general stage
int Fwd::first_stage()
{
    if (path == Path::kSevenPass) return seven_pass();
    if (ctl.unresolved == 0 && ctl.tie_groups <= kTieListCap) {
        if (ctl.base_id >= n) { set_error("primary index not found"); return ARCHON_E_INTERNAL; }
        stream_done = true;                 // (the primary index and the consistency flag came with the summary)
        return ARCHON_OK;
    }
    h0 = (ctl.min_depth < 5 ? ctl.min_depth : 5) * (uint32_t)Q;     // key bytes -> symbols
    ws_ready = period_hint == 0 || period_breaks != 0;
    ARCHON_TRY(first_groups(1, nullptr, nullptr, 0));
    ARCHON_HIP_TRY(hipMemcpyAsync(d_base, &d_ctl->base_id, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return ARCHON_OK;
}

// 7. The general stage, for whatever the first stage left tied
int Fwd::tied_rows()
{
    if (stream_done) return ARCHON_OK;
    // deep ties: the streaming stage compared the tied groups 64 symbols deep and a good part of the block still agrees
    // (when the tie list overflowed only a sample of it was compared -- bs::kTieSample groups: they stand for the rest)
    const bool listed_all = ctl.tie_groups <= kTieListCap;
    deep_ties = path == Path::kStream && big_items == 0 && ctl.min_depth >= 5 && !route_off(kRtNoDeepHint) &&
                (listed_all ? (uint64_t)ctl.unresolved * 64 >= n
                            : (uint64_t)ctl.unresolved * 2 >= bs::kTieSample && (uint64_t)ctl.tie_items * 64 >= n);
    ARCHON_TRY(general_stage());
    e_general = tm.mark();
    ARCHON_HIP_TRY(hipMemcpyAsync(d_base_out, d_base, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    return ARCHON_OK;
}

// 8. The device's consistency flag -- it came with the streaming stage's summary, or it is read now -- and the statistics of
// every route (the general stage and the 7-pass sort keep theirs as they go; launches and waits are what the thread's counters
// have gained since setup).  A stage that did not run left its marks at -1, which StageTimer::ms reads as 0.
int Fwd::finish()
{
    archon_hip_stats &st = c->stats;
    if (path == Path::kClosed) {          // (the nested transform of the 2p-byte block left its own statistics here, and read its own flag)
        memset(&st, 0, sizeof st);
        st.n = n;
        st.period = closed_period;
        st.chain_items = n;
    } else {
        uint32_t dev_err;
        if (stream_done) {
            e_end = e_first;
            dev_err = c->h_mail[mail::kFlag.at];
        } else {
            e_end = tm.mark();
            ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kRead.at, B.sc.d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            ARCHON_SYNC(s);
            dev_err = c->h_mail[mail::kRead.at];
        }
        if (dev_err) { set_error("device consistency flag 0x%x (look-back spin bound)", dev_err); return ARCHON_E_INTERNAL; }
    }
    st.path = (uint32_t)path;
    st.arena_bytes = arena_bytes;
    st.alphabet_bits = alphabet_bits;
    st.radix_passes = path == Path::kStream ? 2u : radix_passes;
    st.kernel_launches = t_launch_count - launches0;
    st.host_syncs = t_sync_count - syncs0;
    st.ms_hist = tm.ms(e_start, e_count);
    st.ms_sort = tm.ms(e_count, e_sorted);
    st.ms_doubling = tm.ms(e_first, e_general);
    st.ms_bwt = tm.ms(e_general, e_end);
    st.ms_total = tm.ms(e_start, e_end);
    for (int i = 0; i + 1 < pt.n; i += 2) {      // 7-pass route: rs::sort_pairs brackets each pass
        st.ms_radix_pass_sum += pt.ms(i, i + 1);
        ++st.radix_pass_timed;
    }
    if (path == Path::kStream) {
        st.tie_groups = ctl.tie_groups;
        st.tie_items = ctl.tie_items;
        st.ms_local_sort = tm.ms(e_sorted, e_local);
        st.ms_resolve = tm.ms(e_local, e_first);
        st.ms_pass_text = ps.ms(iA0, iA1);
        st.ms_pass_rec = ps.ms(iB0, iB1);
        st.ms_radix_pass_sum = st.ms_pass_text + st.ms_pass_rec;
        st.radix_pass_timed = 2;
    }
    return ARCHON_OK;
}

// One forward transform.  depth: 0 = a caller's block, 1 = the 2p-byte block of a clean periodic block's closed form
// (periodic.hiph): its own event banks, no closed form of its own
static int forward_run(Ctx *c, hipStream_t s, const uint8_t *d_x_in, uint32_t n, uint32_t *d_sa_user, uint8_t *d_bwt, uint32_t *d_base_out, int depth = 0)
{
    Fwd f{c, s, n, depth, d_x_in, d_sa_user, d_bwt, d_base_out};
    ARCHON_TRY(f.setup());
    ARCHON_TRY(f.first_look());
    if (f.closed) {
        ARCHON_TRY(f.closed_form());
    } else {
        ARCHON_TRY(f.alphabet());
        ARCHON_TRY(f.period());
        ARCHON_TRY(f.recode());
        ARCHON_TRY(f.first_stage());
        ARCHON_TRY(f.tied_rows());
    }
    ARCHON_TRY(f.finish());
    f.stamp(4);
#ifdef ARCHON_EXPERIMENTS
    if (f.trace_host) {
        auto us = [&](int a, int b) { return std::chrono::duration<double, std::micro>(t_host[b] - t_host[a]).count(); };
        fprintf(stderr, "host phases: entry->first launch %.1f us, queue the rest %.1f us, wait %.1f us, statistics %.1f us (device %.1f us)\n",
                us(0, 1), us(1, 2), us(2, 3), us(3, 4), c->stats.ms_total * 1e3);
    }
#endif
    return ARCHON_OK;
}

}  // namespace archon

// =====================================================================
// C ABI
// =====================================================================
using namespace archon;

extern "C" {

int archon_hip_device_count(void) { return device_count(); }

const char *archon_hip_last_error(void) { return t_err; }

static int check_n(uint32_t n)
{
    if (n < 1 || n > ARCHON_HIP_MAX_N) {
        set_error("block size %u out of range [1, %u]", n, ARCHON_HIP_MAX_N);
        return ARCHON_E_ARG;
    }
    return ARCHON_OK;
}

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

// ---- the repeats of a block (repeats.hiph: the kernels and their drivers; here the argument checks and the statistics)
static int rep_check(const void *lcp, const void *bwt, const void *total, uint32_t n, uint32_t base_id, uint32_t kind)
{
    if (!lcp || !bwt || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    if (base_id >= n) { set_error("primary row %u out of range [0, %u)", base_id, n); return ARCHON_E_ARG; }
    return rep_check_kind(kind);
}

int archon_hip_repeats_dev(const uint32_t *d_lcp, const uint8_t *d_bwt, uint32_t n, uint32_t base_id, uint32_t kind, uint32_t min_len, uint32_t min_occ,
                           archon_hip_repeat *d_out_or_null, uint64_t cap, uint64_t *total, int dev, void *stream)
{
    ARCHON_TRY(rep_check(d_lcp, d_bwt, total, n, base_id, kind));
    *total = 0;
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_repeat_stats> keep(t_rep_stats, dev);
        rep_call_stats(&keep.st, n, kind, min_len, min_occ);
        RepCall q = {d_lcp, d_bwt, n, base_id, kind, min_len, min_occ};
        return rep_dev(c, s, q, d_out_or_null, cap, total, &keep.st);
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
        return rep_to_host(c, s, q, out_or_null, cap, total, &keep.st);
    });
}

int archon_hip_get_repeat_stats(int dev, archon_hip_repeat_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_rep_stats.get(dev, out, "repeats call");
}

// ---- longest previous factors and the LZ77 parse (lz.hiph: the kernels and their drivers; here the argument checks and the statistics)
static int lpf_check(const void *sa, const void *lcp, const void *lpf, uint32_t n, uint32_t dir)
{
    if (!sa || !lcp || !lpf) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return lz_check_dir(dir);
}

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

// *total is written whenever it is given: 0 before any refusal (the cap rule's "always written")
static int parse_check(const void *lpf, uint64_t *total, uint32_t n)
{
    if (total) *total = 0;
    if (!lpf || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    return check_n(n);
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
        return parse_dev(c, s, tm, q, d_out_or_null, cap, total, &keep.st);
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
        return parse_to_host(c, s, tm, q, out_or_null, cap, total, &keep.st);
    });
}

int archon_hip_get_lz_stats(int dev, archon_hip_lz_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_lz_stats.get(dev, out, "LZ call");
}

// ---- k-mers, per-position counts and shortest unique substrings (kmers.hiph: the kernels and their drivers; here the argument
// checks and the statistics).  *total is written whenever it is given: 0 before any refusal
static int kmers_check(const void *sa, const void *lcp, uint64_t *total, uint32_t n, uint32_t k, const void *hist, uint32_t bins)
{
    if (total) *total = 0;
    if (!sa || !lcp || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return kmer_check_args(k, hist, bins);
}

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

// sa and lcp of host buffers through staging buffers 0 and 1
static int kmer_stage(Ctx *c, hipStream_t s, const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t **d_sa, uint32_t **d_lcp)
{
    ARCHON_TRY(ctx_io(c, 0, (size_t)n * 4 + 64, (void **)d_sa));
    ARCHON_TRY(ctx_io(c, 1, (size_t)n * 4 + 64, (void **)d_lcp));
    ARCHON_HIP_TRY(hipMemcpyAsync(*d_sa, sa, (size_t)n * 4, hipMemcpyHostToDevice, s));
    ARCHON_HIP_TRY(hipMemcpyAsync(*d_lcp, lcp, (size_t)n * 4, hipMemcpyHostToDevice, s));
    return ARCHON_OK;
}

int archon_hip_kmers(const uint32_t *sa, const uint32_t *lcp, uint32_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ, archon_hip_kmer *out_or_null,
                     uint64_t cap, uint64_t *total, uint32_t *hist_or_null, uint32_t bins, int dev)
{
    ARCHON_TRY(kmers_check(sa, lcp, total, n, k, hist_or_null, bins));
    return with_ctx(dev, nullptr, [&](Ctx *c, hipStream_t s) -> int {
        KeepStats<archon_hip_kmer_stats> keep(t_kmer_stats, dev);
        kmer_call_stats(&keep.st, n, k, min_occ, max_occ, bins, 0);
        uint32_t *d_sa = nullptr, *d_lcp = nullptr;
        ARCHON_TRY(kmer_stage(c, s, sa, lcp, n, &d_sa, &d_lcp));
        KmerCall q = {d_sa, d_lcp, n, k, min_occ, max_occ, bins};
        return kmer_list(c, s, q, out_or_null, cap, total, hist_or_null, true, &keep.st);
    });
}

static int kmer_occ_check(const void *sa, const void *lcp, const void *occ, uint32_t n, uint32_t k)
{
    if (!sa || !lcp || !occ) { set_error("null pointer"); return ARCHON_E_ARG; }
    ARCHON_TRY(check_n(n));
    return kmer_check_args(k, nullptr, 0);
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
        ARCHON_TRY(kmer_stage(c, s, sa, lcp, n, &d_sa, &d_lcp));
        KmerCall q = {d_sa, d_lcp, n, k};
        return kmer_occ_run(c, s, q, occ, true, &keep.st);
    });
}

static int sus_check(const void *sa, const void *lcp, const void *sus, uint32_t n)
{
    if (!sa || !lcp || !sus) { set_error("null pointer"); return ARCHON_E_ARG; }
    return check_n(n);
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
        ARCHON_TRY(kmer_stage(c, s, sa, lcp, n, &d_sa, &d_lcp));
        return kmer_sus_run(c, s, d_sa, d_lcp, n, sus, true, &keep.st);
    });
}

int archon_hip_get_kmer_stats(int dev, archon_hip_kmer_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_kmer_stats.get(dev, out, "k-mer call");
}

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

int archon_hip_get_fm_stats(int dev, archon_hip_fm_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fm_stats.get(dev, out, "FM call");
}

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

int archon_hip_get_fm_walk_stats(int dev, archon_hip_fm_walk_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fmw_stats.get(dev, out, "sampled FM call");
}

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

int archon_hip_get_fm_approx_stats(int dev, archon_hip_fm_approx_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fma_stats.get(dev, out, "approximate FM call");
}

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

int archon_hip_get_fm_class_stats(int dev, archon_hip_fm_class_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fmc_stats.get(dev, out, "class FM call");
}

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

int archon_hip_get_fm_edit_stats(int dev, archon_hip_fm_edit_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fme_stats.get(dev, out, "edit-distance FM call");
}

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

int archon_hip_get_fm_mem_stats(int dev, archon_hip_fm_mem_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fmm_stats.get(dev, out, "SMEM call");
}

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

int archon_hip_get_fm_ms_stats(int dev, archon_hip_fm_ms_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fms_stats.get(dev, out, "matching-statistics call");
}

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

static int fmt_check(const archon_hip_fm *f, const void *text, const void *len, const void *lo, const void *hi)
{
    if (!f || !text || !len) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (!lo != !hi) { set_error("FM ms text: lo and hi are both given or both null"); return ARCHON_E_ARG; }
    return fmt_check_attached(f);
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

// *total is written whenever it is given: 0 before any refusal
static int rlz_check(const archon_hip_fm *f, const void *text, uint64_t *total)
{
    if (total) *total = 0;
    if (!f || !text || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    return fmt_check_attached(f);
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

int archon_hip_get_fm_text_stats(int dev, archon_hip_fm_text_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fmt_stats.get(dev, out, "text call");
}

// ---- documents
// what an attach asks of host bounds before the handle is read, then with it
static int fmd_attach_check(const archon_hip_fm *f, const uint32_t *bounds, uint32_t ndocs)
{
    ARCHON_TRY(fmd_check_bounds(bounds, ndocs));
    if (!f->sa.mem) { set_error("FM attach docs: the handle has no suffix array (archon_hip_fm_attach_sa)"); return ARCHON_E_ARG; }
    return fmd_check_fit(f->n, bounds, ndocs);
}

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

// *total is written whenever it is given: 0 before any refusal
static int fmd_check(const archon_hip_fm *f, const void *a, const void *b, const void *ndocs, uint64_t *total)
{
    if (total) *total = 0;
    if (!f || !a || !b || !ndocs || !total) { set_error("null pointer"); return ARCHON_E_ARG; }
    return ARCHON_OK;
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

static int fmd_doc_of_check(const archon_hip_fm *f, const void *items, uint64_t count, const void *doc)
{
    if (!f || (!items && count) || (!doc && count)) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (count >> 32) { set_error("FM doc of: %llu items in one call", (unsigned long long)count); return ARCHON_E_ARG; }
    return fmd_check_attached(f);
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

int archon_hip_get_fm_doc_stats(int dev, archon_hip_fm_doc_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_fmd_stats.get(dev, out, "documents call");
}

// ---- resident blocks ---------------------------------------------------------------------------------------------------
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
        return rep_to_host(c, s, q, out_or_null, cap, total, &keep.st);
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
        return parse_to_host(c, s, tm, q, out_or_null, cap, total, &keep.st);     // (its count waits for the stream: the records have arrived)
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
extern "C++" {
template <class Stats>
static int block_fm_table_own(Ctx *c, hipStream_t s, archon_hip_block *b, Stats *st)
{
    archon_hip_fm_stats fst = {};
    ARCHON_TRY(block_fm_table(c, s, b, &fst));
    st->built = fst.built;
    st->ms_build = fst.ms_build;
    return ARCHON_OK;
}
}   // extern "C++"

// a handle given beside a block is one of that block's BWT, on its device
static int block_check_handle(const archon_hip_block *b, const archon_hip_fm *f, const char *what)
{
    if (f->dev != b->dev || f->n != b->n || f->base != b->base) {
        set_error("%s: the handle (%u bytes, primary row %u) is not of this block (%u bytes, primary row %u)", what, f->n, f->base, b->n, b->base);
        return ARCHON_E_ARG;
    }
    return ARCHON_OK;
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

static int sa_to_bwt_run(Ctx *c, hipStream_t s, const uint8_t *d_x, uint32_t n, const uint32_t *d_sa, uint8_t *d_bwt,
                         uint32_t *d_base_out)
{
    uint32_t *res = c->d_mail() + mail::kDevSaRes.at;      // [0] bad value seen, [1] rows holding n, [2] the primary index
    uint32_t *rd = c->h_mail + mail::kRead.at;
    ARCHON_HIP_TRY(hipMemsetAsync(res, 0, 3 * sizeof(uint32_t), s));
    ARCHON_LAUNCH(fwd::k_sa_to_bwt, dim3(div_up(div_up(n, 4), 256)), dim3(256), 0, s, d_x, d_sa, n, d_bwt, res + 2, res);
    ARCHON_HIP_TRY(hipGetLastError());
    ARCHON_HIP_TRY(hipMemcpyAsync(rd, res, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    if (rd[0] || rd[1] != 1) {
        set_error("not a suffix array in a7 order: %s", rd[0] ? "values outside 1..n" : "no single row holds n");
        return ARCHON_E_CORRUPT;
    }
    ARCHON_HIP_TRY(hipMemcpyAsync(d_base_out, res + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    ARCHON_SYNC(s);
    return ARCHON_OK;
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
static int post_run(Ctx *c, hipStream_t s, const uint8_t *d_bwt, uint32_t n, uint8_t *d_out, size_t *out_bytes)
{
    const uint32_t np = post::pieces_of(n);
    if (np == 0) {                                   // an empty block: u32 pieces = 0
        ARCHON_HIP_TRY(hipMemsetAsync(d_out, 0, 4, s));
        ARCHON_SYNC(s);
        *out_bytes = 4;
        return ARCHON_OK;
    }
    uint8_t *slots;
    uint32_t *sizes;
    ARCHON_TRY(ctx_carve(c, [&](Carve &a) {
        slots = a.take<uint8_t>((size_t)np * post::kSlotBytes);
        sizes = a.take<uint32_t>(np);
        return a.off;
    }));
    unsigned long long *d_total = reinterpret_cast<unsigned long long *>(c->d_mail() + mail::kDevPostTotal.at);
    ARCHON_LAUNCH(post::k_post_piece, dim3(np), dim3(post::kLanes), 0, s, d_bwt, n, slots, sizes);
    ARCHON_LAUNCH(post::k_post_gather, dim3(np), dim3(256), 0, s, slots, sizes, np, d_out, d_total);
    ARCHON_HIP_TRY(hipGetLastError());
    ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kPostTotal.at, d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    unsigned long long total;
    memcpy(&total, c->h_mail + mail::kPostTotal.at, sizeof total);
    if (total < 4 + 4ull * np || total > post::block_bound(n)) { set_error("post stage: stream length %llu out of bounds", total); return ARCHON_E_INTERNAL; }
    *out_bytes = (size_t)total;
    return ARCHON_OK;
}

// stream -> BWT (k_post_offsets, k_post_decode); *n_out = the block's length.  Synchronises the stream.
static int post_decode_run(Ctx *c, hipStream_t s, const uint8_t *d_in, size_t in_bytes, uint8_t *d_bwt, uint32_t cap, uint32_t *n_out)
{
    const size_t np_max = (size_t)cap / post::kPiece + 2;
    unsigned long long *off;
    ARCHON_TRY(ctx_carve(c, [&](Carve &a) { off = a.take<unsigned long long>(np_max + 2); return a.off; }));
    uint32_t *meta = c->d_mail() + mail::kDevPostMeta.at;      // [0] n, [1] pieces, [2] bad
    ARCHON_HIP_TRY(hipMemsetAsync(meta, 0, 3 * sizeof(uint32_t), s));
    ARCHON_LAUNCH(post::k_post_offsets, dim3(1), dim3(1024), 0, s, d_in, (unsigned long long)in_bytes, cap, off, meta, meta + 2);
    ARCHON_LAUNCH(post::k_post_decode, dim3(div_up(np_max, post::kDecWaves)), dim3(64 * post::kDecWaves), 0, s, d_in, off, meta, d_bwt, meta + 2);
    ARCHON_HIP_TRY(hipGetLastError());
    const uint32_t *h_meta = c->h_mail + mail::kPostMeta.at;
    ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kPostMeta.at, meta, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    if (h_meta[2]) { set_error("post stage: malformed stream (flag 0x%x)", h_meta[2]); return ARCHON_E_CORRUPT; }
    *n_out = h_meta[0];
    return ARCHON_OK;
}

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

static int lms_select_run(Ctx *c, hipStream_t s, const uint8_t *d_x, uint32_t n, uint32_t *d_count, uint32_t *d_items, uint32_t *n1_out)
{
    // three word arrays over the items, two (key, value) pair buffers over the LMS half, scan and status words
    uint32_t *v, *flag, *dst, *vA, *vB, *scan_tmp, *small;
    uint64_t *kA, *kB;
    rs::Scratch sc;
    ARCHON_TRY(ctx_carve(c, [&](Carve &a) {
        v = a.take<uint32_t>(n); flag = a.take<uint32_t>(n); dst = a.take<uint32_t>(n);
        kA = a.take<uint64_t>((size_t)n / 2 + 8); kB = a.take<uint64_t>((size_t)n / 2 + 8);
        vA = a.take<uint32_t>((size_t)n / 2 + 8); vB = a.take<uint32_t>((size_t)n / 2 + 8);
        scan_tmp = a.take<uint32_t>(scan_temp_words(n));
        sc.d_status = a.take<uint32_t>(rs::status_words(n));
        sc.d_ghist = a.take<uint32_t>(8 * 256);
        sc.d_gstart = a.take<uint32_t>(8 * 256);
        small = a.take<uint32_t>(inv_small::kWords);
        return a.off;
    }));
    sc.d_ticket = small + inv_small::kTicket; sc.d_err = small + inv_small::kErr; sc.h_mail = c->h_mail;
    uint32_t *d_total = small + inv_small::kTotal, *d_starts = small + inv_small::kStarts;
    ARCHON_HIP_TRY(hipMemsetAsync(small, 0, inv_small::kWords * sizeof(uint32_t), s));
    const uint32_t g256 = div_up(n, 256);
    ARCHON_LAUNCH(fwd::k_lms_pairs, dim3(g256), dim3(256), 0, s, d_x, n, v);
    ARCHON_TRY(launch_scan<1>(s, v, v, n, scan_tmp, nullptr));
    ARCHON_LAUNCH(fwd::k_lms_flag, dim3(g256), dim3(256), 0, s, d_x, n, v, flag);
    ARCHON_TRY(launch_scan<0>(s, flag, dst, n, scan_tmp, d_total));
    ARCHON_HIP_TRY(hipMemcpyAsync(c->h_mail + mail::kRead.at, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ARCHON_SYNC(s);
    const uint32_t n1 = c->h_mail[mail::kRead.at];
    *n1_out = n1;
    ARCHON_HIP_TRY(hipMemsetAsync(d_count, 0, 256 * sizeof(uint32_t), s));
    if (n1 == 1) {
        ARCHON_LAUNCH(fwd::k_lms_compact, dim3(g256), dim3(256), 0, s, d_x, n, flag, dst, kA, vA);
        ARCHON_LAUNCH(fwd::k_lms_single, dim3(1), dim3(1), 0, s, kA, vA, d_count, d_items);
    } else if (n1) {
        ARCHON_LAUNCH(fwd::k_lms_compact, dim3(g256), dim3(256), 0, s, d_x, n, flag, dst, kA, vA);
        bool in_b = false;
        uint32_t passes = 0;
        ARCHON_TRY(rs::sort_pairs(s, sc, kA, vA, kB, vB, n1, 0x01u, &in_b, &passes));
        // (sort_pairs has left the digit histogram of byte 0 = the per-bucket counts in d_ghist[0..255])
        ARCHON_HIP_TRY(hipMemcpyAsync(d_count, sc.d_ghist, 256 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        ARCHON_LAUNCH(k_scan257, dim3(1), dim3(64), 0, s, d_count, d_starts);
        ARCHON_LAUNCH(fwd::k_lms_place, dim3(div_up(n1, 256)), dim3(256), 0, s, in_b ? kB : kA, in_b ? vB : vA, n1, d_starts, d_items);
        ARCHON_HIP_TRY(hipGetLastError());
    }
    ARCHON_SYNC(s);
    return ARCHON_OK;
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
    return with_ctx(dev, stream, [&](Ctx *c, hipStream_t s) -> int {
        uint32_t *d_counts = c->d_mail() + mail::kDevCounts.at, *d_starts = c->d_mail() + mail::kDevStarts.at;
        ARCHON_TRY(launch_hist256(s, d_src, n, d_counts, n));
        ARCHON_LAUNCH(k_scan257, dim3(1), dim3(64), 0, s, d_counts, d_starts);
        uint32_t grid = div_up(n, 256 * 16);
        if (grid < 1) grid = 1;
        if (grid > (uint32_t)kNumCU * 8) grid = kNumCU * 8;
        ARCHON_LAUNCH(k_fill_runs, dim3(grid), dim3(256), 0, s, d_starts, d_dst, n);
        ARCHON_HIP_TRY(hipGetLastError());
        ARCHON_SYNC(s);
        return ARCHON_OK;
    });
}

int archon_hip_radix_scatter(const uint8_t *src, size_t n, uint8_t *dst, int dev)
{
    if (!src || !dst) { set_error("null pointer"); return ARCHON_E_ARG; }
    if (n >= 0xFFFFFFFFull) { set_error("n too large"); return ARCHON_E_ARG; }
    DevBuf a, b;        // (freed on the device the calls below leave current: dev)
    // the context only for the allocations and the upload: the _dev call takes it again
    ARCHON_TRY(with_ctx(dev, nullptr, [&](Ctx *, hipStream_t) -> int {
        ARCHON_TRY(a.alloc(n + 64, "radix scatter"));
        ARCHON_TRY(b.alloc(n + 64, "radix scatter"));
        ARCHON_HIP_TRY(hipMemcpy(a.p, src, n, hipMemcpyHostToDevice));
        return ARCHON_OK;
    }));
    ARCHON_TRY(archon_hip_radix_scatter_dev(reinterpret_cast<const uint8_t *>(a.p), n, reinterpret_cast<uint8_t *>(b.p), dev, nullptr));   // (waits for its stream)
    ARCHON_HIP_TRY(hipMemcpy(dst, b.p, n, hipMemcpyDeviceToHost));
    return ARCHON_OK;
}

// ---- several small blocks per call ---------------------------------------------------------------------------------------
// x3's default block is 4 MiB (bwt/final/x3/archon.c:100,108).  One such block is thirty launches of a few microseconds and
// one or two host round trips: alone on the device it runs at a tenth of the rate of a 256 MiB block.  A batch call deals its
// blocks to `workers` host threads, each bound to a compute context of its own (stream, arena, staging buffers): the
// blocks' kernels, copies and launch gaps overlap.  workers <= 0: chosen from the largest block (8 up to 4 MiB, 4 up to
// 16 MiB, 2 beyond).  Blocks are independent; the first error stops the rest and is returned.
static int batch_workers(const uint32_t *n, uint32_t count, int workers)
{
    uint32_t mx = 0;
    for (uint32_t i = 0; i < count; ++i) mx = n[i] > mx ? n[i] : mx;
    int w = workers > 0 ? workers : (mx <= (4u << 20) ? 8 : mx <= (16u << 20) ? 4 : 2);
    if (w > kCtxPerDev) w = kCtxPerDev;
    if ((uint32_t)w > count) w = (int)count;
    return w < 1 ? 1 : w;
}

extern "C++" {
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
}   // extern "C++"

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
#endif

#ifdef ARCHON_EXPERIMENTS
/* cycle stamps of the middle workgroup of the last k_post_piece launch */
int archon_hip_exp_post_stamps(unsigned long long out[16])
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(post::g_post_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? ARCHON_OK : ARCHON_E_HIP;
}
#endif

#ifdef ARCHON_EXPERIMENTS
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
    static const struct { const char *name; uint32_t bit; } kFlags[] = {
        {"NO_ALIGNED", kRtNoAligned}, {"NO_CHAINS", kRtNoChains}, {"NO_DEEP_HINT", kRtNoDeepHint}, {"NO_PACK", kRtNoPack},
        {"NO_PACK_STREAM", kRtNoPackStream}, {"NO_PAIR_CHAINS", kRtNoPairChains}, {"NO_PERIOD_HINT", kRtNoPeriodHint},
        {"NO_BREAK_ROUND", kRtNoBreakRound}, {"NO_PERIOD_PROBE", kRtNoPeriodProbe}, {"NO_PERIOD_STREAM", kRtNoPeriodStream}, {"NO_PROBE", kRtNoProbe},
        {"NO_RANK_WRITER", kRtNoRankWriter}, {"NO_TEXT_ROUNDS", kRtNoTextRounds}, {"NO_MID", kRtNoMid}, {"NO_SHALLOW", kRtNoShallow},
        {"NO_CLOSED_FORM", kRtNoClosedForm}, {"NO_REL_RECORDS", kRtNoRelRecords},
    };
    if (!strcmp(name, "RESET")) { g_route = Route(); return ARCHON_OK; }
    if (!strcmp(name, "FORCE_PATH")) { g_route.force_path = value < 0 ? -1 : (value ? 1 : 0); return ARCHON_OK; }
    if (!strcmp(name, "PASS_RANGES")) {
        if (value < 0 || value > bs::kMaxRanges) { set_error("PASS_RANGES=%ld out of range [1, %d]", value, bs::kMaxRanges); return ARCHON_E_ARG; }
        g_route.pass_ranges = (uint32_t)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "SMALL_BLOCK")) { g_route.small_block = value; return ARCHON_OK; }
    if (!strcmp(name, "ALIGNED_MIN")) { g_route.aligned_min = value; return ARCHON_OK; }
    if (!strcmp(name, "REL_MIN_SEG")) { g_route.rel_min_seg = value; return ARCHON_OK; }
    if (!strcmp(name, "INV_ROWS")) { g_route.inv_rows = value < 0 ? -1 : value > 2 ? 1 : (int)value; return ARCHON_OK; }
    if (!strcmp(name, "INV_SLAB")) { g_route.inv_slab = value > 0 ? (uint32_t)value : 0u; return ARCHON_OK; }
    if (!strcmp(name, "KEY_BYTES")) { g_route.key_bytes = (int)value; return ARCHON_OK; }
    if (!strcmp(name, "INV_SBITS")) { g_route.inv_sbits = (int)value; return ARCHON_OK; }
    if (!strcmp(name, "INV_WALK_WGS")) { g_route.inv_walk_wgs = (int)value; return ARCHON_OK; }
    if (!strcmp(name, "LCP_CAP")) {
        if (value > 4096) { set_error("LCP_CAP=%ld out of range [1, 4096]", value); return ARCHON_E_ARG; }
        g_route.lcp_cap = value > 0 ? (int)value : 0;
        return ARCHON_OK;
    }
    if (!strcmp(name, "LCP_WINDOW")) {
        if (value > (1l << 30)) { set_error("LCP_WINDOW=%ld out of range [1, 2^30]", value); return ARCHON_E_ARG; }
        g_route.lcp_window = value > 0 ? value : 0;
        return ARCHON_OK;
    }
    if (!strcmp(name, "FM_SUB_ROWS")) {
        if (value && (value < 16 || value > 1024 || (value & (value - 1)))) {
            set_error("FM_SUB_ROWS=%ld: not a power of two in [16, 1024]", value);
            return ARCHON_E_ARG;
        }
        g_route.fm_sub_rows = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "REP_FAN")) {
        if (value && (value < 2 || value > 64 || (value & (value - 1)))) {
            set_error("REP_FAN=%ld: not a power of two in [2, 64]", value);
            return ARCHON_E_ARG;
        }
        g_route.rep_fan = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "LZ_FAN")) {
        if (value && (value < 2 || value > 64 || (value & (value - 1)))) {
            set_error("LZ_FAN=%ld: not a power of two in [2, 64]", value);
            return ARCHON_E_ARG;
        }
        g_route.lz_fan = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "LZ_TILE")) {
        if (value && (value < 2 || value > (long)lz::kMaxTile || (value & (value - 1)))) {
            set_error("LZ_TILE=%ld: not a power of two in [2, %u]", value, lz::kMaxTile);
            return ARCHON_E_ARG;
        }
        g_route.lz_tile = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "KMER_TILE")) {
        if (value && (value < (long)kmer::kMinTile || value > (long)kmer::kDefaultTile || (value & (value - 1)))) {
            set_error("KMER_TILE=%ld: not a power of two in [%u, %u]", value, kmer::kMinTile, kmer::kDefaultTile);
            return ARCHON_E_ARG;
        }
        g_route.kmer_tile = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "MS_CHUNK")) {
        if (value < 0 || value > 0xFFFFFFFFl) { set_error("MS_CHUNK=%ld: not a chunk of 1 .. 2^32 - 1 bytes (0: the default)", value); return ARCHON_E_ARG; }
        g_route.ms_chunk = value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "EDIT_TILE")) {
        if (value < 0 || value > 64) { set_error("EDIT_TILE=%ld: not a tile of 1 .. 64 ends (0: the default)", value); return ARCHON_E_ARG; }
        g_route.edit_tile = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "EDIT_BATCH")) {
        if (value < 0 || value > 0x7FFFFFFFl) { set_error("EDIT_BATCH=%ld: not a batch of 1 .. 2^31 - 1 patterns (0: the budget's own)", value); return ARCHON_E_ARG; }
        g_route.edit_batch = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "DOC_TILE")) {
        if (value && (value < (long)fmd::kMinTile || value > (long)fmd::kMaxTile || value % 64)) {
            set_error("DOC_TILE=%ld: not a tile of 64 .. 2^20 rows, a multiple of 64 (0: the default)", value);
            return ARCHON_E_ARG;
        }
        g_route.doc_tile = (int)value;
        return ARCHON_OK;
    }
    if (!strcmp(name, "FM_SAMPLE_WALK")) { g_route.fm_sample_walk = value ? 1 : 0; return ARCHON_OK; }
    if (!strcmp(name, "FM_SUPER_ROWS")) {
        if (value && (value < 16 || value > 65536 || (value & (value - 1)))) {
            set_error("FM_SUPER_ROWS=%ld: not a power of two in [16, 65536]", value);
            return ARCHON_E_ARG;
        }
        g_route.fm_super_rows = (int)value;
        return ARCHON_OK;
    }
    for (const auto &f : kFlags)
        if (!strcmp(name, f.name)) {
            if (value) g_route.flags |= f.bit; else g_route.flags &= ~f.bit;
            return ARCHON_OK;
        }
    set_error("unknown route '%s'", name);
    return ARCHON_E_ARG;
}

int archon_hip_get_lcp_stats(int dev, archon_hip_lcp_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_lcp_stats.get(dev, out, "LCP call");
}

int archon_hip_get_stats(int dev, archon_hip_stats *out)
{
    if (!out) { set_error("null pointer"); return ARCHON_E_ARG; }
    return t_stats.get(dev, out, "transform");
}

}  // extern "C"
