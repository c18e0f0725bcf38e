"""ctypes binding of libarchon_hip.so (include/archon_hip.h).

Host-side plumbing for tests and bench.py only: numpy arrays for the host-buffer
entry points, torch CUDA tensors (raw device pointers + the current HIP stream)
for the device-resident ones.  There is no CPU fallback here or in the library:
if the shared object is missing, importing raises; without a GPU every compute
call returns ARCHON_E_NODEVICE and this module raises ArchonError.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARCHON_HIP_LIB") or os.path.join(_HERE, "libarchon_hip.so")   # override: A/B builds only

OK, E_ARG, E_NODEVICE, E_NOMEM, E_HIP, E_INTERNAL, E_CORRUPT = 0, -1, -2, -3, -4, -5, -6
MAX_N = 0x3FFFFF00

SYMBOLS = [
    "archon_hip_device_count", "archon_hip_last_error",
    "archon_hip_forward", "archon_hip_inverse", "archon_hip_hist256",
    "archon_hip_validate", "archon_hip_radix_scatter",
    "archon_hip_forward_keep", "archon_hip_read_bwt", "archon_hip_host_alloc", "archon_hip_host_free",
    "archon_hip_forward_dev", "archon_hip_inverse_dev", "archon_hip_hist256_dev",
    "archon_hip_validate_dev", "archon_hip_radix_scatter_dev", "archon_hip_sa_to_bwt", "archon_hip_sa_to_bwt_dev",
    "archon_hip_lms_select", "archon_hip_lms_select_dev",
    "archon_hip_reserve", "archon_hip_release", "archon_hip_get_stats",
    "archon_hip_block_create", "archon_hip_block_destroy", "archon_hip_block_forward", "archon_hip_block_read_bwt",
    "archon_hip_block_validate", "archon_hip_block_stats", "archon_hip_validate_keep",
    "archon_hip_bind_context", "archon_hip_context_of_thread", "archon_hip_set_option", "archon_hip_get_option",
    "archon_hip_post_bound", "archon_hip_post_encode_dev", "archon_hip_forward_post", "archon_hip_validate_resident_dev",
    "archon_hip_forward_batch", "archon_hip_inverse_batch", "archon_hip_forward_batch_dev", "archon_hip_inverse_batch_dev",
    "archon_hip_post_decode_dev", "archon_hip_inverse_post",
    "archon_hip_lcp", "archon_hip_lcp_dev", "archon_hip_block_lcp", "archon_hip_lcp_keep", "archon_hip_get_lcp_stats",
    "archon_hip_fm_create", "archon_hip_fm_create_dev", "archon_hip_fm_destroy", "archon_hip_fm_count", "archon_hip_fm_count_dev",
    "archon_hip_block_fm_count", "archon_hip_block_fm_locate", "archon_hip_get_fm_stats",
    "archon_hip_fm_sample", "archon_hip_block_fm_index", "archon_hip_fm_read_samples", "archon_hip_fm_locate", "archon_hip_fm_extract",
    "archon_hip_fm_extract_dev", "archon_hip_get_fm_walk_stats",
    "archon_hip_fm_approx", "archon_hip_fm_approx_dev", "archon_hip_block_fm_approx", "archon_hip_fm_locate_hits",
    "archon_hip_block_fm_locate_hits", "archon_hip_get_fm_approx_stats",
    "archon_hip_fm_classes", "archon_hip_fm_classes_dev", "archon_hip_block_fm_classes", "archon_hip_get_fm_class_stats",
    "archon_hip_fm_edit", "archon_hip_fm_edit_dev", "archon_hip_block_fm_edit", "archon_hip_get_fm_edit_stats",
    "archon_hip_fm_mirror", "archon_hip_fm_mirror_dev", "archon_hip_block_fm_mirror", "archon_hip_fm_read_mirror", "archon_hip_fm_smems",
    "archon_hip_fm_smems_dev", "archon_hip_fm_locate_mems", "archon_hip_block_fm_locate_mems", "archon_hip_get_fm_mem_stats",
    "archon_hip_fm_attach_lcp", "archon_hip_fm_attach_lcp_dev", "archon_hip_block_fm_attach_lcp", "archon_hip_fm_ms", "archon_hip_fm_ms_dev",
    "archon_hip_get_fm_ms_stats",
    "archon_hip_fm_attach_sa", "archon_hip_fm_attach_sa_dev", "archon_hip_block_fm_attach_sa", "archon_hip_fm_ms_text", "archon_hip_fm_ms_text_dev",
    "archon_hip_fm_rlz", "archon_hip_fm_rlz_dev", "archon_hip_get_fm_text_stats",
    "archon_hip_fm_attach_docs", "archon_hip_fm_attach_docs_dev", "archon_hip_block_fm_attach_docs", "archon_hip_fm_docs", "archon_hip_fm_docs_dev",
    "archon_hip_fm_docs_ranges", "archon_hip_fm_docs_ranges_dev", "archon_hip_fm_doc_of", "archon_hip_fm_doc_of_dev", "archon_hip_get_fm_doc_stats",
    "archon_hip_repeats", "archon_hip_repeats_dev", "archon_hip_block_repeats", "archon_hip_get_repeat_stats",
    "archon_hip_lpf", "archon_hip_lpf_dev", "archon_hip_lz_parse", "archon_hip_lz_parse_dev", "archon_hip_block_lz", "archon_hip_get_lz_stats",
    "archon_hip_kmers", "archon_hip_kmers_dev", "archon_hip_block_kmers", "archon_hip_kmer_occ", "archon_hip_kmer_occ_dev", "archon_hip_block_kmer_occ",
    "archon_hip_sus", "archon_hip_sus_dev", "archon_hip_block_sus", "archon_hip_get_kmer_stats",
    "archon_hip_maws", "archon_hip_maws_dev", "archon_hip_block_maws", "archon_hip_maw_last_stats",
    "archon_hip_entropy", "archon_hip_entropy_dev", "archon_hip_block_entropy", "archon_hip_complexity", "archon_hip_complexity_dev",
    "archon_hip_block_complexity", "archon_hip_entropy_last_stats",
    "archon_hip_lce", "archon_hip_lce_dev", "archon_hip_block_lce", "archon_hip_runs", "archon_hip_runs_dev", "archon_hip_block_runs",
    "archon_hip_runs_last_stats",
    "archon_hip_fm_attach_wm", "archon_hip_block_fm_attach_wm", "archon_hip_fm_win_count", "archon_hip_fm_win_count_dev", "archon_hip_fm_win_select",
    "archon_hip_fm_win_select_dev", "archon_hip_fm_win_list", "archon_hip_fm_win_list_dev", "archon_hip_fm_win_last_stats",
    "archon_hip_fm_attach_ends", "archon_hip_fm_attach_ends_dev", "archon_hip_block_fm_attach_ends", "archon_hip_fm_overlaps",
    "archon_hip_fm_overlaps_dev", "archon_hip_fm_ovl_last_stats",
]

# archon_hip_fm_hit: one distinct string within the distance of a pattern (FmIndex.approx, Block.fm_approx)
FM_HIT = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("mismatches", "<u4"), ("pattern", "<u4")])
# archon_hip_fm_edit_hit: one match of a pattern within the edit distance (FmIndex.edit, Block.fm_edit): x[start .. end)
FM_EDIT = np.dtype([("start", "<u4"), ("end", "<u4"), ("distance", "<u4"), ("pattern", "<u4")])
# archon_hip_fm_mem: one super-maximal exact match of a pattern (FmIndex.smems): rows [lo, hi) of the piece [start, end)
FM_MEM = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("start", "<u4"), ("end", "<u4"), ("pattern", "<u4"), ("reserved0", "<u4")])
# archon_hip_fm_doc: one document of a pattern or a row range (FmIndex.docs, docs_ranges): tf rows of the range lie in it, the first is `row`
FM_DOC = np.dtype([("doc", "<u4"), ("tf", "<u4"), ("row", "<u4"), ("range", "<u4")])
# archon_hip_fm_win: one occurrence of a row range inside its item window (FmIndex.win_list): the item where it ends, its range
FM_WIN = np.dtype([("item", "<u4"), ("range", "<u4")])
# archon_hip_fm_ovl: one suffix-prefix overlap (FmIndex.overlaps): document `doc` ends with the first `len` bytes of query `query`; `row` its end row
FM_OVL = np.dtype([("query", "<u4"), ("doc", "<u4"), ("len", "<u4"), ("row", "<u4")])
# archon_hip_repeat: one repeat of a block (repeats, Block.repeats): rows [lo, hi) of a string of len bytes, its representative row
REPEAT = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("len", "<u4"), ("row", "<u4")])
# struct archon_hip_lpf: the longest previous factor that ends at an item and the item where a copy of it ends (lpf, Block.lz)
LPF = np.dtype([("len", "<u4"), ("src", "<u4")])
# archon_hip_phrase: one phrase of the parse (lz_parse, Block.lz): it ends at item `end`; len 0 is a literal
PHRASE = np.dtype([("end", "<u4"), ("len", "<u4"), ("src", "<u4")])
# one phrase of lz77(): it starts at z[pos] and copies len bytes from z[src] (len 0: the literal z[pos])
LZ77 = np.dtype([("pos", "<u4"), ("len", "<u4"), ("src", "<u4")])
# archon_hip_kmer: one k-mer of a block (kmers, Block.kmers): rows [lo, hi) of its occurrences, item = sa[lo]: the bytes x[item-k .. item)
KMER = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("item", "<u4")])
# archon_hip_maw: one minimal absent word of a block (maws, Block.maws): rows [lo, hi) of the word without its last byte, the
# word's length, item = sa[lo]: the bytes x[item-len+1 .. item) followed by `last`
MAW = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("len", "<u4"), ("item", "<u4"), ("last", "<u4")])
# struct archon_hip_entropy: the order-k statistics of a block (entropy, Block.entropy): the contexts of length k that a byte
# follows, those always followed by the same byte, the distinct (context, byte) pairs, n - k, and bits = n * H_k
ENTROPY = np.dtype([("k", "<u4"), ("reserved", "<u4"), ("contexts", "<u8"), ("deterministic", "<u8"), ("pairs", "<u8"), ("symbols", "<u8"),
                    ("bits", "<f8")])
# archon_hip_run: one run (maximal repetition) of a block (runs, Block.runs): x[start .. end) has smallest period `period`, holds at
# least two copies of it and extends neither way; root is the item of the rule that found it, and the output ascends in it
RUN = np.dtype([("start", "<u4"), ("end", "<u4"), ("period", "<u4"), ("root", "<u4")])


class _Record(ctypes.Structure):
    """what every statistics structure shares: its fields as a dict, without the padding (names that start with `_`)"""

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("_")}


class Stats(_Record):
    _fields_ = [
        ("n", ctypes.c_uint32), ("radix_passes", ctypes.c_uint32), ("doubling_rounds", ctypes.c_uint32),
        ("_pad0", ctypes.c_uint32),
        ("unresolved_initial", ctypes.c_uint64), ("unresolved_total", ctypes.c_uint64),
        ("ms_total", ctypes.c_float), ("ms_hist", ctypes.c_float), ("ms_sort", ctypes.c_float),
        ("ms_doubling", ctypes.c_float), ("ms_bwt", ctypes.c_float), ("ms_lf_build", ctypes.c_float),
        ("ms_lf_walk", ctypes.c_float), ("_pad1", ctypes.c_uint32),
        ("walk_chains", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("radix_pass_timed", ctypes.c_uint32),
        ("ms_radix_pass_sum", ctypes.c_float), ("ms_local_sort", ctypes.c_float), ("ms_resolve", ctypes.c_float),
        ("path", ctypes.c_uint32), ("tie_groups", ctypes.c_uint32), ("tie_items", ctypes.c_uint32),
        ("ms_pass_text", ctypes.c_float), ("ms_pass_rec", ctypes.c_float),
        ("alphabet_bits", ctypes.c_uint32), ("period", ctypes.c_uint32),
        ("chain_items", ctypes.c_uint32), ("text_rounds", ctypes.c_uint32), ("seg_big_items", ctypes.c_uint64),
        ("chain_pairs", ctypes.c_uint64), ("break_rounds", ctypes.c_uint32), ("break_settled", ctypes.c_uint32),
        ("mid_items", ctypes.c_uint64), ("arena_bytes", ctypes.c_uint64),
        ("host_syncs", ctypes.c_uint32), ("_pad2", ctypes.c_uint32),
    ]


class LcpStats(_Record):
    """archon_hip_lcp_stats: the calling thread's last LCP call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("long_rounds", ctypes.c_uint32), ("max_lcp", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32),
        ("irreducible", ctypes.c_uint64), ("long_items", ctypes.c_uint64), ("compared_bytes", ctypes.c_uint64),
        ("host_syncs", ctypes.c_uint32), ("ms_total", ctypes.c_float),
    ]


class FmStats(_Record):
    """archon_hip_fm_stats: the calling thread's last FM call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("patterns", ctypes.c_uint32), ("pattern_bytes", ctypes.c_uint64), ("steps", ctypes.c_uint64),
        ("shared_steps", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32), ("built", ctypes.c_uint32),
        ("table_bytes", ctypes.c_uint64), ("ms_build", ctypes.c_float), ("ms_query", ctypes.c_float),
    ]


class FmWalkStats(_Record):
    """archon_hip_fm_walk_stats: the calling thread's last sample / locate / extract call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("rate", ctypes.c_uint32), ("route", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("samples", ctypes.c_uint64), ("sample_bytes", ctypes.c_uint64), ("walks", ctypes.c_uint64),
        ("lf_steps", ctypes.c_uint64), ("max_walk", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("ms_build", ctypes.c_float),
        ("ms_query", ctypes.c_float),
    ]


class FmApproxStats(_Record):
    """archon_hip_fm_approx_stats: the calling thread's last approximate call (approx, locate_hits) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("patterns", ctypes.c_uint32), ("max_mismatches", ctypes.c_uint32), ("built", ctypes.c_uint32),
        ("pattern_bytes", ctypes.c_uint64), ("expansions", ctypes.c_uint64), ("steps", ctypes.c_uint64), ("hits", ctypes.c_uint64),
        ("occurrences", ctypes.c_uint64), ("lf_steps", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("ms_build", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float), ("ms_locate", ctypes.c_float),
    ]


class FmClassStats(_Record):
    """archon_hip_fm_class_stats: the calling thread's last class call (classes, classes_dev, fm_classes) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("patterns", ctypes.c_uint32), ("max_width", ctypes.c_uint32), ("built", ctypes.c_uint32),
        ("pattern_bytes", ctypes.c_uint64), ("expansions", ctypes.c_uint64), ("steps", ctypes.c_uint64), ("hits", ctypes.c_uint64),
        ("occurrences", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("ms_build", ctypes.c_float), ("ms_width", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class FmEditStats(_Record):
    """archon_hip_fm_edit_stats: the calling thread's last edit-distance call (edit, edit_dev, fm_edit) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("patterns", ctypes.c_uint32), ("max_errors", ctypes.c_uint32), ("tile", ctypes.c_uint32),
        ("batches", ctypes.c_uint32), ("built", ctypes.c_uint32),
        ("pattern_bytes", ctypes.c_uint64), ("seed_rows", ctypes.c_uint64), ("tiles", ctypes.c_uint64), ("rows", ctypes.c_uint64),
        ("hits", ctypes.c_uint64), ("lf_steps", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("ms_build", ctypes.c_float), ("ms_seed", ctypes.c_float), ("ms_extract", ctypes.c_float), ("ms_count", ctypes.c_float),
        ("ms_emit", ctypes.c_float),
    ]


class FmMemStats(_Record):
    """archon_hip_fm_mem_stats: the calling thread's last SMEM call (mirror, smems, locate_mems) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("patterns", ctypes.c_uint32), ("min_len", ctypes.c_uint32), ("built", ctypes.c_uint32),
        ("pattern_bytes", ctypes.c_uint64), ("fwd_steps", ctypes.c_uint64), ("bwd_steps", ctypes.c_uint64), ("found", ctypes.c_uint64),
        ("mems", ctypes.c_uint64), ("occurrences", ctypes.c_uint64), ("lf_steps", ctypes.c_uint64), ("mirror_bytes", ctypes.c_uint64),
        ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32), ("ms_mirror", ctypes.c_float), ("ms_count", ctypes.c_float),
        ("ms_emit", ctypes.c_float), ("ms_locate", ctypes.c_float),
    ]


class FmMsStats(_Record):
    """archon_hip_fm_ms_stats: the calling thread's last attach or matching-statistics call (attach_lcp, ms) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("patterns", ctypes.c_uint32), ("fan", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("attached", ctypes.c_uint32),
        ("pattern_bytes", ctypes.c_uint64), ("steps", ctypes.c_uint64), ("parents", ctypes.c_uint64), ("probes", ctypes.c_uint64),
        ("matched", ctypes.c_uint64), ("longest", ctypes.c_uint32), ("lcp_bytes", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("ms_lcp", ctypes.c_float), ("ms_attach", ctypes.c_float), ("ms_query", ctypes.c_float),
    ]


class FmTextStats(_Record):
    """archon_hip_fm_text_stats: the calling thread's last attach_sa, ms_text or rlz call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("m", ctypes.c_uint32), ("chunk", ctypes.c_uint32), ("chunks", ctypes.c_uint32), ("fan", ctypes.c_uint32),
        ("levels", ctypes.c_uint32), ("saturated", ctypes.c_uint64), ("full_chunks", ctypes.c_uint32), ("runs", ctypes.c_uint32),
        ("longest_run", ctypes.c_uint32), ("sa_probes", ctypes.c_uint64), ("lcp_probes", ctypes.c_uint64), ("matched", ctypes.c_uint64),
        ("longest", ctypes.c_uint32), ("phrases", ctypes.c_uint64), ("sa_bytes", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("ms_walk", ctypes.c_float), ("ms_sweep", ctypes.c_float), ("ms_fix", ctypes.c_float),
        ("ms_parse", ctypes.c_float),
    ]


class FmDocStats(_Record):
    """archon_hip_fm_doc_stats: the calling thread's last documents call (attach_docs, docs, docs_ranges, doc_of) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("docs", ctypes.c_uint32), ("ranges", ctypes.c_uint32), ("tile", ctypes.c_uint32), ("attached", ctypes.c_uint32),
        ("sort_passes", ctypes.c_uint32), ("longest_tf", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
        ("pattern_bytes", ctypes.c_uint64), ("rows", ctypes.c_uint64), ("tiles", ctypes.c_uint64), ("listed", ctypes.c_uint64),
        ("probes", ctypes.c_uint64), ("doc_bytes", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("ms_attach", ctypes.c_float), ("ms_search", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class FmWinStats(_Record):
    """archon_hip_fm_win_stats: the calling thread's last window call (attach_wm, win_count, win_select, win_list) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("ranges", ctypes.c_uint32), ("most", ctypes.c_uint32), ("attached", ctypes.c_uint32),
        ("reserved0", ctypes.c_uint32), ("rows", ctypes.c_uint64), ("in_window", ctypes.c_uint64), ("listed", ctypes.c_uint64),
        ("walks", ctypes.c_uint64), ("wm_bytes", ctypes.c_uint64), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("ms_attach", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class FmOvlStats(_Record):
    """archon_hip_fm_ovl_stats: the calling thread's last overlap call (attach_ends, overlaps) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("docs", ctypes.c_uint32), ("queries", ctypes.c_uint32), ("min_len", ctypes.c_uint32), ("attached", ctypes.c_uint32),
        ("longest", ctypes.c_uint32), ("pattern_bytes", ctypes.c_uint64), ("steps", ctypes.c_uint64), ("tested", ctypes.c_uint64),
        ("hit", ctypes.c_uint64), ("overlaps", ctypes.c_uint64), ("emitted", ctypes.c_uint64), ("end_bytes", ctypes.c_uint64),
        ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32), ("ms_attach", ctypes.c_float), ("ms_count", ctypes.c_float),
        ("ms_emit", ctypes.c_float), ("reserved0", ctypes.c_uint32),
    ]


class RepeatStats(_Record):
    """archon_hip_repeat_stats: the calling thread's last repeats call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("min_len", ctypes.c_uint32), ("min_occ", ctypes.c_uint32),
        ("fan", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("longest", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
        ("intervals", ctypes.c_uint64), ("repeats", ctypes.c_uint64), ("occurrences", ctypes.c_uint64), ("sum_lcp", ctypes.c_uint64),
        ("distinct_substrings", ctypes.c_uint64), ("probes", ctypes.c_uint64),
        ("ms_lcp", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float), ("reserved1", ctypes.c_float),
    ]


class LzStats(_Record):
    """archon_hip_lz_stats: the calling thread's last LZ call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("dir", ctypes.c_uint32), ("fan", ctypes.c_uint32), ("levels", ctypes.c_uint32),
        ("tile", ctypes.c_uint32), ("parse_levels", ctypes.c_uint32), ("longest", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
        ("phrases", ctypes.c_uint64), ("literals", ctypes.c_uint64), ("probes", ctypes.c_uint64), ("hops", ctypes.c_uint64),
        ("ms_lcp", ctypes.c_float), ("ms_lpf", ctypes.c_float), ("ms_parse", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class KmerStats(_Record):
    """archon_hip_kmer_stats: the calling thread's last k-mer call (kmers, kmer_occ, sus) on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("k", ctypes.c_uint32), ("min_occ", ctypes.c_uint32), ("max_occ", ctypes.c_uint32),
        ("bins", ctypes.c_uint32), ("tile", ctypes.c_uint32), ("what", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("most", ctypes.c_uint32),
        ("groups", ctypes.c_uint64), ("short_rows", ctypes.c_uint64), ("distinct", ctypes.c_uint64), ("kmers", ctypes.c_uint64),
        ("occurrences", ctypes.c_uint64), ("unique", ctypes.c_uint64),
        ("ms_lcp", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float), ("ms_scatter", ctypes.c_float),
    ]


class MawStats(_Record):
    """archon_hip_maw_stats: the calling thread's last minimal-absent-words call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("min_len", ctypes.c_uint32), ("max_len", ctypes.c_uint32), ("fan", ctypes.c_uint32),
        ("levels", ctypes.c_uint32), ("direct_rows", ctypes.c_uint32), ("built", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32),
        ("host_syncs", ctypes.c_uint32), ("absent_bytes", ctypes.c_uint32), ("shortest", ctypes.c_uint32), ("longest", ctypes.c_uint32),
        ("intervals", ctypes.c_uint64), ("nodes", ctypes.c_uint64), ("children", ctypes.c_uint64), ("sets_direct", ctypes.c_uint64),
        ("sets_table", ctypes.c_uint64), ("words", ctypes.c_uint64), ("probes", ctypes.c_uint64),
        ("ms_lcp", ctypes.c_float), ("ms_build", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class Complexity(_Record):
    """struct archon_hip_complexity: the substring complexity of a block and the runs of its BWT (complexity, Block.complexity)"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("max_len", ctypes.c_uint32), ("lcp_max", ctypes.c_uint32), ("delta_len", ctypes.c_uint32),
        ("delta_count", ctypes.c_uint32), ("delta_exact", ctypes.c_uint32), ("longest_run", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("lcp_sum", ctypes.c_uint64), ("substrings", ctypes.c_uint64), ("runs", ctypes.c_uint64),
    ]


class EntropyStats(_Record):
    """archon_hip_entropy_stats: the calling thread's last entropy or complexity call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("nk", ctypes.c_uint32), ("what", ctypes.c_uint32), ("tile", ctypes.c_uint32),
        ("direct_rows", ctypes.c_uint32), ("built", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("groups_direct", ctypes.c_uint64), ("groups_table", ctypes.c_uint64), ("groups_in_wave", ctypes.c_uint64),
        ("ms_lcp", ctypes.c_float), ("ms_build", ctypes.c_float), ("ms_count", ctypes.c_float),
    ]


class RunStats(_Record):
    """archon_hip_run_stats: the calling thread's last runs or LCE call on a device"""
    _fields_ = [
        ("n", ctypes.c_uint32), ("min_period", ctypes.c_uint32), ("max_period", ctypes.c_uint32), ("min_copies", ctypes.c_uint32),
        ("min_len", ctypes.c_uint32), ("what", ctypes.c_uint32), ("fan", ctypes.c_uint32), ("lcp_fan", ctypes.c_uint32),
        ("levels", ctypes.c_uint32), ("longest_period", ctypes.c_uint32), ("kernel_launches", ctypes.c_uint32), ("host_syncs", ctypes.c_uint32),
        ("candidates", ctypes.c_uint64), ("roots", ctypes.c_uint64), ("lce_queries", ctypes.c_uint64), ("probes", ctypes.c_uint64),
        ("runs", ctypes.c_uint64), ("emitted", ctypes.c_uint64),
        ("ms_forward", ctypes.c_float), ("ms_lcp", ctypes.c_float), ("ms_build", ctypes.c_float), ("ms_count", ctypes.c_float),
        ("ms_emit", ctypes.c_float),
    ]


class ArchonError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("archon_hip error %d: %s" % (code, msg))
        self.code = code


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libarchon_hip.so not built: run `make lib` (hipcc, gfx950); there is no CPU fallback")
    # A process that also uses PyTorch-ROCm must load torch FIRST: torch brings its own HIP runtime, and a library that has
    # already bound to the system's runtime then finds no device ("no HIP device available") once torch has opened the GPU.
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, u32, i32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
    lib.archon_hip_device_count.restype = i32
    lib.archon_hip_last_error.restype = ctypes.c_char_p
    for name, args in {
        "archon_hip_forward": [vp, u32, vp, vp, vp, i32],
        "archon_hip_inverse": [vp, u32, u32, vp, i32],
        "archon_hip_hist256": [vp, sz, vp, i32],
        "archon_hip_validate": [vp, u32, vp, i32],
        "archon_hip_sa_to_bwt": [vp, u32, vp, vp, vp, i32],
        "archon_hip_sa_to_bwt_dev": [vp, u32, vp, vp, vp, i32, vp],
        "archon_hip_radix_scatter": [vp, sz, vp, i32],
        "archon_hip_lms_select": [vp, u32, vp, vp, vp, i32],
        "archon_hip_lms_select_dev": [vp, u32, vp, vp, vp, i32, vp],
        "archon_hip_forward_dev": [vp, u32, vp, vp, vp, i32, vp],
        "archon_hip_inverse_dev": [vp, u32, u32, vp, i32, vp],
        "archon_hip_hist256_dev": [vp, sz, vp, i32, vp],
        "archon_hip_validate_dev": [vp, u32, vp, i32, vp],
        "archon_hip_validate_resident_dev": [vp, u32, vp, vp, u32, i32, vp],
        "archon_hip_radix_scatter_dev": [vp, sz, vp, i32, vp],
        "archon_hip_reserve": [u32, i32, vp],
        "archon_hip_release": [i32],
        "archon_hip_get_stats": [i32, ctypes.POINTER(Stats)],
        "archon_hip_block_create": [i32, vp],
        "archon_hip_block_forward": [vp, vp, u32, vp, vp],
        "archon_hip_block_read_bwt": [vp, u32, u32, vp],
        "archon_hip_block_validate": [vp],
        "archon_hip_block_stats": [vp, ctypes.POINTER(Stats)],
        "archon_hip_forward_keep": [vp, u32, vp, vp, i32],
        "archon_hip_read_bwt": [i32, u32, u32, vp],
        "archon_hip_validate_keep": [i32],
        "archon_hip_bind_context": [i32, i32],
        "archon_hip_context_of_thread": [i32],
        "archon_hip_set_option": [i32, ctypes.c_char_p, ctypes.c_long],
        "archon_hip_get_option": [i32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)],
        "archon_hip_post_decode_dev": [vp, sz, vp, u32, vp, i32, vp],
        "archon_hip_inverse_post": [vp, sz, u32, vp, u32, vp, i32],
        "archon_hip_forward_batch": [vp, vp, u32, vp, vp, i32, i32],
        "archon_hip_inverse_batch": [vp, vp, vp, u32, vp, i32, i32],
        "archon_hip_forward_batch_dev": [vp, vp, u32, vp, vp, vp, i32, i32],
        "archon_hip_inverse_batch_dev": [vp, vp, vp, u32, vp, i32, i32],
        "archon_hip_post_encode_dev": [vp, u32, vp, sz, vp, i32, vp],
        "archon_hip_forward_post": [vp, u32, vp, sz, vp, vp, i32],
        "archon_hip_lcp": [vp, u32, vp, vp, i32],
        "archon_hip_lcp_dev": [vp, u32, vp, vp, i32, vp],
        "archon_hip_block_lcp": [vp, vp],
        "archon_hip_lcp_keep": [i32, vp],
        "archon_hip_get_lcp_stats": [i32, ctypes.POINTER(LcpStats)],
        "archon_hip_fm_create": [vp, u32, u32, i32, vp],
        "archon_hip_fm_create_dev": [vp, u32, u32, i32, vp, vp],
        "archon_hip_fm_count": [vp, vp, vp, u32, vp, vp],
        "archon_hip_fm_count_dev": [vp, vp, vp, u32, vp, vp, vp],
        "archon_hip_block_fm_count": [vp, vp, vp, u32, vp, vp],
        "archon_hip_block_fm_locate": [vp, vp, vp, u32, vp, ctypes.c_uint64, vp],
        "archon_hip_get_fm_stats": [i32, ctypes.POINTER(FmStats)],
        "archon_hip_fm_sample": [vp, u32],
        "archon_hip_block_fm_index": [vp, u32, vp],
        "archon_hip_fm_read_samples": [vp, vp, u32, vp],
        "archon_hip_fm_locate": [vp, vp, vp, u32, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_extract": [vp, vp, vp, u32, vp],
        "archon_hip_fm_extract_dev": [vp, vp, vp, u32, vp, vp],
        "archon_hip_get_fm_walk_stats": [i32, ctypes.POINTER(FmWalkStats)],
        "archon_hip_fm_approx": [vp, vp, vp, u32, u32, vp, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_approx_dev": [vp, vp, vp, u32, u32, vp, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_block_fm_approx": [vp, vp, vp, u32, u32, vp, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_locate_hits": [vp, vp, u32, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp],
        "archon_hip_block_fm_locate_hits": [vp, vp, u32, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp],
        "archon_hip_get_fm_approx_stats": [i32, ctypes.POINTER(FmApproxStats)],
        "archon_hip_fm_classes": [vp, vp, vp, u32, vp, vp, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_classes_dev": [vp, vp, vp, u32, vp, vp, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_block_fm_classes": [vp, vp, vp, u32, vp, vp, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_get_fm_class_stats": [i32, ctypes.POINTER(FmClassStats)],
        "archon_hip_fm_edit": [vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_edit_dev": [vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_block_fm_edit": [vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_get_fm_edit_stats": [i32, ctypes.POINTER(FmEditStats)],
        "archon_hip_fm_mirror": [vp],
        "archon_hip_fm_mirror_dev": [vp, vp, vp],
        "archon_hip_block_fm_mirror": [vp, vp],
        "archon_hip_fm_read_mirror": [vp, vp, u32, vp],
        "archon_hip_fm_smems": [vp, vp, vp, u32, u32, vp, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_smems_dev": [vp, vp, vp, u32, u32, vp, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_fm_locate_mems": [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp],
        "archon_hip_block_fm_locate_mems": [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp],
        "archon_hip_get_fm_mem_stats": [i32, ctypes.POINTER(FmMemStats)],
        "archon_hip_fm_attach_lcp": [vp, vp],
        "archon_hip_fm_attach_lcp_dev": [vp, vp, vp],
        "archon_hip_block_fm_attach_lcp": [vp, vp],
        "archon_hip_fm_ms": [vp, vp, vp, u32, vp, vp, vp],
        "archon_hip_fm_ms_dev": [vp, vp, vp, u32, vp, vp, vp, vp],
        "archon_hip_get_fm_ms_stats": [i32, ctypes.POINTER(FmMsStats)],
        "archon_hip_fm_attach_sa": [vp, vp],
        "archon_hip_fm_attach_sa_dev": [vp, vp, vp],
        "archon_hip_block_fm_attach_sa": [vp, vp],
        "archon_hip_fm_ms_text": [vp, vp, u32, vp, vp, vp],
        "archon_hip_fm_ms_text_dev": [vp, vp, u32, vp, vp, vp, vp],
        "archon_hip_fm_rlz": [vp, vp, u32, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_rlz_dev": [vp, vp, u32, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_get_fm_text_stats": [i32, ctypes.POINTER(FmTextStats)],
        "archon_hip_fm_attach_docs": [vp, vp, u32],
        "archon_hip_fm_attach_docs_dev": [vp, vp, u32, vp],
        "archon_hip_block_fm_attach_docs": [vp, vp, vp, u32],
        "archon_hip_fm_docs": [vp, vp, vp, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_docs_dev": [vp, vp, vp, u32, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_fm_docs_ranges": [vp, vp, vp, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_docs_ranges_dev": [vp, vp, vp, u32, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_fm_doc_of": [vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_fm_doc_of_dev": [vp, vp, ctypes.c_uint64, vp, vp, vp],
        "archon_hip_get_fm_doc_stats": [i32, ctypes.POINTER(FmDocStats)],
        "archon_hip_fm_attach_wm": [vp],
        "archon_hip_block_fm_attach_wm": [vp, vp],
        "archon_hip_fm_win_count": [vp, vp, vp, vp, vp, u32, vp],
        "archon_hip_fm_win_count_dev": [vp, vp, vp, vp, vp, u32, vp, vp],
        "archon_hip_fm_win_select": [vp, vp, vp, vp, vp, vp, u32, vp],
        "archon_hip_fm_win_select_dev": [vp, vp, vp, vp, vp, vp, u32, vp, vp],
        "archon_hip_fm_win_list": [vp, vp, vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_win_list_dev": [vp, vp, vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_fm_win_last_stats": [i32, ctypes.POINTER(FmWinStats)],
        "archon_hip_fm_attach_ends": [vp, vp, u32],
        "archon_hip_fm_attach_ends_dev": [vp, vp, u32, vp],
        "archon_hip_block_fm_attach_ends": [vp, vp, vp, u32],
        "archon_hip_fm_overlaps": [vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_fm_overlaps_dev": [vp, vp, vp, u32, u32, vp, vp, ctypes.c_uint64, vp, vp],
        "archon_hip_fm_ovl_last_stats": [i32, ctypes.POINTER(FmOvlStats)],
        "archon_hip_repeats": [vp, vp, u32, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, i32],
        "archon_hip_repeats_dev": [vp, vp, u32, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, i32, vp],
        "archon_hip_block_repeats": [vp, u32, u32, u32, vp, ctypes.c_uint64, vp],
        "archon_hip_get_repeat_stats": [i32, ctypes.POINTER(RepeatStats)],
        "archon_hip_lpf": [vp, vp, u32, u32, vp, i32],
        "archon_hip_lpf_dev": [vp, vp, u32, u32, vp, i32, vp],
        "archon_hip_lz_parse": [vp, u32, vp, ctypes.c_uint64, vp, i32],
        "archon_hip_lz_parse_dev": [vp, u32, vp, ctypes.c_uint64, vp, i32, vp],
        "archon_hip_block_lz": [vp, u32, vp, vp, ctypes.c_uint64, vp],
        "archon_hip_get_lz_stats": [i32, ctypes.POINTER(LzStats)],
        "archon_hip_kmers": [vp, vp, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, vp, u32, i32],
        "archon_hip_kmers_dev": [vp, vp, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, vp, u32, i32, vp],
        "archon_hip_block_kmers": [vp, u32, u32, u32, vp, ctypes.c_uint64, vp, vp, u32],
        "archon_hip_kmer_occ": [vp, vp, u32, u32, vp, i32],
        "archon_hip_kmer_occ_dev": [vp, vp, u32, u32, vp, i32, vp],
        "archon_hip_block_kmer_occ": [vp, u32, vp],
        "archon_hip_sus": [vp, vp, u32, vp, i32],
        "archon_hip_sus_dev": [vp, vp, u32, vp, i32, vp],
        "archon_hip_block_sus": [vp, vp],
        "archon_hip_get_kmer_stats": [i32, ctypes.POINTER(KmerStats)],
        "archon_hip_maws": [vp, vp, vp, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, i32],
        "archon_hip_maws_dev": [vp, vp, vp, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, i32, vp],
        "archon_hip_block_maws": [vp, u32, u32, vp, ctypes.c_uint64, vp],
        "archon_hip_maw_last_stats": [i32, ctypes.POINTER(MawStats)],
        "archon_hip_lce": [vp, vp, u32, vp, vp, u32, vp, i32],
        "archon_hip_lce_dev": [vp, vp, u32, vp, vp, u32, vp, i32, vp],
        "archon_hip_block_lce": [vp, vp, vp, u32, vp],
        "archon_hip_runs": [vp, vp, vp, u32, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, i32],
        "archon_hip_runs_dev": [vp, vp, vp, u32, u32, u32, u32, u32, vp, ctypes.c_uint64, vp, i32, vp],
        "archon_hip_block_runs": [vp, u32, u32, u32, u32, vp, ctypes.c_uint64, vp],
        "archon_hip_runs_last_stats": [i32, ctypes.POINTER(RunStats)],
        "archon_hip_entropy": [vp, vp, vp, u32, u32, vp, u32, vp, i32],
        "archon_hip_entropy_dev": [vp, vp, vp, u32, u32, vp, u32, vp, i32, vp],
        "archon_hip_block_entropy": [vp, vp, u32, vp],
        "archon_hip_complexity": [vp, vp, u32, u32, vp, ctypes.POINTER(Complexity), i32],
        "archon_hip_complexity_dev": [vp, vp, u32, u32, vp, ctypes.POINTER(Complexity), i32, vp],
        "archon_hip_block_complexity": [vp, u32, vp, ctypes.POINTER(Complexity)],
        "archon_hip_entropy_last_stats": [i32, ctypes.POINTER(EntropyStats)],
    }.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i32
    lib.archon_hip_block_destroy.argtypes = [vp]
    lib.archon_hip_block_destroy.restype = None
    lib.archon_hip_fm_destroy.argtypes = [vp]
    lib.archon_hip_fm_destroy.restype = None
    lib.archon_hip_post_bound.argtypes = [u32]
    lib.archon_hip_post_bound.restype = sz
    lib.archon_hip_test_route.argtypes = [ctypes.c_char_p, ctypes.c_long]      # include/archon_hip_test.h (tests only)
    lib.archon_hip_test_route.restype = i32
    return lib


_lib = None
_routes_seen = None
# Test routing (include/archon_hip_test.h): the library reads nothing from the environment; the tests, bench.py and the
# tools keep saying ARCHON_<NAME>=<value> in os.environ, and this binding hands what it finds to archon_hip_test_route
# before the next call into the library.
_ROUTE_NAMES = ("FORCE_PATH", "SMALL_BLOCK", "PASS_RANGES", "INV_ROWS", "INV_SLAB", "INV_SBITS", "INV_WALK_WGS", "NO_ALIGNED", "NO_CHAINS",
                "NO_PACK", "NO_PAIR_CHAINS", "NO_PERIOD_HINT", "NO_BREAK_ROUND", "NO_PERIOD_STREAM",
                "NO_RANK_WRITER", "NO_TEXT_ROUNDS", "NO_MID", "NO_SHALLOW", "NO_CLOSED_FORM", "NO_REL_RECORDS", "ALIGNED_MIN", "REL_MIN_SEG", "KEY_BYTES",
                "LCP_CAP", "LCP_WINDOW", "FM_SUB_ROWS", "FM_SUPER_ROWS", "FM_SAMPLE_WALK", "REP_FAN", "LZ_FAN", "LZ_TILE", "MS_CHUNK",
                "EDIT_TILE", "EDIT_BATCH", "DOC_TILE", "KMER_TILE", "STRIDE_GRID")


def _sync_routes(L):
    global _routes_seen
    now = tuple(os.environ.get("ARCHON_" + k) for k in _ROUTE_NAMES)
    if now == _routes_seen or (_routes_seen is None and not any(v is not None for v in now)):
        return          # (a process that names no route never touches the test hook)
    _routes_seen = now
    L.archon_hip_test_route(b"RESET", 0)
    for k, v in zip(_ROUTE_NAMES, now):
        if v is None:
            continue
        try:
            iv = int(v)
        except ValueError:
            iv = 1
        if L.archon_hip_test_route(k.encode(), iv) < 0:
            raise ArchonError(-1, L.archon_hip_last_error().decode("utf-8", "replace"))


def lib():
    global _lib
    if _lib is None:
        _lib = load()
    _sync_routes(_lib)
    return _lib


def _check(rc):
    if rc < 0:
        raise ArchonError(rc, lib().archon_hip_last_error().decode("utf-8", "replace"))
    return rc


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def device_count():
    return lib().archon_hip_device_count()


# ---------------------------------------------------------------- host buffers (numpy)
def forward(x, want_sa=True, dev=0):
    """x: uint8 array -> (sa or None, bwt, base_id).  Archon::enCompute + enWrite semantics."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n = x.size
    sa = np.empty(n, dtype=np.uint32) if want_sa else None
    bwt = np.empty(n, dtype=np.uint8)
    base = ctypes.c_uint32(0)
    _check(lib().archon_hip_forward(_p(x), n, _p(sa) if want_sa else None, _p(bwt),
                                    ctypes.cast(ctypes.byref(base), ctypes.c_void_p), dev))
    return sa, bwt, base.value


def inverse(bwt, base_id, dev=0):
    """bwt + base_id -> x.  Archon::deCompute + deWrite semantics."""
    bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
    out = np.empty(bwt.size, dtype=np.uint8)
    _check(lib().archon_hip_inverse(_p(bwt), bwt.size, int(base_id), _p(out), dev))
    return out


def hist256(x, dev=0):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    out = np.zeros(256, dtype=np.uint32)
    _check(lib().archon_hip_hist256(_p(x), x.size, _p(out), dev))
    return out


def validate(x, sa, dev=0):
    x = np.ascontiguousarray(x, dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    return bool(_check(lib().archon_hip_validate(_p(x), x.size, _p(sa), dev)))


def sa_to_bwt(x, sa, dev=0):
    """(bwt, base_id) for a suffix array the caller holds (Archon::enWrite's gather, archon.cpp:887-900)"""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    bwt = np.empty(x.size, np.uint8)
    base = ctypes.c_uint32(0)
    _check(lib().archon_hip_sa_to_bwt(_p(x), x.size, _p(sa), _p(bwt), ctypes.byref(base), dev))
    return bwt, int(base.value)


def lms_select(x, dev=0):
    """(count[256], items) of a7's findLMS (archon.cpp:160-172): the subset the reference sorts directly"""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    count = np.zeros(256, np.uint32)
    items = np.zeros(x.size // 2 + 8, np.uint32)
    n1 = ctypes.c_uint32(0)
    _check(lib().archon_hip_lms_select(_p(x), x.size, _p(count), _p(items), ctypes.cast(ctypes.byref(n1), ctypes.c_void_p), dev))
    return count, items[:n1.value]


def lcp(x, sa, dev=0):
    """the LCP array of suffix array sa of x (include/archon_hip.h: archon_hip_lcp), uint32[n]"""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    out = np.empty(x.size, np.uint32)
    _check(lib().archon_hip_lcp(_p(x), x.size, _p(sa), _p(out), dev))
    return out


def _last_stats(cls, getter_name, dev):
    """the record `cls` of the calling thread's last call of one kind on dev, from the library's getter of that name"""
    s = cls()
    _check(getattr(lib(), getter_name)(dev, ctypes.byref(s)))
    return s


def lcp_stats(dev=0):
    """LcpStats of the calling thread's last LCP call on dev"""
    return _last_stats(LcpStats, "archon_hip_get_lcp_stats", dev)


def fm_stats(dev=0):
    """FmStats of the calling thread's last FM call on dev"""
    return _last_stats(FmStats, "archon_hip_get_fm_stats", dev)


def fm_walk_stats(dev=0):
    """FmWalkStats of the calling thread's last sample / locate / extract call on dev"""
    return _last_stats(FmWalkStats, "archon_hip_get_fm_walk_stats", dev)


def fm_approx_stats(dev=0):
    """FmApproxStats of the calling thread's last approximate call (approx, locate_hits) on dev"""
    return _last_stats(FmApproxStats, "archon_hip_get_fm_approx_stats", dev)


def fm_class_stats(dev=0):
    """FmClassStats of the calling thread's last class call (classes, classes_dev, fm_classes) on dev"""
    return _last_stats(FmClassStats, "archon_hip_get_fm_class_stats", dev)


def fm_edit_stats(dev=0):
    """FmEditStats of the calling thread's last edit-distance call (edit, edit_dev, fm_edit) on dev"""
    return _last_stats(FmEditStats, "archon_hip_get_fm_edit_stats", dev)


def fm_mem_stats(dev=0):
    """FmMemStats of the calling thread's last SMEM call (mirror, smems, locate_mems) on dev"""
    return _last_stats(FmMemStats, "archon_hip_get_fm_mem_stats", dev)


def fm_ms_stats(dev=0):
    """FmMsStats of the calling thread's last attach or matching-statistics call (attach_lcp, ms) on dev"""
    return _last_stats(FmMsStats, "archon_hip_get_fm_ms_stats", dev)


def fm_text_stats(dev=0):
    """FmTextStats of the calling thread's last attach_sa, ms_text or rlz call on dev"""
    return _last_stats(FmTextStats, "archon_hip_get_fm_text_stats", dev)


def fm_doc_stats(dev=0):
    """FmDocStats of the calling thread's last documents call (attach_docs, docs, docs_ranges, doc_of) on dev"""
    return _last_stats(FmDocStats, "archon_hip_get_fm_doc_stats", dev)


def fm_win_stats(dev=0):
    """the calling thread's last window call (attach_wm, win_count, win_select, win_list) on `dev` as a dict"""
    return _last_stats(FmWinStats, "archon_hip_fm_win_last_stats", dev)


def fm_ovl_stats(dev=0):
    """the calling thread's last overlap call (attach_ends, overlaps) on `dev` as a dict"""
    return _last_stats(FmOvlStats, "archon_hip_fm_ovl_last_stats", dev)


def ends_from_bounds(bounds, trim=0):
    """the ends of the documents cut by bounds[0 .. D] for FmIndex.attach_ends: bounds[1:] - trim, trim the bytes every document
    finishes with that are no part of it (1 for a separator).  A document that `trim` would empty is refused"""
    bounds = np.ascontiguousarray(bounds, dtype=np.int64).ravel()
    trim = int(trim)
    if bounds.size < 2:
        raise ValueError("ends_from_bounds: no documents")
    if trim < 0:
        raise ValueError("ends_from_bounds: trim = %d" % trim)
    short = np.flatnonzero(np.diff(bounds) <= trim)
    if short.size:
        raise ValueError("ends_from_bounds: document %d has %d bytes, trim = %d would empty it" % (short[0], bounds[short[0] + 1] - bounds[short[0]], trim))
    return (bounds[1:] - trim).astype(np.uint32)


def best_overlaps(records):
    """the longest overlap of every (query, doc) pair of an FM_OVL array from FmIndex.overlaps, in its order.  The records come
    by query and ascending length, so the longest of a pair is its last one"""
    records = np.ascontiguousarray(records, FM_OVL)
    if records.size == 0:
        return records
    key = (records["query"].astype(np.uint64) << np.uint64(32)) | records["doc"].astype(np.uint64)
    rev = key[::-1]
    _, first_rev = np.unique(rev, return_index=True)            # the first of a pair in reversed order: its last
    return records[np.sort(records.size - 1 - first_rev)]


def drop_self(records, query_doc):
    """the records whose doc is not the query's own document, query_doc[j] the document query j was taken from: the
    all-against-all case where the queries are the documents"""
    records = np.ascontiguousarray(records, FM_OVL)
    query_doc = np.ascontiguousarray(query_doc, dtype=np.int64).ravel()
    if records.size == 0:
        return records
    return records[query_doc[records["query"]] != records["doc"]]


def rlz_decode(x, phrases, m, literals=None):
    """the text of m bytes from the block x and the PHRASE array of FmIndex.rlz: a phrase (end, len, src) copies x[src-len .. src)
    to [end-len .. end).  A literal (len 0) is a byte the block does not hold, and the parse says where it is, not what:
    `literals` gives those bytes in phrase order (text[end - 1] of every phrase with len 0); a parse with literals and none given
    raises ValueError.  numpy only"""
    x = np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)
    phrases = np.ascontiguousarray(phrases, PHRASE)
    lit = phrases["len"] == 0
    nlit = int(lit.sum())
    if nlit:
        if literals is None:
            raise ValueError("rlz_decode: %d literals in the parse and no bytes for them" % nlit)
        literals = np.frombuffer(bytes(literals), np.uint8) if isinstance(literals, (bytes, bytearray)) else np.asarray(literals, np.uint8)
        if literals.size != nlit:
            raise ValueError("rlz_decode: %d literals in the parse, %d bytes given" % (nlit, literals.size))
    out = np.zeros(int(m), np.uint8)
    if nlit:
        out[phrases["end"][lit].astype(np.int64) - 1] = literals
    for end, ln, src in zip(phrases["end"][~lit].tolist(), phrases["len"][~lit].tolist(), phrases["src"][~lit].tolist()):
        out[end - ln:end] = x[src - ln:src]
    return out


def ms_smems(len, lo, hi, offsets, min_len=1):
    """the super-maximal exact matches that follow from matching statistics (FmIndex.ms): P[e - len .. e) is one exactly when
    len > 0 and e is the pattern's end or the next record's len is no larger.  An FM_MEM array of those of at least min_len
    bytes, in the order FmIndex.smems returns.  numpy only"""
    length = np.ascontiguousarray(len, np.uint32).ravel()
    lo, hi = np.ascontiguousarray(lo, np.uint32).ravel(), np.ascontiguousarray(hi, np.uint32).ravel()
    offsets = np.asarray(offsets, np.int64).ravel()
    o0, o1 = (int(offsets[0]), int(offsets[-1])) if offsets.size else (0, 0)
    idx = np.arange(o0, o1, dtype=np.int64)
    pattern = np.searchsorted(offsets, idx, side="right") - 1        # the j with offsets[j] <= i < offsets[j + 1]
    last = idx + 1 == offsets[pattern + 1]
    nxt = np.zeros(idx.size, np.uint32)
    nxt[:-1] = length[o0 + 1:o1]
    here = length[o0:o1]
    keep = (here > 0) & (last | (nxt <= here)) & (here >= max(int(min_len), 1))
    out = np.zeros(int(keep.sum()), FM_MEM)
    end = (idx - offsets[pattern] + 1)[keep]
    out["lo"], out["hi"] = lo[o0:o1][keep], hi[o0:o1][keep]
    out["end"] = end
    out["start"] = end - here[keep]
    out["pattern"] = pattern[keep]
    return out


def repeat_stats(dev=0):
    """RepeatStats of the calling thread's last repeats call on dev"""
    return _last_stats(RepeatStats, "archon_hip_get_repeat_stats", dev)


def _repeats(call, count_only):
    """call(out pointer or None, cap, total pointer) -> rc: the count, or the repeats in an array of the size a first call gave"""
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    _check(call(None, 0, tp))
    if count_only:
        return total.value
    out = np.zeros(total.value, REPEAT)
    if total.value:
        _check(call(_p(out), out.size, tp))
    return out[:total.value]


def repeats(lcp, bwt, base_id, kind=1, min_len=1, min_occ=2, count_only=False, dev=0):
    """the repeats of a block from its LCP array and BWT (include/archon_hip.h: archon_hip_repeats): a REPEAT array in
    ascending representative row; kind 0 = every LCP interval, 1 = maximal, 2 = supermaximal.  count_only: their number"""
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
    if lcp.size != bwt.size:
        raise ValueError("repeats: lcp has %d rows, bwt %d" % (lcp.size, bwt.size))
    fn = lib().archon_hip_repeats
    return _repeats(lambda out, cap, tp: fn(_p(lcp), _p(bwt), bwt.size, int(base_id), int(kind), int(min_len), int(min_occ), out, cap, tp, dev),
                    count_only)


def lz_stats(dev=0):
    """LzStats of the calling thread's last LZ call on dev"""
    return _last_stats(LzStats, "archon_hip_get_lz_stats", dev)


def lpf(sa, lcp, dir=0, dev=0):
    """the longest previous factor of every item from the suffix array and its LCP array (include/archon_hip.h: archon_hip_lpf):
    an LPF array, the record of item s at index s - 1; dir 0 = copies end at earlier items, 1 = at later items"""
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    if sa.size != lcp.size:
        raise ValueError("lpf: sa has %d rows, lcp %d" % (sa.size, lcp.size))
    out = np.zeros(sa.size, LPF)
    _check(lib().archon_hip_lpf(_p(sa), _p(lcp), sa.size, int(dir), _p(out), dev))
    return out


def _phrases(call, count_only):
    """call(out pointer or None, cap, total pointer) -> rc: the count, or the phrases in an array of the size a first call gave"""
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    _check(call(None, 0, tp))
    if count_only:
        return total.value
    out = np.zeros(total.value, PHRASE)
    _check(call(_p(out), out.size, tp))
    return out[:total.value]


def lz_parse(lpf, count_only=False, dev=0):
    """the parse of an LPF array (archon_hip_lz_parse): a PHRASE array in chain order, the phrase ending at n first; only the len
    words decide the chain.  count_only: the number of phrases"""
    lpf = np.ascontiguousarray(lpf, dtype=LPF)
    fn = lib().archon_hip_lz_parse
    return _phrases(lambda out, cap, tp: fn(_p(lpf), lpf.size, out, cap, tp, dev), count_only)


def lz77(z, dev=0):
    """the textbook greedy LZ77 parse of z, left to right: an LZ77 array of (pos, len, src) -- the phrase starts at z[pos] and
    copies len bytes from z[src], src < pos, the two may overlap; len 0 is the literal z[pos].  The reversed text goes through a
    forward on a Block and Block.lz(dir=1)"""
    z = np.frombuffer(z, np.uint8) if isinstance(z, (bytes, bytearray)) else np.ascontiguousarray(z, dtype=np.uint8)
    n = z.size
    blk = Block(dev)
    try:
        blk.forward(z[::-1].copy(), want_sa=True)
        ph = blk.lz(dir=1)
    finally:
        blk.close()
    out = np.zeros(ph.size, LZ77)
    out["pos"] = n - ph["end"]
    out["len"] = ph["len"]
    out["src"] = np.where(ph["len"] > 0, n - ph["src"], 0)
    return out


def kmer_stats(dev=0):
    """KmerStats of the calling thread's last k-mer call (kmers, kmer_occ, sus) on dev"""
    return _last_stats(KmerStats, "archon_hip_get_kmer_stats", dev)


def _kmers(call, count_only, bins):
    """call(out pointer or None, cap, total pointer, hist pointer or None, bins) -> rc: the count, or the k-mers in an array of
    the size a first call gave; with bins the pair (that result, the histogram).  Both calls take the histogram, so that the
    call's record (kmer_stats) is that of the call the user made"""
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    hist = np.zeros(bins, np.uint32) if bins else None
    _check(call(None, 0, tp, _p(hist) if bins else None, bins))
    if count_only:
        got = total.value
    else:
        got = np.zeros(total.value, KMER)
        if total.value:
            _check(call(_p(got), got.size, tp, _p(hist) if bins else None, bins))
    return (got, hist) if bins else got


def _sa_lcp(what, sa, lcp):
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    if sa.size != lcp.size:
        raise ValueError("%s: sa has %d rows, lcp %d" % (what, sa.size, lcp.size))
    return sa, lcp


def kmers(sa, lcp, k, min_occ=1, max_occ=0, count_only=False, bins=0, dev=0):
    """the k-mers of a block from its suffix array and LCP array (include/archon_hip.h: archon_hip_kmers): a KMER array in
    ascending row, those with min_occ <= hi - lo <= max_occ (0: no limit), or their number with count_only; with bins the pair
    (that, hist): hist[c] = distinct k-mers with c occurrences, the last bin those with at least bins - 1 -- over ALL k-mers"""
    sa, lcp = _sa_lcp("kmers", sa, lcp)
    fn = lib().archon_hip_kmers
    return _kmers(lambda out, cap, tp, hp, nb: fn(_p(sa), _p(lcp), sa.size, int(k), int(min_occ), int(max_occ), out, cap, tp, hp, nb, dev),
                  count_only, int(bins))


def kmer_occ(sa, lcp, k, dev=0):
    """occ[p], p in 0 .. n-k: the number of occurrences of x[p .. p+k) in x (archon_hip_kmer_occ); empty when k > n"""
    sa, lcp = _sa_lcp("kmer_occ", sa, lcp)
    words = max(sa.size - int(k) + 1, 0)
    out = np.zeros(max(words, 1), np.uint32)
    _check(lib().archon_hip_kmer_occ(_p(sa), _p(lcp), sa.size, int(k), _p(out), dev))
    return out[:words]


def sus(sa, lcp, dev=0):
    """sus[e-1]: the length of the shortest substring ending at item e that occurs once, 0 when there is none (archon_hip_sus)"""
    sa, lcp = _sa_lcp("sus", sa, lcp)
    out = np.zeros(sa.size, np.uint32)
    _check(lib().archon_hip_sus(_p(sa), _p(lcp), sa.size, _p(out), dev))
    return out


def kmer_bytes(x, recs, k):
    """the bytes of KMER records of the block x: a uint8 array of recs.size rows of k bytes, x[item-k .. item) each (no device)"""
    x = np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)
    recs = np.ascontiguousarray(recs, KMER)
    k = int(k)
    if recs.size and (int(recs["item"].min()) < k or int(recs["item"].max()) > x.size):
        raise ValueError("kmer_bytes: an item outside %d..%d" % (k, x.size))
    return x[(recs["item"].astype(np.int64) - k)[:, None] + np.arange(k, dtype=np.int64)[None, :]]


def maw_stats(dev=0):
    """MawStats of the calling thread's last minimal-absent-words call on dev"""
    return _last_stats(MawStats, "archon_hip_maw_last_stats", dev)


def _maws(call, count_only):
    """call(out pointer or None, cap, total pointer) -> rc: the count, or the words in an array of the size a first call gave"""
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    _check(call(None, 0, tp))
    if count_only:
        return total.value
    out = np.zeros(total.value, MAW)
    if total.value:
        _check(call(_p(out), out.size, tp))
    return out[:total.value]


def maws(sa, lcp, bwt, base_id, min_len=2, max_len=0, count_only=False, dev=0):
    """the minimal absent words of a block from its suffix array, LCP array and BWT (include/archon_hip.h: archon_hip_maws): a MAW
    array in the rule's order, those with min_len <= len <= max_len (0: no limit), or their number with count_only"""
    sa, lcp = _sa_lcp("maws", sa, lcp)
    bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
    if bwt.size != sa.size:
        raise ValueError("maws: sa has %d rows, bwt %d" % (sa.size, bwt.size))
    fn = lib().archon_hip_maws
    return _maws(lambda out, cap, tp: fn(_p(sa), _p(lcp), _p(bwt), sa.size, int(base_id), int(min_len), int(max_len), out, cap, tp, dev), count_only)


def maw_bytes(x, rec):
    """the bytes of one MAW record of the block x: x[item-len+1 .. item) followed by `last` (no device)"""
    x = bytes(x) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8).tobytes()
    item, ln, last = int(rec["item"]), int(rec["len"]), int(rec["last"])
    if ln < 2 or item < ln - 1 or item > len(x) or last > 255:
        raise ValueError("maw_bytes: a record outside the block (item %d, len %d, last %d)" % (item, ln, last))
    return x[item - ln + 1:item] + bytes([last])


def entropy_stats(dev=0):
    """EntropyStats of the calling thread's last entropy or complexity call on dev"""
    return _last_stats(EntropyStats, "archon_hip_entropy_last_stats", dev)


def _orders(ks):
    """(the orders as a uint32 array, an ENTROPY array for their records)"""
    ks = np.ascontiguousarray(np.atleast_1d(ks), dtype=np.uint32)
    return ks, np.zeros(max(ks.size, 1), ENTROPY)


def entropy(sa, lcp, bwt, base_id, ks, dev=0):
    """the order-k statistics of a block from its suffix array, LCP array and BWT (include/archon_hip.h: archon_hip_entropy): an
    ENTROPY array, one record per order in ks (1 .. 64 of them), in that order; bits is n * H_k"""
    sa, lcp = _sa_lcp("entropy", sa, lcp)
    bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
    if bwt.size != sa.size:
        raise ValueError("entropy: sa has %d rows, bwt %d" % (sa.size, bwt.size))
    ks, out = _orders(ks)
    _check(lib().archon_hip_entropy(_p(sa), _p(lcp), _p(bwt), sa.size, int(base_id), _p(ks), ks.size, _p(out), dev))
    return out[:ks.size]


def complexity_len(n, max_len=0):
    """the lengths a complexity call covers: max_len 0 is min(n, 4095), more than n is n"""
    return min(int(max_len) or 4095, int(n))


def complexity(lcp, bwt=None, max_len=0, dev=0):
    """the substring complexity of a block from its LCP array and, with bwt, the runs of its BWT (include/archon_hip.h:
    archon_hip_complexity): (Complexity, counts) with counts[l-1] = the distinct substrings of length l, l = 1 .. max_len (0:
    min(n, 4095); more than n: n)"""
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    if bwt is not None:
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        if bwt.size != lcp.size:
            raise ValueError("complexity: lcp has %d rows, bwt %d" % (lcp.size, bwt.size))
    rec = Complexity()
    counts = np.zeros(max(complexity_len(lcp.size, max_len), 1), np.uint32)
    _check(lib().archon_hip_complexity(_p(lcp), _p(bwt) if bwt is not None else None, lcp.size, int(max_len), _p(counts), ctypes.byref(rec), dev))
    return rec, counts[:rec.max_len]


def run_stats(dev=0):
    """RunStats of the calling thread's last runs or LCE call on dev"""
    return _last_stats(RunStats, "archon_hip_runs_last_stats", dev)


def _pairs(what, s, t):
    s = np.ascontiguousarray(np.atleast_1d(s), dtype=np.uint32)
    t = np.ascontiguousarray(np.atleast_1d(t), dtype=np.uint32)
    if s.size != t.size:
        raise ValueError("%s: %d items s, %d items t" % (what, s.size, t.size))
    return s, t, np.zeros(max(s.size, 1), np.uint32)


def lce(sa, lcp, s, t, dev=0):
    """the longest common extensions of pairs of items from a block's suffix array and LCP array (include/archon_hip.h:
    archon_hip_lce): out[i] = the leading symbols the keys of items s[i] and t[i] (0 .. n) share, the longest common suffix of
    x[0..s) and x[0..t)"""
    sa, lcp = _sa_lcp("lce", sa, lcp)
    s, t, out = _pairs("lce", s, t)
    _check(lib().archon_hip_lce(_p(sa), _p(lcp), sa.size, _p(s), _p(t), s.size, _p(out), dev))
    return out[:s.size]


def _runs(call, count_only):
    """call(out pointer or None, cap, total pointer) -> rc: the count, or the runs in an array of the size a first call gave"""
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    _check(call(None, 0, tp))
    if count_only:
        return total.value
    out = np.zeros(total.value, RUN)
    if total.value:
        _check(call(_p(out), out.size, tp))
    return out[:total.value]


def runs(sa, lcp, sa_c, min_period=0, max_period=0, min_copies=2, min_len=0, count_only=False, dev=0):
    """the runs (maximal repetitions) of a block from its suffix array, its LCP array and the suffix array sa_c of the complemented
    block 255 - x (include/archon_hip.h: archon_hip_runs): a RUN array in ascending root, those with min_period <= period <=
    max_period (0: no limit), at least min_copies copies and min_len bytes, or their number with count_only"""
    sa, lcp = _sa_lcp("runs", sa, lcp)
    sa_c = np.ascontiguousarray(sa_c, dtype=np.uint32)
    if sa_c.size != sa.size:
        raise ValueError("runs: sa has %d rows, sa_c %d" % (sa.size, sa_c.size))
    fn = lib().archon_hip_runs
    return _runs(lambda out, cap, tp: fn(_p(sa), _p(lcp), _p(sa_c), sa.size, int(min_period), int(max_period), int(min_copies), int(min_len), out, cap,
                                         tp, dev), count_only)


def runs_of(x, min_period=0, max_period=0, min_copies=2, min_len=0, count_only=False, dev=0):
    """the runs of the block x: two forwards (x and its complement), one lcp, one runs call"""
    x = np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)
    sa = forward(x, True, dev)[0]
    sa_c = forward(255 - x, True, dev)[0]
    return runs(sa, lcp(x, sa, dev), sa_c, min_period, max_period, min_copies, min_len, count_only, dev)


def _kmers_as_mems(recs, k):
    """KMER records as the FM_MEM records the locate calls take: rows [lo, hi) of a piece of k bytes"""
    recs = np.ascontiguousarray(recs, KMER)
    mems = np.zeros(recs.size, FM_MEM)
    mems["lo"], mems["hi"], mems["end"] = recs["lo"], recs["hi"], int(k)
    return mems


def _as_mems(reps):
    """REPEAT records as the FM_MEM records the locate calls take: rows [lo, hi) of a piece of len bytes"""
    reps = np.ascontiguousarray(reps, REPEAT)
    mems = np.zeros(reps.size, FM_MEM)
    mems["lo"], mems["hi"], mems["end"] = reps["lo"], reps["hi"], reps["len"]
    return mems


def _locate_mems(fn, h, mems):
    """the starts of every SMEM's occurrences: a list of uint32 arrays, one per SMEM, each in row order"""
    mems = np.ascontiguousarray(mems, FM_MEM)
    cuts = np.zeros(mems.size + 1, np.int64)
    np.cumsum(mems["hi"].astype(np.int64) - mems["lo"], out=cuts[1:])
    pos = np.zeros(max(int(cuts[-1]), 1), np.uint32)
    total = ctypes.c_uint64(0)
    _check(fn(h, _p(mems) if mems.size else None, mems.size, _p(pos), int(cuts[-1]), ctypes.cast(ctypes.byref(total), ctypes.c_void_p)))
    return [pos[cuts[i]:cuts[i + 1]] for i in range(mems.size)]


def _approx(fn, h, patterns, k, hits):
    """(nhits, nocc, hits or None) of an approximate call: counting first, then the hits into an array of the size it gave"""
    packed, offsets = _pack_patterns(patterns)
    npat = offsets.size - 1
    nhits, nocc = np.zeros(npat, np.uint32), np.zeros(npat, np.uint32)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    if not hits:
        _check(fn(h, _p(packed), _p(offsets), npat, int(k), _p(nhits), _p(nocc), None, 0, tp))
        return nhits, nocc, None
    # one call when the hits fit a first guess, a second with the exact size when they do not
    out = np.zeros(max(4 * npat, 1), FM_HIT)
    rc = fn(h, _p(packed), _p(offsets), npat, int(k), _p(nhits), _p(nocc), _p(out), out.size, tp)
    if rc == E_ARG and total.value > out.size:
        out = np.zeros(total.value, FM_HIT)
        rc = fn(h, _p(packed), _p(offsets), npat, int(k), _p(nhits), _p(nocc), _p(out), out.size, tp)
    _check(rc)
    return nhits, nocc, out[:total.value]


def classes_identity():
    """the class table under which every byte accepts itself alone: a (256, 8) uint32 array, bit c of row b is word c >> 5,
    bit c & 31 (archon_hip_fm_classes)"""
    t = np.zeros((256, 8), np.uint32)
    b = np.arange(256)
    t[b, b >> 5] = np.uint32(1) << (b & 31).astype(np.uint32)
    return t


def classes_set(table, byte, accepted_bytes):
    """the table with the class of `byte` set to exactly accepted_bytes (a new array)"""
    t = np.array(table, np.uint32).reshape(256, 8)
    b = byte[0] if isinstance(byte, (bytes, bytearray)) else int(byte)
    t[b] = 0
    for c in accepted_bytes:            # bytes, or any iterable of values below 256
        t[b, int(c) >> 5] |= np.uint32(1 << (int(c) & 31))
    return t


def classes_fold_case():
    """the identity with every ASCII letter accepting both of its cases"""
    t = classes_identity()
    for lower in range(ord("a"), ord("z") + 1):
        both = bytes([lower, lower - 32])
        t = classes_set(classes_set(t, lower, both), lower - 32, both)
    return t


IUPAC = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def classes_iupac():
    """the identity with the 11 IUPAC ambiguity codes (upper case) accepting their bases among ACGT and not themselves"""
    t = classes_identity()
    for code, bases in IUPAC.items():
        t = classes_set(t, ord(code), bases.encode())
    return t


def _class_table(table):
    t = np.ascontiguousarray(table, np.uint32)
    if t.size != 256 * 8:
        raise ValueError("class table: %d words, not 256 x 8" % t.size)
    return t


def _classes(fn, h, patterns, table, hits):
    """(nhits, nocc, hits or None) of a class call, as _approx gives them"""
    t = _class_table(table)
    return _approx(lambda h_, pat, off, n, _k, *rest: fn(h_, pat, off, n, _p(t), *rest), h, patterns, 0, hits)


def _edit(fn, h, patterns, k, emit):
    """(nhits, hits or None) of an edit-distance call: the hits into an array of a first guess, then of the size the call gave"""
    packed, offsets = _pack_patterns(patterns)
    npat = offsets.size - 1
    nhits = np.zeros(npat, np.uint32)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    if not emit:
        _check(fn(h, _p(packed), _p(offsets), npat, int(k), _p(nhits), None, 0, tp))
        return nhits, None
    out = np.zeros(max(8 * npat, 1), FM_EDIT)
    rc = fn(h, _p(packed), _p(offsets), npat, int(k), _p(nhits), _p(out), out.size, tp)
    if rc == E_ARG and total.value > out.size:
        out = np.zeros(total.value, FM_EDIT)
        rc = fn(h, _p(packed), _p(offsets), npat, int(k), _p(nhits), _p(out), out.size, tp)
    _check(rc)
    return nhits, out[:total.value]


def _docs(call, k, emit):
    """(ndocs, records or None) of a documents call(ndocs, out, cap, total): the records into an array of a first guess, then of
    the size the call gave"""
    ndocs = np.zeros(max(k, 1), np.uint32)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    if not emit:
        _check(call(_p(ndocs), None, 0, tp))
        return ndocs[:k], None
    out = np.zeros(max(4 * k, 1), FM_DOC)
    rc = call(_p(ndocs), _p(out), out.size, tp)
    if rc == E_ARG and total.value > out.size:
        out = np.zeros(total.value, FM_DOC)
        rc = call(_p(ndocs), _p(out), out.size, tp)
    _check(rc)
    return ndocs[:k], out[:total.value]


def _win_queries(lo, hi, a, b, idx=None):
    """the queries of a window call as uint32 arrays of one length k (never of size 0: a pointer is always there) and k"""
    if (a is None) != (b is None):
        raise ValueError("window: a and b are both given or both None")
    arrs = [np.ascontiguousarray(v, dtype=np.uint32).ravel() if v is not None else None for v in (lo, hi, a, b, idx)]
    k = arrs[0].size
    if any(v is not None and v.size != k for v in arrs):
        raise ValueError("window: lo, hi, a, b and idx differ in length")
    return [(v if k else np.zeros(1, np.uint32)) if v is not None else None for v in arrs], k


def _tp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bounds(bounds):
    bounds = np.ascontiguousarray(bounds, dtype=np.uint32).ravel()
    if bounds.size < 1:
        raise ValueError("bounds: at least bounds[0]")
    return bounds


def _locate_hits(fn, h, patterns, hits):
    """the starts of every hit's occurrences: a list of uint32 arrays, one per hit, each in row order"""
    _, offsets = _pack_patterns(patterns)
    hits = np.ascontiguousarray(hits, FM_HIT)
    cuts = np.zeros(hits.size + 1, np.int64)
    np.cumsum(hits["hi"].astype(np.int64) - hits["lo"], out=cuts[1:])
    pos = np.zeros(max(int(cuts[-1]), 1), np.uint32)
    total = ctypes.c_uint64(0)
    _check(fn(h, _p(offsets), offsets.size - 1, _p(hits) if hits.size else None, hits.size, _p(pos), int(cuts[-1]),
              ctypes.cast(ctypes.byref(total), ctypes.c_void_p)))
    return [pos[cuts[i]:cuts[i + 1]] for i in range(hits.size)]


def _pack_patterns(patterns):
    """a list of bytes / uint8 arrays -> (packed bytes, uint32 offsets[k + 1])"""
    parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p, dtype=np.uint8).ravel()
             for p in patterns]
    offsets = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([q.size for q in parts], out=offsets[1:])
    if offsets[-1] > 0xFFFFFFFF:
        raise ValueError("patterns: more than 2^32 - 1 bytes in one call")
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return np.concatenate([packed, np.zeros(1, np.uint8)]), offsets.astype(np.uint32)


class FmIndex:
    """archon_hip_fm: the rank table of a BWT on the device (include/archon_hip.h).  count(patterns) -> (lo, hi), the rows
    [lo[j], hi[j]) of pattern j; hi - lo is its number of occurrences"""

    def __init__(self, bwt=None, base_id=0, dev=0, _handle=None):
        self.h = _handle
        self.dev = dev
        if self.h is None:
            bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
            h = ctypes.c_void_p(None)
            _check(lib().archon_hip_fm_create(_p(bwt), bwt.size, int(base_id), dev, ctypes.byref(h)))
            self.h = h
            self.n = bwt.size

    @classmethod
    def from_dev(cls, bwt_t, base_id):
        """from a torch uint8 tensor on the device, on the current stream"""
        dev = bwt_t.device.index or 0
        h = ctypes.c_void_p(None)
        _check(lib().archon_hip_fm_create_dev(ctypes.c_void_p(bwt_t.data_ptr()), bwt_t.numel(), int(base_id), dev, _stream_ptr(), ctypes.byref(h)))
        f = cls(dev=dev, _handle=h)
        f.n = bwt_t.numel()
        return f

    def count(self, patterns):
        packed, offsets = _pack_patterns(patterns)
        k = offsets.size - 1
        lo, hi = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        _check(lib().archon_hip_fm_count(self.h, _p(packed), _p(offsets), k, _p(lo), _p(hi)))
        return lo, hi

    def count_dev(self, patterns_t, offsets_t, lo_t, hi_t):
        """torch tensors on the device: patterns uint8, offsets int32[k + 1], lo and hi int32[k] (written); current stream"""
        _check(lib().archon_hip_fm_count_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), lo_t.numel(),
                                             ctypes.c_void_p(lo_t.data_ptr()), ctypes.c_void_p(hi_t.data_ptr()), _stream_ptr()))

    def sample(self, rate):
        """ISA / SA samples of rate `rate` (a power of two <= 65536) by the LF walk over the handle's BWT; returns self"""
        _check(lib().archon_hip_fm_sample(self.h, int(rate)))
        return self

    def samples(self):
        """the ISA samples: uint32 array, entry k the row of item k * rate"""
        cnt = ctypes.c_uint32(0)
        probe = np.zeros(1, np.uint32)
        rc = lib().archon_hip_fm_read_samples(self.h, _p(probe), 0, ctypes.cast(ctypes.byref(cnt), ctypes.c_void_p))
        if rc < 0 and cnt.value == 0:
            _check(rc)
        out = np.zeros(max(cnt.value, 1), np.uint32)
        _check(lib().archon_hip_fm_read_samples(self.h, _p(out), cnt.value, ctypes.cast(ctypes.byref(cnt), ctypes.c_void_p)))
        return out[:cnt.value]

    def locate(self, patterns):
        """the starts of every pattern's occurrences from the samples: a list of uint32 arrays, each in row order (the shape and
        order of Block.fm_locate)"""
        lo, hi = self.count(patterns)
        cuts = np.zeros(lo.size + 1, np.int64)
        np.cumsum(hi.astype(np.int64) - lo, out=cuts[1:])
        packed, offsets = _pack_patterns(patterns)
        pos = np.zeros(max(int(cuts[-1]), 1), np.uint32)
        total = ctypes.c_uint64(0)
        _check(lib().archon_hip_fm_locate(self.h, _p(packed), _p(offsets), lo.size, _p(pos), int(cuts[-1]),
                                          ctypes.cast(ctypes.byref(total), ctypes.c_void_p)))
        return [pos[cuts[j]:cuts[j + 1]] for j in range(lo.size)]

    def approx(self, patterns, k, hits=True):
        """every distinct string within k substituted bytes of each pattern: (nhits, nocc, hits), hits an FM_HIT array in the
        order of the header's rule (None with hits=False: counting only)"""
        return _approx(lib().archon_hip_fm_approx, self.h, patterns, k, hits)

    def approx_dev(self, patterns_t, offsets_t, k, nhits_t, nocc_t, hits_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[n + 1], nhits and nocc int32[n] (written), hits an int32
        tensor of 4 words per hit or None; current stream.  Returns the number of hits"""
        total = ctypes.c_uint64(0)
        cap = hits_t.numel() // 4 if hits_t is not None else 0
        _check(lib().archon_hip_fm_approx_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), nhits_t.numel(),
                                              int(k), ctypes.c_void_p(nhits_t.data_ptr()), ctypes.c_void_p(nocc_t.data_ptr()),
                                              ctypes.c_void_p(hits_t.data_ptr()) if hits_t is not None else None, cap,
                                              ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def classes(self, patterns, table, hits=True):
        """every distinct string of the block that lies in each pattern's classes under a (256, 8) class table (classes_identity,
        classes_fold_case, classes_iupac, classes_set): (nhits, nocc, hits), hits an FM_HIT array in ascending order of the
        strings (None with hits=False: counting only)"""
        return _classes(lib().archon_hip_fm_classes, self.h, patterns, table, hits)

    def classes_dev(self, patterns_t, offsets_t, table_t, nhits_t, nocc_t, hits_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[n + 1], the table int32[256 * 8], nhits and nocc int32[n]
        (written), hits an int32 tensor of 4 words per hit or None; current stream.  Returns the number of hits"""
        total = ctypes.c_uint64(0)
        cap = hits_t.numel() // 4 if hits_t is not None else 0
        _check(lib().archon_hip_fm_classes_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), nhits_t.numel(),
                                               ctypes.c_void_p(table_t.data_ptr()), ctypes.c_void_p(nhits_t.data_ptr()),
                                               ctypes.c_void_p(nocc_t.data_ptr()), ctypes.c_void_p(hits_t.data_ptr()) if hits_t is not None else None, cap,
                                               ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def locate_hits(self, patterns, hits):
        """the starts of every hit's occurrences from the samples (a list of uint32 arrays, one per hit, in the shape of locate)"""
        return _locate_hits(lib().archon_hip_fm_locate_hits, self.h, patterns, hits)

    def edit(self, patterns, k, emit=True):
        """every end in the block where a pattern matches with at most k substituted, inserted or deleted bytes: (nhits, hits),
        hits an FM_EDIT array, pattern by pattern and by ascending end (None with emit=False: counting only); needs samples"""
        return _edit(lib().archon_hip_fm_edit, self.h, patterns, k, emit)

    def edit_dev(self, patterns_t, offsets_t, k, nhits_t, hits_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[n + 1], nhits int32[n] (written), hits an int32 tensor of
        4 words per hit or None; current stream.  Returns the number of hits"""
        total = ctypes.c_uint64(0)
        cap = hits_t.numel() // 4 if hits_t is not None else 0
        _check(lib().archon_hip_fm_edit_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), nhits_t.numel(), int(k),
                                            ctypes.c_void_p(nhits_t.data_ptr()), ctypes.c_void_p(hits_t.data_ptr()) if hits_t is not None else None, cap,
                                            ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def mirror(self, text=None):
        """builds the mirror (the index of the reversed block) that smems() needs: from the handle's own BWT, or from the
        block's text -- a host uint8 array or a torch uint8 tensor on the device -- which saves the inverse; returns self"""
        if text is None:
            _check(lib().archon_hip_fm_mirror(self.h))
        elif hasattr(text, "data_ptr"):
            if text.numel() != self.n:
                raise ValueError("mirror: the text has %d bytes, the index %d" % (text.numel(), self.n))
            _check(lib().archon_hip_fm_mirror_dev(self.h, ctypes.c_void_p(text.data_ptr()), _stream_ptr()))
        else:
            import torch
            text = np.ascontiguousarray(text, dtype=np.uint8)
            if text.size != self.n:
                raise ValueError("mirror: the text has %d bytes, the index %d" % (text.size, self.n))
            t = torch.from_numpy(text).to("cuda:%d" % self.dev)
            _check(lib().archon_hip_fm_mirror_dev(self.h, ctypes.c_void_p(t.data_ptr()), _stream_ptr()))
        return self

    def read_mirror(self):
        """(bwt, base_id) of the mirror: the a7 transform of the reversed block"""
        out = np.zeros(max(self.n, 1), np.uint8)
        base = ctypes.c_uint32(0)
        _check(lib().archon_hip_fm_read_mirror(self.h, _p(out), self.n, ctypes.cast(ctypes.byref(base), ctypes.c_void_p)))
        return out[:self.n], base.value

    def smems(self, patterns, min_len=1, mems=True):
        """the super-maximal exact matches of every pattern: (nmems, nocc, mems), mems an FM_MEM array in the order of the
        header's procedure (None with mems=False: counting only).  Needs mirror()"""
        packed, offsets = _pack_patterns(patterns)
        npat = offsets.size - 1
        nmems, nocc = np.zeros(npat, np.uint32), np.zeros(npat, np.uint32)
        total = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        fn = lib().archon_hip_fm_smems
        if not mems:
            _check(fn(self.h, _p(packed), _p(offsets), npat, int(min_len), _p(nmems), _p(nocc), None, 0, tp))
            return nmems, nocc, None
        # one call when the SMEMs fit a first guess, a second with the exact size when they do not
        out = np.zeros(max(4 * npat, 1), FM_MEM)
        rc = fn(self.h, _p(packed), _p(offsets), npat, int(min_len), _p(nmems), _p(nocc), _p(out), out.size, tp)
        if rc == E_ARG and total.value > out.size:
            out = np.zeros(total.value, FM_MEM)
            rc = fn(self.h, _p(packed), _p(offsets), npat, int(min_len), _p(nmems), _p(nocc), _p(out), out.size, tp)
        _check(rc)
        return nmems, nocc, out[:total.value]

    def smems_dev(self, patterns_t, offsets_t, min_len, nmems_t, nocc_t, mems_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[k + 1], nmems and nocc int32[k] (written), mems an int32
        tensor of 6 words per SMEM or None; current stream.  Returns the number of SMEMs"""
        total = ctypes.c_uint64(0)
        cap = mems_t.numel() // 6 if mems_t is not None else 0
        _check(lib().archon_hip_fm_smems_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), nmems_t.numel(),
                                             int(min_len), ctypes.c_void_p(nmems_t.data_ptr()), ctypes.c_void_p(nocc_t.data_ptr()),
                                             ctypes.c_void_p(mems_t.data_ptr()) if mems_t is not None else None, cap,
                                             ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def attach_lcp(self, lcp):
        """attaches the block's LCP array (uint32[n], host) that ms() needs: copied into the handle, a minimum hierarchy built
        behind it; replaces an earlier one; returns self"""
        lcp = np.ascontiguousarray(lcp, dtype=np.uint32).ravel()
        if lcp.size != self.n:
            raise ValueError("attach_lcp: the array has %d entries, the index %d" % (lcp.size, self.n))
        _check(lib().archon_hip_fm_attach_lcp(self.h, _p(lcp)))
        return self

    def attach_lcp_dev(self, ptr, stream=None):
        """the same from n words on the device: a raw device pointer (or a torch int32 tensor), on `stream` (a raw HIP stream;
        None: the current torch stream); returns self"""
        if hasattr(ptr, "data_ptr"):
            if ptr.numel() != self.n:
                raise ValueError("attach_lcp_dev: the array has %d entries, the index %d" % (ptr.numel(), self.n))
            ptr = ptr.data_ptr()
        _check(lib().archon_hip_fm_attach_lcp_dev(self.h, ctypes.c_void_p(int(ptr)), _stream_ptr() if stream is None else ctypes.c_void_p(stream)))
        return self

    def ms(self, patterns, rows=True):
        """the matching statistics of every pattern: (len, lo, hi, offsets), uint32 arrays with the record of end e of pattern j
        at offsets[j] + e - 1: the longest piece ending there that occurs in the block, and its rows [lo, hi) (both None with
        rows=False).  Needs attach_lcp()"""
        packed, offsets = _pack_patterns(patterns)
        k = offsets.size - 1
        total = max(int(offsets[-1]), 1)
        length = np.zeros(total, np.uint32)
        lo, hi = (np.zeros(total, np.uint32), np.zeros(total, np.uint32)) if rows else (None, None)
        _check(lib().archon_hip_fm_ms(self.h, _p(packed), _p(offsets), k, _p(length), _p(lo) if rows else None, _p(hi) if rows else None))
        t = int(offsets[-1])
        return length[:t], (lo[:t] if rows else None), (hi[:t] if rows else None), offsets

    def ms_dev(self, patterns_t, offsets_t, len_t, lo_t=None, hi_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[k + 1], len and (both or neither) lo and hi int32 of
        offsets[k] words (written); current stream"""
        _check(lib().archon_hip_fm_ms_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()),
                                          offsets_t.numel() - 1, ctypes.c_void_p(len_t.data_ptr()),
                                          ctypes.c_void_p(lo_t.data_ptr()) if lo_t is not None else None,
                                          ctypes.c_void_p(hi_t.data_ptr()) if hi_t is not None else None, _stream_ptr()))

    def attach_sa(self, sa):
        """attaches the block's suffix array (uint32[n], host, values 1 .. n) that ms_text() and rlz() need beside attach_lcp():
        copied into the handle with its inverse behind it; replaces an earlier one; returns self"""
        sa = np.ascontiguousarray(sa, dtype=np.uint32).ravel()
        if sa.size != self.n:
            raise ValueError("attach_sa: the array has %d entries, the index %d" % (sa.size, self.n))
        _check(lib().archon_hip_fm_attach_sa(self.h, _p(sa)))
        return self

    def attach_sa_dev(self, ptr, stream=None):
        """the same from n words on the device: a raw device pointer (or a torch int32 tensor), on `stream` (a raw HIP stream;
        None: the current torch stream); returns self"""
        if hasattr(ptr, "data_ptr"):
            if ptr.numel() != self.n:
                raise ValueError("attach_sa_dev: the array has %d entries, the index %d" % (ptr.numel(), self.n))
            ptr = ptr.data_ptr()
        _check(lib().archon_hip_fm_attach_sa_dev(self.h, ctypes.c_void_p(int(ptr)), _stream_ptr() if stream is None else ctypes.c_void_p(stream)))
        return self

    def ms_text(self, text, rows=True):
        """the matching statistics of ONE long text, spread over the device: (len, lo, hi), uint32 arrays with the record of end
        e at e - 1, exactly what ms([text]) gives (lo and hi None with rows=False).  Needs attach_lcp() and attach_sa()"""
        text = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8).ravel()
        m = text.size
        text = np.concatenate([text, np.zeros(1, np.uint8)])
        length = np.zeros(max(m, 1), np.uint32)
        lo, hi = (np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)) if rows else (None, None)
        _check(lib().archon_hip_fm_ms_text(self.h, _p(text), m, _p(length), _p(lo) if rows else None, _p(hi) if rows else None))
        return length[:m], (lo[:m] if rows else None), (hi[:m] if rows else None)

    def ms_text_dev(self, text_t, len_t, lo_t=None, hi_t=None):
        """torch tensors on the device: text uint8[m], len and (both or neither) lo and hi int32[m] (written); current stream"""
        _check(lib().archon_hip_fm_ms_text_dev(self.h, ctypes.c_void_p(text_t.data_ptr()), text_t.numel(), ctypes.c_void_p(len_t.data_ptr()),
                                               ctypes.c_void_p(lo_t.data_ptr()) if lo_t is not None else None,
                                               ctypes.c_void_p(hi_t.data_ptr()) if hi_t is not None else None, _stream_ptr()))

    def rlz(self, text, count_only=False):
        """the relative LZ parse of a text against the block, greedy from the right: a PHRASE array in chain order, the phrase
        ending at m first; (end, len, src) says text[end-len .. end) = x[src-len .. src), len 0 is the literal text[end-1].
        count_only: the number of phrases.  Without count_only the text is parsed twice: once for the count, once with room for
        the phrases.  Needs attach_lcp() and attach_sa()"""
        text = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8).ravel()
        m = text.size
        text = np.concatenate([text, np.zeros(1, np.uint8)])
        fn = lib().archon_hip_fm_rlz
        return _phrases(lambda out, cap, tp: fn(self.h, _p(text), m, out, cap, tp), count_only)

    def rlz_dev(self, text_t, out_t=None):
        """torch tensors on the device: text uint8[m], out an int32 tensor of 3 words per phrase or None (counting only); on the
        current stream.  Returns the number of phrases (raises when out_t holds fewer)"""
        total = ctypes.c_uint64(0)
        cap = out_t.numel() // 3 if out_t is not None else 0
        _check(lib().archon_hip_fm_rlz_dev(self.h, ctypes.c_void_p(text_t.data_ptr()), text_t.numel(),
                                           ctypes.c_void_p(out_t.data_ptr()) if out_t is not None else None, cap,
                                           ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def attach_docs(self, bounds):
        """cuts the block into documents (uint32 bounds[D + 1], 0 = bounds[0] < ... < bounds[D] = n) for docs(), docs_ranges()
        and doc_of(): 12 n + 4 (D + 1) bytes on the device.  Needs attach_sa(); replaces an earlier one; returns self"""
        bounds = _bounds(bounds)
        _check(lib().archon_hip_fm_attach_docs(self.h, _p(bounds), bounds.size - 1))
        return self

    def attach_docs_dev(self, bounds_t, stream=None):
        """the same from a torch int32 tensor of D + 1 words on the device, on `stream` (a raw HIP stream; None: the current torch
        stream); returns self"""
        _check(lib().archon_hip_fm_attach_docs_dev(self.h, ctypes.c_void_p(bounds_t.data_ptr()), bounds_t.numel() - 1,
                                                   _stream_ptr() if stream is None else ctypes.c_void_p(stream)))
        return self

    def docs(self, patterns, emit=True):
        """the documents that hold each pattern: (ndocs, records), ndocs[j] the distinct documents of pattern j, records an FM_DOC
        array pattern by pattern and by ascending first row (None with emit=False: document frequencies only).  An occurrence
        belongs to the document of its LAST byte.  Needs attach_docs()"""
        packed, offsets = _pack_patterns(patterns)
        k = offsets.size - 1
        fn = lib().archon_hip_fm_docs
        return _docs(lambda nd, out, cap, tp: fn(self.h, _p(packed), _p(offsets), k, nd, out, cap, tp), k, emit)

    def docs_dev(self, patterns_t, offsets_t, ndocs_t, docs_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[k + 1], ndocs int32[k] (written), docs an int32 tensor of
        4 words per record or None; current stream.  Returns the number of records"""
        total = ctypes.c_uint64(0)
        cap = docs_t.numel() // 4 if docs_t is not None else 0
        _check(lib().archon_hip_fm_docs_dev(self.h, ctypes.c_void_p(patterns_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), ndocs_t.numel(),
                                            ctypes.c_void_p(ndocs_t.data_ptr()), ctypes.c_void_p(docs_t.data_ptr()) if docs_t is not None else None, cap,
                                            ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def docs_ranges(self, lo, hi, emit=True):
        """the documents of the row ranges [lo[j], hi[j]) -- a count's, or the lo and hi of SMEMs, hits or repeats: (ndocs, records)
        as docs()"""
        lo = np.ascontiguousarray(lo, dtype=np.uint32).ravel()
        hi = np.ascontiguousarray(hi, dtype=np.uint32).ravel()
        if lo.size != hi.size:
            raise ValueError("docs_ranges: %d lo and %d hi" % (lo.size, hi.size))
        k = lo.size
        lo_, hi_ = (lo, hi) if k else (np.zeros(1, np.uint32), np.zeros(1, np.uint32))
        fn = lib().archon_hip_fm_docs_ranges
        return _docs(lambda nd, out, cap, tp: fn(self.h, _p(lo_), _p(hi_), k, nd, out, cap, tp), k, emit)

    def docs_ranges_dev(self, lo_t, hi_t, ndocs_t, docs_t=None):
        """torch int32 tensors on the device: lo and hi [k], ndocs [k] (written), docs 4 words per record or None; current stream.
        Returns the number of records"""
        total = ctypes.c_uint64(0)
        cap = docs_t.numel() // 4 if docs_t is not None else 0
        _check(lib().archon_hip_fm_docs_ranges_dev(self.h, ctypes.c_void_p(lo_t.data_ptr()), ctypes.c_void_p(hi_t.data_ptr()), lo_t.numel(),
                                                   ctypes.c_void_p(ndocs_t.data_ptr()), ctypes.c_void_p(docs_t.data_ptr()) if docs_t is not None else None,
                                                   cap, ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def doc_of(self, items, offsets=True):
        """(doc, off) of items in 1 .. n -- what locate() returns plus the pattern's length, or a start p as p + 1: the document
        that holds byte items - 1 and the byte's offset in it (off None with offsets=False)"""
        items = np.ascontiguousarray(items, dtype=np.uint32).ravel()
        doc = np.zeros(max(items.size, 1), np.uint32)
        off = np.zeros(max(items.size, 1), np.uint32) if offsets else None
        _check(lib().archon_hip_fm_doc_of(self.h, _p(items) if items.size else None, items.size, _p(doc), _p(off) if offsets else None))
        return doc[:items.size], (off[:items.size] if offsets else None)

    def attach_wm(self):
        """builds the wavelet matrix over the attached suffix array for win_count(), win_select(), win_list(), first() and
        locate_sorted(): about bits(n) * (n/8 + n/64) bytes on the device.  Needs attach_sa(); replaces an earlier one; returns self"""
        _check(lib().archon_hip_fm_attach_wm(self.h))
        return self

    def win_count(self, lo, hi, a=None, b=None):
        """count[j] = how many rows r of [lo[j], hi[j]) have a[j] <= sa[r] < b[j] (a and b None: all of them).  Needs attach_wm()"""
        (lo, hi, a, b, _), k = _win_queries(lo, hi, a, b)
        count = np.zeros(max(k, 1), np.uint32)
        _check(lib().archon_hip_fm_win_count(self.h, _p(lo), _p(hi), _p(a) if a is not None else None, _p(b) if b is not None else None, k, _p(count)))
        return count[:k]

    def win_count_dev(self, lo_t, hi_t, count_t, a_t=None, b_t=None):
        """torch int32 tensors on the device: lo, hi [k], a, b [k] or None, count [k] (written); current stream"""
        _check(lib().archon_hip_fm_win_count_dev(self.h, _tp(lo_t), _tp(hi_t), _tp(a_t), _tp(b_t), lo_t.numel(), _tp(count_t), _stream_ptr()))

    def win_select(self, lo, hi, idx, a=None, b=None):
        """item[j] = the idx[j]-th smallest sa[r] (0-based) of the rows of [lo[j], hi[j]) with a[j] <= sa[r] < b[j], 0 when there
        are idx[j] of them or fewer"""
        (lo, hi, a, b, idx), k = _win_queries(lo, hi, a, b, idx)
        item = np.zeros(max(k, 1), np.uint32)
        _check(lib().archon_hip_fm_win_select(self.h, _p(lo), _p(hi), _p(a) if a is not None else None, _p(b) if b is not None else None, _p(idx), k,
                                              _p(item)))
        return item[:k]

    def win_select_dev(self, lo_t, hi_t, idx_t, item_t, a_t=None, b_t=None):
        """torch int32 tensors on the device: lo, hi, idx [k], a, b [k] or None, item [k] (written); current stream"""
        _check(lib().archon_hip_fm_win_select_dev(self.h, _tp(lo_t), _tp(hi_t), _tp(a_t), _tp(b_t), _tp(idx_t), lo_t.numel(), _tp(item_t),
                                                  _stream_ptr()))

    def win_list(self, lo, hi, a=None, b=None, most=0, emit=True):
        """(count, records): count[j] the size of window j, records an FM_WIN array with the min(count[j], most) smallest items of
        every window (most 0: all), range by range and ascending within a range (None with emit=False: counts only)"""
        (lo, hi, a, b, _), k = _win_queries(lo, hi, a, b)
        count = np.zeros(max(k, 1), np.uint32)
        total = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        fn = lib().archon_hip_fm_win_list
        call = lambda out, cap: fn(self.h, _p(lo), _p(hi), _p(a) if a is not None else None, _p(b) if b is not None else None, k, int(most),  # noqa: E731
                                   _p(count), out, cap, tp)
        if not emit:
            _check(call(None, 0))
            return count[:k], None
        out = np.zeros(max(4 * k, 1), FM_WIN)
        rc = call(_p(out), out.size)
        if rc == E_ARG and total.value > out.size:
            out = np.zeros(total.value, FM_WIN)
            rc = call(_p(out), out.size)
        _check(rc)
        return count[:k], out[:total.value]

    def win_list_dev(self, lo_t, hi_t, count_t, out_t=None, a_t=None, b_t=None, most=0):
        """torch int32 tensors on the device: lo, hi [k], a, b [k] or None, count [k] (written), out 2 words per record or None;
        current stream.  Returns the number of records"""
        total = ctypes.c_uint64(0)
        cap = out_t.numel() // 2 if out_t is not None else 0
        _check(lib().archon_hip_fm_win_list_dev(self.h, _tp(lo_t), _tp(hi_t), _tp(a_t), _tp(b_t), lo_t.numel(), int(most), _tp(count_t), _tp(out_t), cap,
                                                ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def count_ranges(self, patterns):
        """count() as valid row ranges: a pattern that does not occur has an empty range wherever it lies, here [0, 0)"""
        lo, hi = self.count(patterns)
        occurs = lo < hi
        return np.where(occurs, lo, 0).astype(np.uint32), np.where(occurs, hi, 0).astype(np.uint32)

    def first(self, patterns, after=0):
        """the first start of every pattern at or after `after`, -1 when there is none: an int64 array.  The count, then select 0
        with a = after + m"""
        _, offsets = _pack_patterns(patterns)
        m = np.diff(offsets.astype(np.int64))
        lo, hi = self.count_ranges(patterns)
        a = np.minimum(int(after) + m, self.n + 1).astype(np.uint32)
        b = np.full(lo.size, self.n + 1, np.uint32)
        item = self.win_select(lo, hi, np.zeros(lo.size, np.uint32), a, b).astype(np.int64)
        return np.where(item > 0, item - m, -1)

    def locate_sorted(self, patterns, most=0):
        """the starts of every pattern's occurrences in ascending order, the first `most` of them (0: all): a list of uint32
        arrays -- sorted(locate()) without the locate"""
        _, offsets = _pack_patterns(patterns)
        m = np.diff(offsets.astype(np.int64))
        lo, hi = self.count_ranges(patterns)
        count, recs = self.win_list(lo, hi, most=most)
        cuts = np.zeros(lo.size + 1, np.int64)
        np.cumsum(np.minimum(count, most) if most else count, out=cuts[1:])
        starts = (recs["item"].astype(np.int64) - m[recs["range"]]).astype(np.uint32)
        return [starts[cuts[j]:cuts[j + 1]] for j in range(lo.size)]

    def attach_ends(self, ends):
        """marks where the documents of the block end (uint32 ends[D], 1 <= ends[0] < ... < ends[D-1] <= n; ends_from_bounds) for
        overlaps(): 256 ceil(12 D / 256) + 256 ceil(4 (9 ceil(n / 256) + 1) / 256) bytes on the device, about 0.14 n + 12 D.
        Needs attach_sa(); replaces earlier ends; returns self"""
        ends = np.ascontiguousarray(ends, dtype=np.uint32).ravel()
        _check(lib().archon_hip_fm_attach_ends(self.h, _p(ends) if ends.size else None, ends.size))
        return self

    def attach_ends_dev(self, ends_t, stream=None):
        """the same from a torch int32 tensor of D words on the device, on `stream` (a raw HIP stream; None: the current torch
        stream); returns self"""
        _check(lib().archon_hip_fm_attach_ends_dev(self.h, ctypes.c_void_p(ends_t.data_ptr()), ends_t.numel(),
                                                   _stream_ptr() if stream is None else ctypes.c_void_p(stream)))
        return self

    def overlaps(self, patterns, min_len, emit=True):
        """the suffix-prefix overlaps of every pattern with the documents: (novl, records), novl[j] the overlaps of pattern j,
        records an FM_OVL array pattern by pattern, by ascending length and by ascending end row (None with emit=False: counts
        only).  A record says that document `doc` ends with the first `len` >= min_len bytes of the pattern.  Needs attach_ends()"""
        packed, offsets = _pack_patterns(patterns)
        k = offsets.size - 1
        novl = np.zeros(max(k, 1), np.uint32)
        total = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        fn = lib().archon_hip_fm_overlaps
        call = lambda out, cap: fn(self.h, _p(packed), _p(offsets), k, int(min_len), _p(novl), out, cap, tp)  # noqa: E731
        if not emit:
            _check(call(None, 0))
            return novl[:k], None
        out = np.zeros(max(4 * k, 1), FM_OVL)
        rc = call(_p(out), out.size)
        if rc == E_ARG and total.value > out.size:
            out = np.zeros(total.value, FM_OVL)
            rc = call(_p(out), out.size)
        _check(rc)
        return novl[:k], out[:total.value]

    def overlaps_dev(self, patterns_t, offsets_t, min_len, novl_t, ovl_t=None):
        """torch tensors on the device: patterns uint8, offsets int32[k + 1], novl int32[k] (written), ovl an int32 tensor of 4
        words per record or None; current stream.  Returns the number of records"""
        total = ctypes.c_uint64(0)
        cap = ovl_t.numel() // 4 if ovl_t is not None else 0
        _check(lib().archon_hip_fm_overlaps_dev(self.h, _tp(patterns_t), _tp(offsets_t), novl_t.numel(), int(min_len), _tp(novl_t), _tp(ovl_t), cap,
                                                ctypes.cast(ctypes.byref(total), ctypes.c_void_p), _stream_ptr()))
        return total.value

    def locate_mems(self, mems):
        """the starts of every SMEM's occurrences from the samples (a list of uint32 arrays, one per SMEM, each in row order)"""
        return _locate_mems(lib().archon_hip_fm_locate_mems, self.h, mems)

    def locate_repeats(self, reps):
        """the starts of every repeat's occurrences (REPEAT records of the block this index was made from) from the samples: a
        list of uint32 arrays, one per repeat, each in row order"""
        return _locate_mems(lib().archon_hip_fm_locate_mems, self.h, _as_mems(reps))

    def locate_kmers(self, recs, k):
        """the starts of every k-mer's occurrences (KMER records of the block this index was made from) from the samples: a list
        of uint32 arrays, one per k-mer, each in row order"""
        return _locate_mems(lib().archon_hip_fm_locate_mems, self.h, _kmers_as_mems(recs, k))

    def extract(self, starts, lengths):
        """x[starts[j] .. starts[j] + lengths[j]) for every j: a list of uint8 arrays"""
        starts = np.ascontiguousarray(starts, dtype=np.uint32).ravel()
        lengths = np.asarray(lengths, dtype=np.uint64).ravel()
        offsets = np.zeros(starts.size + 1, np.uint64)
        np.cumsum(lengths, out=offsets[1:])
        if offsets[-1] > 0xFFFFFFFF:
            raise ValueError("extract: more than 2^32 - 1 bytes in one call")
        offsets = offsets.astype(np.uint32)
        out = np.zeros(max(int(offsets[-1]), 1), np.uint8)
        _check(lib().archon_hip_fm_extract(self.h, _p(starts), _p(offsets), starts.size, _p(out)))
        return [out[offsets[j]:offsets[j + 1]] for j in range(starts.size)]

    def extract_dev(self, starts_t, offsets_t, out_t):
        """torch tensors on the device: starts int32[k], offsets int32[k + 1], out uint8 (written at offsets[j]); current stream"""
        _check(lib().archon_hip_fm_extract_dev(self.h, ctypes.c_void_p(starts_t.data_ptr()), ctypes.c_void_p(offsets_t.data_ptr()), starts_t.numel(),
                                               ctypes.c_void_p(out_t.data_ptr()), _stream_ptr()))

    def close(self):
        if self.h:
            lib().archon_hip_fm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def radix_scatter(src, dev=0):
    src = np.ascontiguousarray(src, dtype=np.uint8)
    dst = np.empty_like(src)
    _check(lib().archon_hip_radix_scatter(_p(src), src.size, _p(dst), dev))
    return dst


def stats(dev=0):
    return stats_raw(dev).asdict()


def stats_raw(dev=0):
    """the Stats structure itself (asdict() later): what a timed loop takes per step"""
    s = Stats()
    _check(_lib.archon_hip_get_stats(dev, ctypes.byref(s)) if _lib is not None else lib().archon_hip_get_stats(dev, ctypes.byref(s)))
    return s


def reserve(n, dev=0):
    b = ctypes.c_size_t(0)
    _check(lib().archon_hip_reserve(n, dev, ctypes.cast(ctypes.byref(b), ctypes.c_void_p)))
    return b.value


def set_option(name, value, dev=0):
    """product option of a device (include/archon_hip.h: "pass_ranges", "pass_b_buckets")"""
    _check(lib().archon_hip_set_option(dev, name.encode(), int(value)))


def get_option(name, dev=0):
    v = ctypes.c_long(0)
    _check(lib().archon_hip_get_option(dev, name.encode(), ctypes.byref(v)))
    return int(v.value)


def bind_context(slot, dev=0):
    _check(lib().archon_hip_bind_context(dev, slot))


def context_of_thread(dev=0):
    return _check(lib().archon_hip_context_of_thread(dev))


class Block:
    """archon_hip_block: the device side of one block-coder object (x, SA and BWT resident between compute, validate, write)"""

    def __init__(self, dev=0):
        h = ctypes.c_void_p(None)
        _check(lib().archon_hip_block_create(dev, ctypes.byref(h)))
        self.h = h
        self.dev = dev

    def close(self):
        if self.h:
            lib().archon_hip_block_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, x, want_sa=True):
        x = np.ascontiguousarray(x, dtype=np.uint8)
        self.n = x.size
        sa = np.empty(x.size, dtype=np.uint32) if want_sa else None
        base = ctypes.c_uint32(0)
        _check(lib().archon_hip_block_forward(self.h, _p(x), x.size, _p(sa) if want_sa else None,
                                              ctypes.cast(ctypes.byref(base), ctypes.c_void_p)))
        return sa, base.value

    def read_bwt(self, offset=0, length=None):
        length = self.n - offset if length is None else length
        out = np.empty(length, dtype=np.uint8)
        _check(lib().archon_hip_block_read_bwt(self.h, offset, length, _p(out)))
        return out

    def validate(self):
        return bool(_check(lib().archon_hip_block_validate(self.h)))

    def lcp(self):
        """the LCP array of the resident block's suffix array (needs forward(want_sa=True))"""
        out = np.empty(self.n, np.uint32)
        _check(lib().archon_hip_block_lcp(self.h, _p(out)))
        return out

    def fm_count(self, patterns):
        """(lo, hi) of every pattern in the resident block's BWT (the FM index is built on the first call after a forward)"""
        packed, offsets = _pack_patterns(patterns)
        k = offsets.size - 1
        lo, hi = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        _check(lib().archon_hip_block_fm_count(self.h, _p(packed), _p(offsets), k, _p(lo), _p(hi)))
        return lo, hi

    def fm_locate(self, patterns):
        """the starts of every pattern's occurrences: a list of uint32 arrays, each in row order (not sorted); needs
        forward(want_sa=True)"""
        lo, hi = self.fm_count(patterns)
        cuts = np.zeros(lo.size + 1, np.int64)
        np.cumsum(hi.astype(np.int64) - lo, out=cuts[1:])
        packed, offsets = _pack_patterns(patterns)
        pos = np.zeros(max(int(cuts[-1]), 1), np.uint32)
        total = ctypes.c_uint64(0)
        _check(lib().archon_hip_block_fm_locate(self.h, _p(packed), _p(offsets), lo.size, _p(pos), int(cuts[-1]),
                                                ctypes.cast(ctypes.byref(total), ctypes.c_void_p)))
        return [pos[cuts[j]:cuts[j + 1]] for j in range(lo.size)]

    def fm_approx(self, patterns, k, hits=True):
        """FmIndex.approx on the resident block's BWT (its FM index built on the first FM call after a forward)"""
        return _approx(lib().archon_hip_block_fm_approx, self.h, patterns, k, hits)

    def fm_classes(self, patterns, table, hits=True):
        """FmIndex.classes on the resident block's BWT (its FM index built on the first FM call after a forward)"""
        return _classes(lib().archon_hip_block_fm_classes, self.h, patterns, table, hits)

    def fm_edit(self, patterns, k, emit=True):
        """FmIndex.edit on the resident block: its text and the suffix array of its last forward (want_sa=True)"""
        return _edit(lib().archon_hip_block_fm_edit, self.h, patterns, k, emit)

    def fm_locate_hits(self, patterns, hits):
        """the starts of every hit's occurrences from the resident SA (needs forward(want_sa=True)): a list of uint32 arrays"""
        return _locate_hits(lib().archon_hip_block_fm_locate_hits, self.h, patterns, hits)

    def fm_locate_mems(self, mems):
        """the starts of every SMEM's occurrences from the resident SA (needs forward(want_sa=True)): a list of uint32 arrays"""
        return _locate_mems(lib().archon_hip_block_fm_locate_mems, self.h, mems)

    def repeats(self, kind=1, min_len=1, min_occ=2, count_only=False):
        """the repeats of the resident block (needs forward(want_sa=True)): its LCP array is made and consumed on the device.
        A REPEAT array in ascending representative row, or their number with count_only"""
        fn = lib().archon_hip_block_repeats
        return _repeats(lambda out, cap, tp: fn(self.h, int(kind), int(min_len), int(min_occ), out, cap, tp), count_only)

    def locate_repeats(self, reps):
        """the starts of every repeat's occurrences from the resident SA: a list of uint32 arrays, one per repeat, in row order"""
        return _locate_mems(lib().archon_hip_block_fm_locate_mems, self.h, _as_mems(reps))

    def kmers(self, k, min_occ=1, max_occ=0, count_only=False, bins=0):
        """the k-mers of the resident block (needs forward(want_sa=True)): its LCP array is made and consumed on the device.
        A KMER array in ascending row, or their number with count_only; with bins the pair (that, the histogram of ALL k-mers)"""
        fn = lib().archon_hip_block_kmers
        return _kmers(lambda out, cap, tp, hp, nb: fn(self.h, int(k), int(min_occ), int(max_occ), out, cap, tp, hp, nb), count_only, int(bins))

    def kmer_occ(self, k):
        """occ[p], p in 0 .. n-k: the number of occurrences of x[p .. p+k) in the resident block (needs forward(want_sa=True))"""
        words = max(self.n - int(k) + 1, 0)
        out = np.zeros(max(words, 1), np.uint32)
        _check(lib().archon_hip_block_kmer_occ(self.h, int(k), _p(out)))
        return out[:words]

    def sus(self):
        """sus[e-1]: the length of the shortest substring ending at item e of the resident block that occurs once, 0 when there
        is none (needs forward(want_sa=True))"""
        out = np.zeros(self.n, np.uint32)
        _check(lib().archon_hip_block_sus(self.h, _p(out)))
        return out

    def locate_kmers(self, recs, k):
        """the starts of every k-mer's occurrences from the resident SA: a list of uint32 arrays, one per k-mer, in row order"""
        return _locate_mems(lib().archon_hip_block_fm_locate_mems, self.h, _kmers_as_mems(recs, k))

    def maws(self, min_len=2, max_len=0, count_only=False):
        """the minimal absent words of the resident block (needs forward(want_sa=True)): its LCP array is made and consumed on
        the device, the rank table is the block's own (built here when no FM call has).  A MAW array in the rule's order, those
        with min_len <= len <= max_len (0: no limit), or their number with count_only"""
        fn = lib().archon_hip_block_maws
        return _maws(lambda out, cap, tp: fn(self.h, int(min_len), int(max_len), out, cap, tp), count_only)

    def lce(self, s, t):
        """the longest common extensions of pairs of items of the resident block (needs forward(want_sa=True)): out[i] = the
        longest common suffix of x[0..s[i]) and x[0..t[i])"""
        s, t, out = _pairs("Block.lce", s, t)
        _check(lib().archon_hip_block_lce(self.h, _p(s), _p(t), s.size, _p(out)))
        return out[:s.size]

    def runs(self, min_period=0, max_period=0, min_copies=2, min_len=0, count_only=False):
        """the runs of the resident block (needs forward(want_sa=True)): the complemented block is sorted on the device beside
        the resident one, which stays as it is; the LCP array is made and consumed on the device.  A RUN array in ascending root,
        or the number of runs with count_only.  Without count_only the block is taken twice: once for the count, once with room
        for the records"""
        fn = lib().archon_hip_block_runs
        return _runs(lambda out, cap, tp: fn(self.h, int(min_period), int(max_period), int(min_copies), int(min_len), out, cap, tp), count_only)

    def entropy(self, ks):
        """the order-k statistics of the resident block (needs forward(want_sa=True)): its LCP array is made and consumed on the
        device, the rank table is the block's own (built here when no FM call has).  An ENTROPY array, one record per order"""
        ks, out = _orders(ks)
        _check(lib().archon_hip_block_entropy(self.h, _p(ks), ks.size, _p(out)))
        return out[:ks.size]

    def complexity(self, max_len=0):
        """the substring complexity of the resident block and the runs of its BWT (needs forward(want_sa=True)): (Complexity,
        counts) with counts[l-1] = the distinct substrings of length l, l = 1 .. max_len (0: min(n, 4095); more than n: n)"""
        rec = Complexity()
        counts = np.zeros(max(complexity_len(self.n, max_len), 1), np.uint32)
        _check(lib().archon_hip_block_complexity(self.h, int(max_len), _p(counts), ctypes.byref(rec)))
        return rec, counts[:rec.max_len]

    def lz(self, dir=0, want_lpf=False, count_only=False):
        """the LZ77 parse of the resident block (needs forward(want_sa=True)): its LCP array and its LPF records are made and
        consumed on the device.  A PHRASE array in chain order (the phrase ending at n first), or the number of phrases with
        count_only; with want_lpf a pair (the LPF array, that result).  Without count_only the block is parsed twice: once
        for the count, once with room for the phrases"""
        fn = lib().archon_hip_block_lz
        rec = np.zeros(self.n, LPF) if want_lpf else None
        got = _phrases(lambda out, cap, tp: fn(self.h, int(dir), _p(rec) if rec is not None and out is None else None, out, cap, tp), count_only)
        return (rec, got) if want_lpf else got

    def fm_index(self, rate, mirror=False, sa=False, docs=None, wm=False, ends=None, lcp=False):
        """a standalone sampled FmIndex of the last forward's BWT (samples from the SA when that forward kept one, else by the
        LF walk); it outlives later forwards and close().  mirror=True: with its mirror, built from the resident block.
        lcp=True: with the block's LCP array attached (needs forward(want_sa=True)); the array is made on the device.
        sa=True: with the block's suffix array attached, device to device (needs forward(want_sa=True)).
        docs=bounds: cut into documents (FmIndex.attach_docs) from the resident suffix array (needs forward(want_sa=True)).
        wm=True: with the wavelet matrix (FmIndex.attach_wm) built from the resident suffix array (needs forward(want_sa=True)).
        ends=ends: with the documents' ends (FmIndex.attach_ends) from the resident suffix array (needs forward(want_sa=True))"""
        h = ctypes.c_void_p(None)
        _check(lib().archon_hip_block_fm_index(self.h, int(rate), ctypes.byref(h)))
        f = FmIndex(_handle=h)
        f.n = self.n
        f.dev = self.dev
        if mirror:
            _check(lib().archon_hip_block_fm_mirror(self.h, f.h))
        if lcp:
            _check(lib().archon_hip_block_fm_attach_lcp(self.h, f.h))
        if sa:
            _check(lib().archon_hip_block_fm_attach_sa(self.h, f.h))
        if docs is not None:
            bounds = _bounds(docs)
            _check(lib().archon_hip_block_fm_attach_docs(self.h, f.h, _p(bounds), bounds.size - 1))
        if wm:
            _check(lib().archon_hip_block_fm_attach_wm(self.h, f.h))
        if ends is not None:
            ends = np.ascontiguousarray(ends, dtype=np.uint32).ravel()
            _check(lib().archon_hip_block_fm_attach_ends(self.h, f.h, _p(ends) if ends.size else None, ends.size))
        return f

    def stats(self):
        s = Stats()
        _check(lib().archon_hip_block_stats(self.h, ctypes.byref(s)))
        return s.asdict()


# ---------------------------------------------------------------- device resident (torch)
def _stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def forward_dev(x_t, sa_t, bwt_t, base_t):
    """torch CUDA tensors: x uint8[n], sa int32[n] or None, bwt uint8[n], base int32[1]."""
    dev = x_t.device.index or 0
    _check(lib().archon_hip_forward_dev(ctypes.c_void_p(x_t.data_ptr()), x_t.numel(),
                                        ctypes.c_void_p(sa_t.data_ptr()) if sa_t is not None else None,
                                        ctypes.c_void_p(bwt_t.data_ptr()), ctypes.c_void_p(base_t.data_ptr()),
                                        dev, _stream_ptr()))


def inverse_dev(bwt_t, base_id, out_t):
    dev = bwt_t.device.index or 0
    _check(lib().archon_hip_inverse_dev(ctypes.c_void_p(bwt_t.data_ptr()), bwt_t.numel(), int(base_id),
                                        ctypes.c_void_p(out_t.data_ptr()), dev, _stream_ptr()))


def hist256_dev(x_t, out_t):
    dev = x_t.device.index or 0
    _check(lib().archon_hip_hist256_dev(ctypes.c_void_p(x_t.data_ptr()), x_t.numel(),
                                        ctypes.c_void_p(out_t.data_ptr()), dev, _stream_ptr()))


def validate_dev(x_t, sa_t):
    """True if and only if sa_t is the a7 suffix array of x_t (include/archon_hip.h: archon_hip_validate)"""
    dev = x_t.device.index or 0
    return bool(_check(lib().archon_hip_validate_dev(ctypes.c_void_p(x_t.data_ptr()), x_t.numel(),
                                                     ctypes.c_void_p(sa_t.data_ptr()), dev, _stream_ptr())))


def lcp_dev(x_t, sa_t, lcp_t):
    """torch CUDA tensors: x uint8[n], sa int32[n], lcp int32[n] (written; must not overlap x or sa), on the current stream"""
    dev = x_t.device.index or 0
    _check(lib().archon_hip_lcp_dev(ctypes.c_void_p(x_t.data_ptr()), x_t.numel(), ctypes.c_void_p(sa_t.data_ptr()),
                                    ctypes.c_void_p(lcp_t.data_ptr()), dev, _stream_ptr()))


def repeats_dev(lcp_t, bwt_t, base_id, kind=1, min_len=1, min_occ=2, out_t=None):
    """torch CUDA tensors: lcp int32[n], bwt uint8[n], out an int32 tensor of 4 words per repeat or None (counting only); on the
    current stream.  Returns the number of repeats (raises when out_t holds fewer)"""
    dev = lcp_t.device.index or 0
    total = ctypes.c_uint64(0)
    cap = out_t.numel() // 4 if out_t is not None else 0
    _check(lib().archon_hip_repeats_dev(ctypes.c_void_p(lcp_t.data_ptr()), ctypes.c_void_p(bwt_t.data_ptr()), bwt_t.numel(), int(base_id), int(kind),
                                        int(min_len), int(min_occ), ctypes.c_void_p(out_t.data_ptr()) if out_t is not None else None, cap,
                                        ctypes.cast(ctypes.byref(total), ctypes.c_void_p), dev, _stream_ptr()))
    return total.value


def lpf_dev(sa_t, lcp_t, dir, lpf_t):
    """torch CUDA tensors: sa and lcp int32[n], lpf an int32 tensor of 2 words per item (8-byte aligned); on the current stream"""
    dev = sa_t.device.index or 0
    _check(lib().archon_hip_lpf_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), sa_t.numel(), int(dir),
                                    ctypes.c_void_p(lpf_t.data_ptr()), dev, _stream_ptr()))


def lz_parse_dev(lpf_t, out_t=None):
    """torch CUDA tensors: lpf an int32 tensor of 2 words per item, out an int32 tensor of 3 words per phrase or None (counting
    only); on the current stream.  Returns the number of phrases (raises when out_t holds fewer)"""
    dev = lpf_t.device.index or 0
    total = ctypes.c_uint64(0)
    cap = out_t.numel() // 3 if out_t is not None else 0
    _check(lib().archon_hip_lz_parse_dev(ctypes.c_void_p(lpf_t.data_ptr()), lpf_t.numel() // 2, ctypes.c_void_p(out_t.data_ptr()) if out_t is not None else None,
                                         cap, ctypes.cast(ctypes.byref(total), ctypes.c_void_p), dev, _stream_ptr()))
    return total.value


def kmers_dev(sa_t, lcp_t, k, min_occ=1, max_occ=0, out_t=None, hist_t=None):
    """torch CUDA tensors: sa and lcp int32[n], out an int32 tensor of 3 words per k-mer or None (counting only), hist an int32
    tensor of 2 .. 4096 bins or None; on the current stream.  Returns the number of k-mers (raises when out_t holds fewer)"""
    dev = sa_t.device.index or 0
    total = ctypes.c_uint64(0)
    cap = out_t.numel() // 3 if out_t is not None else 0
    _check(lib().archon_hip_kmers_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), sa_t.numel(), int(k), int(min_occ), int(max_occ),
                                      ctypes.c_void_p(out_t.data_ptr()) if out_t is not None else None, cap, ctypes.cast(ctypes.byref(total), ctypes.c_void_p),
                                      ctypes.c_void_p(hist_t.data_ptr()) if hist_t is not None else None, hist_t.numel() if hist_t is not None else 0,
                                      dev, _stream_ptr()))
    return total.value


def kmer_occ_dev(sa_t, lcp_t, k, occ_t):
    """torch CUDA tensors: sa and lcp int32[n], occ int32[n - k + 1] (written); on the current stream"""
    dev = sa_t.device.index or 0
    _check(lib().archon_hip_kmer_occ_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), sa_t.numel(), int(k),
                                         ctypes.c_void_p(occ_t.data_ptr()), dev, _stream_ptr()))


def sus_dev(sa_t, lcp_t, sus_t):
    """torch CUDA tensors: sa and lcp int32[n], sus int32[n] (written); on the current stream"""
    dev = sa_t.device.index or 0
    _check(lib().archon_hip_sus_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), sa_t.numel(), ctypes.c_void_p(sus_t.data_ptr()),
                                    dev, _stream_ptr()))


def maws_dev(sa_t, lcp_t, bwt_t, base_id, min_len=2, max_len=0, out_t=None):
    """torch CUDA tensors: sa and lcp int32[n], bwt uint8[n], out an int32 tensor of 5 words per word or None (counting only); on
    the current stream.  Returns the number of minimal absent words (raises when out_t holds fewer)"""
    dev = sa_t.device.index or 0
    total = ctypes.c_uint64(0)
    cap = out_t.numel() // 5 if out_t is not None else 0
    _check(lib().archon_hip_maws_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), ctypes.c_void_p(bwt_t.data_ptr()), sa_t.numel(),
                                     int(base_id), int(min_len), int(max_len), ctypes.c_void_p(out_t.data_ptr()) if out_t is not None else None, cap,
                                     ctypes.cast(ctypes.byref(total), ctypes.c_void_p), dev, _stream_ptr()))
    return total.value


def lce_dev(sa_t, lcp_t, s_t, t_t, out_t):
    """torch CUDA tensors: sa and lcp int32[n], items s and t int32[k], out int32[k] (written); on the current stream"""
    dev = sa_t.device.index or 0
    _check(lib().archon_hip_lce_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), sa_t.numel(), ctypes.c_void_p(s_t.data_ptr()),
                                    ctypes.c_void_p(t_t.data_ptr()), s_t.numel(), ctypes.c_void_p(out_t.data_ptr()), dev, _stream_ptr()))


def runs_dev(sa_t, lcp_t, sa_c_t, min_period=0, max_period=0, min_copies=2, min_len=0, out_t=None):
    """torch CUDA tensors: sa, lcp and sa_c int32[n], out an int32 tensor of 4 words per run or None (counting only); on the current
    stream.  Returns the number of runs (raises when out_t holds fewer)"""
    dev = sa_t.device.index or 0
    total = ctypes.c_uint64(0)
    cap = out_t.numel() // 4 if out_t is not None else 0
    _check(lib().archon_hip_runs_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), ctypes.c_void_p(sa_c_t.data_ptr()), sa_t.numel(),
                                     int(min_period), int(max_period), int(min_copies), int(min_len),
                                     ctypes.c_void_p(out_t.data_ptr()) if out_t is not None else None, cap,
                                     ctypes.cast(ctypes.byref(total), ctypes.c_void_p), dev, _stream_ptr()))
    return total.value


def entropy_dev(sa_t, lcp_t, bwt_t, base_id, ks):
    """torch CUDA tensors: sa and lcp int32[n], bwt uint8[n]; ks on the host; on the current stream.  An ENTROPY array, one record
    per order"""
    dev = sa_t.device.index or 0
    ks, out = _orders(ks)
    _check(lib().archon_hip_entropy_dev(ctypes.c_void_p(sa_t.data_ptr()), ctypes.c_void_p(lcp_t.data_ptr()), ctypes.c_void_p(bwt_t.data_ptr()), sa_t.numel(),
                                        int(base_id), _p(ks), ks.size, _p(out), dev, _stream_ptr()))
    return out[:ks.size]


def complexity_dev(lcp_t, bwt_t=None, max_len=0, counts_t=None):
    """torch CUDA tensors: lcp int32[n], bwt uint8[n] or None, counts an int32 tensor of at least complexity_len(n, max_len) words or
    None; on the current stream.  Returns the Complexity record"""
    dev = lcp_t.device.index or 0
    if counts_t is not None and counts_t.numel() < complexity_len(lcp_t.numel(), max_len):
        raise ValueError("complexity_dev: counts holds %d words, the call writes %d" % (counts_t.numel(), complexity_len(lcp_t.numel(), max_len)))
    rec = Complexity()
    _check(lib().archon_hip_complexity_dev(ctypes.c_void_p(lcp_t.data_ptr()), ctypes.c_void_p(bwt_t.data_ptr()) if bwt_t is not None else None, lcp_t.numel(),
                                           int(max_len), ctypes.c_void_p(counts_t.data_ptr()) if counts_t is not None else None, ctypes.byref(rec), dev,
                                           _stream_ptr()))
    return rec


def validate_resident_dev(x_t, sa_t, bwt_t, base_id):
    """Archon::validate on the outputs of a forward pass that are still on the device: True if and only if sa_t is the a7
    suffix array of x_t, bwt_t its BWT (bwt_t[i] == x_t[sa_t[i]], x_t[0] where sa_t[i] == n, compared row by row) and
    base_id its primary index"""
    dev = x_t.device.index or 0
    return bool(_check(lib().archon_hip_validate_resident_dev(ctypes.c_void_p(x_t.data_ptr()), x_t.numel(), ctypes.c_void_p(sa_t.data_ptr()),
                                                              ctypes.c_void_p(bwt_t.data_ptr()), int(base_id), dev, _stream_ptr())))


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def forward_batch(blocks, dev=0, workers=0):
    """several small blocks per call (archon_hip_forward_batch): list of uint8 arrays -> list of (bwt, base_id)"""
    xs = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
    outs = [np.empty(b.size, np.uint8) for b in xs]
    ns = (ctypes.c_uint32 * len(xs))(*[b.size for b in xs])
    base = (ctypes.c_uint32 * len(xs))()
    _check(lib().archon_hip_forward_batch(_ptr_array([b.ctypes.data for b in xs]), ns, len(xs), _ptr_array([o.ctypes.data for o in outs]), base, dev, workers))
    return [(o, int(base[i])) for i, o in enumerate(outs)]


def inverse_batch(bwts, bases, dev=0, workers=0):
    bs = [np.ascontiguousarray(b, dtype=np.uint8) for b in bwts]
    outs = [np.empty(b.size, np.uint8) for b in bs]
    ns = (ctypes.c_uint32 * len(bs))(*[b.size for b in bs])
    base = (ctypes.c_uint32 * len(bs))(*[int(v) for v in bases])
    _check(lib().archon_hip_inverse_batch(_ptr_array([b.ctypes.data for b in bs]), ns, base, len(bs), _ptr_array([o.ctypes.data for o in outs]), dev, workers))
    return outs


def forward_batch_dev(x_ts, bwt_ts, base_ts, sa_ts=None, workers=0):
    dev = x_ts[0].device.index or 0
    ns = (ctypes.c_uint32 * len(x_ts))(*[t.numel() for t in x_ts])
    sa = _ptr_array([t.data_ptr() if t is not None else None for t in sa_ts]) if sa_ts is not None else None
    _check(lib().archon_hip_forward_batch_dev(_ptr_array([t.data_ptr() for t in x_ts]), ns, len(x_ts), sa, _ptr_array([t.data_ptr() for t in bwt_ts]),
                                              _ptr_array([t.data_ptr() for t in base_ts]), dev, workers))


def inverse_batch_dev(bwt_ts, bases, out_ts, workers=0):
    dev = bwt_ts[0].device.index or 0
    ns = (ctypes.c_uint32 * len(bwt_ts))(*[t.numel() for t in bwt_ts])
    base = (ctypes.c_uint32 * len(bwt_ts))(*[int(v) for v in bases])
    _check(lib().archon_hip_inverse_batch_dev(_ptr_array([t.data_ptr() for t in bwt_ts]), ns, base, len(bwt_ts), _ptr_array([t.data_ptr() for t in out_ts]), dev, workers))


def post_decode_dev(stream_t, nbytes, bwt_t):
    """a block's stream of the post stage on the device -> its BWT on the device; returns the block's length"""
    dev = stream_t.device.index or 0
    n = ctypes.c_uint32(0)
    _check(lib().archon_hip_post_decode_dev(ctypes.c_void_p(stream_t.data_ptr()), int(nbytes), ctypes.c_void_p(bwt_t.data_ptr()), bwt_t.numel(),
                                            ctypes.cast(ctypes.byref(n), ctypes.c_void_p), dev, _stream_ptr()))
    return int(n.value)


def inverse_post(stream, base_id, cap, dev=0):
    """host stream of the post stage + primary index -> the block (decoded and inverted on the device)"""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    out = np.empty(cap, dtype=np.uint8)
    n = ctypes.c_uint32(0)
    _check(lib().archon_hip_inverse_post(_p(stream), stream.size, int(base_id), _p(out), cap, ctypes.cast(ctypes.byref(n), ctypes.c_void_p), dev))
    return out[:n.value]
