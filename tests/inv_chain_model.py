"""A plain numpy / Python model of the inverse's cut (dark-archon_amd/csrc/inverse.hiph, "A9: lf_walk"), and the table of
inputs and geometries the inverse's tests run.

The walk cuts the LF cycle of a block at one pseudo-random row per 2^sbits rows, plus row `base`, into sub-chains; each is
stored in a slab of `slab_bytes`, the chains longer than their slab are walked again.  Which chain lengths an input has at a
geometry decides which branches of k_walk_store / k_walk_queue / k_walk_rows / k_chain_copy / k_walk_emit it executes -- and
nothing the library reports says so.  This model does: `chains` gives (len, next) of every chain id, `route` names the
kernel the driver picks, and `EDGES` states the conditions ("a chain of exactly slab_bytes symbols") as predicates.

`CASES` is the one table of (input, geometry, edges): tests/test_inv_chain_model.py proves on the CPU that every edge a case
lists occurs in its input (the census), tests/test_gpu_inverse.py runs the cases on the GPU.  A new walk variant, slab rule
or row flush gets a row here, with the edges it exists for.

No GPU, nothing of the oracle: `emit` is itself an inverse, and test_inv_chain_model.py holds it against oracle.inverse.
"""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dark-archon_amd", "csrc")

NIL = 0xFFFFFFFF
_M32 = 0xFFFFFFFF
HASH_MUL = 0x9E3779B1
SALT_MUL = 0x85EBCA6B


# ---------------------------------------------------------------- the LF table and the walk
def lf_table(bwt, base):
    """T of k_lf_chunk: rows in a stable order by byte, row `base` moved behind its whole bucket; T[order[r]] = r"""
    bwt = np.ascontiguousarray(bwt, np.uint8)
    n = bwt.size
    order = np.argsort(bwt, kind="stable")
    sym = int(bwt[base])
    lo, hi = np.searchsorted(bwt[order], [sym, sym + 1])
    bucket = order[lo:hi]
    order[lo:hi] = np.concatenate([bucket[bucket != base], [base]])
    T = np.empty(n, np.int64)
    T[order] = np.arange(n)
    return T


def bucket_starts(bwt):
    """starts[0..256]: first row of every byte's bucket, starts[256] = n"""
    s = np.zeros(257, np.int64)
    np.cumsum(np.bincount(np.ascontiguousarray(bwt, np.uint8), minlength=256), out=s[1:])
    return s


def walk_order(T, base):
    """the rows in the order the walk visits them: seq[i] = T^(i+1)(base).  One cycle over all rows ends at seq[n-1] = base"""
    t = T.tolist()
    seq = [0] * len(t)
    k = base
    for i in range(len(t)):
        k = t[k]
        seq[i] = k
    return np.array(seq, np.int64)


def emit(bwt, base):
    """the text the walk produces: the bucket of each visited row (the symbol is never read from bwt[])"""
    bwt = np.ascontiguousarray(bwt, np.uint8)
    seq = walk_order(lf_table(bwt, base), base)
    return (np.searchsorted(bucket_starts(bwt), seq, side="right") - 1).astype(np.uint8)


# ---------------------------------------------------------------- the cut (32-bit arithmetic, as on the device)
def cut_row(j, n, sbits, salt=0):
    """the head row of region j (inv::cut_row); j may be an array"""
    j = np.asarray(j, np.uint64)
    h = ((j ^ np.uint64(salt & _M32)) * np.uint64(HASH_MUL)) & np.uint64(_M32)
    h ^= h >> np.uint64(15)
    r = ((j << np.uint64(sbits)) & np.uint64(_M32)) + (h & np.uint64((1 << sbits) - 1))
    r = np.where(r < n, r, n - 1).astype(np.int64)
    return int(r) if r.ndim == 0 else r


def cut_row_unclamped(j, sbits, salt=0):
    h = ((j ^ (salt & _M32)) * HASH_MUL) & _M32
    h ^= h >> 15
    return ((j << sbits) & _M32) + (h & ((1 << sbits) - 1))


def salt_of(attempt):
    return (attempt * SALT_MUL) & _M32


def head_id(k, n, base, sbits, salt=0):
    """chain id of row k if k is a head, else NIL; id nreg is the extra head at `base` (inv::head_id)"""
    j = k >> sbits
    if cut_row(j, n, sbits, salt) == k:
        return j
    if k == base:
        return -(-n >> sbits)
    return NIL


def head_row(j, n, base, sbits, salt=0):
    nreg = -(-n >> sbits)
    return cut_row(j, n, sbits, salt) if j < nreg else base


Chains = collections.namedtuple("Chains", "len next start nchains nreg base_on_head")


def chains(bwt, base, sbits, salt=0, order=None):
    """One walk of the single cycle from `base`: per chain id the number of symbols (`len`), the id of the chain that follows
    (`next`; NIL and len 0 for the unused slot) and the output position of its first symbol (`start`); nchains = ceil(n /
    2^sbits) + 1; base_on_head = row `base` is its region's cut row (then id nreg is the unused slot).
    order: walk_order of the input, when the caller holds it already."""
    n = len(bwt)
    if order is None:
        order = walk_order(lf_table(bwt, base), base)
    assert order[-1] == base and np.unique(order).size == n, "the LF permutation is not one cycle: not a BWT"
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)                      # pos[base] = n - 1
    nreg = -(-n >> sbits)
    nchains = nreg + 1
    heads = cut_row(np.arange(nreg), n, sbits, salt)
    assert np.unique(heads).size == nreg
    base_on_head = bool(heads[base >> sbits] == base)
    ids = np.arange(nreg) if base_on_head else np.arange(nchains)
    rows = heads if base_on_head else np.concatenate([heads, [base]])
    o = np.argsort(pos[rows])
    p, ids = pos[rows][o], ids[o]                  # heads in walk order; the last one is at row `base`
    assert p[-1] == n - 1
    ln = np.zeros(nchains, np.int64)
    nx = np.full(nchains, NIL, np.int64)
    st = np.zeros(nchains, np.int64)
    # the chain of head i holds the rows behind it up to and including the next head
    ln[ids[:-1]] = p[1:] - p[:-1]
    nx[ids[:-1]] = ids[1:]
    st[ids[:-1]] = p[:-1] + 1
    ln[ids[-1]] = p[0] + 1
    nx[ids[-1]] = ids[0]
    st[ids[-1]] = 0
    return Chains(ln, nx, st, nchains, nreg, base_on_head)


# ---------------------------------------------------------------- the driver's choices
def num_cu():
    """kNumCU of common.hiph"""
    src = open(os.path.join(CSRC, "common.hiph")).read()
    return int(re.search(r"constexpr\s+int\s+kNumCU\s*=\s*(\d+)\s*;", src).group(1))


def inv_sbits(n, forced=-1):
    """log2 rows per chain head (inv_sbits of inverse.hiph): the product's rule, or INV_SBITS; clamped to 3..12 either way"""
    lg = n.bit_length() - 1
    sb = min(lg - 18 - (lg >= 25) - (lg >= 27), 8)
    if forced >= 0:
        sb = forced
    return max(3, min(12, sb))


def nchains_of(n, sbits):
    """one chain per 2^sbits rows, and the one from row `base`"""
    return -(-n >> sbits) + 1


def rank_rounds(nchains):
    """launches of k_rank_jump: the span a word covers grows fourfold per launch"""
    rounds, span = 0, 1
    while span < nchains:
        span *= 4
        rounds += 1
    return rounds


def inverse_launches(nchains):
    """kernel_launches of an inverse whose first cut closes: the LF build's three, the walk, the ranking's rounds, and
    k_rank_init + k_chain_copy + k_walk_emit"""
    return 3 + 1 + rank_rounds(nchains) + 3


Route = collections.namedtuple("Route", "kernel slab_bytes per_cu")
# bytes a lane collects before it stores: k_walk_store 8, k_walk_queue 16, k_walk_rows one row
STORE_UNIT = {"walk_store": 8, "walk_queue": 16, "walk_rows64": 64, "walk_rows128": 128}


def route(n, sbits, inv_rows=-1, inv_slab=0, walk_wgs=-1, num_cu=256):
    """The walk kernel inverse_run launches, its slab_bytes and its workgroups per CU (0 for k_walk_store, which takes one
    chain per lane).  The library does not report the route, so it is derived: this mirrors, line by line, the slab rule
    and the if / else-if chain over `rows`, `per_cu` and `nchains >= kNumCU * 64` in inverse_run (inverse.hiph), and must
    move with them.  inv_rows, inv_slab, walk_wgs: the test routes INV_ROWS, INV_SLAB, INV_WALK_WGS (-1 / 0 / -1: unset)."""
    nchains = -(-n >> sbits) + 1
    slab_bytes = 16 << sbits
    if inv_slab:
        v = inv_slab & ~15
        if 16 <= v < slab_bytes:
            slab_bytes = v
    per_cu = 3 if walk_wgs < 0 else walk_wgs
    inv_rows = -1 if inv_rows < 0 else 1 if inv_rows > 2 else inv_rows          # (archon_hip_test_route)
    rows = ((inv_rows > 0 or (inv_rows < 0 and n > (128 << 20))) and slab_bytes % 64 == 0
            and (nchains + 1) * (slab_bytes >> 4) < 0x80000000)
    big = nchains >= num_cu * 64
    if per_cu != 0 and big and rows and (inv_rows == 2 or slab_bytes % 128):
        return Route("walk_rows64", slab_bytes, per_cu)
    if per_cu != 0 and big and rows:
        return Route("walk_rows128", slab_bytes, min(per_cu, 2))
    if per_cu == 0 or not big:
        return Route("walk_store", slab_bytes, 0)
    return Route("walk_queue", slab_bytes, per_cu)


def route_of_env(n, env):
    """(sbits, Route) of a block of n rows under a case's ARCHON_INV_* variables"""
    g = lambda k, d: int(env.get("ARCHON_" + k, d))          # (pyarchon hands ARCHON_<NAME> to archon_hip_test_route)
    sbits = inv_sbits(n, g("INV_SBITS", -1))
    return sbits, route(n, sbits, g("INV_ROWS", -1), g("INV_SLAB", 0), g("INV_WALK_WGS", -1), num_cu())


# ---------------------------------------------------------------- the edges
def copy_reads_past_slab(ch, slab_bytes, out_offset=0, only=None):
    """chains whose k_chain_copy reads its fifth word behind the chain's own slab: with `head` bytes up to the output's first
    16-byte boundary and nq 16-byte stores, the last store reads words (head >> 2) + 4 nq - 4 .. + 4 nq of the slab"""
    L = ch.len if only is None else ch.len[only:only + 1]
    st = ch.start if only is None else ch.start[only:only + 1]
    head = np.minimum((-(out_offset + st)) & 15, L)
    nq = (L - head) >> 4
    return (L > 0) & (L <= slab_bytes) & (nq > 0) & (4 * ((head >> 2) + 4 * nq) >= slab_bytes)


def _mult(m):
    return lambda c: bool(((c.ch.len > 0) & (c.ch.len % m == 0) & (c.ch.len < c.slab)).any())


Ctx = collections.namedtuple("Ctx", "ch n base sbits salt slab unit out_offset")

# name -> predicate over a Ctx.  `unit` = STORE_UNIT of the case's kernel
EDGES = {
    # the last store / row of the slab is written, k_chain_copy takes the whole slab, k_walk_emit must skip the chain
    "exact_slab": lambda c: bool((c.ch.len == c.slab).any()),
    # stored up to the slab, measured one symbol further, walked again by k_walk_emit
    "slab_plus_one": lambda c: bool((c.ch.len == c.slab + 1).any()),
    # k_walk_emit's 8-byte stores: a chain that outgrows its slab by more than a word
    "over_slab": lambda c: bool((c.ch.len > c.slab + 16).any()),
    # a chain in its slab that takes several stores of the kernel (k_walk_rows: a full row flushed, then on in the same slab)
    "multi_row": lambda c: bool(((c.ch.len > c.unit) & (c.ch.len <= c.slab)).any()),
    # a chain that ends exactly on a store boundary below the slab: `done` and a full row at once, no tail store
    "ends_on_row": lambda c: bool(((c.ch.len > 0) & (c.ch.len % c.unit == 0) & (c.ch.len < c.slab)).any()),
    "len_mult_16": _mult(16), "len_mult_64": _mult(64), "len_mult_128": _mult(128),
    "len_one": lambda c: bool((c.ch.len == 1).any()),
    # row `base` is its region's cut row: id nreg is the unused slot (next = NIL, len = 0)
    "base_on_head": lambda c: c.ch.base_on_head and c.ch.len[c.ch.nreg] == 0 and c.ch.next[c.ch.nreg] == NIL,
    "base_off_head": lambda c: not c.ch.base_on_head and c.ch.len[c.ch.nreg] > 0,
    # the last region's hashed row lies behind the block and is clamped to n - 1
    "clamped_last_head": lambda c: cut_row_unclamped(c.ch.nreg - 1, c.sbits, c.salt) >= c.n and cut_row(c.ch.nreg - 1, c.n, c.sbits, c.salt) == c.n - 1,
    "base_zero": lambda c: c.base == 0,
    "base_last": lambda c: c.base == c.n - 1,
    # k_chain_copy's fifth word lies behind the chain's slab (in the next chain's) -- and behind the LAST chain's slab
    "copy_reads_next_slab": lambda c: bool(copy_reads_past_slab(c.ch, c.slab, c.out_offset).any()),
    "copy_reads_past_last_slab": lambda c: bool(copy_reads_past_slab(c.ch, c.slab, c.out_offset, only=c.ch.nchains - 1).any()),
}


# ---------------------------------------------------------------- inputs and cases
# name -> (shape, n, block[, tail]) : archon_synth.gen_shape(shape, n, block), its last bytes replaced by `tail`.  Lengths and
# tails were chosen by running this model over candidates (odd lengths 2^20 + 1 .. 2^20 + 63 for the two large ones), not
# guessed; tests/test_inv_chain_model.py proves what each is listed for.
INPUTS = {
    # 2^20 + odd rows: sbits <= 6 still gives >= 16384 chains, which the queue and rows walks need
    "text_1m": ("text", (1 << 20) + 51, 0),          # base on its region's cut row at sbits 4; last cut row clamped at sbits 4
    "dna_1m": ("dna", (1 << 20) + 49, 0),            # base on its region's cut row at sbits 5; last cut row clamped at sbits 4
    "a_70k": ("a", 70001, 0),                        # base == 0
    "text_100k_last": ("text", 100003, 0, b"\xff"),  # the largest byte last: base == n - 1 (reachable in a7 format), which is the clamped cut row at sbits 3
    "text_3k": ("text", 3129, 0),                    # the chain from `base` -- the last slab -- has exactly 16 symbols at sbits 3
}
# (off_in, off_out) of the caller's device buffers
OFFSETS = ((0, 0), (1, 3), (7, 2), (16, 5))

Case = collections.namedtuple("Case", "id group input env kernel edges in_offset out_offset")
CASES = []


def _case(id, group, input, env, kernel, edges, offsets=(0, 0)):
    assert edges and all(e in EDGES for e in edges) and kernel in STORE_UNIT and input in INPUTS
    CASES.append(Case(id, group, input, {"ARCHON_INV_" + k: str(v) for k, v in env.items()}, kernel, tuple(edges), offsets[0], offsets[1]))


_FULL = ("exact_slab", "slab_plus_one", "over_slab")       # k_walk_emit's work; k_chain_copy takes the exact ones whole
# ---- test_inverse_chain_geometries.  Every kernel of the walk at every slab shape:
#      kernel          exact slab / slab + 1            several stores per slab        base on a head (group "base")
#      k_walk_store    store_wgs0_s5_slab128            store_wgs0_s5, store_s8/s12    base_store_*
#      k_walk_queue    queue_s5_slab128                 queue_s4 / s5 / s6             base_queue_*
#      k_walk_rows<64> rows64_s4_slab64, _s5_slab192    rows64_s5_slab192, rows64_s5   base_rows64_*
#      k_walk_rows<128> rows128_s5_slab128              rows128_s5 / s6                base_rows128_*
#      k_chain_copy and k_walk_emit run behind each of them: the first takes the chains up to exact_slab, the second the rest
_case("queue_s4", "geometry", "dna_1m", dict(SBITS=4, ROWS=0), "walk_queue", ("multi_row", "ends_on_row", "len_mult_128", "len_one", "clamped_last_head"))
_case("queue_s5", "geometry", "text_1m", dict(SBITS=5, ROWS=0), "walk_queue", ("multi_row", "ends_on_row", "len_mult_128", "base_off_head"))
_case("queue_s6", "geometry", "dna_1m", dict(SBITS=6, ROWS=0), "walk_queue", ("multi_row", "ends_on_row", "len_mult_128"))
_case("queue_s5_slab128", "geometry", "text_1m", dict(SBITS=5, ROWS=0, SLAB=128), "walk_queue", _FULL + ("copy_reads_next_slab",))
_case("rows128_s5", "geometry", "text_1m", dict(SBITS=5, ROWS=1), "walk_rows128", ("multi_row", "ends_on_row", "len_mult_128", "len_one"))
_case("rows128_s6", "geometry", "dna_1m", dict(SBITS=6, ROWS=1), "walk_rows128", ("multi_row", "ends_on_row", "len_mult_64"))
_case("rows128_s5_slab128", "geometry", "text_1m", dict(SBITS=5, ROWS=1, SLAB=128), "walk_rows128", _FULL + ("len_mult_64", "copy_reads_next_slab"))
_case("rows64_s4_slab64", "geometry", "dna_1m", dict(SBITS=4, ROWS=2, SLAB=64), "walk_rows64", _FULL + ("len_mult_16", "clamped_last_head", "copy_reads_next_slab"))
_case("rows64_s5_slab192", "geometry", "text_1m", dict(SBITS=5, ROWS=1, SLAB=192), "walk_rows64", _FULL + ("multi_row", "ends_on_row", "len_mult_128"))
_case("rows64_s5", "geometry", "text_1m", dict(SBITS=5, ROWS=2), "walk_rows64", ("multi_row", "ends_on_row", "len_one"))
# INV_WALK_WGS: 0 = one chain per lane (k_walk_store whatever INV_ROWS says, here with >= 16384 chains), 1 and 2 workgroups per CU
_case("store_wgs0_s5", "geometry", "text_1m", dict(SBITS=5, ROWS=0, WALK_WGS=0), "walk_store", ("multi_row", "ends_on_row", "len_one"))
_case("store_wgs0_s5_slab128", "geometry", "text_1m", dict(SBITS=5, ROWS=0, WALK_WGS=0, SLAB=128), "walk_store", _FULL + ("copy_reads_next_slab",))
_case("store_wgs0_rows1_s5", "geometry", "dna_1m", dict(SBITS=5, ROWS=1, WALK_WGS=0), "walk_store", ("multi_row", "len_mult_128"))
_case("store_wgs0_rows2_s4_slab64", "geometry", "dna_1m", dict(SBITS=4, ROWS=2, SLAB=64, WALK_WGS=0), "walk_store", _FULL)
_case("queue_wgs1_s5", "geometry", "text_1m", dict(SBITS=5, ROWS=0, WALK_WGS=1), "walk_queue", ("multi_row", "ends_on_row"))
_case("queue_wgs2_s5_slab128", "geometry", "text_1m", dict(SBITS=5, ROWS=0, WALK_WGS=2, SLAB=128), "walk_queue", _FULL)
_case("rows64_wgs1_s4_slab64", "geometry", "dna_1m", dict(SBITS=4, ROWS=2, SLAB=64, WALK_WGS=1), "walk_rows64", _FULL)
_case("rows64_wgs2_s5_slab192", "geometry", "text_1m", dict(SBITS=5, ROWS=1, SLAB=192, WALK_WGS=2), "walk_rows64", _FULL + ("multi_row",))
_case("rows128_wgs1_s5", "geometry", "text_1m", dict(SBITS=5, ROWS=1, WALK_WGS=1), "walk_rows128", ("multi_row", "ends_on_row"))    # per_cu = 1 under the cap of 2
_case("rows128_wgs2_s5_slab128", "geometry", "text_1m", dict(SBITS=5, ROWS=1, WALK_WGS=2, SLAB=128), "walk_rows128", _FULL)
# few long chains on a small block
_case("store_s8", "geometry", "text_100k_last", dict(SBITS=8), "walk_store", ("multi_row", "ends_on_row", "len_mult_128", "len_one", "base_last"))
_case("store_s12", "geometry", "text_100k_last", dict(SBITS=12), "walk_store", ("multi_row", "ends_on_row", "len_mult_128", "base_last"))

# ---- test_inverse_base_edges: row `base` on a regular head (the unused slot), base == 0, base == n - 1, the clamped last head
_case("base_store_zero", "base", "a_70k", dict(), "walk_store", ("base_zero", "base_on_head", "clamped_last_head"))
_case("base_store_zero_s8", "base", "a_70k", dict(SBITS=8), "walk_store", ("base_zero", "base_on_head", "clamped_last_head"))
_case("base_store_last_is_clamped_head", "base", "text_100k_last", dict(), "walk_store", ("base_last", "base_on_head", "clamped_last_head"))
_case("base_store_last_off_head", "base", "text_100k_last", dict(SBITS=6), "walk_store", ("base_last", "base_off_head"))
_case("base_store_last_slab_full", "base", "text_3k", dict(SLAB=16), "walk_store", ("copy_reads_past_last_slab", "base_off_head", "clamped_last_head"))
_case("base_store_on_head_wgs0", "base", "dna_1m", dict(SBITS=5, WALK_WGS=0), "walk_store", ("base_on_head",))
_case("base_queue_on_head_s5", "base", "dna_1m", dict(SBITS=5, ROWS=0), "walk_queue", ("base_on_head",))
_case("base_queue_on_head_s4_clamped", "base", "text_1m", dict(SBITS=4, ROWS=0), "walk_queue", ("base_on_head", "clamped_last_head"))
_case("base_rows128_on_head_s5", "base", "dna_1m", dict(SBITS=5, ROWS=1), "walk_rows128", ("base_on_head", "multi_row"))
_case("base_rows128_on_head_s5_slab128", "base", "dna_1m", dict(SBITS=5, ROWS=1, SLAB=128), "walk_rows128", ("base_on_head", "exact_slab"))
_case("base_rows128_on_head_s4_clamped", "base", "text_1m", dict(SBITS=4, ROWS=1), "walk_rows128", ("base_on_head", "clamped_last_head"))
_case("base_rows64_on_head_s5_slab64", "base", "dna_1m", dict(SBITS=5, ROWS=2, SLAB=64), "walk_rows64", ("base_on_head", "exact_slab"))
_case("base_rows64_on_head_s4_slab64_clamped", "base", "text_1m", dict(SBITS=4, ROWS=2, SLAB=64), "walk_rows64", ("base_on_head", "clamped_last_head", "exact_slab"))

# ---- test_inverse_unaligned_under_rows: the caller's buffers at any byte offset
for _oi, _oo in OFFSETS:
    _case("unaligned_rows128_s5_%d_%d" % (_oi, _oo), "unaligned", "dna_1m", dict(SBITS=5, ROWS=1), "walk_rows128", ("multi_row", "base_on_head"), (_oi, _oo))
    _case("unaligned_rows64_s4_slab64_%d_%d" % (_oi, _oo), "unaligned", "dna_1m", dict(SBITS=4, SLAB=64, ROWS=2), "walk_rows64",
          _FULL + ("copy_reads_next_slab", "clamped_last_head"), (_oi, _oo))


def gen_input(name):
    import archon_synth as S
    spec = INPUTS[name]
    x = S.gen_shape(*spec[:3])
    if len(spec) > 3:
        x[x.size - len(spec[3]):] = np.frombuffer(spec[3], np.uint8)
    return x


def cases(group):
    return [c for c in CASES if c.group == group]


def census(case, bwt, base, order=None):
    """({edge: bool} of a case on its input's (bwt, base), the Ctx they were taken on, the derived Route)"""
    n = len(bwt)
    sbits, rt = route_of_env(n, case.env)
    ch = chains(bwt, base, sbits, 0, order)
    ctx = Ctx(ch, n, base, sbits, 0, rt.slab_bytes, STORE_UNIT[rt.kernel], case.out_offset)
    return {e: bool(EDGES[e](ctx)) for e in case.edges}, ctx, rt
