"""GPU: the order-k statistics of a block, its substring complexity and the runs of its BWT (archon_hip_entropy*,
archon_hip_complexity*; include/archon_hip.h) against the definitions by the text (tests/entropy_naive.py: Counter and fsum at
tiny sizes, windows through np.unique above them; tests/test_entropy_abi.py pins the row rules to them): every integer exactly,
`bits` within a derived bound, through the host, device and block forms; the three kinds of group at every edge of a wave's
window by construction; a block of one byte; the statistics, determinism and bad input.

The bound on bits.  The reference is math.fsum over exact ratios.  The terms are non-negative, so any summation order errs by at
most T 2^-53 want with T = pairs terms; a term c log2(m / c) errs by a few ulp of c, and the c sum to at most n.  So
|got - want| <= 2^-48 n + 2^-52 pairs want, and bits is exactly 0.0 when every context is deterministic."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import entropy_naive as E
import repeats_naive as R
import stride_util as G

pytestmark = pytest.mark.gpu

PARTS = 8
SENT = 0xA5A5A5A5
INTS = ("k", "contexts", "deterministic", "pairs", "symbols")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _odd(t):
    """the same values at an odd device address (one element past an allocation's start)"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def _check_orders(got, ks, wants, n, where=""):
    """ENTROPY records against (contexts, deterministic, pairs, symbols, bits) per order: the integers exactly, bits in its bound"""
    assert got.size == len(ks)
    for rec, k, want in zip(got, ks, wants):
        assert tuple(int(rec[f]) for f in INTS) == (k,) + tuple(want[:4]), (where, k, rec, want)
        bound = E.bits_bound(n, want[2], want[4])
        print("    %s n %d k %d: bits %.17g want %.17g diff %.3g bound %.3g" % (where, n, k, rec["bits"], want[4], abs(rec["bits"] - want[4]), bound))
        assert abs(float(rec["bits"]) - want[4]) <= bound, (where, k)
        if want[0] == want[1]:
            assert float(rec["bits"]) == 0.0, (where, k)


def _check_complexity(rec, counts, want, want_counts, where=""):
    got = {f: getattr(rec, f) for f in want}
    assert got == want, (where, got, want)
    assert counts.tolist() == want_counts.tolist(), where


def _groups(st):
    return (st.groups_direct, st.groups_table, st.groups_in_wave)


def _model_groups(sa, lcp, bwt, base, ks, tile):
    return tuple(sum(v) for v in zip(*[E.order_rows(sa, lcp, bwt, base, k, tile)[1] for k in ks]))


def _launches(ks, n):
    """5 per order in 1..n (bounds, scan, starts, follow, reduce), 1 for order 0, none above n"""
    return sum(1 if k == 0 else 5 if k <= n else 0 for k in ks)


@pytest.fixture(scope="module")
def tiny():
    """every string of length 1-7 over {0, 1, 255}: (x, sa, lcp, bwt, base, the record of every k in 0 .. n+1, d) from the text"""
    out = []
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            sa, lcp, bwt, base = R.a7_arrays(x)
            out.append((x, np.array(sa, np.uint32), np.array(lcp, np.uint32), np.frombuffer(bwt, np.uint8).copy(), base,
                        [E.order_text(x, k) for k in range(n + 2)], E.distinct_text(x)))
    return out


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("tile", [4, 0])
def test_exhaustive_tiny(archon, tiny, tile, part, monkeypatch):
    """every string of length 1-7 over {0, 1, 255} (in eight parts), every k in 0 .. n+1 in ONE call and every l, through the
    device forms (every other string at odd device addresses) and the block forms, with tiles of 4 rows and the default"""
    if tile:
        monkeypatch.setenv("ARCHON_KMER_TILE", str(tile))
    blk = archon.Block()
    for i, (x, sa, lcp, bwt, base, wants, d) in enumerate(tiny):
        if i % PARTS != part:
            continue
        n = len(x)
        ks = list(range(n + 2))
        sa_t, lcp_t, bwt_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt)
        if i & 8:
            sa_t, lcp_t, bwt_t = _odd(sa_t), _odd(lcp_t), _odd(bwt_t)
        got = archon.entropy_dev(sa_t, lcp_t, bwt_t, base, ks)
        _check_orders(got, ks, wants, n, repr(x))
        st = archon.entropy_stats()
        assert (st.n, st.nk, st.what, st.tile, st.direct_rows, st.built) == (n, n + 2, 0, tile or E.DEFAULT_TILE, 64, 1)
        assert _groups(st) == _model_groups(sa, lcp, bwt, base, ks, tile or E.DEFAULT_TILE), x
        assert (st.kernel_launches, st.host_syncs) == (3 + _launches(ks, n), 2)
        want_rec, want_counts = E.complexity_rows(lcp, bwt, n)
        assert want_counts.tolist() == d
        import torch
        counts_t = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda:0")
        rec = archon.complexity_dev(lcp_t, bwt_t, n, counts_t[1:n + 1])
        counts = counts_t.cpu().numpy().view(np.uint32)
        assert counts[0] == counts[-1] == 0xFFFFFFFF
        _check_complexity(rec, counts[1:-1], want_rec, want_counts, repr(x))
        got_sa, got_base = blk.forward(np.frombuffer(x, np.uint8), want_sa=True)
        assert got_base == base and (got_sa == sa).all()
        _check_orders(blk.entropy(ks), ks, wants, n, repr(x))
        assert _groups(archon.entropy_stats()) == _groups(st)
        for L in (0, 1 + i % n):
            want_rec, want_counts = E.complexity_rows(lcp, bwt, L)
            rec, counts = blk.complexity(L)
            _check_complexity(rec, counts, want_rec, want_counts, repr(x))
    blk.close()


_shape_cache = {}


def _shape(archon, shape, n):
    """(x, sa, lcp, bwt, base) of a synthetic shape, made once"""
    if (shape, n) not in _shape_cache:
        x = S.gen_shape(shape, n)
        sa, bwt, base = archon.forward(x)
        lcp = archon.lcp(x, sa)
        for a in (x, sa, lcp, bwt):
            a.setflags(write=False)
        _shape_cache[(shape, n)] = (x, sa, lcp, bwt, int(base))
    return _shape_cache[(shape, n)]


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65536])
def test_shapes(archon, shape, n):
    """every synthetic shape at k = 0, 1, 2, 3, 8, 16 in one call through the host, device and block forms: the integers exactly
    against the windows of the text, the groups against the model; complexity with max_len n at 1000, 0 and 5000 at 65536 (5000:
    bins in LDS and bins in global memory)"""
    x, sa, lcp, bwt, base = _shape(archon, shape, n)
    ks = [0, 1, 2, 3, 8, 16]
    wants = [E.order_windows(x, k) for k in ks]
    model = _model_groups(sa, lcp, bwt, base, ks, E.DEFAULT_TILE)
    got = archon.entropy(sa, lcp, bwt, base, ks)
    _check_orders(got, ks, wants, n, shape)
    st = archon.entropy_stats()
    assert _groups(st) == model and (st.kernel_launches, st.host_syncs, st.built) == (3 + _launches(ks, n), 2, 1)
    got_d = archon.entropy_dev(_cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt), base, ks)
    assert got_d.tobytes() == got.tobytes() and _groups(archon.entropy_stats()) == model
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    got_b = blk.entropy(ks)
    assert got_b.tobytes() == got.tobytes() and _groups(archon.entropy_stats()) == model
    bits = got["bits"]
    assert (bits[1:] <= bits[:-1] + 2 * E.bits_bound(n, n, float(bits[0]))).all()        # never grows with k
    for L in ((n,) if n == 1000 else (0, 5000)):
        want_rec, want_counts = E.complexity_rows(lcp, bwt, L)
        assert want_rec["max_len"] == (L or 4095)
        rec, counts = archon.complexity(lcp, bwt, L)
        _check_complexity(rec, counts, want_rec, want_counts, shape)
        rec, counts = blk.complexity(L)
        _check_complexity(rec, counts, want_rec, want_counts, shape)
    if n == 1000:
        want = E.distinct_text(x)
        assert counts.tolist() == want and rec.substrings == sum(want)
    rec, counts = archon.complexity(lcp, None, 7)
    assert (rec.runs, rec.longest_run, rec.max_len) == (0, 0, 7) and counts.tolist() == E.complexity_rows(lcp, None, 7)[1].tolist()
    blk.close()


@pytest.mark.parametrize("ending", ["a", "own"])
def test_group_edges(archon, ending):
    """p bytes below 'a', then m times 'a', then nothing (the block ends in 'a': the primary row inside the group) or one 'z'
    (the primary row a group of its own, which is no context).  At k = 1 the group of 'a' is the rows [p, p + m): m on both
    sides of direct_rows and of 256, p so that its first row falls on, just before and just after a multiple of 64, of 256 and
    of the tile.  The three counters match the model, and the group of 'a' is of the kind the construction says"""
    for m in (63, 64, 65, 66, 255, 256, 257):
        for p in (63, 64, 65, 255, 256, 257, 2047, 2048):
            x = np.concatenate(((np.arange(p) % 89 + 1).astype(np.uint8), np.full(m, ord("a"), np.uint8),
                                np.frombuffer(b"z" if ending == "own" else b"", np.uint8)))
            n = x.size
            sa, bwt, base = archon.forward(x)
            lcp = archon.lcp(x, sa)
            assert lcp[p] == 0 and (lcp[p + 1:p + m] >= 1).all() and (p + m == n or lcp[p + m] == 0)
            assert (p <= base < p + m) == (ending == "a") and (ending == "a" or base == n - 1)
            want = E.order_windows(x, 1)
            _, model = E.order_rows(sa, lcp, bwt, int(base), 1)
            lo, hi, kind = E.group_kinds(sa, lcp, 1)
            at = int(np.flatnonzero(lo == p)[0])
            same_window = p // 64 == (p + m - 1) // 64 and p // E.DEFAULT_TILE == (p + m - 1) // E.DEFAULT_TILE
            assert (hi[at], kind[at]) == (p + m, 1 if m > 64 else 2 if same_window else 0), (m, p)
            got = archon.entropy_dev(_cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt), int(base), [1])
            _check_orders(got, [1], [want], n, "m %d p %d" % (m, p))
            st = archon.entropy_stats()
            print("    m %d p %d %s: groups (direct, table, in wave) %s" % (m, p, ending, _groups(st)))
            assert _groups(st) == model, (m, p)
            if ending == "own":
                assert want[0] == int(got["contexts"][0]) == len(set(x[:-1].tolist()))      # 'z' is followed by nothing


def test_one_byte_block(archon):
    """70 000 equal bytes: at most one expansion per order, whatever k; d_l = 1 for every l, delta (1, 1), exact only at max_len n"""
    n = 70000
    x = np.full(n, ord("a"), np.uint8)
    blk = archon.Block()
    sa, base = blk.forward(x, want_sa=True)
    assert base == 0 and sa[0] == n and sa[-1] == 1
    ks = [0, 1, 5, n - 1, n, n + 1]
    got = blk.entropy(ks)
    wants = [(1, 1, 1, n - k, 0.0) if k < n else (0, 0, 0, 0, 0.0) for k in ks]
    _check_orders(got, ks, wants, n, "a")
    st = archon.entropy_stats()
    lcp = np.concatenate(([0], np.arange(n - 1, 0, -1))).astype(np.uint32)
    # k = 0, 1, 5: one expansion each; k = n-1: the rows [0, 2) inside a wave; k = n: the primary row alone, no context
    assert _groups(st) == _model_groups(sa, lcp, x, 0, ks, E.DEFAULT_TILE) == (0, 3, 2)
    for k in ks:
        blk.entropy([k])
        assert archon.entropy_stats().groups_table <= 1 and archon.entropy_stats().groups_direct == 0
    for L in (0, 5000, n):
        rec, counts = blk.complexity(L)
        assert (counts == 1).all() and counts.size == (L or 4095)
        assert (rec.delta_len, rec.delta_count, rec.delta_exact) == (1, 1, int(L == n))
        assert (rec.runs, rec.longest_run, rec.lcp_max, rec.lcp_sum, rec.substrings) == (1, n, n - 1, n * (n - 1) // 2, n)
    blk.close()


@pytest.mark.parametrize("shape", ["text", "dna"])
def test_cross_checks(archon, shape):
    """pairs(k) is `distinct` of a k-mer call at k + 1 on the same block; the same call twice gives the same 64 bits, on either
    form; a different tile gives the same integers"""
    x, sa, lcp, bwt, base = _shape(archon, shape, 65536)
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    ks = [0, 1, 2, 3, 5, 8, 11]
    a = blk.entropy(ks)
    for rec in a:
        blk.kmers(int(rec["k"]) + 1, count_only=True)
        assert archon.kmer_stats().distinct == rec["pairs"]
    b = blk.entropy(ks)
    assert a.tobytes() == b.tobytes()
    c = archon.entropy(sa, lcp, bwt, base, ks)
    d = archon.entropy(sa, lcp, bwt, base, ks)
    assert c.tobytes() == d.tobytes() == a.tobytes()
    blk.close()


def test_other_tile_same_integers(archon, monkeypatch):
    x, sa, lcp, bwt, base = _shape(archon, "text", 65536)
    ks = [1, 2, 3, 8]
    a = archon.entropy(sa, lcp, bwt, base, ks)
    monkeypatch.setenv("ARCHON_KMER_TILE", "16")
    b = archon.entropy(sa, lcp, bwt, base, ks)
    st = archon.entropy_stats()
    assert st.tile == 16 and _groups(st) == _model_groups(sa, lcp, bwt, base, ks, 16)
    for f in INTS:
        assert (a[f] == b[f]).all()
    _check_orders(b, ks, [E.order_windows(x, k) for k in ks], x.size, "tile 16")
    want_rec, want_counts = E.complexity_rows(lcp, bwt, 0)
    rec, counts = archon.complexity(lcp, bwt)
    _check_complexity(rec, counts, want_rec, want_counts, "tile 16")


def test_statistics_stay_apart(archon):
    """the launch and wait counts the header states; the records of lcp, fm, k-mer and maw calls stay byte-equal across the
    family's calls; a forward without its suffix array is refused"""
    x, sa, lcp, bwt, base = _shape(archon, "dna", 65536)
    n = x.size
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    blk.fm_count([b"ACGT"])
    archon.lcp(x, sa)
    archon.kmers(sa, lcp, 3, count_only=True)
    archon.maws(sa, lcp, bwt, base, count_only=True)
    before = (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.stats_raw()), bytes(archon.kmer_stats()), bytes(archon.maw_stats()))
    sa_t, lcp_t, bwt_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt)

    def counts():
        st = archon.entropy_stats()
        return st.kernel_launches, st.host_syncs, st.what, st.nk

    archon.entropy_dev(sa_t, lcp_t, bwt_t, base, [4])
    assert counts() == (8, 2, 0, 1) and archon.entropy_stats().ms_count > 0 and archon.entropy_stats().ms_build > 0
    archon.entropy_dev(sa_t, lcp_t, bwt_t, base, [0, 4, 9, n + 1])
    assert counts() == (14, 2, 0, 4)
    archon.entropy(sa, lcp, bwt, base, list(range(64)))
    assert counts() == (3 + 1 + 63 * 5, 2, 0, 64)                  # ONE wait for 64 orders, and the table's
    archon.complexity_dev(lcp_t, bwt_t)
    assert counts() == (3, 1, 1, 0)
    archon.complexity_dev(lcp_t)
    assert counts() == (2, 1, 1, 0)
    archon.complexity(lcp, bwt, 100)
    assert counts() == (3, 1, 1, 0) and archon.entropy_stats().ms_lcp == 0
    assert before == (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.stats_raw()), bytes(archon.kmer_stats()), bytes(archon.maw_stats()))
    # the block forms: the same launches, the waits of the LCP step on top, its record kept; the table is the block's own
    blk.entropy([0, 4, 9])
    assert archon.lcp_stats().n == n and counts() == (11, 1 + archon.lcp_stats().host_syncs, 0, 3)
    assert archon.entropy_stats().built == 0 and archon.entropy_stats().ms_lcp > 0
    blk.complexity()
    assert counts() == (3, 1 + archon.lcp_stats().host_syncs, 1, 0)
    assert bytes(archon.fm_stats()) == before[1] and bytes(archon.stats_raw()) == before[2] and bytes(archon.kmer_stats()) == before[3]
    blk.forward(x, want_sa=True)                   # a new forward drops the block's table: the next call builds it and says so
    blk.entropy([4])
    assert archon.entropy_stats().built == 1 and counts()[0] == 8
    blk.entropy([4])
    assert archon.entropy_stats().built == 0 and counts()[0] == 5
    blk.forward(x, want_sa=False)
    for call in (lambda: blk.entropy([1]), blk.complexity):
        with pytest.raises(archon.ArchonError) as e:
            call()
        assert e.value.code == archon.E_ARG
    blk.close()


def test_two_contexts_concurrently(archon):
    blocks = [S.gen_shape("text", (1 << 20) + 1), S.gen_shape("dna", (1 << 20) + 1)]
    ks = [0, 2, 6, 12]
    solo = []
    for x in blocks:
        blk = archon.Block()
        blk.forward(x, want_sa=True)
        rec, counts = blk.complexity()
        solo.append((blk.entropy(ks), bytes(rec), counts))
        blk.close()
    assert solo[0][0].tobytes() != solo[1][0].tobytes()
    errors = []

    def run(j):
        try:
            archon.bind_context(j)
            blk = archon.Block()
            blk.forward(blocks[j], want_sa=True)
            for _ in range(3):
                assert blk.entropy(ks).tobytes() == solo[j][0].tobytes()
                assert archon.entropy_stats().n == blocks[j].size and archon.entropy_stats().what == 0
                rec, counts = blk.complexity()
                assert bytes(rec) == solo[j][1] and (counts == solo[j][2]).all()
            blk.close()
        except Exception as ex:          # noqa: BLE001 -- reported below
            errors.append(ex)

    threads = [threading.Thread(target=run, args=(j,)) for j in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("bad", ["zero", "past"])
def test_bad_sa_is_corrupt(archon, bad):
    """an sa value outside 1..n is ARCHON_E_CORRUPT from the host and the device form, the records untouched"""
    _, sa, lcp, bwt, base = _shape(archon, "dna", 65536)
    n = sa.size
    sa = sa.copy()
    sa[n // 3] = 0 if bad == "zero" else n + 1
    L, p = archon.lib(), archon._p
    ks = np.array([0, 3, 7], np.uint32)
    out = np.zeros(3, archon.ENTROPY)
    out.view(np.uint32)[:] = SENT
    assert L.archon_hip_entropy(p(sa), p(lcp), p(bwt), n, base, p(ks), 3, p(out), 0) == archon.E_CORRUPT
    assert (out.view(np.uint32) == SENT).all() and b"outside 1..65536" in L.archon_hip_last_error()
    assert L.archon_hip_entropy_dev(ctypes.c_void_p(_cuda(sa.view(np.int32)).data_ptr()), ctypes.c_void_p(_cuda(lcp.view(np.int32)).data_ptr()),
                                    ctypes.c_void_p(_cuda(bwt).data_ptr()), n, base, p(ks), 3, p(out), 0, None) == archon.E_CORRUPT
    assert (out.view(np.uint32) == SENT).all()
    ks0 = np.array([0], np.uint32)              # order 0 reads no sa: nothing to refuse
    assert L.archon_hip_entropy(p(sa), p(lcp), p(bwt), n, base, p(ks0), 1, p(out), 0) == 0 and out["symbols"][0] == n


def test_arrays_of_nothing_stay_inside(archon):
    """arrays that are not the SA, LCP array or BWT of anything: ARCHON_OK, whatever comes out, sentinel words behind the counts,
    and the next good call is right.  The complexity rule is a rule about the array, so the array helper still says which"""
    import torch
    rng = np.random.default_rng(5)
    n = 5000
    for trial in range(4):
        sa = rng.integers(1, n + 1, n).astype(np.uint32)
        lcp = rng.integers(0, (2, 8, n, 1 << 32)[trial], n, dtype=np.uint64).astype(np.uint32)
        bwt = rng.integers(0, (256, 2, 256, 1)[trial] + 1, n).astype(np.uint8)
        base = int(rng.integers(0, n))
        got = archon.entropy(sa, lcp, bwt, base, [0, 1, 2, 5, 1 << 31])
        assert got["k"].tolist() == [0, 1, 2, 5, 1 << 31] and not np.isnan(got["bits"][:1]).any()
        for L in (0, n, 4500):
            counts_t = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda:0")
            used = archon.complexity_len(n, L)
            rec = archon.complexity_dev(_cuda(lcp.view(np.int32)), _cuda(bwt), L, counts_t[1:used + 1])
            counts = counts_t.cpu().numpy().view(np.uint32)
            assert counts[0] == 0xFFFFFFFF and (counts[used + 1:] == 0xFFFFFFFF).all()
            want_rec, want_counts = E.complexity_rows(lcp, bwt, L)
            _check_complexity(rec, counts[1:used + 1], want_rec, want_counts, "trial %d max_len %d" % (trial, L))
    x, sa, lcp, bwt, base = _shape(archon, "text", 1000)
    _check_orders(archon.entropy(sa, lcp, bwt, base, [2]), [2], [E.order_windows(x, 2)], 1000, "after garbage")


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text and dna at 65 536 (32 tiles): the six orders 0, 1, 2, 3, 8, 16 in
    one call through the host and block forms -- the integers exactly, bits in its bound, the groups against the model -- and
    complexity with max_len 0 and 5000; byte-equal to the same calls without the route, so that `bits` is the same 64 bits (the
    sums are kept per tile and added in tile order, whatever workgroup took the tile), with their counters, launches and waits"""
    ks = [0, 1, 2, 3, 8, 16]
    for shape in ("text", "dna"):
        x, sa, lcp, bwt, base = _shape(archon, shape, 65536)
        n = x.size
        wants = [E.order_windows(x, k) for k in ks]
        model = _model_groups(sa, lcp, bwt, base, ks, E.DEFAULT_TILE)
        blk = archon.Block()
        try:
            blk.forward(x, want_sa=True)
            blk.fm_count([b"a"])                     # (the block's table built: `built` is 0 in every block call below)

            def call():
                out, stats = [], []
                got = archon.entropy(sa, lcp, bwt, base, ks)
                _check_orders(got, ks, wants, n, shape)
                st = archon.entropy_stats()
                assert _groups(st) == model and (st.kernel_launches, st.host_syncs, st.built) == (3 + _launches(ks, n), 2, 1)
                got_b = blk.entropy(ks)
                assert got_b.tobytes() == got.tobytes() and _groups(archon.entropy_stats()) == model
                out += [got, got_b]
                stats += [st, archon.entropy_stats()]
                for L in (0, 5000):
                    want_rec, want_counts = E.complexity_rows(lcp, bwt, L)
                    for form in (lambda: archon.complexity(lcp, bwt, L), lambda: blk.complexity(L)):
                        rec, counts = form()
                        _check_complexity(rec, counts, want_rec, want_counts, shape)
                        out += [rec, counts]
                        stats.append(archon.entropy_stats())
                return out, stats
            G.same_under(monkeypatch, grid, call)
        finally:
            blk.close()


@pytest.mark.parametrize("shape", ["a", "dna"])
def test_second_trip_at_the_product_grid(archon, shape):
    """no route: 2048 * 2048 + 3 * 2048 + 5 rows are 2052 tiles, so workgroups 0-3 of the 2048 take a second tile and the last
    tile has 5 rows.  One byte: the tuples of test_one_byte_block.  DNA at k = 12 against the windows of the text, and
    complexity at max_len 5000 against the rule over the LCP array"""
    n = G.N2
    x = S.gen_shape(shape, n)
    blk = archon.Block()
    try:
        sa, base = blk.forward(x, want_sa=True)
        assert blk.validate() == 1
        if shape == "a":
            ks = [0, 1, 5, n - 1, n, n + 1]
            _check_orders(blk.entropy(ks), ks, [(1, 1, 1, n - k, 0.0) if k < n else (0, 0, 0, 0, 0.0) for k in ks], n, "a")
            assert _groups(archon.entropy_stats()) == (0, 3, 2)
            rec, counts = blk.complexity(5000)
            assert (counts == 1).all() and counts.size == 5000 and (rec.delta_len, rec.delta_count, rec.delta_exact) == (1, 1, 0)
            assert (rec.runs, rec.longest_run, rec.lcp_max, rec.lcp_sum, rec.substrings) == (1, n, n - 1, n * (n - 1) // 2, n)
        else:
            ks = [0, 12]
            got = blk.entropy(ks)
            _check_orders(got, ks, [E.order_windows(x, k) for k in ks], n, "dna")
            assert blk.entropy(ks).tobytes() == got.tobytes()
            lcp, bwt = blk.lcp(), blk.read_bwt()
            want_rec, want_counts = E.complexity_rows(lcp, bwt, 5000)
            rec, counts = blk.complexity(5000)
            _check_complexity(rec, counts, want_rec, want_counts, "dna")
    finally:
        blk.close()
