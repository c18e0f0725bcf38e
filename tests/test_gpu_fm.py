"""GPU: counting and locating patterns with the FM index (archon_hip_fm_*, archon_hip_block_fm_*; include/archon_hip.h)
against a KMP scan of the text on the CPU (tests/fm_naive.c, pinned to the definition by test_fm_abi.py): counts, starts
and the exact number of rank steps, across the rank table's boundaries, through every entry point, and bad input."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import fm_naive
import stride_util as G

pytestmark = pytest.mark.gpu

MiB = 1 << 20
LOCATE_MAX = 1 << 18            # occurrences a test locates in one call at most (the counts cover the rest)


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return fm_naive.build(tmp_path_factory.mktemp("fm_naive"))


def _steps(naive_L, patterns, n):
    return sum(fm_naive.expected_steps(len(p), n, int(L)) for p, L in zip(patterns, naive_L))


def _patterns(x, rng, long=False):
    """substrings of lengths 1-64, random patterns, substrings with one byte changed, the empty pattern and one pattern
    longer than the block; with `long`, substrings up to 65 536 bytes and such substrings changed near their end"""
    n = x.size
    pats = []
    for m in range(1, 65):
        if m <= n:
            for q in rng.integers(0, n - m + 1, 2):
                pats.append(x[q:q + m].tobytes())
    for m in rng.integers(1, 24, 48):
        pats.append(rng.integers(0, 256, m, dtype=np.uint8).tobytes())
    for p in list(pats[:96:3]):
        b = bytearray(p)
        b[int(rng.integers(0, len(b)))] ^= 1 + int(rng.integers(0, 255))
        pats.append(bytes(b))
    pats.append(b"")
    pats.append(np.resize(x, n + 1).tobytes())
    if long:
        for m in (256, 1024, 4096, 16384, 65536):
            if m <= n:
                q = int(rng.integers(0, n - m + 1))
                p = x[q:q + m].tobytes()
                pats.append(p)
                b = bytearray(p)
                b[m - 2] ^= 0x5A
                pats.append(bytes(b))
    return pats


def _want(naive, x, pats, locate=False):
    """the KMP scan's (count, matched lengths, the rarer patterns, their sorted starts)"""
    count, L = naive(x, pats)
    some, starts = [], []
    if locate:
        some = [p for p, c in zip(pats, count) if c <= LOCATE_MAX // 64][:64]
        _, _, starts = naive(x, some, starts=True)
    return count, L, some, starts


def _check_against(archon, want, x, pats, lo, hi, locate_block=None):
    count, L, some, starts = want
    assert ((hi.astype(np.int64) - lo) == count).all()
    assert (lo <= hi).all() and (hi <= x.size).all()
    st = archon.fm_stats()
    assert st.steps == _steps(L, pats, x.size)
    assert st.shared_steps <= st.steps
    if locate_block is not None:
        got = locate_block.fm_locate(some)
        for p, g, w in zip(some, got, starts):
            assert (np.sort(g) == w).all(), p
        return got
    return None


def _check(archon, naive, x, pats, lo, hi, locate_block=None):
    _check_against(archon, _want(naive, x, pats, locate_block is not None), x, pats, lo, hi, locate_block)


def test_exhaustive_tiny(archon, oracle):
    """every string of length 1-7 over {0, 1, 255} with every pattern of length 0-3 over {0, 1, 2, 255}: count through the
    block and a host-built index, locate as sorted starts, against the rule of the header"""
    pats = [bytes(t) for m in range(4) for t in itertools.product((0, 1, 2, 255), repeat=m)]
    b = archon.Block()
    try:
        for n in range(1, 8):
            for t in itertools.product((0, 1, 255), repeat=n):
                x = np.array(t, np.uint8)
                sa, base = b.forward(x)
                bwt = b.read_bwt()
                lo, hi = b.fm_count(pats)
                f = archon.FmIndex(bwt, base)
                lo2, hi2 = f.count(pats)
                f.close()
                assert (lo == lo2).all() and (hi == hi2).all(), x
                starts = b.fm_locate(pats)
                for j, p in enumerate(pats):
                    want = fm_naive.backward_search(bwt.tobytes(), base, p)
                    assert (lo[j], hi[j]) == want[:2], (x, p)
                    occ = [q for q in range(n - len(p) + 1) if x[q:q + len(p)].tobytes() == p and q + len(p) >= 1]
                    assert sorted(starts[j].tolist()) == occ, (x, p)
    finally:
        b.close()


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65536, MiB + 3])
def test_shapes(archon, naive, shape, n):
    """every synthetic shape: counts and the exact rank steps against the KMP scan, starts of the rarer patterns"""
    x = S.gen_shape(shape, n)
    rng = np.random.default_rng(n + len(shape))
    pats = _patterns(x, rng, long=shape in ("a", "ab", "motif"))
    b = archon.Block()
    try:
        b.forward(x)
        lo, hi = b.fm_count(pats)
        assert archon.fm_stats().built == 1
        _check(archon, naive, x, pats, lo, hi, locate_block=b)
    finally:
        b.close()


def _boundary_inputs(n):
    """text and dna blocks of n bytes, and the text block with x[0] set to its most common byte and to that byte's
    neighbours: the primary row holds x[0], so the rows around it and the bucket it falls in move"""
    out = [S.gen_shape("dna", n)]
    x = S.gen_shape("text", n)
    out.append(x)
    common = int(np.bincount(x, minlength=256).argmax())
    for v in (common, common - 1, common + 1):
        y = x.copy()
        y[0] = v & 0xFF
        out.append(y)
    return out


@pytest.mark.parametrize("sub,sup", [(16, 64), (64, 4096), (1024, 65536)])
@pytest.mark.parametrize("n", [1024, 3 * 1024, 65535, 65537, 2 * 65536 - 1, 2 * 65536 + 1])
def test_table_boundaries(archon, naive, monkeypatch, sub, sup, n):
    """small sub-chunks and superblocks: ranges cross many table entries, and the primary row falls near their edges.  No
    table size changes a range"""
    for x in _boundary_inputs(n):
        rng = np.random.default_rng(int(x[0]) + n)
        pats = _patterns(x, rng)
        b = archon.Block()
        try:
            _, base = b.forward(x)
            monkeypatch.delenv("ARCHON_FM_SUB_ROWS", raising=False)
            monkeypatch.delenv("ARCHON_FM_SUPER_ROWS", raising=False)
            f = archon.FmIndex(b.read_bwt(), base)
            want = f.count(pats)
            f.close()
            monkeypatch.setenv("ARCHON_FM_SUB_ROWS", str(sub))
            monkeypatch.setenv("ARCHON_FM_SUPER_ROWS", str(sup))
            lo, hi = b.fm_count(pats)
            st = archon.fm_stats()
            assert st.built == 1 and st.table_bytes >= ((n // sub) + 1) * 512
            assert (lo == want[0]).all() and (hi == want[1]).all()
            _check(archon, naive, x, pats, lo, hi)
        finally:
            b.close()


def _odd(t):
    """the same values at an odd device address (one element past an allocation's start)"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def test_entry_points_agree(archon, naive):
    """fm_create (host BWT), fm_create_dev (device BWT at an odd address), fm_count_dev and block_fm_count give the same ranges"""
    import torch
    x = S.gen_shape("prose", 300000)
    pats = _patterns(x, np.random.default_rng(5))
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        bl = b.fm_count(pats)
        bwt = b.read_bwt()
    finally:
        b.close()
    f1 = archon.FmIndex(bwt, base)
    h1 = f1.count(pats)
    f2 = archon.FmIndex.from_dev(_odd(torch.from_numpy(bwt).to("cuda:0")), base)
    torch.cuda.synchronize()
    h2 = f2.count(pats)
    packed, off = fm_naive.pack(pats)
    p_t = _odd(torch.from_numpy(packed).to("cuda:0"))
    o_t = torch.from_numpy(off.view(np.int32)).to("cuda:0")
    lo_t = torch.full((len(pats),), -1, dtype=torch.int32, device="cuda:0")
    hi_t = torch.full((len(pats),), -1, dtype=torch.int32, device="cuda:0")
    f2.count_dev(p_t, o_t, lo_t, hi_t)
    d = (lo_t.cpu().numpy().view(np.uint32), hi_t.cpu().numpy().view(np.uint32))
    f1.close()
    f2.close()
    for got in (h1, h2, d):
        assert (got[0] == bl[0]).all() and (got[1] == bl[1]).all()
    _check(archon, naive, x, pats, d[0], d[1])


def test_block_lifetime(archon, naive):
    """a forward drops the block's index: the next count answers for the new block and builds once; locate needs the SA
    of the last forward; a cap below the total reports the total and writes nothing"""
    L = archon.lib()
    x1, x2 = S.gen_shape("text", 70000), S.gen_shape("dna", 50001)
    pats = [b"e", b"the", b"ACG", b"GATTACA", b"", x2[100:120].tobytes()]
    b = archon.Block()
    try:
        b.forward(x1)
        b.fm_count(pats)
        b.forward(x2)
        lo, hi = b.fm_count(pats)
        assert archon.fm_stats().built == 1
        assert ((hi.astype(np.int64) - lo) == naive(x2, pats)[0]).all()
        lo2, hi2 = b.fm_count(pats)
        assert archon.fm_stats().built == 0 and (lo2 == lo).all() and (hi2 == hi).all()
        packed, off = fm_naive.pack(pats[2:4])
        want = int((hi[2:4].astype(np.int64) - lo[2:4]).sum())
        assert want > 1
        pos = np.full(want, 0xEEEEEEEE, np.uint32)
        total = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
        assert L.archon_hip_block_fm_locate(b.h, p(packed), p(off), 2, p(pos), want - 1, tp) == archon.E_ARG
        assert total.value == want and (pos == 0xEEEEEEEE).all()
        assert L.archon_hip_block_fm_locate(b.h, p(packed), p(off), 2, p(pos), want, tp) == 0 and total.value == want
        b.forward(x2, want_sa=False)
        assert L.archon_hip_block_fm_locate(b.h, p(packed), p(off), 2, p(pos), want, tp) == archon.E_ARG
        lo3, hi3 = b.fm_count(pats)                     # counting needs no SA
        assert (lo3 == lo).all() and (hi3 == hi).all()
    finally:
        b.close()


def test_threads(archon, naive):
    """two threads, each with its own index on one device"""
    xs = [S.gen_shape("text", 200000), S.gen_shape("random_copy", 300001)]
    out = [None, None]

    def work(i):
        try:
            x = xs[i]
            pats = _patterns(x, np.random.default_rng(i))
            b = archon.Block()
            _, base = b.forward(x, want_sa=False)
            bwt = b.read_bwt()
            b.close()
            f = archon.FmIndex(bwt, base)
            for _ in range(3):
                lo, hi = f.count(pats)
                assert ((hi.astype(np.int64) - lo) == naive(x, pats)[0]).all()
            f.close()
            out[i] = True
        except BaseException as e:          # noqa: BLE001
            out[i] = e

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert out == [True, True], out


def test_other_stats_untouched(archon):
    """FM calls leave archon_hip_get_stats and archon_hip_get_lcp_stats as they were"""
    x = S.gen_shape("text", 100000)
    b = archon.Block()
    try:
        b.forward(x)
        sa, bwt, base = archon.forward(x)
        archon.lcp(x, sa)
        before = (archon.stats(), archon.lcp_stats().asdict())
        f = archon.FmIndex(bwt, base)
        f.count([b"the", b"and"])
        f.close()
        b.fm_count([b"e"])
        b.fm_locate([b"the"])
        assert archon.fm_stats().patterns == 1
        assert (archon.stats(), archon.lcp_stats().asdict()) == before
    finally:
        b.close()


def test_bad_offsets_and_empty_calls(archon):
    """decreasing offsets are ARCHON_E_ARG in the host form (checked on the host) and in the device form (found by the
    kernel); k = 0 is ARCHON_OK and writes nothing"""
    import torch
    L = archon.lib()
    bwt = np.frombuffer(b"nnbaaa", np.uint8).copy()
    f = archon.FmIndex(bwt, 2)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    packed = np.frombuffer(b"anana\0", np.uint8).copy()
    off = np.array([0, 2, 1, 5], np.uint32)
    lo, hi = np.full(3, 7, np.uint32), np.full(3, 7, np.uint32)
    assert L.archon_hip_fm_count(f.h, p(packed), p(off), 3, p(lo), p(hi)) == archon.E_ARG
    assert L.archon_hip_fm_count(f.h, p(packed), p(off), 0, p(lo), p(hi)) == 0
    assert (lo == 7).all() and (hi == 7).all()
    p_t = torch.from_numpy(packed).to("cuda:0")
    o_t = torch.from_numpy(off.view(np.int32)).to("cuda:0")
    lo_t = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    hi_t = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    with pytest.raises(archon.ArchonError):
        f.count_dev(p_t, o_t, lo_t, hi_t)
    o_t = torch.from_numpy(np.array([0, 2, 5, 5], np.int32)).to("cuda:0")
    f.count_dev(p_t, o_t, lo_t, hi_t)
    assert lo_t.cpu().tolist() == [4, 1, 0] and hi_t.cpu().tolist() == [6, 3, 6]
    assert archon.fm_stats().steps == 3
    f.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, naive, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID): the 260 patterns of text and dna at 65 536 and of one byte x (MiB + 3)
    with its long patterns, so that every wave counts 20 to 65 patterns one behind another -- counts and the exact rank steps
    against the KMP scan through the block and a host-built index, the starts of the rarer patterns, byte-equal to the same
    calls without the route, with their counters"""
    for shape, n in (("text", 65536), ("dna", 65536), ("a", MiB + 3)):
        x = S.gen_shape(shape, n)
        pats = _patterns(x, np.random.default_rng(n + len(shape)), long=shape == "a")
        want = _want(naive, x, pats, locate=True)
        b = archon.Block()
        try:
            _, base = b.forward(x)
            f = archon.FmIndex(b.read_bwt(), base)
            b.fm_count([b"a"])
            f.count([b"a"])                  # (both tables built: `built` is 0 in every call below)

            def call():
                lo, hi = b.fm_count(pats)
                st = [archon.fm_stats()]
                starts = _check_against(archon, want, x, pats, lo, hi, locate_block=b)
                st.append(archon.fm_stats())
                lo2, hi2 = f.count(pats)
                st.append(archon.fm_stats())
                _check_against(archon, want, x, pats, lo2, hi2)
                return [lo, hi, lo2, hi2] + list(starts), st
            G.same_under(monkeypatch, grid, call)
            f.close()
        finally:
            b.close()


def test_second_trip_at_the_product_grid(archon, naive):
    """no route: 8192 + 13 patterns of 1-24 bytes on 64 KiB of text, so that waves 0-12 of the 2048 workgroups count a second
    pattern -- counts and the exact rank steps against the KMP scan through the block and a host-built index, and the sorted
    starts of the 7700 patterns with at most four occurrences"""
    n = 65536
    x = S.gen_shape("text", n)
    pats = G.k2_patterns(x)
    count, L = naive(x, pats)
    assert len(pats) == G.K2 > 4 * 2048 and (count[-13:] > 0).any() and (count == 0).sum() > 1000
    b = archon.Block()
    try:
        _, base = b.forward(x)
        lo, hi = b.fm_count(pats)
        _check_against(archon, (count, L, [], []), x, pats, lo, hi)
        st = archon.fm_stats()
        assert st.patterns == G.K2 and st.kernel_launches >= 1
        f = archon.FmIndex(b.read_bwt(), base)
        lo2, hi2 = f.count(pats)
        _check_against(archon, (count, L, [], []), x, pats, lo2, hi2)
        f.close()
        assert (lo2 == lo).all() and (hi2 == hi).all()
        rare = [p for p, c in zip(pats, count) if c <= 4]
        assert len(rare) > 7000
        _, _, starts = naive(x, rare, starts=True)
        got = b.fm_locate(rare)
        assert len(got) == len(rare)
        for p, g, w in zip(rare, got, starts):
            assert (np.sort(g) == w).all(), p
    finally:
        b.close()
