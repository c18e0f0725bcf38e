"""GPU: the mirror and the SMEM search (archon_hip_fm_mirror, _fm_mirror_dev, _block_fm_mirror, _fm_read_mirror, _fm_smems,
_fm_smems_dev, _fm_locate_mems, _block_fm_locate_mems; include/archon_hip.h) against the C brute force of the definition
(tests/fm_mem_naive.c, pinned to the header's procedure by test_fm_mem_abi.py), which decides "occurs" by binary search in
the oracle's suffix array: every SMEM with its rows in order, nmems, nocc, both step counters and found; the mirror against a
forward transform of the reversed block; the interface rules; the starts from the SA and from the samples; and the other
statistics records, which SMEM calls leave alone."""
import ctypes

import numpy as np
import pytest

import archon_synth as S
import fm_mem_naive as N
import fm_naive
import stride_util as G

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
LENGTHS = (12, 32, 63, 64, 65, 100, 127, 129, 1000)     # both phases cross the ends of the 64-byte pattern window
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "64"}


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return N.build(tmp_path_factory.mktemp("fm_mem_naive"))


def _patterns(x, rng, lengths=LENGTHS, per=2):
    """substrings with 0 .. 3 substitutions, random bytes, chimeras, a byte the block does not hold at the start, in the
    middle and at the end of a substring, m = 0 and m = 1.  A block that holds all 256 byte values (random, random_copy,
    long random motifs) has no absent byte and gets no such pattern; test_256k_against_brute_force asserts that text, dna, a, ab
    and prose do"""
    n = x.size
    pats = []
    for m in lengths:
        if m > n:
            continue
        for subs in range(4):
            for _ in range(per if subs < 3 else 1):
                q = int(rng.integers(0, n - m + 1))
                p = x[q:q + m].copy()
                for _ in range(subs):
                    p[int(rng.integers(0, m))] = rng.integers(0, 256)
                pats.append(p.tobytes())
    for m in (3, 9, 40, 200):
        pats.append(rng.integers(0, 256, m, dtype=np.uint8).tobytes())
    for m1, m2 in ((20, 20), (50, 50), (70, 130), (1, 64)):
        q1, q2 = int(rng.integers(0, n - m1 + 1)), int(rng.integers(0, n - m2 + 1))
        pats.append(x[q1:q1 + m1].tobytes() + x[q2:q2 + m2].tobytes())
    absent = np.flatnonzero(np.bincount(x, minlength=256) == 0)
    if absent.size:
        z = bytes([int(absent[0])])
        q = int(rng.integers(0, n - 80))
        w = x[q:q + 80].tobytes()
        pats += [z + w, w[:40] + z + w[40:], w + z, z, z + z, w[:64] + z, w[:63] + z + w[63:]]
    pats += [b"", x[:1].tobytes(), x[n - 1:].tobytes()]
    return pats


def _check(archon, naive, f, x, sa, pats, min_len=1):
    """smems() of f against the brute force: every field of every SMEM in order, the counts, the counters"""
    want, w_nmems, w_nocc, fwd, bwd, found = naive(x, sa, pats, min_len)
    nmems, nocc, mems = f.smems(pats, min_len)
    st = archon.fm_mem_stats()
    print("    %d patterns, %d bytes: %d SMEMs (%d of any length), %d + %d steps" % (len(pats), st.pattern_bytes, mems.size, found, fwd, bwd))
    assert (nmems == w_nmems).all()
    assert (nocc == w_nocc).all()
    for k in ("lo", "hi", "start", "end", "pattern"):
        assert (mems[k] == want[k]).all(), k
    assert (st.fwd_steps, st.bwd_steps, st.found) == (fwd, bwd, found)
    assert st.mems == mems.size and st.occurrences == int(w_nocc.astype(np.int64).sum())
    assert st.patterns == len(pats) and st.min_len == min_len and st.n == x.size
    return mems


@pytest.mark.parametrize("shape", S.SHAPES)
def test_256k_against_brute_force(archon, oracle, naive, shape):
    """all nine shapes at 256 KiB"""
    n = 256 * KiB
    x = _shape(shape, n)
    sa, bwt, base = oracle.forward(x)
    f = archon.FmIndex(bwt, base)
    try:
        f.mirror(x)
        rng = np.random.default_rng(n + len(shape))
        pats = _patterns(x, rng)
        if shape in ("text", "dna", "a", "ab", "prose"):
            assert np.bincount(x, minlength=256).min() == 0, "the absent-byte patterns are in"
        mems = _check(archon, naive, f, x, sa, pats)
        assert mems.size > 0
        _check(archon, naive, f, x, sa, pats, 20)
    finally:
        f.close()


@pytest.mark.parametrize("shape", ["text", "dna", "random_copy"])
def test_4mib_against_brute_force(archon, oracle, naive, shape):
    """three shapes at 4 MiB, the mirror from the handle's own BWT"""
    n = 4 * MiB
    x = _shape(shape, n)
    sa, bwt, base = oracle.forward(x)
    f = archon.FmIndex(bwt, base)
    try:
        f.mirror()
        rng = np.random.default_rng(n + len(shape))
        _check(archon, naive, f, x, sa, _patterns(x, rng, per=3))
    finally:
        f.close()


def test_tiny_blocks_and_long_patterns(archon, oracle, naive):
    """blocks of 1 .. 40 bytes over two and three symbols: patterns longer than the block, of one byte, of none"""
    rng = np.random.default_rng(77)
    for n in (1, 2, 3, 5, 16, 17, 40):
        for sigma in (2, 3):
            x = rng.integers(0, sigma, n, dtype=np.uint8)
            sa, bwt, base = oracle.forward(x)
            f = archon.FmIndex(bwt, base)
            try:
                f.mirror()
                pats = [np.resize(x, n + 1).tobytes(), np.resize(x, 3 * n + 70).tobytes(), rng.integers(0, sigma + 1, 90, dtype=np.uint8).tobytes(),
                        b"", bytes([0]), bytes([sigma]), x.tobytes(), x[::-1].tobytes()]
                _check(archon, naive, f, x, sa, pats)
            finally:
                f.close()


def test_small_table_routes(archon, oracle, naive, monkeypatch):
    """16-row sub-chunks and 64-row superblocks in both tables: the same results"""
    for k, v in SMALL_ROUTE.items():
        monkeypatch.setenv(k, v)
    x = S.gen_text(64 * KiB)
    sa, bwt, base = oracle.forward(x)
    f = archon.FmIndex(bwt, base)
    try:
        f.mirror()
        _check(archon, naive, f, x, sa, _patterns(x, np.random.default_rng(3)))
    finally:
        f.close()


@pytest.mark.parametrize("n", [256 * KiB + 5, 1 * MiB])
def test_mirror_routes(archon, n):
    """the mirror from the handle's own BWT, from the text (host array, device tensor at an odd address) and from the block
    is the forward transform of the reversed block; its size stays within the header's bound"""
    import torch
    x = S.gen_text(n)
    _, want_bwt, want_base = archon.forward(x[::-1].copy(), want_sa=False)
    b = archon.Block()
    try:
        _, base = b.forward(x)
        bwt = b.read_bwt()
        handles = [archon.FmIndex(bwt, base).mirror(), archon.FmIndex(bwt, base).mirror(x), b.fm_index(32, mirror=True)]
        odd = torch.zeros(n + 3, dtype=torch.uint8, device="cuda:0")
        odd[3:] = torch.from_numpy(x).to("cuda:0")
        handles.append(archon.FmIndex(bwt, base).mirror(odd[3:]))
        st = archon.fm_mem_stats()
        assert st.built == 1 and st.n == n and 0 < st.mirror_bytes <= 1.5 * n + n / 64 + 4096
        for f in handles:
            got_bwt, got_base = f.read_mirror()
            assert got_base == want_base and (got_bwt == want_bwt).all()
            f.close()
    finally:
        b.close()


def test_mirror_refuses(archon):
    """a text with other byte counts: ARCHON_E_ARG; bytes that are no BWT: ARCHON_E_CORRUPT; a handle of another block:
    ARCHON_E_ARG; the handle keeps working without a mirror"""
    n = 64 * KiB
    x = S.gen_text(n)
    b = archon.Block()
    try:
        _, base = b.forward(x)
        f = archon.FmIndex(b.read_bwt(), base)
        other = x.copy()
        other[100] = other[100] + 1 if other[100] != other[101] else other[100] + 2
        with pytest.raises(archon.ArchonError) as e:
            f.mirror(other)
        assert e.value.code == archon.E_ARG
        with pytest.raises(archon.ArchonError) as e:
            f.smems([b"abc"])
        assert e.value.code == archon.E_ARG
        junk = archon.FmIndex(np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8), 5)
        with pytest.raises(archon.ArchonError) as e:
            junk.mirror()
        assert e.value.code == archon.E_CORRUPT
        junk.close()
        wrong = archon.FmIndex(b.read_bwt()[:n - 1].copy(), 0)
        with pytest.raises(archon.ArchonError) as e:
            archon._check(archon.lib().archon_hip_block_fm_mirror(b.h, wrong.h))
        assert e.value.code == archon.E_ARG
        wrong.close()
        lo, hi = f.count([x[50:60].tobytes()])
        assert hi[0] > lo[0]
        # a refused replacement leaves the earlier mirror answering
        f.mirror()
        pats = [x[200:260].tobytes(), x[1000:1020].tobytes() + x[5000:5030].tobytes(), b"abc"]
        nm, no, mems = f.smems(pats)
        mirror_bwt, mirror_base = f.read_mirror()
        assert mems.size >= 2
        with pytest.raises(archon.ArchonError) as e:
            f.mirror(other)
        assert e.value.code == archon.E_ARG
        nm2, no2, mems2 = f.smems(pats)
        assert (nm2 == nm).all() and (no2 == no).all() and (mems2 == mems).all()
        again_bwt, again_base = f.read_mirror()
        assert again_base == mirror_base and (again_bwt == mirror_bwt).all()
        f.close()
    finally:
        b.close()


def test_interface_rules(archon, oracle, naive):
    """count / locate / approx of a mirrored handle are what they were; the device form equals the host form and finds
    decreasing offsets; a cap below the total reports the total and writes nothing; mems=False launches no emit pass; min_len
    filters without changing the counters"""
    import torch
    import pyarchon
    n = 256 * KiB
    x = S.gen_dna(n)
    sa, bwt, base = oracle.forward(x)
    rng = np.random.default_rng(11)
    pats = _patterns(x, rng, lengths=(12, 32, 65, 100))
    f = archon.FmIndex(bwt, base).sample(32)
    try:
        with pytest.raises(archon.ArchonError) as e:
            f.smems(pats)
        assert e.value.code == archon.E_ARG
        short = [p for p in pats if 0 < len(p) <= 32]
        before = (f.count(pats), f.locate(short), f.approx(short, 1))
        f.mirror()
        after = (f.count(pats), f.locate(short), f.approx(short, 1))
        assert all((u == v).all() for u, v in zip(before[0], after[0]))
        assert all((u == v).all() for u, v in zip(before[1], after[1]))
        assert all((u == v).all() for u, v in zip(before[2], after[2]))

        mems = _check(archon, naive, f, x, sa, pats)
        full = archon.fm_mem_stats()
        assert full.kernel_launches == 2
        c_nmems, c_nocc, none = f.smems(pats, mems=False)
        st = archon.fm_mem_stats()
        assert none is None and st.kernel_launches == 1 and st.ms_emit == 0
        nmems, nocc, _ = f.smems(pats)
        assert (c_nmems == nmems).all() and (c_nocc == nocc).all()
        for min_len in (2, 13, 33, 1001):
            m_nmems, _, m_mems = f.smems(pats, min_len)
            st = archon.fm_mem_stats()
            assert (st.fwd_steps, st.bwd_steps, st.found) == (full.fwd_steps, full.bwd_steps, full.found)
            keep = mems[mems["end"] - mems["start"] >= min_len]
            assert (m_mems == keep).all() and m_mems.size == keep.size == int(m_nmems.sum())

        # the device form
        packed, off = fm_naive.pack(pats)
        k = len(pats)
        pt = torch.tensor(packed, device="cuda:0")
        ot = torch.tensor(off.astype(np.int32), device="cuda:0")
        nt = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        ct = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        mt = torch.full((6 * mems.size + 12,), -1, dtype=torch.int32, device="cuda:0")
        assert f.smems_dev(pt, ot, 1, nt, ct, mt) == mems.size
        torch.cuda.synchronize()
        assert (nt.cpu().numpy().view(np.uint32) == nmems).all() and (ct.cpu().numpy().view(np.uint32) == nocc).all()
        md = mt.cpu().numpy()
        assert (md[:6 * mems.size].view(np.uint32).view(pyarchon.FM_MEM) == mems).all() and (md[6 * mems.size:] == -1).all()
        assert archon.fm_mem_stats().pattern_bytes == int(off[-1])
        bad = off.astype(np.int32).copy()
        bad[3], bad[4] = bad[4], bad[3]
        assert bad[4] < bad[3]
        mt.fill_(-1)
        with pytest.raises(archon.ArchonError) as e:
            f.smems_dev(pt, torch.tensor(bad, device="cuda:0"), 1, nt, ct, mt)
        assert e.value.code == archon.E_ARG and (mt.cpu().numpy() == -1).all()

        # the cap rule on the host form
        L = pyarchon.lib()
        small = np.zeros(mems.size - 1, pyarchon.FM_MEM)
        small["lo"] = 7
        nm2, no2 = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        total = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        rc = L.archon_hip_fm_smems(f.h, pyarchon._p(packed), pyarchon._p(off), k, 1, pyarchon._p(nm2), pyarchon._p(no2), pyarchon._p(small),
                                   mems.size - 1, tp)
        assert rc == pyarchon.E_ARG and total.value == mems.size
        assert (nm2 == nmems).all() and (no2 == nocc).all() and (small["lo"] == 7).all()
        assert L.archon_hip_fm_smems(f.h, pyarchon._p(packed), pyarchon._p(off), 0, 1, pyarchon._p(nm2), pyarchon._p(no2), None, 0, tp) == 0
        assert total.value == 0
    finally:
        f.close()


@pytest.mark.parametrize("rate", [1, 32, 1024])
def test_locate_mems(archon, oracle, naive, rate):
    """the starts of every SMEM from a sampled mirrored handle and from the block's SA: sa[r] - (end - start) in row order"""
    n = 256 * KiB
    x = S.gen_prose(n, S.SEED_BASE + 6)
    sa, bwt, base = oracle.forward(x)
    rng = np.random.default_rng(rate)
    pats = _patterns(x, rng, lengths=(12, 32, 100), per=2)
    want, *_ = naive(x, sa, pats, 4)
    b = archon.Block()
    try:
        _, b0 = b.forward(x)
        assert b0 == base
        f = b.fm_index(rate, mirror=True)
        _, _, mems = f.smems(pats, 4)
        assert (mems == want).all() and mems.size > 0
        starts = [sa[int(q["lo"]):int(q["hi"])].astype(np.int64) - (int(q["end"]) - int(q["start"])) for q in want]
        for q, s in zip(want, starts):
            p = pats[int(q["pattern"])][int(q["start"]):int(q["end"])]
            assert all(x[int(v):int(v) + len(p)].tobytes() == p for v in s[:3])
        via_samples = f.locate_mems(mems)
        st = archon.fm_mem_stats()
        assert st.mems == mems.size and st.occurrences == sum(s.size for s in starts) and (st.lf_steps > 0) == (rate > 1)
        via_sa = b.fm_locate_mems(mems)
        assert len(via_samples) == len(via_sa) == len(starts)
        for u, v, w in zip(via_samples, via_sa, starts):
            assert (u == w).all() and (v == w).all()
        # what is refused
        for field, value in (("hi", n + 1), ("lo", n), ("end", 0)):
            bad = mems.copy()
            bad[field][0] = value
            if field == "lo":
                bad["hi"][0] = n - 1
            if field == "end":
                bad["start"][0] = 1
            with pytest.raises(archon.ArchonError):
                f.locate_mems(bad)
            with pytest.raises(archon.ArchonError):
                b.fm_locate_mems(bad)
        f.close()
        plain = archon.FmIndex(bwt, base).mirror()
        with pytest.raises(archon.ArchonError):
            plain.locate_mems(mems)                          # no samples
        plain.close()
    finally:
        b.close()


def test_other_statistics_unchanged(archon):
    """mirror(), smems() and locate_mems() leave the forward, LCP, FM, sampled and approximate records of the thread alone"""
    n = 256 * KiB
    x = S.gen_text(n)
    b = archon.Block()
    try:
        b.forward(x)
        b.lcp()
        f = b.fm_index(32)
        pats = [x[q:q + 40].tobytes() for q in (5, 1000, 70000)] + [b"zzzzqq"]
        f.count(pats)
        f.locate(pats)
        f.approx(pats, 1)

        def records():
            return (archon.stats(), archon.lcp_stats().asdict(), archon.fm_stats().asdict(), archon.fm_walk_stats().asdict(),
                    archon.fm_approx_stats().asdict())

        before = records()
        f.mirror()
        assert records() == before
        assert archon.fm_mem_stats().host_syncs >= 3
        f.mirror(x)
        assert records() == before
        _, _, mems = f.smems(pats)
        assert records() == before
        f.locate_mems(mems)
        b.fm_locate_mems(mems)
        assert records() == before
        g = b.fm_index(32, mirror=True)
        g.close()
        f.close()
    finally:
        b.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, naive, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text and dna at 64 KiB with some ninety patterns, so that every wave
    takes pattern after pattern (one with hundreds of SMEMs ahead of one with none): the brute force's SMEMs, counts and
    step counters at min_len 1 and 20, counting only and emitting; byte-equal to the same calls without the route, with
    their counters"""
    for shape in ("text", "dna"):
        x = _shape(shape, 64 * KiB)
        sa, bwt, base = oracle.forward(x)
        f = archon.FmIndex(bwt, base)
        try:
            f.mirror()
            pats = _patterns(x, np.random.default_rng(64 * KiB + len(shape)))
            f.smems(pats[:1])                # (both tables in use before the calls that are compared)

            def call():
                out, stats = [], []
                for min_len in (1, 20):
                    nmems, nocc, none = f.smems(pats, min_len, mems=False)
                    assert none is None
                    stats.append(archon.fm_mem_stats())
                    mems = _check(archon, naive, f, x, sa, pats, min_len)
                    stats.append(archon.fm_mem_stats())
                    got = f.smems(pats, min_len)
                    assert (got[0] == nmems).all() and (got[1] == nocc).all()
                    out += [nmems, nocc, mems, got[0], got[1]]
                return out, stats
            G.same_under(monkeypatch, grid, call)
        finally:
            f.close()


def test_second_trip_at_the_product_grid(archon, oracle, naive):
    """no route: 8192 + 13 patterns of 1-24 bytes on 64 KiB of text, so that waves 0-12 of the 2048 workgroups take a second
    pattern: the brute force's SMEMs, counts and step counters"""
    x = _shape("text", 64 * KiB)
    sa, bwt, base = oracle.forward(x)
    f = archon.FmIndex(bwt, base)
    try:
        f.mirror()
        pats = G.k2_patterns(x)
        assert len(pats) == G.K2 > 4 * 2048
        mems = _check(archon, naive, f, x, sa, pats)
        assert (mems["pattern"] >= 8192).any()
    finally:
        f.close()
