"""GPU: the attached LCP array and the matching statistics (archon_hip_fm_attach_lcp, _fm_attach_lcp_dev,
_block_fm_attach_lcp, _fm_ms, _fm_ms_dev; include/archon_hip.h) against the C brute force of the definition
(tests/fm_ms_naive.c, pinned to the header's procedure by test_fm_ms_abi.py), which decides "occurs" by binary search in the
oracle's suffix array: every record, both work counters, matched and longest; the probe bound; tiny blocks at every fan-out
against the pure Python procedure; the SMEMs that follow from the records against archon_hip_fm_smems of the same handle; the
interface rules; and the other statistics records, which these calls leave alone."""
import numpy as np
import pytest

import archon_synth as S
import fm_ms_naive as N
import fm_naive
import lcp_kasai
import stride_util as G

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
LENGTHS = (12, 32, 63, 64, 65, 100, 127, 129, 1000)     # the records cross the ends of the 64-byte pattern window
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "64"}
DEFAULT_FAN = 16


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return N.build(tmp_path_factory.mktemp("fm_ms_naive"))


@pytest.fixture(scope="module")
def kasai(tmp_path_factory):
    return lcp_kasai.build(tmp_path_factory.mktemp("fm_ms_kasai"))


@pytest.fixture(scope="module")
def dna(oracle, kasai):
    """one block shared by the interface tests: (x, sa, bwt, base, lcp), left unchanged"""
    x = S.gen_dna(256 * KiB)
    sa, bwt, base = oracle.forward(x)
    return x, sa, bwt, base, kasai(x, sa)


def _patterns(x, rng, lengths=LENGTHS, per=2):
    """substrings with 0 .. 3 substitutions, random bytes, chimeras, a byte the block does not hold at the start, in the
    middle and at the end of a substring, m = 0 and m = 1 (the patterns of test_gpu_fm_mem.py).  A block that holds all 256
    byte values has no absent byte and gets no such pattern"""
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


def _levels(n, fan):
    levels, c = 0, n
    while c > 1:
        c = (c + fan - 1) // fan
        levels += 1
    return levels


def _tree_words(n, fan):
    words, c = 0, n
    while c > 1:
        c = (c + fan - 1) // fan
        words += c
    return words


def _check(archon, naive, f, x, sa, lcp, pats, fan=DEFAULT_FAN):
    """ms() of f against the brute force: every record, the counters, the probe bound"""
    w_len, w_lo, w_hi, w_off, steps, parents, matched, longest = naive(x, sa, lcp, pats)
    length, lo, hi, off = f.ms(pats)
    st = archon.fm_ms_stats()
    print("    %d patterns, %d bytes: %d steps, %d parents, %d probes, matched %d, longest %d"
          % (len(pats), st.pattern_bytes, st.steps, st.parents, st.probes, st.matched, st.longest))
    assert (off == w_off).all()
    assert (length == w_len).all()
    assert (lo == w_lo).all() and (hi == w_hi).all()
    assert (st.steps, st.parents, st.matched, st.longest) == (steps, parents, matched, longest)
    assert st.probes <= 2 * (2 * fan - 1) * _levels(x.size, fan) * parents
    assert (st.n, st.patterns, st.pattern_bytes, st.fan, st.levels) == (x.size, len(pats), int(off[-1]), fan, _levels(x.size, fan))
    assert st.steps <= 2 * st.pattern_bytes and st.parents <= st.pattern_bytes
    assert st.lcp_bytes == 4 * x.size + 64 + 4 * _tree_words(x.size, fan) and st.attached == 0 and st.kernel_launches == 1
    return length, lo, hi, off


@pytest.mark.parametrize("shape", S.SHAPES)
def test_256k_against_brute_force(archon, oracle, naive, kasai, shape):
    """all nine shapes at 256 KiB (4 superblocks, 5 hierarchy levels at F = 16): the handle from the oracle's BWT, the LCP
    array from Kasai's algorithm, attached from the host"""
    n = 256 * KiB
    x = _shape(shape, n)
    sa, bwt, base = oracle.forward(x)
    lcp = kasai(x, sa)
    f = archon.FmIndex(bwt, base)
    try:
        f.attach_lcp(lcp)
        st = archon.fm_ms_stats()
        assert (st.attached, st.fan, st.levels, st.n) == (1, DEFAULT_FAN, 5, n)
        rng = np.random.default_rng(n + len(shape))
        pats = _patterns(x, rng)
        if shape in ("text", "dna", "a", "ab", "prose"):
            assert np.bincount(x, minlength=256).min() == 0, "the absent-byte patterns are in"
        length, _, _, _ = _check(archon, naive, f, x, sa, lcp, pats)
        assert length.max() > 0
    finally:
        f.close()


@pytest.mark.parametrize("shape", ["text", "random_copy"])
def test_1mib_through_the_block(archon, oracle, naive, kasai, shape):
    """1 MiB through Block.fm_index(32, lcp=True): the LCP array is made on the device and attached from there; lcp_stats holds
    the LCP step"""
    n = 1 * MiB
    x = _shape(shape, n)
    sa, bwt, base = oracle.forward(x)
    lcp = kasai(x, sa)
    b = archon.Block()
    try:
        _, b0 = b.forward(x)
        assert b0 == base
        f = b.fm_index(32, lcp=True)
        st = archon.fm_ms_stats()
        assert st.attached == 1 and st.ms_lcp > 0 and st.n == n
        ls = archon.lcp_stats()
        assert ls.n == n and ls.max_lcp == int(lcp[1:].max()) and ls.ms_total == st.ms_lcp
        try:
            _check(archon, naive, f, x, sa, lcp, _patterns(x, np.random.default_rng(n + len(shape))))
        finally:
            f.close()
    finally:
        b.close()


@pytest.mark.parametrize("fan", [2, 4, 64])
def test_tiny_blocks_at_every_fan(archon, oracle, fan, monkeypatch):
    """blocks of 1 .. 40 bytes over two and three symbols and of one repeated byte, small rank tables, fan-out 2, 4 and 64:
    patterns of 0 and 1 bytes, longer than the block, with an absent byte first, in the middle and last, and a...ab against
    a x n, against the pure Python procedure"""
    monkeypatch.setenv("ARCHON_REP_FAN", str(fan))
    for k, v in SMALL_ROUTE.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(77)
    for n in (1, 2, 3, 5, 16, 17, 40):
        for sigma in (1, 2, 3):
            x = rng.integers(0, sigma, n, dtype=np.uint8)
            z = bytes([sigma])                                          # the absent byte
            xb = x.tobytes()
            pats = [b"", bytes([0]), z, xb, np.resize(x, n + 1).tobytes(), np.resize(x, 3 * n + 70).tobytes(),
                    rng.integers(0, sigma + 1, 90, dtype=np.uint8).tobytes(), z + xb, xb[:n // 2] + z + xb[n // 2:], xb + z,
                    bytes(n) + b"\x01", bytes(n + 70) + b"\x01", bytes(70) + z + bytes(3)]
            r = N.Rule(xb)
            sa, bwt, base = oracle.forward(x)
            assert list(sa) == r.sa
            f = archon.FmIndex(bwt, base)
            try:
                f.attach_lcp(np.array(r.lcp, np.uint32))
                length, lo, hi, off = f.ms(pats)
                st = archon.fm_ms_stats()
                want = [r.search(P) for P in pats]
                flat = [rec for w in want for rec in w[0]]
                assert list(zip(length.tolist(), lo.tolist(), hi.tolist())) == flat, (n, sigma, fan)
                assert (st.steps, st.parents) == (sum(w[1] for w in want), sum(w[2] for w in want)), (n, sigma, fan)
                assert st.matched == sum(rec[0] for rec in flat) and st.longest == max(rec[0] for rec in flat)
                assert (st.fan, st.levels) == (fan, _levels(n, fan))
                assert st.probes <= 2 * (2 * fan - 1) * st.levels * st.parents
                assert st.lcp_bytes == 4 * n + 64 + 4 * _tree_words(n, fan)
            finally:
                f.close()


@pytest.mark.parametrize("shape", ["text", "dna", "prose"])
def test_smems_from_the_records(archon, oracle, kasai, shape):
    """existing code as the reference: ms_smems of the records equals smems() of the same handle with a mirror, field by field,
    for min_len 1 and 20"""
    n = 256 * KiB
    x = _shape(shape, n)
    sa, bwt, base = oracle.forward(x)
    f = archon.FmIndex(bwt, base)
    try:
        f.mirror(x).attach_lcp(kasai(x, sa))
        pats = _patterns(x, np.random.default_rng(n + 3 * len(shape)))
        length, lo, hi, off = f.ms(pats)
        for min_len in (1, 20):
            got = archon.ms_smems(length, lo, hi, off, min_len)
            _, _, want = f.smems(pats, min_len)
            assert got.size == want.size > 0
            for k in ("lo", "hi", "start", "end", "pattern", "reserved0"):
                assert (got[k] == want[k]).all(), (k, min_len)
    finally:
        f.close()


def test_interface_rules(archon, naive, dna):
    """rows=False gives the same len; the device forms equal the host forms and write nothing else; decreasing offsets are found
    on the device; count and locate of a handle with an array are what they were"""
    import torch
    x, sa, bwt, base, lcp = dna
    n = x.size
    pats = _patterns(x, np.random.default_rng(11), lengths=(12, 32, 65, 100))
    f = archon.FmIndex(bwt, base)
    g = archon.FmIndex(bwt, base)
    try:
        before = f.count(pats)
        f.attach_lcp(lcp)
        after = f.count(pats)
        assert all((u == v).all() for u, v in zip(before, after))
        length, lo, hi, off = _check(archon, naive, f, x, sa, lcp, pats)
        full = archon.fm_ms_stats()
        only, none_lo, none_hi, off2 = f.ms(pats, rows=False)
        st = archon.fm_ms_stats()
        assert none_lo is None and none_hi is None and (only == length).all() and (off2 == off).all()
        assert (st.steps, st.parents, st.probes, st.matched, st.longest) == (full.steps, full.parents, full.probes, full.matched, full.longest)
        assert st.host_syncs == 1 and full.host_syncs == 1

        # the device forms
        g.attach_lcp_dev(torch.from_numpy(lcp.view(np.int32)).to("cuda:0"))
        assert archon.fm_ms_stats().attached == 1
        packed, offs = fm_naive.pack(pats)
        total = int(offs[-1])
        pt = torch.tensor(packed, device="cuda:0")
        ot = torch.tensor(offs.astype(np.int32), device="cuda:0")
        lt, at, bt = (torch.full((total + 8,), -1, dtype=torch.int32, device="cuda:0") for _ in range(3))
        g.ms_dev(pt, ot, lt, at, bt)
        torch.cuda.synchronize()
        st = archon.fm_ms_stats()
        assert st.pattern_bytes == total and (st.steps, st.parents, st.probes) == (full.steps, full.parents, full.probes)
        for t, want in ((lt, length), (at, lo), (bt, hi)):
            got = t.cpu().numpy()
            assert (got[:total].view(np.uint32) == want).all() and (got[total:] == -1).all()
        lt.fill_(-1)
        g.ms_dev(pt, ot, lt)
        torch.cuda.synchronize()
        assert (lt.cpu().numpy()[:total].view(np.uint32) == length).all()
        bad = offs.astype(np.int32).copy()
        bad[3], bad[4] = bad[4], bad[3]
        assert bad[4] < bad[3]
        with pytest.raises(archon.ArchonError) as e:
            g.ms_dev(pt, torch.tensor(bad, device="cuda:0"), lt, at, bt)
        assert e.value.code == archon.E_ARG

        # offsets that do not start at 0: only the records of offsets[0] .. offsets[k] are written
        import pyarchon
        shifted = offs[2:].copy()
        k2 = shifted.size - 1
        l2, a2, b2 = (np.full(total, 7, np.uint32) for _ in range(3))
        archon._check(pyarchon.lib().archon_hip_fm_ms(f.h, pyarchon._p(packed), pyarchon._p(shifted), k2, pyarchon._p(l2), pyarchon._p(a2), pyarchon._p(b2)))
        o0 = int(shifted[0])
        assert o0 > 0 and (l2[:o0] == 7).all() and (a2[:o0] == 7).all() and (b2[:o0] == 7).all()
        assert (l2[o0:] == length[o0:]).all() and (a2[o0:] == lo[o0:]).all() and (b2[o0:] == hi[o0:]).all()
        assert archon.fm_ms_stats().pattern_bytes == total - o0
        # k = 0 writes nothing
        archon._check(pyarchon.lib().archon_hip_fm_ms(f.h, pyarchon._p(packed), pyarchon._p(shifted), 0, pyarchon._p(l2), None, None))
        assert (l2[:o0] == 7).all()
    finally:
        f.close()
        g.close()


def test_refusals(archon, dna):
    """a handle without an LCP array, a handle of another block or a forward without its SA in the block form: ARCHON_E_ARG; the
    handle keeps working"""
    x, sa, bwt, base, lcp = dna
    n = x.size
    f = archon.FmIndex(bwt, base)
    b = archon.Block()
    try:
        with pytest.raises(archon.ArchonError) as e:
            f.ms([b"ACGT"])
        assert e.value.code == archon.E_ARG
        b.forward(x)
        wrong = archon.FmIndex(bwt[:n - 1].copy(), 0)
        with pytest.raises(archon.ArchonError) as e:
            archon._check(archon.lib().archon_hip_block_fm_attach_lcp(b.h, wrong.h))
        assert e.value.code == archon.E_ARG
        wrong.close()
        b.forward(x, want_sa=False)
        with pytest.raises(archon.ArchonError) as e:
            b.fm_index(32, lcp=True)
        assert e.value.code == archon.E_ARG
        with pytest.raises(ValueError):
            f.attach_lcp(lcp[:n - 1])
        lo, hi = f.count([x[50:60].tobytes()])
        assert hi[0] > lo[0]
    finally:
        f.close()
        b.close()


def test_guard_and_replacement(archon, naive, dna):
    """an array with one word >= n is ARCHON_E_CORRUPT and leaves the earlier attachment in place; re-attaching replaces the
    array; lcp_bytes is 4 n + 64 + 4 tree_words before and after"""
    x, sa, bwt, base, lcp = dna
    n = x.size
    pats = _patterns(x, np.random.default_rng(21), lengths=(12, 65, 100))
    want_bytes = 4 * n + 64 + 4 * _tree_words(n, DEFAULT_FAN)
    f = archon.FmIndex(bwt, base)
    try:
        # lcp[0] is read as 0 whatever it holds: no guard on it
        first = lcp.copy()
        first[0] = n + 5
        f.attach_lcp(first)
        assert archon.fm_ms_stats().lcp_bytes == want_bytes
        length, lo, hi, off = _check(archon, naive, f, x, sa, lcp, pats)
        for at, value in ((1, n), (n // 2, n), (n - 1, 0xFFFFFFFF)):
            bad = lcp.copy()
            bad[at] = value
            with pytest.raises(archon.ArchonError) as e:
                f.attach_lcp(bad)
            assert e.value.code == archon.E_CORRUPT
            got = f.ms(pats)
            assert (got[0] == length).all() and (got[1] == lo).all() and (got[2] == hi).all()
        # an array of zeros passes the guard: every parent move goes to the whole block, so a failed byte forgets the match
        f.attach_lcp(np.zeros(n, np.uint32))
        assert archon.fm_ms_stats().lcp_bytes == want_bytes and archon.fm_ms_stats().attached == 1
        zl, zlo, zhi, _ = f.ms(pats)
        st = archon.fm_ms_stats()
        assert st.steps <= 2 * st.pattern_bytes and st.parents <= st.pattern_bytes
        assert (zl <= length).all() and (zl < length).any() and (zlo < zhi).all() and (zhi <= n).all()
        f.attach_lcp(lcp)
        assert archon.fm_ms_stats().lcp_bytes == want_bytes
        got = f.ms(pats)
        assert (got[0] == length).all() and (got[1] == lo).all() and (got[2] == hi).all()
    finally:
        f.close()


def test_other_statistics_unchanged(archon):
    """attach and ms calls leave the forward, FM, sampled, approximate, SMEM, repeats and LZ records of the thread alone; only
    the block form keeps the LCP record of its LCP step"""
    import torch
    n = 256 * KiB
    x = S.gen_text(n)
    b = archon.Block()
    try:
        b.forward(x)
        lcp = b.lcp()
        f = b.fm_index(32, mirror=True)
        pats = [x[q:q + 40].tobytes() for q in (5, 1000, 70000)] + [b"zzzzqq"]
        f.count(pats)
        f.locate(pats)
        f.approx(pats, 1)
        f.smems(pats)
        b.repeats(count_only=True)
        b.lz(count_only=True)

        def records():
            return (archon.stats(), archon.fm_stats().asdict(), archon.fm_walk_stats().asdict(), archon.fm_approx_stats().asdict(),
                    archon.fm_mem_stats().asdict(), archon.repeat_stats().asdict(), archon.lz_stats().asdict())

        before, lcp_before = records(), archon.lcp_stats().asdict()
        f.attach_lcp(lcp)
        f.ms(pats)
        f.ms(pats, rows=False)
        f.attach_lcp_dev(torch.from_numpy(lcp.view(np.int32)).to("cuda:0"))
        f.ms(pats)
        assert records() == before and archon.lcp_stats().asdict() == lcp_before
        g = b.fm_index(32, lcp=True)
        assert (g.ms(pats)[0] == f.ms(pats)[0]).all()
        g.close()
        f.close()
        # fm_index itself builds a table and samples: those two records are its own; the rest stays
        after = records()
        assert (after[0], after[3], after[4], after[5], after[6]) == (before[0], before[3], before[4], before[5], before[6])
    finally:
        b.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, naive, kasai, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text and dna at 64 KiB with some ninety patterns, so that every wave
    takes pattern after pattern: every record, the work counters and the probe bound against the brute force, with and
    without the rows; byte-equal to the same calls without the route, with their counters"""
    for shape in ("text", "dna"):
        x = _shape(shape, 64 * KiB)
        sa, bwt, base = oracle.forward(x)
        lcp = kasai(x, sa)
        f = archon.FmIndex(bwt, base)
        try:
            f.attach_lcp(lcp)
            pats = _patterns(x, np.random.default_rng(64 * KiB + len(shape)))
            f.ms(pats[:1])

            def call():
                length, lo, hi, off = _check(archon, naive, f, x, sa, lcp, pats)
                st = archon.fm_ms_stats()
                only = f.ms(pats, rows=False)
                assert only[1] is None and only[2] is None and (only[0] == length).all()
                return [length, lo, hi, off, only[0]], [st, archon.fm_ms_stats()]
            G.same_under(monkeypatch, grid, call)
        finally:
            f.close()


def test_second_trip_at_the_product_grid(archon, oracle, naive, kasai):
    """no route: 8192 + 13 patterns of 1-24 bytes on 64 KiB of text, so that waves 0-12 of the 2048 workgroups take a second
    pattern: every record and the work counters against the brute force"""
    x = _shape("text", 64 * KiB)
    sa, bwt, base = oracle.forward(x)
    lcp = kasai(x, sa)
    f = archon.FmIndex(bwt, base)
    try:
        f.attach_lcp(lcp)
        pats = G.k2_patterns(x)
        assert len(pats) == G.K2 > 4 * 2048
        length, _, _, off = _check(archon, naive, f, x, sa, lcp, pats)
        assert length[off[-14]:].max() > 0
    finally:
        f.close()
