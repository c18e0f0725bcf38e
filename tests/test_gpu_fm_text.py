"""GPU: the attached suffix array, the matching statistics of a long text and its relative LZ parse (archon_hip_fm_attach_sa*,
_block_fm_attach_sa, _fm_ms_text*, _fm_rlz*; include/archon_hip.h).  Expected records: the C brute force of the definition
(tests/fm_ms_naive.c) with the text as ONE pattern, so no expected record knows about chunks; the counters that follow from the
block, the text and the chunk alone from the Python model (tests/fm_text_naive.py, pinned to the definition by
test_fm_text_abi.py); tiny blocks at every chunk and fan-out against the model; the two worst cases; the parse against the chain
over the expected records; the interface rules; and the other statistics records, which these calls leave alone."""
import numpy as np
import pytest

import archon_synth as S
import fm_ms_naive as N
import fm_text_naive as T
import lcp_kasai
import stride_util as G

pytestmark = pytest.mark.gpu

KiB = 1 << 10
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "64"}
DEFAULT_CHUNK = 1024
CHUNKS = (0, 64, 65, 100)       # the default, then chunk ends on, after and off the 64-byte pattern window of the walk


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return N.build(tmp_path_factory.mktemp("fm_text_naive"))


@pytest.fixture(scope="module")
def kasai(tmp_path_factory):
    return lcp_kasai.build(tmp_path_factory.mktemp("fm_text_kasai"))


def _text(x, rng):
    """32 KiB: an 8 KiB slice of x, a 12 KiB slice with a substitution every ~200 bytes, 4 KiB of random bytes, pieces around an
    absent byte where the block has one, the first 100 and the last 100 bytes of x; padded with further slices of x"""
    n = x.size
    q = int(rng.integers(0, n - 8 * KiB))
    parts = [x[q:q + 8 * KiB]]
    q = int(rng.integers(0, n - 12 * KiB))
    mut = x[q:q + 12 * KiB].copy()
    at = 0
    while True:
        at += int(rng.integers(100, 300))
        if at >= mut.size:
            break
        mut[at] = rng.integers(0, 256)
    parts.append(mut)
    parts.append(rng.integers(0, 256, 4 * KiB, dtype=np.uint8))
    absent = np.flatnonzero(np.bincount(x, minlength=256) == 0)
    if absent.size:
        z = np.array([absent[0]], np.uint8)
        q = int(rng.integers(0, n - 300))
        w = x[q:q + 300]
        parts += [z, w[:64], z, w[:63], z, z, w[:130], z, w[130:]]
    parts += [x[:100], x[n - 100:]]
    have = sum(p.size for p in parts)
    while have < 32 * KiB:
        m = min(32 * KiB - have, 1500)
        q = int(rng.integers(0, n - m))
        parts.append(x[q:q + m])
        have += m
    return np.concatenate(parts)[:32 * KiB].copy()


_REFERENCE = {}


def _reference(oracle, naive, kasai, shape):
    """(x, sa, bwt, base, lcp, text, (len, lo, hi)) of a shape at 64 KiB: computed once, shared, left unchanged"""
    if shape not in _REFERENCE:
        n = 64 * KiB
        x = _shape(shape, n)
        sa, bwt, base = oracle.forward(x)
        lcp = kasai(x, sa)
        text = _text(x, np.random.default_rng(n + len(shape)))
        w_len, w_lo, w_hi = naive(x, sa, lcp, [text.tobytes()])[:3]
        for a in (x, sa, bwt, lcp, text, w_len, w_lo, w_hi):
            a.setflags(write=False)
        _REFERENCE[shape] = (x, sa, bwt, base, lcp, text, (w_len, w_lo, w_hi))
    return _REFERENCE[shape]


def _index(archon, bwt, base, lcp, sa):
    return archon.FmIndex(bwt, base).attach_lcp(lcp).attach_sa(sa)


def _check_stats(st, n, m, C, want):
    assert (st.n, st.m, st.chunk, st.chunks) == (n, m, C, T.chunks_of(m, C))
    assert (st.saturated, st.full_chunks, st.runs, st.longest_run) == (want["saturated"], want["full_chunks"], want["runs"], want["longest_run"])
    assert st.sa_bytes == 4 * n + 4 * (n + 1)


@pytest.mark.parametrize("shape", S.SHAPES)
def test_64k_against_brute_force(archon, oracle, naive, kasai, shape, monkeypatch):
    """all nine shapes at a 64 KiB block and a 32 KiB text, at the default chunk and at 64, 65 and 100: every len, lo and hi, and
    the four counters that follow from x, P and C"""
    x, sa, bwt, base, lcp, text, (w_len, w_lo, w_hi) = _reference(oracle, naive, kasai, shape)
    n, m = x.size, text.size
    # the condition, from the model before the GPU is asked
    at64 = T.counters(T.walk_len_of(w_len, 64), 64)
    print("    %s at C = 64: %s" % (shape, at64))
    assert at64["saturated"] > 0 and at64["full_chunks"] >= 8 and at64["longest_run"] >= 3
    if shape in ("text", "dna", "a", "ab", "prose"):
        assert (w_len == 0).any(), "the absent-byte pieces are in"
    f = _index(archon, bwt, base, lcp, sa)
    try:
        for chunk in CHUNKS:
            monkeypatch.setenv("ARCHON_MS_CHUNK", str(chunk))
            C = chunk or DEFAULT_CHUNK
            length, lo, hi = f.ms_text(text)
            st = archon.fm_text_stats()
            print("    C = %d: %s" % (C, st.asdict()))
            assert (length == w_len).all(), C
            assert (lo == w_lo).all() and (hi == w_hi).all(), C
            _check_stats(st, n, m, C, T.counters(T.walk_len_of(w_len, C), C))
            assert (st.matched, st.longest) == (int(w_len.sum(dtype=np.uint64)), int(w_len.max()))
            assert (st.kernel_launches, st.host_syncs) == (4, 1)
    finally:
        f.close()


@pytest.mark.parametrize("fan", [2, 4, 16])
def test_tiny_blocks_at_every_chunk_and_fan(archon, oracle, fan, monkeypatch):
    """blocks of 1 .. 300 bytes over one to three symbols, small rank tables, texts up to 200 bytes, chunks of 1, 2, 3, 63 and
    64 bytes: the records and the four counters of the Python model"""
    monkeypatch.setenv("ARCHON_REP_FAN", str(fan))
    for k, v in SMALL_ROUTE.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(700 + fan)
    joins = 0
    for n in (1, 2, 3, 17, 64, 65, 300):
        for sigma in (1, 2, 3):
            x = rng.integers(0, sigma, n, dtype=np.uint8)
            xb = x.tobytes()
            z = bytes([sigma])                                          # the absent byte
            texts = [xb, np.resize(x, 200).tobytes(), rng.integers(0, sigma + 1, 150, dtype=np.uint8).tobytes(),
                     xb[:n // 2] + z + xb[n // 2:], bytes(min(n, 199)) + b"\x01", xb[n // 3:][:70] + xb[:50], z, xb[:1]]
            model = T.Model(xb)
            sa, bwt, base = oracle.forward(x)
            assert list(sa) == model.sa
            f = _index(archon, bwt, base, np.array(model.rule.lcp, np.uint32), sa)
            try:
                for C in (1, 2, 3, 63, 64):
                    monkeypatch.setenv("ARCHON_MS_CHUNK", str(C))
                    for P in texts:
                        want, ctr = model.run(P, C)
                        length, lo, hi = f.ms_text(P)
                        assert list(zip(length.tolist(), lo.tolist(), hi.tolist())) == want, (n, sigma, fan, C, P)
                        st = archon.fm_text_stats()
                        _check_stats(st, n, len(P), C, ctr)
                        assert (st.fan, st.matched) == (fan, sum(r[0] for r in want))
            finally:
                f.close()
            joins += model.joins
    assert joins > 10000


def test_worst_cases(archon, oracle, naive, kasai, monkeypatch):
    """64 KiB at C = 64.  The block as its own text: 1024 full chunks, one chain of chunks - 2 joins, every record of the
    definition.  a...ab on a block of one repeated byte: the records of ms([text]) of the same handle"""
    monkeypatch.setenv("ARCHON_MS_CHUNK", "64")
    x, sa, bwt, base, lcp, _, _ = _reference(oracle, naive, kasai, "text")
    n = x.size
    f = _index(archon, bwt, base, lcp, sa)
    try:
        length, lo, hi = f.ms_text(x)
        st = archon.fm_text_stats()
        print("    the block itself: %s" % st.asdict())
        assert (st.chunks, st.full_chunks, st.runs, st.longest_run, st.saturated) == (1024, 1024, 1, 1022, n - 64)
        assert (length == np.arange(1, n + 1)).all()
        isa = np.zeros(n + 1, np.int64)
        isa[sa] = np.arange(n)
        # x[0 .. e) ends at item e and at the items that share its whole key: the last e with a longer match has lcp >= e
        assert (lo <= isa[1:]).all() and (isa[1:] < hi).all()
        w_len, w_lo, w_hi = naive(x, sa, lcp, [x[:2000].tobytes()])[:3]
        assert (lo[:2000] == w_lo).all() and (hi[:2000] == w_hi).all() and (length[:2000] == w_len).all()
        one, one_lo, one_hi, _ = f.ms([x.tobytes()])
        assert (one == length).all() and (one_lo == lo).all() and (one_hi == hi).all()
    finally:
        f.close()
    a = np.zeros(n, np.uint8) + 97
    sa, bwt, base = oracle.forward(a)
    f = _index(archon, bwt, base, kasai(a, sa), sa)
    try:
        text = a.copy()
        text[n - 1] = 98
        length, lo, hi = f.ms_text(text)
        st = archon.fm_text_stats()
        print("    a...ab: %s" % st.asdict())
        assert (st.chunks, st.full_chunks, st.runs, st.longest_run) == (1024, 1023, 1, 1022)
        assert (length[:n - 1] == np.arange(1, n)).all() and (length[n - 1], lo[n - 1], hi[n - 1]) == (0, 0, n)
        assert (lo[:n - 1] == 0).all() and (hi[:n - 1] == n - np.arange(1, n) + 1).all()
        one, one_lo, one_hi, _ = f.ms([text.tobytes()])
        assert (one == length).all() and (one_lo == lo).all() and (one_hi == hi).all()
    finally:
        f.close()


@pytest.mark.parametrize("shape", ["text", "dna", "random_copy"])
def test_rlz(archon, oracle, naive, kasai, shape):
    """the phrases are the chain of the parse over the expected (len, sa[lo]) records; rlz_decode gives the text back; the
    lengths, a literal read as 1, sum to m; the cap rule"""
    import pyarchon
    x, sa, bwt, base, lcp, text, (w_len, w_lo, _) = _reference(oracle, naive, kasai, shape)
    m = text.size
    f = _index(archon, bwt, base, lcp, sa)
    try:
        rec = np.zeros(m, archon.LPF)
        rec["len"] = w_len
        rec["src"] = np.where(w_len > 0, sa[np.minimum(w_lo, x.size - 1)], 0)
        want = archon.lz_parse(rec)
        assert [tuple(int(v) for v in p) for p in want[:50]] == T.chain(list(zip(w_len.tolist(), rec["src"].tolist())))[:50]
        lz_before = archon.lz_stats().asdict()
        got = f.rlz(text)
        st = archon.fm_text_stats()
        print("    %s: %d phrases of %d bytes, %s" % (shape, got.size, m, st.asdict()))
        assert archon.lz_stats().asdict() == lz_before
        assert got.size == want.size == st.phrases and (got == want).all()
        assert int(np.maximum(got["len"], 1).sum()) == m
        lit = got["len"] == 0
        assert (archon.rlz_decode(x, got, m, text[got["end"][lit] - 1]) == text).all()
        if lit.any():
            with pytest.raises(ValueError):
                archon.rlz_decode(x, got, m)
        assert f.rlz(text, count_only=True) == want.size
        # the cap rule: a cap too small leaves out untouched and writes total
        import ctypes
        total = ctypes.c_uint64(7)
        out = np.zeros(want.size, archon.PHRASE)
        out.view(np.uint8)[:] = 0xAB
        keep = out.copy()
        padded = np.concatenate([text, np.zeros(1, np.uint8)])
        rc = pyarchon.lib().archon_hip_fm_rlz(f.h, pyarchon._p(padded), m, pyarchon._p(out), want.size - 1,
                                              ctypes.cast(ctypes.byref(total), ctypes.c_void_p))
        assert rc == archon.E_ARG and total.value == want.size and (out == keep).all()
    finally:
        f.close()


def test_interface_rules(archon, oracle, naive, kasai, monkeypatch):
    """no SA or no LCP array: ARCHON_E_ARG; an sa holding 0 or n + 1: ARCHON_E_CORRUPT and the earlier attachment still answers;
    lo without hi; m = 0; m > n; the device forms equal the host forms and write nothing else; rows=False gives the same len"""
    import ctypes
    import pyarchon
    import torch
    monkeypatch.setenv("ARCHON_MS_CHUNK", "100")
    x, sa, bwt, base, lcp, text, (w_len, w_lo, w_hi) = _reference(oracle, naive, kasai, "dna")
    n, m = x.size, text.size
    L = pyarchon.lib()
    f = archon.FmIndex(bwt, base)
    g = archon.FmIndex(bwt, base)
    try:
        with pytest.raises(archon.ArchonError) as e:
            f.ms_text(text)
        assert e.value.code == archon.E_ARG
        f.attach_sa(sa)
        assert archon.fm_text_stats().sa_bytes == 8 * n + 4
        with pytest.raises(archon.ArchonError) as e:
            f.rlz(text)
        assert e.value.code == archon.E_ARG                                   # an SA and no LCP array
        g.attach_lcp(lcp)
        with pytest.raises(archon.ArchonError) as e:
            g.ms_text(text)
        assert e.value.code == archon.E_ARG                                   # an LCP array and no SA
        f.attach_lcp(lcp)
        length, lo, hi = f.ms_text(text)
        assert (length == w_len).all() and (lo == w_lo).all() and (hi == w_hi).all()
        full = archon.fm_text_stats()
        for at, value in ((0, 0), (n // 2, n + 1), (n - 1, 0xFFFFFFFF)):
            bad = sa.copy()
            bad[at] = value
            with pytest.raises(archon.ArchonError) as e:
                f.attach_sa(bad)
            assert e.value.code == archon.E_CORRUPT
            got = f.ms_text(text)
            assert (got[0] == w_len).all() and (got[1] == w_lo).all() and (got[2] == w_hi).all()
        with pytest.raises(ValueError):
            f.attach_sa(sa[:n - 1])
        only, none_lo, none_hi = f.ms_text(text, rows=False)
        st = archon.fm_text_stats()
        assert none_lo is None and none_hi is None and (only == w_len).all()
        assert (st.saturated, st.sa_probes, st.lcp_probes, st.host_syncs) == (full.saturated, full.sa_probes, full.lcp_probes, 1)
        # lo without hi, m = 0
        padded = np.concatenate([text, np.zeros(1, np.uint8)])
        a, b = np.full(m, 7, np.uint32), np.full(m, 7, np.uint32)
        assert L.archon_hip_fm_ms_text(f.h, pyarchon._p(padded), m, pyarchon._p(a), pyarchon._p(b), None) == archon.E_ARG
        assert L.archon_hip_fm_ms_text(f.h, pyarchon._p(padded), m, pyarchon._p(a), None, pyarchon._p(b)) == archon.E_ARG
        assert L.archon_hip_fm_ms_text(f.h, pyarchon._p(padded), 0, pyarchon._p(a), pyarchon._p(b), pyarchon._p(b)) == 0
        assert (a == 7).all() and (b == 7).all()
        assert f.ms_text(b"")[0].size == 0 and f.rlz(b"").size == 0
        # a text longer than the block: the block twice, at C = 100
        twice = np.concatenate([x, x])
        length2, lo2, hi2 = f.ms_text(twice)
        one, one_lo, one_hi, _ = f.ms([twice.tobytes()])
        assert (length2 == one).all() and (lo2 == one_lo).all() and (hi2 == one_hi).all()
        assert (length2[:n] == np.arange(1, n + 1)).all() and length2.max() == n

        # the device forms
        g.attach_sa_dev(torch.from_numpy(sa.copy().view(np.int32)).to("cuda:0"))
        tt = torch.from_numpy(text.copy()).to("cuda:0")
        lt, at_, bt = (torch.full((m + 8,), -1, dtype=torch.int32, device="cuda:0") for _ in range(3))
        g.ms_text_dev(tt, lt, at_, bt)
        torch.cuda.synchronize()
        st = archon.fm_text_stats()
        assert (st.saturated, st.sa_probes, st.lcp_probes, st.host_syncs, st.kernel_launches) == (full.saturated, full.sa_probes, full.lcp_probes, 1, 4)
        for t, want in ((lt, w_len), (at_, w_lo), (bt, w_hi)):
            got = t.cpu().numpy()
            assert (got[:m].view(np.uint32) == want).all() and (got[m:] == -1).all()
        lt.fill_(-1)
        g.ms_text_dev(tt, lt)
        torch.cuda.synchronize()
        got = lt.cpu().numpy()
        assert (got[:m].view(np.uint32) == w_len).all() and (got[m:] == -1).all()
        want = f.rlz(text)
        assert g.rlz_dev(tt) == want.size
        ot = torch.full((3 * want.size + 6,), -1, dtype=torch.int32, device="cuda:0")
        assert g.rlz_dev(tt, ot) == want.size
        torch.cuda.synchronize()
        got = ot.cpu().numpy()
        assert (got[:3 * want.size].view(np.uint32) == want.view(np.uint32)).all() and (got[3 * want.size:] == -1).all()
        with pytest.raises(archon.ArchonError) as e:
            g.rlz_dev(tt, ot[:3 * (want.size - 1)])
        assert e.value.code == archon.E_ARG
    finally:
        f.close()
        g.close()


def test_other_statistics_unchanged(archon):
    """attach_sa, ms_text and rlz leave the forward, LCP, FM, sampled, approximate, SMEM, matching-statistics, repeats and LZ
    records of the thread alone (the list of test_gpu_fm_ms.py, with its own record added)"""
    import torch
    n = 64 * KiB
    x = S.gen_text(n)
    b = archon.Block()
    try:
        sa, _ = b.forward(x)
        lcp = b.lcp()
        f = b.fm_index(32, mirror=True, lcp=True)
        pats = [x[q:q + 40].tobytes() for q in (5, 1000, 7000)] + [b"zzzzqq"]
        f.count(pats)
        f.locate(pats)
        f.approx(pats, 1)
        f.smems(pats)
        f.ms(pats)
        b.repeats(count_only=True)
        b.lz(count_only=True)

        def records():
            return (archon.stats(), archon.lcp_stats().asdict(), archon.fm_stats().asdict(), archon.fm_walk_stats().asdict(),
                    archon.fm_approx_stats().asdict(), archon.fm_mem_stats().asdict(), archon.fm_ms_stats().asdict(),
                    archon.repeat_stats().asdict(), archon.lz_stats().asdict())

        before = records()
        f.attach_sa(sa)
        text = np.concatenate([x[3000:9000], x[100:4000]])
        f.ms_text(text)
        f.ms_text(text, rows=False)
        f.rlz(text)
        f.attach_sa_dev(torch.from_numpy(sa.view(np.int32)).to("cuda:0"))
        f.rlz(text, count_only=True)
        assert records() == before
        assert archon._check(archon.lib().archon_hip_block_fm_attach_sa(b.h, f.h)) == 0
        assert records() == before
        f.close()
    finally:
        b.close()


def test_block_form(archon, oracle, naive, kasai):
    """256 KiB of DNA: Block.fm_index(32, lcp=True, sa=True) gives the records and the phrases of the host-attached handle;
    the refusals of the block form are those of the LCP attachment"""
    n = 256 * KiB
    x = S.gen_dna(n)
    sa, bwt, base = oracle.forward(x)
    text = _text(x, np.random.default_rng(5))
    h = _index(archon, bwt, base, kasai(x, sa), sa)
    b = archon.Block()
    try:
        _, b0 = b.forward(x)
        assert b0 == base
        f = b.fm_index(32, lcp=True, sa=True)
        try:
            assert archon.fm_text_stats().sa_bytes == 8 * n + 4
            want, got = h.ms_text(text), f.ms_text(text)
            assert all((u == v).all() for u, v in zip(want, got))
            w_len, w_lo, w_hi = naive(x, sa, kasai(x, sa), [text[:3000].tobytes()])[:3]
            assert (got[0][:3000] == w_len).all() and (got[1][:3000] == w_lo).all() and (got[2][:3000] == w_hi).all()
            assert (h.rlz(text) == f.rlz(text)).all()
            wrong = archon.FmIndex(bwt[:n - 1].copy(), 0)
            with pytest.raises(archon.ArchonError) as e:
                archon._check(archon.lib().archon_hip_block_fm_attach_sa(b.h, wrong.h))
            assert e.value.code == archon.E_ARG
            wrong.close()
            b.forward(x, want_sa=False)
            with pytest.raises(archon.ArchonError) as e:
                b.fm_index(32, sa=True)
            assert e.value.code == archon.E_ARG
            assert (f.ms_text(text)[0] == want[0]).all()          # the handle outlives the forward
        finally:
            f.close()
    finally:
        h.close()
        b.close()


@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, naive, kasai, grid, chunk, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) at the default chunk (32 chunks: every wave walks several) and at
    ARCHON_MS_CHUNK=64 (512 chunks), on text and dna: every len, lo and hi of ms_text against the brute force, the counters of
    the model, and the phrases of rlz against the chain over the expected records, counted and emitted; byte-equal to the same
    calls without the route, with their counters, launches and host waits"""
    if chunk:
        monkeypatch.setenv("ARCHON_MS_CHUNK", str(chunk))
    C = chunk or DEFAULT_CHUNK
    for shape in ("text", "dna"):
        x, sa, bwt, base, lcp, text, (w_len, w_lo, w_hi) = _reference(oracle, naive, kasai, shape)
        n, m = x.size, text.size
        rec = np.zeros(m, archon.LPF)
        rec["len"] = w_len
        rec["src"] = np.where(w_len > 0, sa[np.minimum(w_lo, n - 1)], 0)
        chain = T.chain(list(zip(w_len.tolist(), rec["src"].tolist())))
        want_counters = T.counters(T.walk_len_of(w_len, C), C)
        f = _index(archon, bwt, base, lcp, sa)
        try:
            def call():
                length, lo, hi = f.ms_text(text)
                st = archon.fm_text_stats()
                assert (length == w_len).all() and (lo == w_lo).all() and (hi == w_hi).all()
                _check_stats(st, n, m, C, want_counters)
                assert (st.matched, st.longest) == (int(w_len.sum(dtype=np.uint64)), int(w_len.max()))
                assert (st.kernel_launches, st.host_syncs) == (4, 1)
                only = f.ms_text(text, rows=False)
                assert (only[0] == w_len).all() and only[1] is None
                st2 = archon.fm_text_stats()
                got = f.rlz(text)
                st3 = archon.fm_text_stats()
                assert got.size == len(chain) == st3.phrases and [tuple(int(v) for v in p) for p in got] == chain
                assert f.rlz(text, count_only=True) == got.size
                return [length, lo, hi, only[0], got], [st, st2, st3, archon.fm_text_stats()]
            G.same_under(monkeypatch, grid, call)
        finally:
            f.close()
