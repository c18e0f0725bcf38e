"""GPU: the suffix-prefix overlaps (include/archon_hip.h, archon_hip_fm_attach_ends*, _block_fm_attach_ends, _fm_overlaps*)
against tests/fm_ovl_naive.py, the model over a suffix array that tests/test_fm_ovl_abi.py pins to the definition by the text:
every case compares the records byte for byte, and novl, the total and the counters, with the model's."""
import ctypes
import itertools

import numpy as np
import pytest

import archon_synth as S
import fm_ovl_naive as N
import stride_util as G

pytestmark = pytest.mark.gpu

RATE = 32
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "64"}
COUNTERS = ("steps", "tested", "hit", "overlaps", "longest")

_refs = {}


def _letters(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].copy()


def _reference(oracle, key, make):
    """(x, sa, bwt, base, walker) of the CPU oracle for the block make(): computed once, shared, left unchanged"""
    if key not in _refs:
        x = make()
        sa, bwt, base = oracle.forward(x)
        for a in (x, sa, bwt):
            a.setflags(write=False)
        _refs[key] = (x, sa, bwt, int(base), N.Walker(x, sa))
    return _refs[key]


def _dev(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _zeros(n):
    import torch
    return torch.zeros(max(n, 1), dtype=torch.int32, device="cuda:0")


def _host(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def _pack(pats):
    import pyarchon
    return pyarchon._pack_patterns(pats)


def _stats(archon, w, D, pats, min_len, ctr, emitted, attached=0):
    """the record of the last overlap call against the model's counters"""
    st = archon.fm_ovl_stats()
    got = {key: getattr(st, key) for key in ("n", "docs", "queries", "min_len", "attached", "pattern_bytes", "emitted", "end_bytes") + COUNTERS}
    want = dict(n=w.n, docs=D, queries=len(pats), min_len=min_len, attached=attached, pattern_bytes=sum(len(bytes(p)) for p in pats),
                emitted=emitted, end_bytes=N.end_bytes(w.n, D), **{key: ctr[key] for key in COUNTERS})
    assert got == want
    return st


_ZERO = dict(steps=0, tested=0, hit=0, overlaps=0, longest=0)


def _same(got, want):
    equal = got.tobytes() == want.tobytes()             # (compared outside the assert: pytest would diff kilobytes)
    assert got.dtype == want.dtype and got.size == want.size and equal


def _check(archon, f, w, ends, pats, min_len, dev_forms=True, m=None):
    """the host search with and without records and the device search against the model; returns the model's answer"""
    rec, novl, ctr = m if m is not None else N.model(w, ends, pats, min_len)
    D = len(ends)
    gn, gr = f.overlaps(pats, min_len)
    assert (gn == novl).all()
    _same(gr, rec)
    _stats(archon, w, D, pats, min_len, ctr, rec.size)
    gn, none = f.overlaps(pats, min_len, emit=False)
    assert none is None and (gn == novl).all()
    _stats(archon, w, D, pats, min_len, ctr, 0)
    if dev_forms and pats:
        packed, off = _pack(pats)
        pat_t, off_t, novl_t, rec_t = _dev(packed), _dev(off), _zeros(len(pats)), _zeros(4 * rec.size)
        assert f.overlaps_dev(pat_t, off_t, min_len, novl_t, rec_t) == rec.size
        assert (_host(novl_t, len(pats)) == novl).all()
        _same(_host(rec_t, 4 * rec.size).view(archon.FM_OVL), rec)
        _stats(archon, w, D, pats, min_len, ctr, rec.size)
        novl_t.zero_()
        assert f.overlaps_dev(pat_t, off_t, min_len, novl_t) == rec.size
        assert (_host(novl_t, len(pats)) == novl).all()
        _stats(archon, w, D, pats, min_len, ctr, 0)
    return rec, novl, ctr


def _handle(archon, bwt, base, sa, ends):
    return archon.FmIndex(bwt, base).attach_sa(sa).attach_ends(ends)


@pytest.mark.parametrize("n", (1, 2, 5))
def test_tiny_blocks(archon, oracle, n):
    """n = 1, 2, 5 with D = 1, with D = n (every item an end), with ends[D-1] = n (the end row is the primary row) and with
    ends[D-1] = n - 1; every query of up to 3 bytes, the block itself and a query longer than the block"""
    x, sa, bwt, base, w = _reference(oracle, ("tiny", n), lambda: _letters(n, n, b"ab"))
    pats = [bytes(p) for m in (1, 2, 3) for p in itertools.product(b"ab", repeat=m)] + [x.tobytes(), x.tobytes() + b"a", b""]
    sets = [[n], list(range(1, n + 1))] + ([[n - 1], list(range(1, n))] if n > 1 else []) + ([[1, n]] if n > 2 else [])
    seen = 0
    for ends in sets:
        f = _handle(archon, bwt, base, sa, ends)
        try:
            _stats(archon, w, len(ends), [], 0, _ZERO, 0, attached=1)
            for min_len in (1, 2):
                rec, _, _ = _check(archon, f, w, ends, pats, min_len)
                seen += rec.size
                if ends[-1] == n and min_len == 1:
                    assert (rec["row"] == base).any(), "the primary row is an end row and is found"
        finally:
            f.close()
    assert seen > 0


@pytest.mark.parametrize("n", (255, 256, 257, 512, 513))
def test_directory_edges(archon, oracle, n):
    """end rows forced at rows 0, 255, 256 and n - 1 (by isa of the oracle's suffix array) among random others; queries whose
    ranges end at hi = n (at n % 256 == 0 that rank reads no block) and ranges that begin and end inside one 32-byte block"""
    x, sa, bwt, base, w = _reference(oracle, ("edges", n), lambda: _letters(n, n))
    rng = np.random.default_rng(n)
    rows = sorted({r for r in (0, 255, 256, n - 1) if r < n} | set(rng.integers(0, n, 24).tolist()))
    ends = np.sort(np.asarray(sa, np.int64)[rows]).astype(np.uint32)
    last = int(sa[n - 1])
    pats = [x[last - l:last].tobytes() for l in range(1, min(last, 8) + 1)]                    # row n - 1 holds them: hi = n
    pats += [x[s - l:s].tobytes() for r in (0, 255, 256) if r < n for s in [int(sa[r])] for l in range(1, min(s, 8) + 1)]
    pats += [x[q:q + m].tobytes() for q, m in zip(rng.integers(0, n - 12, 200).tolist(), rng.integers(1, 13, 200).tolist())]
    ranges = [r for P in pats for r in w.walk(P)[0]]
    assert any(hi == n for lo, hi in ranges) and any(lo >> 8 == hi >> 8 and hi - lo > 1 and lo & 255 for lo, hi in ranges)
    assert any(lo == 0 for lo, hi in ranges) and (n <= 257 or any(lo <= 255 and hi >= 257 for lo, hi in ranges))
    f = _handle(archon, bwt, base, sa, ends)
    try:
        for min_len in (1, 3):
            rec, _, _ = _check(archon, f, w, ends, pats, min_len, dev_forms=min_len == 1)
            if min_len == 1:
                assert {0, n - 1} <= set(rec["row"].tolist()) and (n <= 256 or {255, 256} <= set(rec["row"].tolist()))
    finally:
        f.close()


def test_query_lengths(archon, oracle):
    """queries of 0, 1, 63, 64, 65 and 130 bytes (the second and third 64-byte window of the pattern) with documents that end at
    every one of those lengths, min_len above m, m > n, a first byte the block does not hold and a query that dies after its
    first byte"""
    n = 4096
    x, sa, bwt, base, w = _reference(oracle, ("lengths", n), lambda: _letters(n, 4096))
    p = 1000
    ends = sorted({p + l for l in (1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130)} | {7, 300, 2500, n})
    pats = [x[p:p + m].tobytes() for m in (0, 1, 63, 64, 65, 130)] + [x.tobytes() + x.tobytes(), b"\xff" + x[:9].tobytes(),
                                                                       x[p:p + 1].tobytes() + b"\xff", x[p:p + 64].tobytes() + b"\xff" + x[:70].tobytes()]
    f = _handle(archon, bwt, base, sa, ends)
    try:
        for min_len in (1, 64, 131, n, n + 1):
            rec, novl, ctr = _check(archon, f, w, ends, pats, min_len)
            if min_len == 1:
                assert {1, 63, 64, 65, 128, 129, 130, n} <= set(rec["len"].tolist()) and ctr["longest"] == n
                assert novl[0] == 0 and novl[7] == 0 and novl[6] >= 1
            if min_len == n + 1:
                assert rec.size == 0 and ctr["tested"] == 0 and ctr["steps"] > 0
    finally:
        f.close()


def _copies():
    return np.frombuffer(b"ACGTTGCA\n" * 200, np.uint8).copy()


@pytest.mark.parametrize("D", (65, 128, 129, 200))
def test_more_than_64_overlaps_in_one_range(archon, oracle, D):
    """200 copies of ACGTTGCA\\n, the ends of the first D of them with trim = 1: every prefix of TGCA... and of ACGTTGCA that a
    document ends with has D end rows in one range, which crosses the 64-lane emit chunk at 65, 128 and 129"""
    x, sa, bwt, base, w = _reference(oracle, "copies", _copies)
    ends = archon.ends_from_bounds(np.arange(0, 9 * 200 + 1, 9), trim=1)[:D]
    pats = [b"TGCAZZ", b"TGCA\nACGT", b"ACGTTGCA", b"A", b"CA", b"GCATT", b"\nACG", b"TTGCA\nACGTTGCA\nAC"]
    f = _handle(archon, bwt, base, sa, ends)
    try:
        rec, novl, ctr = _check(archon, f, w, ends, pats, 1)
        assert novl.tolist() == [D, D, 2 * D, D, D, D, 0, 2 * D - 1]      # (the last: 5 bytes, and 14 that begin in the document before)
        rec, novl, ctr = _check(archon, f, w, ends, pats, 4)
        assert novl.tolist() == [D, D, D, 0, 0, 0, 0, 2 * D - 1]
    finally:
        f.close()


def _block4k():
    return S.gen_shape("dna", 4096)


def _case4k(oracle):
    x, sa, bwt, base, w = _reference(oracle, "4k", _block4k)
    rng = np.random.default_rng(44)
    ends = np.unique(np.concatenate([rng.integers(1, x.size + 1, 300), [x.size]])).astype(np.uint32)
    pats = []
    for j in range(600):
        m = int(rng.integers(1, 40))
        e = int(ends[rng.integers(0, ends.size)]) if j % 2 else int(rng.integers(40, x.size))
        q = max(0, e - int(rng.integers(1, m + 1)))
        pats.append(x[q:q + m].tobytes())
    if "4k-model" not in _refs:
        _refs["4k-model"] = N.model(w, ends, pats, 3)
    return x, sa, bwt, base, w, ends, pats, _refs["4k-model"]


def test_small_table_routes(archon, oracle, monkeypatch):
    """16-row sub-chunks and 64-row superblocks on a 4 KiB block: lo and hi cross sub-chunks and superblocks at nearly every step;
    the same records"""
    for k, v in SMALL_ROUTE.items():
        monkeypatch.setenv(k, v)
    x, sa, bwt, base, w, ends, pats, m = _case4k(oracle)
    f = _handle(archon, bwt, base, sa, ends)
    try:
        assert m[0].size > 500
        _check(archon, f, w, ends, pats, 3, m=m)
    finally:
        f.close()


def test_resident_form_against_the_handle_form(archon, oracle):
    """Block.fm_index(32, ends=e), FmIndex(bwt, base).attach_sa(sa).attach_ends(e) and attach_ends_dev give byte-equal records, the
    model's; so do the host and the device searches (inside _check)"""
    x, sa, bwt, base, w, ends, pats, m = _case4k(oracle)
    blk = archon.Block()
    try:
        got_sa, got_base = blk.forward(x)
        assert (got_sa == sa).all() and got_base == base
        f = blk.fm_index(RATE, ends=ends)
        try:
            _stats(archon, w, ends.size, [], 0, _ZERO, 0, attached=1)
            _check(archon, f, w, ends, pats, 3, m=m)
        finally:
            f.close()
    finally:
        blk.close()
    f = _handle(archon, bwt, base, sa, ends)
    try:
        _stats(archon, w, ends.size, [], 0, _ZERO, 0, attached=1)
        _check(archon, f, w, ends, pats, 3, m=m)
    finally:
        f.close()
    f = archon.FmIndex(bwt, base).attach_sa(sa).attach_ends_dev(_dev(ends))
    try:
        _stats(archon, w, ends.size, [], 0, _ZERO, 0, attached=1)
        _check(archon, f, w, ends, pats, 3, m=m)
    finally:
        f.close()


def test_read_set(archon):
    """4096 reads of 100 bytes cut at random offsets from a 64 KiB four-letter text, joined with \\n; the queries are the reads,
    min_len = 20, trim = 1.  The GPU's records are the model's; the model's are those of a dictionary of the reads' suffixes
    written here; drop_self leaves no (q, q) pair; best_overlaps has one record per pair"""
    rng = np.random.default_rng(4096)
    text = _letters(64 << 10, 64)
    starts = rng.integers(0, text.size - 100 + 1, 4096)
    reads = [text[s:s + 100].tobytes() for s in starts.tolist()]
    x = np.frombuffer(b"".join(r + b"\n" for r in reads), np.uint8).copy()
    ends = archon.ends_from_bounds(np.arange(0, 101 * 4096 + 1, 101), trim=1)
    blk = archon.Block()
    try:
        sa, _ = blk.forward(x)
        f = blk.fm_index(RATE, ends=ends)
        try:
            w = N.Walker(x, sa)
            rec, novl, ctr = N.model(w, ends, reads, 20)
            gn, gr = f.overlaps(reads, 20)
            assert (gn == novl).all()
            _same(gr, rec)
            _stats(archon, w, ends.size, reads, 20, ctr, rec.size)
        finally:
            f.close()
    finally:
        blk.close()
    # independently: every suffix of 20 .. 100 bytes of every read, then every prefix of every query looked up
    by_suffix = {}
    for d, r in enumerate(reads):
        for l in range(20, 101):
            by_suffix.setdefault(r[100 - l:], []).append(d)
    want = {(q, d, l) for q, r in enumerate(reads) for l in range(20, 101) for d in by_suffix.get(r[:l], ())}
    got = set(zip(rec["query"].tolist(), rec["doc"].tolist(), rec["len"].tolist()))
    assert got == want and len(got) == rec.size
    assert all((q, q, 100) in got for q in range(0, 4096, 97)) and len({(q, d) for q, d, _ in got if q != d}) > 4096, "real overlaps exist"
    kept = archon.drop_self(gr, np.arange(4096))
    assert kept.size == np.count_nonzero(rec["query"] != rec["doc"]) and (kept["query"] != kept["doc"]).all()
    best = archon.best_overlaps(kept)
    pairs = list(zip(best["query"].tolist(), best["doc"].tolist()))
    assert len(set(pairs)) == len(pairs) == len({(q, d) for q, d, _ in got if q != d})
    longest = {}
    for q, d, l in got:
        longest[q, d] = max(longest.get((q, d), 0), l)
    assert all(longest[q, d] == l for (q, d), l in zip(pairs, best["len"].tolist()))


def test_cap_and_refusals(archon, oracle):
    """cap = total - 1 refuses with a sentinel-filled record buffer untouched and novl and *total written; cap = total succeeds;
    k = 0 writes *total = 0 and nothing else; decreasing offsets refuse in both forms, on the device from the kernel's flag;
    min_len = 0 and a handle without ends refuse; *total is 0 after those"""
    x, sa, bwt, base, w, ends, pats, (rec, novl, ctr) = _case4k(oracle)
    L, E = archon.lib(), archon.E_ARG
    p = lambda v: ctypes.c_void_p(v.ctypes.data)       # noqa: E731
    tp = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    packed, off = _pack(pats)
    k = len(pats)
    total = ctypes.c_uint64(7)
    tot = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    try:
        gn = np.full(k, 9, np.uint32)
        out = np.frombuffer(bytes([0xAB]) * (16 * rec.size), np.uint8).copy().view(archon.FM_OVL)
        assert L.archon_hip_fm_overlaps(f.h, p(packed), p(off), k, 3, p(gn), p(out), rec.size, tot) == E
        assert b"no ends" in L.archon_hip_last_error() and total.value == 0 and (gn == 9).all()
        pat_t, off_t, novl_t, rec_t = _dev(packed), _dev(off), _zeros(k), _zeros(4 * rec.size)
        s = archon._stream_ptr()
        assert L.archon_hip_fm_overlaps_dev(f.h, tp(pat_t), tp(off_t), k, 3, tp(novl_t), tp(rec_t), rec.size, tot, s) == E
        f.attach_ends(ends)
        # the cap rule, host form
        total.value = 7
        assert L.archon_hip_fm_overlaps(f.h, p(packed), p(off), k, 3, p(gn), p(out), rec.size - 1, tot) == E
        assert total.value == rec.size and (gn == novl).all() and (out.view(np.uint8) == 0xAB).all()
        _stats(archon, w, ends.size, pats, 3, ctr, 0)
        assert L.archon_hip_fm_overlaps(f.h, p(packed), p(off), k, 3, p(gn), p(out), rec.size, tot) == 0
        assert total.value == rec.size
        _same(out, rec)
        # the device form
        rec_t.fill_(-1)
        total.value = 7
        assert L.archon_hip_fm_overlaps_dev(f.h, tp(pat_t), tp(off_t), k, 3, tp(novl_t), tp(rec_t), rec.size - 1, tot, s) == E
        assert total.value == rec.size and (_host(novl_t, k) == novl).all() and (_host(rec_t, 4 * rec.size) == 0xFFFFFFFF).all()
        assert L.archon_hip_fm_overlaps_dev(f.h, tp(pat_t), tp(off_t), k, 3, tp(novl_t), tp(rec_t), rec.size, tot, s) == 0
        _same(_host(rec_t, 4 * rec.size).view(archon.FM_OVL), rec)
        # k = 0
        gn[:] = 9
        total.value = 7
        assert L.archon_hip_fm_overlaps(f.h, p(packed), p(off), 0, 3, p(gn), p(out), rec.size, tot) == 0
        assert total.value == 0 and (gn == 9).all()
        # decreasing offsets: the bad pair last, so that the good ones in front of it would have answered
        bad = off.copy()
        bad[k] = bad[k - 1] - 1
        out.view(np.uint8)[:] = 0xAB
        total.value = 7
        assert L.archon_hip_fm_overlaps(f.h, p(packed), p(bad), k, 3, p(gn), p(out), rec.size, tot) == E
        assert total.value == 0 and (gn == 9).all() and (out.view(np.uint8) == 0xAB).all()
        rec_t.fill_(-1)
        total.value = 7
        assert L.archon_hip_fm_overlaps_dev(f.h, tp(pat_t), tp(_dev(bad)), k, 3, tp(novl_t), tp(rec_t), rec.size, tot, s) == E
        assert b"offsets decrease" in L.archon_hip_last_error() and total.value == 0 and (_host(rec_t, 4 * rec.size) == 0xFFFFFFFF).all()
        # min_len = 0
        total.value = 7
        assert L.archon_hip_fm_overlaps(f.h, p(packed), p(off), k, 0, p(gn), p(out), rec.size, tot) == E and total.value == 0
        assert L.archon_hip_fm_overlaps_dev(f.h, tp(pat_t), tp(off_t), k, 0, tp(novl_t), tp(rec_t), rec.size, tot, s) == E
        # and the handle answers as before
        _check(archon, f, w, ends, pats, 3, m=(rec, novl, ctr))
    finally:
        f.close()


def test_attach_robustness(archon, oracle):
    """ends that hold 0, an item above n, equal neighbours or decreasing ones are refused in the host, the device and the block
    form, as is an attach without a suffix array, and the earlier ends still answer as before; other ends replace them"""
    x, sa, bwt, base, w, ends, pats, m = _case4k(oracle)
    n = x.size
    L, E = archon.lib(), archon.E_ARG
    p = lambda v: ctypes.c_void_p(v.ctypes.data)       # noqa: E731
    f = archon.FmIndex(bwt, base)
    blk = archon.Block()
    try:
        assert L.archon_hip_fm_attach_ends(f.h, p(ends), ends.size) == E and b"no suffix array" in L.archon_hip_last_error()
        assert L.archon_hip_fm_attach_ends_dev(f.h, ctypes.c_void_p(_dev(ends).data_ptr()), ends.size, None) == E
        f.attach_sa(sa)
        assert (f.count([x[:3].tobytes()])[1] > 0).all()         # the handle without ends behaves as before
        f.attach_ends(ends)
        blk.forward(x)
        g = blk.fm_index(RATE, ends=ends)
        bads = [[0, 5, 9], [5, 9, n + 1], [5, 9, 9, 12], [5, 12, 9], [n, n + 1], [1 << 31, (1 << 32) - 1]]
        for bad in bads:
            bb = np.array(bad, np.uint32)
            assert L.archon_hip_fm_attach_ends(f.h, p(bb), bb.size) == E, bad
            assert b"FM attach ends" in L.archon_hip_last_error()
            bt = _dev(bb)
            assert L.archon_hip_fm_attach_ends_dev(f.h, ctypes.c_void_p(bt.data_ptr()), bb.size, archon._stream_ptr()) == E, bad
            assert b"ends do not increase inside 1 .. 4096" in L.archon_hip_last_error()
            assert L.archon_hip_block_fm_attach_ends(blk.h, g.h, p(bb), bb.size) == E, bad
        too_many = np.arange(1, n + 2, dtype=np.uint32)
        assert L.archon_hip_fm_attach_ends(f.h, p(too_many), too_many.size) == E
        assert L.archon_hip_fm_attach_ends_dev(f.h, ctypes.c_void_p(_dev(too_many).data_ptr()), too_many.size, archon._stream_ptr()) == E
        # a handle that is not of the block
        other = archon.Block()
        try:
            other.forward(x[:4000].copy())
            assert L.archon_hip_block_fm_attach_ends(other.h, f.h, p(ends), ends.size) == E and b"is not of this block" in L.archon_hip_last_error()
        finally:
            other.close()
        _check(archon, f, w, ends, pats, 3, m=m)
        _check(archon, g, w, ends, pats, 3, dev_forms=False, m=m)
        g.close()
        # a second attach replaces the first
        ends2 = np.array([1, 2, 3, 1000, 1001, n - 1], np.uint32)
        f.attach_ends(ends2)
        _stats(archon, w, ends2.size, [], 0, _ZERO, 0, attached=1)
        rec2, _, _ = _check(archon, f, w, ends2, pats, 1)
        assert rec2.tobytes() != m[0].tobytes()
        f.attach_ends_dev(_dev(ends))
        _check(archon, f, w, ends, pats, 3, m=m)
    finally:
        f.close()
        blk.close()


def test_memory_returns(archon):
    """the device memory of the ends is back after close().  The library keeps no account of what it owns that a caller can read,
    so this compares the device's free memory (torch.cuda.mem_get_info), with the slack test_gpu_fm_win.py uses: at 16 MiB with
    4 Mi documents the part is 50.3 MiB, and after the handle is destroyed the free figure is within a quarter of that of what it
    was before the handle was made -- a quarter of what a leak of the part would take, and wide enough for an allocator that
    rounds; after a second attach the handle holds at most one and a half parts more than without one.  The arena has grown to
    what the attach takes before the first figure is read"""
    import torch
    n = 16 << 20
    ends = np.arange(4, n + 1, 4, dtype=np.uint32)
    part = N.end_bytes(n, ends.size)
    slack = part // 4
    blk = archon.Block()
    try:
        blk.forward(S.gen_shape("random", n), want_sa=True)
        blk.fm_index(RATE, ends=ends).close()
        free0 = torch.cuda.mem_get_info()[0]
        f = blk.fm_index(RATE)
        bare = free0 - torch.cuda.mem_get_info()[0]
        attach = lambda: archon._check(archon.lib().archon_hip_block_fm_attach_ends(blk.h, f.h, ctypes.c_void_p(ends.ctypes.data), ends.size))  # noqa: E731
        attach()
        assert archon.fm_ovl_stats().end_bytes == part and archon.fm_ovl_stats().docs == ends.size
        attach()                                        # replaces: the first part is freed
        held = free0 - torch.cuda.mem_get_info()[0] - bare
        f.close()
        back = free0 - torch.cuda.mem_get_info()[0]
        print("    free before %d; the handle %d, its ends %d (end_bytes %d); short after close %d" % (free0, bare, held, part, back))
        assert held <= part + 2 * slack                 # one part, not two
        assert back <= slack
    finally:
        blk.close()


def _snapshot(archon):
    """the counters of the calling thread's last call of every other family: every *_stats getter pyarchon has but the overlaps'
    own, and stats() of the transforms; a family with no record gives its refusal text"""
    names = sorted(k for k in dir(archon) if k.endswith("_stats") and not k.startswith("_") and k != "fm_ovl_stats" and callable(getattr(archon, k)))
    snap = {}
    for name in names + ["stats"]:
        try:
            snap[name] = G.counters(getattr(archon, name)())
        except archon.ArchonError as e:
            snap[name] = str(e)
    return snap


def test_other_parts_are_left_alone(archon, oracle):
    """on a handle with mirror, sa, docs, wm, lcp and ends, a count, a docs call, a win_count, an ms, the SMEMs and a text call give
    what they gave before the ends were attached, and the record of every other family is untouched by the overlap calls of
    every form"""
    x, sa, bwt, base, w, ends, pats, m = _case4k(oracle)
    n = x.size
    bounds = np.array([0, 1000, 3000, n], np.uint32)
    some = [x[100:124].tobytes(), x[2000:2024].tobytes(), x[7:10].tobytes()]
    lo, hi = np.array([0, 5, 100], np.uint32), np.array([n, 300, 101], np.uint32)
    text = np.concatenate([x[300:700], x[50:90]])
    blk = archon.Block()
    try:
        blk.forward(x)
        blk.lcp()
        blk.fm_count(some)
        f = blk.fm_index(RATE, mirror=True, sa=True, docs=bounds, wm=True, lcp=True)
        f.approx(some, 1)
        f.classes(some, archon.classes_identity())
        f.edit(some[:2], 1)
        f.locate(some)
        blk.repeats()
        blk.lz()
        blk.kmers(4)
        blk.maws()
        blk.entropy([0, 1])
        blk.runs()

        def parts():
            plo, phi = f.count(some)
            return [plo, phi] + list(f.smems(some)) + list(f.ms(some)) + list(f.ms_text(text)) + list(f.docs(some)) + [f.win_count(lo, hi)]

        answers = parts()
        before = _snapshot(archon)
        assert all(isinstance(v, dict) for v in before.values()), [k for k, v in before.items() if not isinstance(v, dict)]
        assert len(before) >= 18
        assert archon.lib().archon_hip_block_fm_attach_ends(blk.h, f.h, ctypes.c_void_p(ends.ctypes.data), ends.size) == 0
        f.attach_ends(ends)
        f.attach_ends_dev(_dev(ends))
        _check(archon, f, w, ends, pats, 3, m=m)
        assert _snapshot(archon) == before
        again = parts()
        assert len(again) == len(answers) and all(G._bytes(u) == G._bytes(v) for u, v in zip(again, answers))
        f.close()
    finally:
        blk.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) over the 4 KiB case: the attach is inside the call, so its kernels take
    their later trips too (16 blocks on 1 or 3 workgroups), as do the 600 queries (150 workgroups' worth); the model's records,
    byte-equal to the same calls without the route, with their counters"""
    x, sa, bwt, base, w, ends, pats, (rec, novl, ctr) = _case4k(oracle)
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    try:
        def call():
            f.attach_ends(ends)
            stats = [archon.fm_ovl_stats()]
            gn, gr = f.overlaps(pats, 3)
            stats.append(archon.fm_ovl_stats())
            _same(gr, rec)
            assert (gn == novl).all()
            packed, off = _pack(pats)
            novl_t, rec_t = _zeros(len(pats)), _zeros(4 * rec.size)
            assert f.overlaps_dev(_dev(packed), _dev(off), 3, novl_t, rec_t) == rec.size
            stats.append(archon.fm_ovl_stats())
            dr = _host(rec_t, 4 * rec.size).view(archon.FM_OVL)
            _same(dr, rec)
            return [gn, gr, _host(novl_t, len(pats)), dr], stats

        call()                                          # (the arena grows to what the calls take before their launches are compared)
        G.same_under(monkeypatch, grid, call)
    finally:
        f.close()


def test_second_trip_at_the_product_grid(archon):
    """no route.  stride_util.K2 = 8205 short queries on a 64 KiB block: 2052 workgroups' worth on the product's grid of 2048, so
    the waves of workgroups 0 .. 3 take a second query each, the last of them one of the 13 ragged ones"""
    x = S.gen_shape("dna", 64 << 10)
    n = x.size
    rng = np.random.default_rng(G.K2)
    ends = np.unique(np.concatenate([rng.integers(1, n + 1, 3000), [n]])).astype(np.uint32)
    pats = G.k2_patterns(x)
    assert len(pats) == G.K2 == 8205
    blk = archon.Block()
    try:
        sa, _ = blk.forward(x)
        f = blk.fm_index(RATE, ends=ends)
        try:
            w = N.Walker(x, sa)
            rec, novl, ctr = _check(archon, f, w, ends, pats, 2)
            assert rec.size > 8205 and novl[8192:].any() and novl[:16].any()
        finally:
            f.close()
    finally:
        blk.close()


def test_calls(archon, oracle):
    """kernel launches and host waits of every form, as the header states them, equal on two runs (the first run grows the
    arena where it has to).  Step by step (fm_host.hiph):
      fmo_attach_run   the ends kernel, the bits kernel, the scan of the block popcounts (3) and the compaction: 6 launches; one
                       wait at the end
      fmo_run          the count pass (1) and, when records are asked for, the scan of novl (3); one wait for the counters, with
                       which a host form's counts travel; with records that exist and fit the emit pass (1) and one wait"""
    x, sa, bwt, base, w, ends, pats, (rec, novl, ctr) = _case4k(oracle)
    lw = lambda: (archon.fm_ovl_stats().kernel_launches, archon.fm_ovl_stats().host_syncs)       # noqa: E731
    packed, off = _pack(pats)
    absent = [b"\xff\xfe", b"\xfd"]
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    blk = archon.Block()
    try:
        blk.forward(x)
        pat_t, off_t, novl_t, rec_t, ends_t = _dev(packed), _dev(off), _zeros(len(pats)), _zeros(4 * rec.size), _dev(ends)
        seen = []
        for run in range(3):
            got = []
            f.attach_ends(ends)
            got.append(lw())
            f.attach_ends_dev(ends_t)
            got.append(lw())
            blk.fm_index(RATE, ends=ends).close()
            got.append(lw())
            f.overlaps(pats, 3, emit=False)
            got.append(lw())
            f.overlaps_dev(pat_t, off_t, 3, novl_t)
            got.append(lw())
            out = np.zeros(rec.size, archon.FM_OVL)
            total = ctypes.c_uint64(0)
            gn = np.zeros(len(pats), np.uint32)
            p = lambda v: ctypes.c_void_p(v.ctypes.data)       # noqa: E731
            tot = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
            assert archon.lib().archon_hip_fm_overlaps(f.h, p(packed), p(off), len(pats), 3, p(gn), p(out), out.size, tot) == 0
            got.append(lw())
            f.overlaps_dev(pat_t, off_t, 3, novl_t, rec_t)
            got.append(lw())
            assert archon.lib().archon_hip_fm_overlaps(f.h, p(packed), p(off), len(pats), 3, p(gn), p(out), out.size - 1, tot) == archon.E_ARG
            got.append(lw())
            assert f.overlaps(absent, 1)[1].size == 0
            got.append(lw())
            if run:
                seen.append(got)
        want = [(6, 1), (6, 1), (6, 1), (1, 1), (1, 1), (5, 2), (5, 2), (4, 1), (4, 1)]
        assert seen[0] == want and seen[1] == want
    finally:
        f.close()
        blk.close()
