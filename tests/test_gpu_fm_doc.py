"""GPU: the document listing (archon_hip_fm_attach_docs*, _block_fm_attach_docs, _fm_docs*, _fm_docs_ranges*, _fm_doc_of*;
include/archon_hip.h).  Expected records and counters: the numpy model over the oracle's suffix array (tests/fm_doc_naive.py, pinned
to the definition from the text alone by test_fm_doc_abi.py), and for a few patterns the definition itself.  Every tiny block with
every boundary set and every range; 64 KiB blocks at every document count that changes the sort and at tiles of 64, 128 and the
default; a 128 KiB block of 70 000 documents; the block form; doc_of over locate; the cap rule; the other statistics records."""
import ctypes
import itertools

import numpy as np
import pytest

import archon_synth as S
import fm_doc_naive as N
import stride_util as G

pytestmark = pytest.mark.gpu

KiB = 1 << 10
TILES = (0, 64, 128)
SHAPES = ("text", "dna", "a", "random")

_REFERENCE = {}


def _reference(oracle, shape, n=64 * KiB):
    """(x, sa, bwt, base) of a shape: computed once, shared, left unchanged"""
    key = (shape, n)
    if key not in _REFERENCE:
        x = S.gen_shape(shape, n)
        sa, bwt, base = oracle.forward(x)
        for a in (x, sa, bwt):
            a.setflags(write=False)
        _REFERENCE[key] = (x, sa, bwt, base)
    return _REFERENCE[key]


def _bounds(n, D, rng):
    """random bounds of D documents (every byte its own document at D = n)"""
    if D == n:
        return np.arange(n + 1, dtype=np.uint32)
    cuts = np.sort(rng.choice(np.arange(1, n), D - 1, replace=False)) if D > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [n]]).astype(np.uint32)


def _patterns(x, rng):
    """substrings of 1, 2 and 8 bytes, and absent ones"""
    n = x.size
    out = []
    for m in (1, 2, 8):
        for _ in range(6):
            q = int(rng.integers(0, n - m))
            out.append(x[q:q + m].tobytes())
    absent = np.flatnonzero(np.bincount(x, minlength=256) == 0)
    if absent.size:
        z = bytes([int(absent[0])])
        out += [z, x[:3].tobytes() + z, z + x[5:9].tobytes()]
    else:
        out += [bytes(rng.integers(0, 256, 24, dtype=np.uint8))]        # 24 random bytes do not occur in 64 KiB of random bytes
    return out


def _raw_ranges(n, rng):
    """the whole block, empty ranges at both ends, and ranges of lengths around one and two waves, none starting on a multiple of 64"""
    out = [(0, n), (0, 0), (n, n)]
    for ln in (1, 63, 64, 65, 127, 128, 129):
        lo = 64 * int(rng.integers(1, (n - 256) // 64)) + int(rng.integers(1, 64))
        out.append((lo, lo + ln))
    return out


def _same(got, want):
    assert got.size == want.size, (got.size, want.size)
    for k in ("range", "row", "doc", "tf"):
        assert (got[k] == want[k]).all(), k


def _check_stats(st, n, D, k, T, ctr, want):
    assert (st["n"], st["docs"], st["ranges"], st["tile"]) == (n, D, k, T)
    assert (st["rows"], st["tiles"], st["listed"]) == (ctr["rows"], ctr["tiles"], ctr["listed"])
    assert st["longest_tf"] == (int(want["tf"].max()) if want.size else 0)
    assert st["probes"] <= ctr["listed"] * (int(np.ceil(np.log2(D + 1))) + int(np.ceil(np.log2(n + 1))))
    assert 12 * n + 4 * (D + 1) <= st["doc_bytes"] <= 12 * n + 4 * (D + 1) + 4 * 256


def test_every_tiny_block_boundary_set_and_range(archon, oracle):
    """every block of <= 6 bytes over two symbols, every boundary set, all ranges 0 <= lo <= hi <= n in one call each"""
    combos = 0
    for n in range(1, 7):
        ranges = [(lo, hi) for lo in range(n + 1) for hi in range(lo, n + 1)]
        lo = np.array([r[0] for r in ranges], np.uint32)
        hi = np.array([r[1] for r in ranges], np.uint32)
        for tt in itertools.product((0, 1), repeat=n):
            x = np.array(tt, np.uint8)
            sa, bwt, base = oracle.forward(x)
            f = archon.FmIndex(bwt, base).attach_sa(sa)
            try:
                for bounds in N.boundary_sets(n):
                    f.attach_docs(bounds)
                    ndocs, got = f.docs_ranges(lo, hi)
                    want, wnd, ctr = N.listing(sa, bounds, ranges, N.DEFAULT_TILE)
                    _same(got, want)
                    assert (ndocs == wnd).all(), (tt, bounds)
                    combos += 1
            finally:
                f.close()
    assert combos == sum((1 << n) * (1 << (n - 1)) for n in range(1, 7))


@pytest.mark.parametrize("shape", SHAPES)
def test_64k_blocks(archon, oracle, shape, monkeypatch):
    """64 KiB of four shapes; D of 1, 2, 255, 256, 257 and n (no sort byte, one, one full, two, every row alone), each attach
    replacing the one before; the ranges of patterns and raw ranges; tiles of 64, 128 and the default with the counters at each"""
    x, sa, bwt, base = _reference(oracle, shape)
    n = x.size
    rng = np.random.default_rng(n + len(shape))
    patterns = _patterns(x, rng)
    raw = _raw_ranges(n, rng)
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    try:
        plo, phi = f.count(patterns)
        pranges = [(int(a), int(b)) if a < b else (0, 0) for a, b in zip(plo, phi)]
        assert sum(b > a for a, b in pranges) >= 18 and any(a == b for a, b in pranges)
        for D in (1, 2, 255, 256, 257, n):
            bounds = _bounds(n, D, rng)
            monkeypatch.delenv("ARCHON_DOC_TILE", raising=False)
            f.attach_docs(bounds)
            st = archon.fm_doc_stats().asdict()
            print("    %s D = %d attach: %s" % (shape, D, st))
            assert st["attached"] == 1 and st["sort_passes"] <= (int(D - 1).bit_length() + 7) // 8
            assert st["sort_passes"] == {1: 0, 2: 1, 255: 1, 256: 1, 257: 2, n: 2}[D]
            for tile in TILES:
                monkeypatch.setenv("ARCHON_DOC_TILE", str(tile))
                T = tile or N.DEFAULT_TILE
                want, wnd, ctr = N.listing(sa, bounds, pranges, T)
                ndocs, got = f.docs(patterns)
                st = archon.fm_doc_stats().asdict()
                _same(got, want)
                assert (ndocs == wnd).all()
                _check_stats(st, n, D, len(patterns), T, ctr, want)
                assert st["pattern_bytes"] == sum(len(p) for p in patterns)
                want, wnd, ctr = N.listing(sa, bounds, raw, T)
                ndocs, got = f.docs_ranges([r[0] for r in raw], [r[1] for r in raw])
                st = archon.fm_doc_stats().asdict()
                if tile == 0:
                    print("    %s D = %d ranges: %s" % (shape, D, st))
                _same(got, want)
                assert (ndocs == wnd).all() and int(ndocs[0]) == D and ndocs[1] == 0 and ndocs[2] == 0
                assert int(got["tf"][got["range"] == 0].sum()) == n
                _check_stats(st, n, D, len(raw), T, ctr, want)
            if D == 257:
                # the definition itself, from the text alone
                ndocs, got = f.docs(patterns[:3] + patterns[6:8] + patterns[12:13])
                for j, P in enumerate(patterns[:3] + patterns[6:8] + patterns[12:13]):
                    mine = got[got["range"] == j]
                    assert {int(r["doc"]): int(r["tf"]) for r in mine} == N.definition(x, list(bounds), P), P
    finally:
        f.close()


def test_128k_block_of_70000_documents(archon, oracle):
    """D - 1 = 69 999 has three bytes and the middle one varies: three radix passes, none skipped"""
    x, sa, bwt, base = _reference(oracle, "text", 128 * KiB)
    n, D = x.size, 70000
    rng = np.random.default_rng(70000)
    bounds = _bounds(n, D, rng)
    patterns = _patterns(x, rng)
    f = archon.FmIndex(bwt, base).attach_sa(sa).attach_docs(bounds)
    try:
        st = archon.fm_doc_stats().asdict()
        print("    attach: %s" % st)
        assert (st["docs"], st["sort_passes"], st["attached"]) == (D, 3, 1)
        plo, phi = f.count(patterns)
        ranges = [(0, n)] + [(int(a), int(b)) if a < b else (0, 0) for a, b in zip(plo, phi)]
        want, wnd, ctr = N.listing(sa, bounds, ranges)
        ndocs, got = f.docs_ranges([r[0] for r in ranges], [r[1] for r in ranges])
        _same(got, want)
        assert (ndocs == wnd).all() and int(ndocs[0]) == D
        _check_stats(archon.fm_doc_stats().asdict(), n, D, len(ranges), N.DEFAULT_TILE, ctr, want)
    finally:
        f.close()


def test_block_form_replace_and_attach_sa_after(archon, oracle):
    """the block form reads the resident suffix array and equals the handle form; an attach replaces the earlier one; a refused
    attach leaves it in place; attach_sa after attach_docs leaves the listing unchanged"""
    x, sa, bwt, base = _reference(oracle, "dna")
    n = x.size
    rng = np.random.default_rng(5)
    b1, b2 = _bounds(n, 300, rng), _bounds(n, 7, rng)
    raw = _raw_ranges(n, rng)
    lo, hi = [r[0] for r in raw], [r[1] for r in raw]
    want1, wnd1, _ = N.listing(sa, b1, raw)
    want2, wnd2, _ = N.listing(sa, b2, raw)
    blk = archon.Block()
    f = g = None
    try:
        gsa, gbase = blk.forward(x, want_sa=True)
        assert gbase == base and (gsa == sa).all()
        g = blk.fm_index(32, docs=b1)            # no attach_sa: the resident array
        nd, got = g.docs_ranges(lo, hi)
        _same(got, want1)
        assert (nd == wnd1).all()
        f = archon.FmIndex(bwt, base)
        with pytest.raises(archon.ArchonError):
            f.attach_docs(b1)                    # the handle form needs an attached suffix array
        f.attach_sa(sa).attach_docs(b1)
        nd, got = f.docs_ranges(lo, hi)
        _same(got, want1)
        f.attach_docs(b2)
        nd, got = f.docs_ranges(lo, hi)
        _same(got, want2)
        assert (nd == wnd2).all()
        for bad in (np.append(b2[:-1], n - 1), np.append(b2[:-1], n + 1), b2[1:], np.concatenate([b2[:3], b2[2:]]),
                    np.arange(n + 2, dtype=np.uint32)):
            with pytest.raises(archon.ArchonError) as e:
                f.attach_docs(bad.astype(np.uint32))
            assert e.value.code == archon.E_ARG
            with pytest.raises(archon.ArchonError):
                lib_rc = archon.lib().archon_hip_block_fm_attach_docs(blk.h, g.h, ctypes.c_void_p(bad.astype(np.uint32).ctypes.data), bad.size - 1)
                archon._check(lib_rc)
        nd, got = f.docs_ranges(lo, hi)
        _same(got, want2)
        f.attach_sa(sa)
        nd, got = f.docs_ranges(lo, hi)
        _same(got, want2)
        nd, got = g.docs_ranges(lo, hi)
        _same(got, want1)
    finally:
        for h in (f, g, blk):
            if h is not None:
                h.close()


def test_device_forms(archon, oracle):
    """bounds, patterns, ranges, counts and records on the device equal the host forms; bad device bounds are found on the device
    and leave the earlier attachment; a bad device range is ARCHON_E_ARG and emits nothing"""
    import torch
    x, sa, bwt, base = _reference(oracle, "text")
    n = x.size
    rng = np.random.default_rng(11)
    bounds = _bounds(n, 500, rng)
    patterns = _patterns(x, rng)
    raw = _raw_ranges(n, rng)
    dev = "cuda:0"

    def t32(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)

    f = archon.FmIndex(bwt, base).attach_sa(sa)
    try:
        f.attach_docs_dev(t32(bounds))
        for bad in (np.append(bounds[:-1], n - 1), np.concatenate([[1], bounds[1:]]), np.concatenate([bounds[:9], bounds[8:]])):
            with pytest.raises(archon.ArchonError) as e:
                f.attach_docs_dev(t32(bad))
            assert e.value.code == archon.E_ARG
        want, wnd, _ = N.listing(sa, bounds, raw)
        lo_t, hi_t = t32([r[0] for r in raw]), t32([r[1] for r in raw])
        nd_t = torch.full((len(raw),), -1, dtype=torch.int32, device=dev)
        assert f.docs_ranges_dev(lo_t, hi_t, nd_t) == want.size
        out_t = torch.full((4 * want.size + 8,), -1, dtype=torch.int32, device=dev)
        assert f.docs_ranges_dev(lo_t, hi_t, nd_t, out_t) == want.size
        torch.cuda.synchronize()
        got = out_t.cpu().numpy().view(np.uint32)
        _same(got[:4 * want.size].view(N.FM_DOC), want)
        assert (got[4 * want.size:] == 0xFFFFFFFF).all()
        assert (nd_t.cpu().numpy().view(np.uint32) == wnd).all()
        # a bad range among good ones: found on the device, nothing emitted
        for bad in ((9, 8), (0, n + 1)):
            blo, bhi = [r[0] for r in raw] + [bad[0]], [r[1] for r in raw] + [bad[1]]
            out_t.fill_(-1)
            total = ctypes.c_uint64(7)
            blo_t, bhi_t, bnd_t = t32(blo), t32(bhi), torch.zeros(len(blo), dtype=torch.int32, device=dev)
            rc = archon.lib().archon_hip_fm_docs_ranges_dev(f.h, ctypes.c_void_p(blo_t.data_ptr()), ctypes.c_void_p(bhi_t.data_ptr()), len(blo),
                                                           ctypes.c_void_p(bnd_t.data_ptr()), ctypes.c_void_p(out_t.data_ptr()), out_t.numel() // 4,
                                                           ctypes.cast(ctypes.byref(total), ctypes.c_void_p), None)
            torch.cuda.synchronize()
            assert rc == archon.E_ARG and total.value == 0
            assert (out_t == -1).all()
            with pytest.raises(archon.ArchonError):
                f.docs_ranges(blo, bhi)
        # patterns on the device
        hnd, hgot = f.docs(patterns)
        packed, offsets = archon._pack_patterns(patterns)
        p_t, o_t = torch.from_numpy(packed.copy()).to(dev), t32(offsets)
        nd_t = torch.full((len(patterns),), -1, dtype=torch.int32, device=dev)
        assert f.docs_dev(p_t, o_t, nd_t) == hgot.size
        out_t = torch.full((4 * hgot.size,), -1, dtype=torch.int32, device=dev)
        assert f.docs_dev(p_t, o_t, nd_t, out_t) == hgot.size
        torch.cuda.synchronize()
        _same(out_t.cpu().numpy().view(N.FM_DOC), hgot)
        assert (nd_t.cpu().numpy().view(np.uint32) == hnd).all()
        assert archon.fm_doc_stats().pattern_bytes == sum(len(p) for p in patterns)
    finally:
        f.close()


def test_doc_of_on_locate_output(archon, oracle):
    """per pattern, the documents of start + m over every located start are the records' (doc, tf); the offsets are the items' own"""
    import torch
    x, sa, bwt, base = _reference(oracle, "text")
    n = x.size
    rng = np.random.default_rng(23)
    bounds = _bounds(n, 257, rng)
    patterns = [p for p in _patterns(x, rng) if len(p) <= 2][:10]
    f = archon.FmIndex(bwt, base).sample(32).attach_sa(sa).attach_docs(bounds)
    try:
        ndocs, rec = f.docs(patterns)
        starts = f.locate(patterns)
        seen = 0
        for j, P in enumerate(patterns):
            items = starts[j].astype(np.uint32) + len(P)
            doc, off = f.doc_of(items)
            assert (doc == N.doc_of_items(bounds, items)).all()
            assert (off == items - 1 - bounds[doc]).all()
            mine = rec[rec["range"] == j]
            u, c = np.unique(doc, return_counts=True)
            assert dict(zip(u.tolist(), c.tolist())) == {int(r["doc"]): int(r["tf"]) for r in mine}, P
            assert (x[starts[j][:4].astype(np.int64)] == P[0]).all()
            seen += items.size
        assert seen > 1000
        every = np.arange(1, n + 1, dtype=np.uint32)
        doc, off = f.doc_of(every)
        assert (doc == N.doc_of_items(bounds, every)).all() and (off == every - 1 - bounds[doc]).all()
        doc, off = f.doc_of(every[:100], offsets=False)
        assert off is None and (doc == N.doc_of_items(bounds, every[:100])).all()
        # an item outside 1 .. n: ARCHON_E_ARG, nothing written -- on the host and on the device
        L = archon.lib()
        for bad in (0, n + 1):
            items = np.array([5, bad, 9], np.uint32)
            d, o = np.full(3, 77, np.uint32), np.full(3, 77, np.uint32)
            assert L.archon_hip_fm_doc_of(f.h, ctypes.c_void_p(items.ctypes.data), 3, ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(o.ctypes.data)) == archon.E_ARG
            assert (d == 77).all() and (o == 77).all()
            it = torch.from_numpy(items.view(np.int32).copy()).to("cuda:0")
            dt = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
            ot = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
            rc = L.archon_hip_fm_doc_of_dev(f.h, ctypes.c_void_p(it.data_ptr()), 3, ctypes.c_void_p(dt.data_ptr()), ctypes.c_void_p(ot.data_ptr()), None)
            torch.cuda.synchronize()
            assert rc == archon.E_ARG and (dt == 77).all() and (ot == 77).all()
        it = torch.from_numpy(every.view(np.int32).copy()).to("cuda:0")
        dt = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        assert L.archon_hip_fm_doc_of_dev(f.h, ctypes.c_void_p(it.data_ptr()), n, ctypes.c_void_p(dt.data_ptr()), None, None) == 0
        torch.cuda.synchronize()
        assert (dt.cpu().numpy().view(np.uint32) == N.doc_of_items(bounds, every)).all()
    finally:
        f.close()


def test_cap_rule(archon, oracle):
    """counting only; cap = total - 1; k = 0; a handle without documents"""
    x, sa, bwt, base = _reference(oracle, "dna")
    n = x.size
    rng = np.random.default_rng(31)
    bounds = _bounds(n, 64, rng)
    raw = _raw_ranges(n, rng)
    lo, hi = np.array([r[0] for r in raw], np.uint32), np.array([r[1] for r in raw], np.uint32)
    want, wnd, ctr = N.listing(sa, bounds, raw)
    L = archon.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    try:
        with pytest.raises(archon.ArchonError) as e:
            f.docs_ranges(lo, hi)
        assert e.value.code == archon.E_ARG and "documents" in str(e.value)
        with pytest.raises(archon.ArchonError):
            f.docs([b"A"])
        with pytest.raises(archon.ArchonError):
            f.doc_of([1])
        f.attach_docs(bounds)
        nd, got = f.docs_ranges(lo, hi, emit=False)
        st = archon.fm_doc_stats().asdict()
        assert got is None and (nd == wnd).all()
        assert (st["listed"], st["probes"], st["longest_tf"], st["ms_emit"]) == (want.size, 0, 0, 0.0)
        nd, got = f.docs([b"A", b"CG"], emit=False)
        nd2, got2 = f.docs([b"A", b"CG"])
        assert got is None and (nd == nd2).all() and got2.size == int(nd2.sum())
        assert list(nd) == [len(N.definition(x, list(bounds), b"A")), len(N.definition(x, list(bounds), b"CG"))]
        total = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        nd = np.zeros(len(raw), np.uint32)
        out = np.zeros(want.size, N.FM_DOC)
        assert L.archon_hip_fm_docs_ranges(f.h, p(lo), p(hi), len(raw), p(nd), p(out), want.size - 1, tp) == archon.E_ARG
        assert total.value == want.size and (nd == wnd).all() and not out.view(np.uint32).any()
        assert L.archon_hip_fm_docs_ranges(f.h, p(lo), p(hi), len(raw), p(nd), p(out), want.size, tp) == 0
        _same(out, want)
        total.value = 9
        nd[:] = 5
        assert L.archon_hip_fm_docs_ranges(f.h, p(lo), p(hi), 0, p(nd), p(out), want.size, tp) == 0
        assert total.value == 0 and (nd == 5).all()
        nd, got = f.docs_ranges([], [])
        assert nd.size == 0 and got.size == 0
        nd, got = f.docs_ranges([0, n, 17], [0, n, 17])       # only empty ranges
        assert (nd == 0).all() and got.size == 0
    finally:
        f.close()


def test_other_statistics_records_are_left_alone(archon, oracle):
    """fm_stats, fm_text_stats and fm_ms_stats after documents calls are what they were before"""
    x, sa, bwt, base = _reference(oracle, "text")
    n = x.size
    bounds = _bounds(n, 100, np.random.default_rng(3))
    f = archon.FmIndex(bwt, base)
    try:
        f.attach_lcp(archon.lcp(x, sa)).attach_sa(sa)
        f.count([b"the", b"e"])
        f.ms([b"the end"])
        before = (archon.fm_stats().asdict(), archon.fm_text_stats().asdict(), archon.fm_ms_stats().asdict())
        f.attach_docs(bounds)
        f.docs([b"the", b"e", b"zzzzqq"])
        f.docs_ranges([0, 5], [n, 700])
        f.doc_of([1, n])
        assert (archon.fm_stats().asdict(), archon.fm_text_stats().asdict(), archon.fm_ms_stats().asdict()) == before
        assert archon.fm_doc_stats().n == n
    finally:
        f.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) with tiles of 64 rows, text and dna at 64 KiB in 257 documents: ranges
    of 65, 4096 and 12 345 rows, the raw ranges and the ranges of the patterns in ONE call, so that a wave takes many tiles of
    one range and then tiles of the next -- attach_docs under the route, docs_ranges and docs with and without the records
    against the numpy model with its counters; byte-equal to the same calls without the route, with their counters"""
    monkeypatch.setenv("ARCHON_DOC_TILE", "64")
    T, D = 64, 257
    for shape in ("text", "dna"):
        x, sa, bwt, base = _reference(oracle, shape)
        n = x.size
        rng = np.random.default_rng(n + 3 * len(shape))
        bounds = _bounds(n, D, rng)
        patterns = _patterns(x, rng)
        f = archon.FmIndex(bwt, base).attach_sa(sa)
        try:
            plo, phi = f.count(patterns)
            pranges = [(int(a), int(b)) if a < b else (0, 0) for a, b in zip(plo, phi)]
            ranges = [(1001, 1001 + 65), (5003, 5003 + 4096), (20011, 20011 + 12345)] + _raw_ranges(n, rng)[1:] + pranges
            lo, hi = [r[0] for r in ranges], [r[1] for r in ranges]
            want, wnd, ctr = N.listing(sa, bounds, ranges, T)
            pwant, pwnd, pctr = N.listing(sa, bounds, pranges, T)
            assert ctr["tiles"] > 2 + 64 + 192 and want.size > 3 * D // 2

            def call():
                f.attach_docs(bounds)
                stats = [archon.fm_doc_stats()]
                ndocs, got = f.docs_ranges(lo, hi)
                st = archon.fm_doc_stats()
                _same(got, want)
                assert (ndocs == wnd).all()
                _check_stats(st.asdict(), n, D, len(ranges), T, ctr, want)
                only, none = f.docs_ranges(lo, hi, emit=False)
                assert none is None and (only == wnd).all()
                stats += [st, archon.fm_doc_stats()]
                pdocs, pgot = f.docs(patterns)
                st = archon.fm_doc_stats()
                _same(pgot, pwant)
                assert (pdocs == pwnd).all()
                _check_stats(st.asdict(), n, D, len(patterns), T, pctr, pwant)
                ponly, none = f.docs(patterns, emit=False)
                assert none is None and (ponly == pwnd).all()
                stats += [st, archon.fm_doc_stats()]
                return [ndocs, got, only, pdocs, pgot, ponly], stats
            G.same_under(monkeypatch, grid, call)
        finally:
            f.close()
