"""GPU: the edit-distance search (archon_hip_fm_edit, _fm_edit_dev, _block_fm_edit; include/archon_hip.h) against the rule
of the header in Python (tests/fm_edit_naive.py, pinned to the definition by test_fm_edit_abi.py): the matches exactly and in
order, the work counters of the filter, every tile width and batch size, the block against a sampled handle, the device
form, the refusals and repeatability."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import fm_edit_naive as E
import fm_naive
import fm_sampled_naive as M
import stride_util as G

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "256"}
ROUTES = ("ARCHON_EDIT_TILE", "ARCHON_EDIT_BATCH")


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


def _want(archon, cells, K):
    """(nhits, hits) of the patterns whose rule_cells are given, as the calls return them"""
    parts, nh = [], []
    for j, (d, s) in enumerate(cells):
        e = np.flatnonzero(d <= K)
        rec = np.zeros(e.size, archon.FM_EDIT)
        rec["start"], rec["end"], rec["distance"], rec["pattern"] = s[e], e, d[e], j
        parts.append(rec)
        nh.append(e.size)
    return np.array(nh, np.uint32), np.concatenate(parts) if parts else np.zeros(0, archon.FM_EDIT)


def _same(got, want):
    assert (got[0] == want[0]).all(), (got[0], want[0])
    assert got[1].size == want[1].size
    bad = np.flatnonzero(got[1] != want[1])
    assert not bad.size, (bad[:4], got[1][bad[:4]], want[1][bad[:4]])


def _counters(x, pats, K, W):
    tot = {"seed_rows": 0, "tiles": 0, "rows": 0}
    for p in pats:
        c = E.tile_model(x, p, K, W, with_hits=False)[1]
        for k in tot:
            tot[k] += c[k]
    return tot


def _check_stats(archon, want, counters, K, W, npat):
    st = archon.fm_edit_stats()
    assert (st.seed_rows, st.tiles, st.rows) == (counters["seed_rows"], counters["tiles"], counters["rows"]), (K, W)
    assert st.hits == want[1].size and st.max_errors == K and st.tile == W and st.patterns == npat
    return st


def _edited(x, rng, q, m, K):
    """m bytes: a cut of x at q with up to K substitutions, insertions and deletions"""
    ops = [int(rng.integers(0, 3)) for _ in range(int(rng.integers(0, K + 1)))]
    L = m - ops.count(1) + ops.count(2)
    if L < 1 or q + L > x.size:
        ops, L = [], m
    p = bytearray(x[q:q + L].tobytes())
    for op in ops:
        i = int(rng.integers(0, len(p)))
        if op == 0:
            p[i] = int(rng.integers(0, 256))
        elif op == 1:
            p.insert(i, int(rng.integers(0, 256)))
        else:
            del p[i]
    assert len(p) == m
    return bytes(p)


def _patterns(x, rng, K, lengths):
    """cuts of x with up to K edits of all three kinds; a cut at offset 0 that lost its first bytes (the pattern has K more in
    front: a negative diagonal, start 0); a cut that ends at n; two random strings"""
    n = x.size
    pats = [_edited(x, rng, int(rng.integers(0, n - m - K)), m, K) for m in lengths]
    if len(lengths) > 3:
        pats.append(rng.integers(0, 256, K, dtype=np.uint8).tobytes() + x[:24].tobytes())
        pats.append(_edited(x, rng, n - 24, 24, 0)[:11] + b"\x01" + x[n - 12:].tobytes())
        pats.append(rng.integers(0, 256, 12, dtype=np.uint8).tobytes())
        pats.append(rng.integers(65, 69, 12, dtype=np.uint8).tobytes())
    return pats


def test_tiny_exhaustive(archon):
    """every block of length <= 5 over {0, 1, 255}, every pattern of length <= 3 over {0, 1, 2, 255}, every K < m, through a
    block and through a host-built handle sampled at 2: hits, nhits, seed_rows, tiles and hits of the statistics"""
    patterns = [bytes(p) for m in range(1, 4) for p in itertools.product((0, 1, 2, 255), repeat=m)]
    b = archon.Block()
    try:
        for n in range(1, 6):
            for tt in itertools.product((0, 1, 255), repeat=n):
                x = np.array(tt, np.uint8)
                _, bwt, base = M.a7_forward(bytes(tt))
                _, b0 = b.forward(x)
                assert b0 == base
                f = archon.FmIndex(np.frombuffer(bwt, np.uint8).copy(), base).sample(2)
                cells = {p: E.rule_cells(x, p) for p in patterns}
                for K in range(3):
                    pats = [p for p in patterns if len(p) > K]
                    want = _want(archon, [cells[p] for p in pats], K)
                    counters = _counters(x, pats, K, 32)
                    for call in (b.fm_edit, f.edit):
                        _same(call(pats, K), want)
                        _check_stats(archon, want, counters, K, 32, len(pats))
                f.close()
    finally:
        b.close()


@pytest.mark.parametrize("n", [4 * KiB, 64 * KiB])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_blocks_every_route(archon, monkeypatch, shape, n):
    """blocks of every shape at K = 1 and 3 on the default route, tiles of 1, 5 and 64 - 2K ends, batches of 1 and 3
    patterns and the small rank table: matches from rule_np, counters from tile_model; the block and a sampled handle of its
    BWT give identical arrays, and the handle walks LF"""
    x = _shape(shape, n)
    rng = np.random.default_rng(n + len(shape))
    wants = {}
    b = archon.Block()
    try:
        b.forward(x)
        f = b.fm_index(32)
        for K in (1, 3):
            pats = _patterns(x, rng, K, (K + 1, 33, 130) if shape in ("a", "ab") else (K + 1, 7, 33, 64, 65, 130))
            want = _want(archon, [E.rule_cells(x, p) for p in pats], K)
            wants[K] = (pats, want)
            counters = {}
            for route in ({}, {"ARCHON_EDIT_TILE": 1}, {"ARCHON_EDIT_TILE": 5}, {"ARCHON_EDIT_TILE": 64 - 2 * K}, {"ARCHON_EDIT_BATCH": 1},
                          {"ARCHON_EDIT_BATCH": 3}):
                for name in ROUTES:
                    monkeypatch.delenv(name, raising=False)
                for name, v in route.items():
                    monkeypatch.setenv(name, str(v))
                W = route.get("ARCHON_EDIT_TILE", 32)
                if W not in counters:
                    counters[W] = _counters(x, pats, K, W)
                got = b.fm_edit(pats, K)
                _same(got, want)
                st = _check_stats(archon, want, counters[W], K, W, len(pats))
                per = route.get("ARCHON_EDIT_BATCH")
                assert st.batches == (-(-len(pats) // per) if per else 1) and st.lf_steps == 0
                got_f = f.edit(pats, K)
                assert (got_f[0] == got[0]).all() and (got_f[1] == got[1]).all()
                assert _check_stats(archon, want, counters[W], K, W, len(pats)).lf_steps > 0
            for name in ROUTES:
                monkeypatch.delenv(name, raising=False)
        f.close()
    finally:
        b.close()
    for k, v in SMALL_ROUTE.items():
        monkeypatch.setenv(k, v)
    b = archon.Block()
    try:
        b.forward(x)
        f = b.fm_index(32)
        for K, (pats, want) in wants.items():
            _same(b.fm_edit(pats, K), want)
            _same(f.edit(pats, K), want)
        f.close()
    finally:
        b.close()


def test_long_patterns(archon):
    """m = 64, 65, 128, 129, 300 and 4096 at K = 2 on a 64 KiB text block: the pattern window's and the text shift's 64-byte refills"""
    x = S.gen_text(64 * KiB)
    rng = np.random.default_rng(41)
    K = 2
    pats = [_edited(x, rng, int(rng.integers(0, x.size - m - K)), m, K) for m in (64, 65, 128, 129, 300, 4096)]
    want = _want(archon, [E.rule_cells(x, p) for p in pats], K)
    assert (want[0] > 0).all()
    b = archon.Block()
    try:
        b.forward(x)
        _same(b.fm_edit(pats, K), want)
        f = b.fm_index(16)
        _same(f.edit(pats, K), want)
        f.close()
    finally:
        b.close()


def test_k0_is_locate(archon):
    """K = 0: the ends are the sorted locate starts plus m, start = end - m, distance 0, and seed_rows is the count's range"""
    x = S.gen_text(64 * KiB)
    rng = np.random.default_rng(3)
    pats = [x[q:q + m].tobytes() for m in (1, 4, 9, 40) for q in rng.integers(0, x.size - 40, 3)] + [b"\x00\x01\x02"]
    b = archon.Block()
    try:
        b.forward(x)
        starts = b.fm_locate(pats)
        nhits, h = b.fm_edit(pats, 0)
        assert archon.fm_edit_stats().seed_rows == sum(s.size for s in starts) == h.size
        at = 0
        for j, (p, s) in enumerate(zip(pats, starts)):
            part = h[at:at + int(nhits[j])]
            at += int(nhits[j])
            assert (part["end"] == np.sort(s) + len(p)).all() and (part["start"] == part["end"] - len(p)).all()
            assert (part["distance"] == 0).all() and (part["pattern"] == j).all()
        assert at == h.size
    finally:
        b.close()


def test_flood(archon):
    """K = 8, m = 9 on a 4 KiB DNA block: the pieces are single bytes, nearly every tile is marked, the result is the rule's"""
    x = S.gen_dna(4 * KiB)
    rng = np.random.default_rng(8)
    pats = [_edited(x, rng, int(q), 9, 8) for q in rng.integers(0, x.size - 20, 4)]
    want = _want(archon, [E.rule_cells(x, p) for p in pats], 8)
    b = archon.Block()
    try:
        b.forward(x)
        _same(b.fm_edit(pats, 8), want)
        st = _check_stats(archon, want, _counters(x, pats, 8, 32), 8, 32, len(pats))
        assert st.tiles >= 4 * (x.size // 32 - 1)
        f = b.fm_index(8)
        _same(f.edit(pats, 8), want)
        f.close()
    finally:
        b.close()


def test_against_approx(archon):
    """every occurrence of every fm_approx hit (substitutions only) is an edit match that ends at its end with at most its
    mismatches"""
    x = S.gen_dna(64 * KiB)
    rng = np.random.default_rng(12)
    b = archon.Block()
    try:
        b.forward(x)
        for K in (1, 2):
            pats = []
            for m in (8, 12, 20, 40):
                for q in rng.integers(0, x.size - m, 3):
                    p = x[q:q + m].copy()
                    for _ in range(int(rng.integers(0, K + 1))):
                        p[int(rng.integers(0, m))] = rng.choice(np.frombuffer(b"ACGT", np.uint8))
                    pats.append(p.tobytes())
            _, _, ah = b.fm_approx(pats, K)
            starts = b.fm_locate_hits(pats, ah)
            nhits, h = b.fm_edit(pats, K)
            first = np.concatenate([[0], np.cumsum(nhits.astype(np.int64))])
            assert ah.size >= len(pats)
            for hit, ss in zip(ah, starts):
                j = int(hit["pattern"])
                mine = h[first[j]:first[j + 1]]
                for p in ss:
                    at = np.searchsorted(mine["end"], int(p) + len(pats[j]))
                    assert at < mine.size and mine["end"][at] == int(p) + len(pats[j]), (K, j, p)
                    assert mine["distance"][at] <= hit["mismatches"], (K, j, p)
    finally:
        b.close()


@pytest.mark.parametrize("shape", ["random", "dna", "text", "prose"])
def test_1mib(archon, shape):
    """1 MiB blocks: six patterns of 24 and 100 bytes at K = 2 and 4 against rule_np, through the block and a sampled handle"""
    x = _shape(shape, MiB)
    rng = np.random.default_rng(17 + len(shape))
    pats = [_edited(x, rng, int(rng.integers(0, x.size - 200)), m, 2) for m in (24, 24, 24, 100, 100, 100)]
    cells = [E.rule_cells(x, p) for p in pats]
    b = archon.Block()
    try:
        b.forward(x)
        f = b.fm_index(32)
        for K in (2, 4):
            want = _want(archon, cells, K)
            assert (want[0] > 0).all()
            _same(b.fm_edit(pats, K), want)
            _same(f.edit(pats, K), want)
        f.close()
    finally:
        b.close()


def test_forms_and_refusals(archon, monkeypatch):
    """the device form equals the host form; counting only; cap < total is ARCHON_E_ARG with the counts written and the hits
    untouched; a pattern with m <= K in the device form is ARCHON_E_ARG with nothing emitted; a handle without samples, a
    block without its SA and a tile too wide for K are refused; the edit calls leave the other FM records alone"""
    import torch
    import pyarchon
    x = S.gen_dna(256 * KiB)
    rng = np.random.default_rng(11)
    K = 2
    pats = [_edited(x, rng, int(rng.integers(0, x.size - 100)), m, K) for m in (6, 15, 15, 40, 40, 90)]
    b = archon.Block()
    try:
        _, base = b.forward(x)
        f = b.fm_index(32)
        b.fm_count(pats)
        f.locate(pats[3:])
        b.fm_approx(pats[:2], 1)
        before = (archon.fm_stats().asdict(), archon.fm_walk_stats().asdict(), archon.fm_approx_stats().asdict())
        nhits, h = f.edit(pats, K)
        assert (b.fm_edit(pats, K)[1] == h).all()
        assert before == (archon.fm_stats().asdict(), archon.fm_walk_stats().asdict(), archon.fm_approx_stats().asdict())
        c_nhits, none = f.edit(pats, K, emit=False)
        assert none is None and (c_nhits == nhits).all() and archon.fm_edit_stats().hits == h.size
        # the device form
        packed, off = fm_naive.pack(pats)
        pt = torch.tensor(packed, device="cuda:0")
        ot = torch.tensor(off.astype(np.int32), device="cuda:0")
        nt = torch.full((len(pats),), -1, dtype=torch.int32, device="cuda:0")
        ht = torch.full((4 * h.size + 8,), -1, dtype=torch.int32, device="cuda:0")
        assert f.edit_dev(pt, ot, K, nt, ht) == h.size
        torch.cuda.synchronize()
        assert (nt.cpu().numpy().view(np.uint32) == nhits).all()
        hd = ht.cpu().numpy()
        assert (hd[:4 * h.size].view(np.uint32).view(pyarchon.FM_EDIT) == h).all() and (hd[4 * h.size:] == -1).all()
        nt.fill_(-1)
        assert f.edit_dev(pt, ot, K, nt) == h.size
        assert (nt.cpu().numpy().view(np.uint32) == nhits).all()
        # a pattern of m <= K bytes, found on the device: nothing emitted
        bad = off.astype(np.int32).copy()
        bad[1:] -= 4                    # the first pattern keeps 2 of its 6 bytes
        nt.fill_(-1)
        ht.fill_(-1)
        with pytest.raises(pyarchon.ArchonError):
            f.edit_dev(pt, torch.tensor(bad, device="cuda:0"), K, nt, ht)
        torch.cuda.synchronize()
        assert (nt.cpu().numpy() == -1).all() and (ht.cpu().numpy() == -1).all()
        # the cap rule on the host form
        assert h.size > 1
        L = pyarchon.lib()
        hits_small = np.zeros(h.size - 1, pyarchon.FM_EDIT)
        hits_small["start"] = 7
        nh2 = np.zeros(len(pats), np.uint32)
        total = ctypes.c_uint64(0)
        for fn, handle in ((L.archon_hip_fm_edit, f.h), (L.archon_hip_block_fm_edit, b.h)):
            nh2[:] = 0
            rc = fn(handle, pyarchon._p(packed), pyarchon._p(off), len(pats), K, pyarchon._p(nh2), pyarchon._p(hits_small), h.size - 1,
                    ctypes.cast(ctypes.byref(total), ctypes.c_void_p))
            assert rc == pyarchon.E_ARG and total.value == h.size
            assert (nh2 == nhits).all() and (hits_small["start"] == 7).all() and (hits_small["end"] == 0).all()
        # refusals
        monkeypatch.setenv("ARCHON_EDIT_TILE", "61")
        with pytest.raises(pyarchon.ArchonError):
            b.fm_edit(pats, K)
        monkeypatch.delenv("ARCHON_EDIT_TILE")
        plain = archon.FmIndex(b.read_bwt(), base)
        with pytest.raises(pyarchon.ArchonError):
            plain.edit(pats, K)
        plain.close()
        b.forward(x, want_sa=False)
        with pytest.raises(pyarchon.ArchonError):
            b.fm_edit(pats, K)
        assert (f.edit(pats, K)[1] == h).all()
        f.close()
    finally:
        b.close()


def test_repeatable_and_two_threads(archon):
    """identical output on two runs, and from two threads with a handle each on two contexts at once"""
    x = S.gen_dna(256 * KiB)
    rng = np.random.default_rng(23)
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        bwt = b.read_bwt()
    finally:
        b.close()
    pats = [_edited(x, rng, int(rng.integers(0, x.size - 100)), m, 3) for m in (10, 24, 50) for _ in range(6)]
    f0 = archon.FmIndex(bwt, base).sample(32)
    one = f0.edit(pats, 3)
    two = f0.edit(pats, 3)
    assert one[1].size and all((u == v).all() for u, v in zip(one, two))
    out = [None, None]

    def work(slot):
        archon.bind_context(slot)
        f = archon.FmIndex(bwt, base).sample(32)
        out[slot] = f.edit(pats, 3)
        f.close()

    ts = [threading.Thread(target=work, args=(s,)) for s in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r in out:
        assert r is not None and all((u == v).all() for u, v in zip(r, one))
    f0.close()


@pytest.mark.parametrize("batch", [0, 1])
@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, grid, batch, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) at K = 2 and 4 on 64 KiB of text, 22 patterns, in one batch and with
    ARCHON_EDIT_BATCH=1: every wave of the piece count, the tile count, the tile list and the banded check takes item after
    item -- matches from rule_np, counters from tile_model, through the block and a sampled handle, counting only and
    emitting; byte-equal to the same calls without the route, with their counters, launches and host waits"""
    if batch:
        monkeypatch.setenv("ARCHON_EDIT_BATCH", str(batch))
    x = _shape("text", 64 * KiB)
    rng = np.random.default_rng(64 * KiB + 77)
    b = archon.Block()
    try:
        b.forward(x)
        f = b.fm_index(32)
        b.fm_count([b"a"])                   # (the table built before the calls that are compared)
        for K in (2, 4):
            pats = _patterns(x, rng, K, (K + 1, 7, 33, 64, 65, 130) * 3)
            want = _want(archon, [E.rule_cells(x, p) for p in pats], K)
            counters = _counters(x, pats, K, 32)
            assert len(pats) == 22 and want[1].size > 22

            def call():
                out, stats = [], []
                for search in (b.fm_edit, f.edit):
                    nhits, none = search(pats, K, emit=False)
                    assert none is None and (nhits == want[0]).all()
                    stats.append(archon.fm_edit_stats())
                    got = search(pats, K)
                    _same(got, want)
                    st = _check_stats(archon, want, counters, K, 32, len(pats))
                    assert st.batches == (len(pats) if batch else 1) and (st.lf_steps > 0) == (search == f.edit)
                    stats.append(st)
                    out += [nhits, got[0], got[1]]
                return out, stats
            G.same_under(monkeypatch, grid, call)
        f.close()
    finally:
        b.close()
