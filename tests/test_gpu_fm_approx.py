"""GPU: the approximate FM search (archon_hip_fm_approx, _fm_approx_dev, _block_fm_approx, _fm_locate_hits,
_block_fm_locate_hits; include/archon_hip.h) against the rule of the header in Python (tests/fm_approx_naive.py, pinned to
brute force by test_fm_approx_abi.py) and the C brute force (tests/fm_approx_naive.c): hits in order, both work counters,
the starts of every hit from the SA and from the samples, the device form, the cap rule and repeatability."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import fm_approx_naive as A
import fm_naive
import fm_sampled_naive as M
import stride_util as G

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
NODE_BUDGET = 20_000_000        # expansions + steps one call may take at most (the C brute force predicts them first)
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "256"}


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


def _hits(h):
    return [(int(a), int(b), int(d)) for a, b, d in zip(h["lo"], h["hi"], h["mismatches"])]


def _per_pattern(nhits, h):
    """the hit array cut into one list of (lo, hi, d) per pattern (checking the pattern field on the way)"""
    out, at = [], 0
    for j, c in enumerate(nhits):
        part = h[at:at + int(c)]
        assert (part["pattern"] == j).all()
        out.append(_hits(part))
        at += int(c)
    assert at == h.size
    return out


def _patterns(x, rng, K, lengths, count):
    """substrings of x with 0 .. K random substitutions, random patterns, the empty pattern, one longer than the block"""
    n = x.size
    pats = []
    for m in lengths:
        if m > n:
            continue
        for _ in range(count):
            q = int(rng.integers(0, n - m + 1))
            p = x[q:q + m].copy()
            for _ in range(int(rng.integers(0, K + 1))):
                p[int(rng.integers(0, m))] = rng.integers(0, 256)
            pats.append(p.tobytes())
    pats.append(rng.integers(0, 256, 6, dtype=np.uint8).tobytes())
    pats.append(b"")
    pats.append(np.resize(x, n + 1).tobytes())
    return pats


def _check_against_rule(archon, want, got, pats, K):
    """want: the rule's (hits, expansions, steps) of every pattern"""
    nhits, nocc, h = got
    per = _per_pattern(nhits, h)
    for p, g, (w, _, _) in zip(pats, per, want):
        assert g == w, (p, K)
    assert (nocc == [sum(b - a for a, b, _ in w) for w, _, _ in want]).all()
    st = archon.fm_approx_stats()
    assert st.expansions == sum(e for _, e, _ in want)
    assert st.steps == sum(s for _, _, s in want)
    assert st.hits == h.size and st.max_mismatches == K and st.patterns == len(pats)


def test_tiny_exhaustive(archon):
    """every string of length <= 6 over {0, 1, 255}, every pattern of length <= 3 over {0, 1, 2, 255}, K = 0 .. 3, through a
    block and through a host-built index: the rule's hits in its order, and its counters"""
    patterns = [b""] + [bytes(p) for m in range(1, 4) for p in itertools.product((0, 1, 2, 255), repeat=m)]
    b = archon.Block()
    try:
        for n in range(1, 7):
            for tt in itertools.product((0, 1, 255), repeat=n):
                x = np.array(tt, np.uint8)
                _, bwt, base = M.a7_forward(bytes(tt))
                sa, b0 = b.forward(x)
                assert b0 == base
                rule = A.Rule(bwt, base)
                f = archon.FmIndex(np.frombuffer(bwt, np.uint8).copy(), base)
                for K in range(4):
                    want = [rule.search(p, K) for p in patterns]
                    _check_against_rule(archon, want, b.fm_approx(patterns, K), patterns, K)
                    _check_against_rule(archon, want, f.approx(patterns, K), patterns, K)
                f.close()
    finally:
        b.close()


@pytest.mark.parametrize("route", ["default", "small"])
@pytest.mark.parametrize("n", [4 * KiB, 64 * KiB])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_blocks_against_rule(archon, monkeypatch, shape, n, route):
    """blocks of every shape, the default table and 16-row sub-chunks / 256-row superblocks: hits in order, counters; the
    block and a host-built index of its BWT agree; approx leaves the FM statistics alone"""
    if route == "small":
        for k, v in SMALL_ROUTE.items():
            monkeypatch.setenv(k, v)
    x = _shape(shape, n)
    rng = np.random.default_rng(n + len(shape))
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        bwt = b.read_bwt()
        rule = A.Rule(bwt, base)
        b.fm_count([b"a"])
        for K in (1, 2):
            pats = _patterns(x, rng, K, (1, 2, 5, 12, 30, 70), 2 if K == 2 else 3)
            fm_before = archon.fm_stats().asdict()
            got = b.fm_approx(pats, K)
            _check_against_rule(archon, [rule.search(p, K) for p in pats], got, pats, K)
            assert archon.fm_stats().asdict() == fm_before
            f = archon.FmIndex(bwt, base)
            g2 = f.approx(pats, K)
            assert (g2[0] == got[0]).all() and (g2[1] == got[1]).all() and (g2[2] == got[2]).all()
            f.close()
    finally:
        b.close()


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return A.build(tmp_path_factory.mktemp("fm_approx_naive"))


@pytest.mark.parametrize("shape", ["random", "dna", "text", "prose"])
def test_1mib_against_brute_force(archon, naive, shape):
    """1 MiB blocks at K = 1, 2 against the C brute force: the hit sets with their distances, the starts of every hit by
    locate_hits (the block's SA and a sampled handle give identical arrays), and both counters"""
    n = MiB
    x = _shape(shape, n)
    rng = np.random.default_rng(17 + len(shape))
    b = archon.Block()
    try:
        sa, base = b.forward(x)
        f = b.fm_index(32)
        for K in (1, 2):
            pats, want = [], []
            for p in _patterns(x, rng, K, (8, 20, 32), 2)[:-3]:
                groups, ex, st = naive(x, p, K)
                assert ex + st < NODE_BUDGET
                pats.append(p)
                want.append((groups, ex, st))
            nhits, nocc, h = b.fm_approx(pats, K)
            stats = archon.fm_approx_stats()
            assert stats.expansions == sum(w[1] for w in want) and stats.steps == sum(w[2] for w in want)
            starts = b.fm_locate_hits(pats, h)
            assert stats.hits == h.size
            starts_s = f.locate_hits(pats, h)
            assert all((u == v).all() for u, v in zip(starts, starts_s))
            ws = archon.fm_approx_stats()
            assert ws.occurrences == sum(u.size for u in starts) and ws.lf_steps > 0
            at = 0
            for j, (p, (groups, _, _)) in enumerate(zip(pats, want)):
                mine = [(int(h[i]["mismatches"]), sorted(int(v) for v in starts[i])) for i in range(at, at + int(nhits[j]))]
                at += int(nhits[j])
                assert sorted(mine) == sorted(groups), (shape, K, p)
                assert int(nocc[j]) == sum(len(s) for _, s in groups)
        f.close()
    finally:
        b.close()


def test_k0_is_count_and_hits_are_counts(archon):
    """K = 0 gives exactly fm_count's range and steps; for every hit at K = 2, fm_count of its string (extracted from the
    sampled index at its first start) gives its rows"""
    x = S.gen_text(64 * KiB)
    rng = np.random.default_rng(3)
    b = archon.Block()
    try:
        b.forward(x)
        pats = _patterns(x, rng, 1, (1, 4, 9, 40), 4)
        lo, hi = b.fm_count(pats)
        steps = archon.fm_stats().steps
        nhits, nocc, h = b.fm_approx(pats, 0)
        assert archon.fm_approx_stats().steps == steps and archon.fm_approx_stats().expansions == 0
        per = _per_pattern(nhits, h)
        for p, a, z, g in zip(pats, lo, hi, per):
            assert g == ([(int(a), int(z), 0)] if z > a else []), p
        nhits, nocc, h = b.fm_approx(pats[:-3], 2)
        f = b.fm_index(16)
        starts = f.locate_hits(pats[:-3], h)
        m = [len(pats[j]) for j in h["pattern"]]
        words = f.extract([int(s[0]) for s in starts], m)
        clo, chi = b.fm_count(words)
        assert (clo == h["lo"]).all() and (chi == h["hi"]).all()
        assert ((b.fm_approx(words, 0)[1]) == chi - clo).all()
        f.close()
    finally:
        b.close()


def test_dev_form_cap_and_counting_only(archon):
    """the device form equals the host form; cap < total is ARCHON_E_ARG with counts and total written and the hits untouched;
    hits=False gives the same counts"""
    import torch
    import pyarchon
    x = S.gen_dna(256 * KiB)
    rng = np.random.default_rng(11)
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        f = archon.FmIndex(b.read_bwt(), base)
        pats = _patterns(x, rng, 2, (6, 15, 40), 3)
        nhits, nocc, h = f.approx(pats, 2)
        c_nhits, c_nocc, none = f.approx(pats, 2, hits=False)
        assert none is None and (c_nhits == nhits).all() and (c_nocc == nocc).all()
        packed, off = fm_naive.pack(pats)
        pt = torch.tensor(packed, device="cuda:0")
        ot = torch.tensor(off.astype(np.int32), device="cuda:0")
        nt = torch.zeros(len(pats), dtype=torch.int32, device="cuda:0")
        ct = torch.zeros(len(pats), dtype=torch.int32, device="cuda:0")
        ht = torch.full((4 * h.size + 8,), -1, dtype=torch.int32, device="cuda:0")
        assert f.approx_dev(pt, ot, 2, nt, ct, ht) == h.size
        torch.cuda.synchronize()
        assert (nt.cpu().numpy().view(np.uint32) == nhits).all() and (ct.cpu().numpy().view(np.uint32) == nocc).all()
        hd = ht.cpu().numpy()
        assert (hd[:4 * h.size].view(np.uint32).view(pyarchon.FM_HIT) == h).all() and (hd[4 * h.size:] == -1).all()
        # the cap rule on the host form
        assert h.size > 1
        L = pyarchon.lib()
        hits_small = np.zeros(h.size - 1, pyarchon.FM_HIT)
        hits_small["lo"] = 7
        nh2, no2 = np.zeros(len(pats), np.uint32), np.zeros(len(pats), np.uint32)
        total = ctypes.c_uint64(0)
        rc = L.archon_hip_fm_approx(f.h, pyarchon._p(packed), pyarchon._p(off), len(pats), 2, pyarchon._p(nh2), pyarchon._p(no2),
                                    pyarchon._p(hits_small), h.size - 1, ctypes.cast(ctypes.byref(total), ctypes.c_void_p))
        assert rc == pyarchon.E_ARG and total.value == h.size
        assert (nh2 == nhits).all() and (no2 == nocc).all() and (hits_small["lo"] == 7).all()
        f.close()
    finally:
        b.close()


def test_locate_hits_refuses(archon):
    """hits naming a pattern past k, lo > hi or hi > n; a handle without samples; a block without its SA: ARCHON_E_ARG"""
    import pyarchon
    x = S.gen_text(16 * KiB)
    b = archon.Block()
    try:
        b.forward(x, want_sa=False)
        pats = [x[100:110].tobytes()]
        _, _, h = b.fm_approx(pats, 1)
        with pytest.raises(pyarchon.ArchonError):
            b.fm_locate_hits(pats, h)                       # no SA
        f = archon.FmIndex(b.read_bwt(), 0)
        with pytest.raises(pyarchon.ArchonError):
            f.locate_hits(pats, h)                          # no samples
        f.close()
        fs = b.fm_index(32)
        assert len(fs.locate_hits(pats, h)) == h.size
        for field, value in (("pattern", 1), ("hi", x.size + 1), ("lo", x.size)):
            bad = h.copy()
            bad[field][0] = value
            if field == "lo":
                bad["hi"][0] = x.size - 1
            with pytest.raises(pyarchon.ArchonError):
                fs.locate_hits(pats, bad)
        fs.close()
    finally:
        b.close()


def test_repeatable_and_two_threads(archon):
    """identical output on two runs, and from two threads on two contexts at once"""
    x = S.gen_random(1 * MiB)
    rng = np.random.default_rng(23)
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        bwt = b.read_bwt()
    finally:
        b.close()
    pats = _patterns(x, rng, 2, (10, 24, 50), 6)
    f0 = archon.FmIndex(bwt, base)
    one = f0.approx(pats, 2)
    two = f0.approx(pats, 2)
    assert all((u == v).all() for u, v in zip(one, two))
    out = [None, None]

    def work(slot):
        archon.bind_context(slot)
        f = archon.FmIndex(bwt, base)
        out[slot] = f.approx(pats, 2)
        f.close()

    ts = [threading.Thread(target=work, args=(s,)) for s in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r in out:
        assert r is not None and all((u == v).all() for u, v in zip(r, one))
    f0.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) at K = 1, 2 on 64 KiB of text: every wave takes several patterns, and a
    three-byte pattern with 150 (K = 1) and 4500 (K = 2) hits lies directly ahead of patterns with none on the same wave (patterns j, j + 4 under
    one workgroup, j, j + 12 under three) -- the rule's hits and counters from the count pass alone and with the emit pass,
    through a block and a host-built index, byte-equal to the same call without the route, with its counters"""
    n = 64 * KiB
    x = _shape("text", n)
    rng = np.random.default_rng(n + 99)
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        bwt = b.read_bwt()
        rule = A.Rule(bwt, base)
        f = archon.FmIndex(bwt, base)
        f.count([b"a"])
        b.fm_count([b"a"])                       # (both tables built: `built` is 0 in every call below)
        absent = bytes([1, 2, 3, 4, 5, 6])
        for K in (1, 2):
            pats = _patterns(x, rng, K, (1, 2, 5, 12, 30, 70), 8)
            pats[0] = pats[1] = pats[2] = pats[3] = b"the"
            for j in (4, 5, 6, 7, 12, 13, 14, 15):
                pats[j] = absent
            want = [rule.search(p, K) for p in pats]
            assert len(pats) > 48 and len(want[0][0]) > 100 and not want[4][0] and not want[12][0]

            def call():
                out, st = [], []
                for search in (b.fm_approx, f.approx):
                    nhits, nocc, none = search(pats, K, hits=False)
                    assert none is None
                    st.append(archon.fm_approx_stats())
                    got = search(pats, K)
                    _check_against_rule(archon, want, got, pats, K)
                    assert (got[0] == nhits).all() and (got[1] == nocc).all()
                    st.append(archon.fm_approx_stats())
                    out += [nhits, nocc, got[0], got[1], got[2]]
                return out, st
            G.same_under(monkeypatch, grid, call)
        f.close()
    finally:
        b.close()
