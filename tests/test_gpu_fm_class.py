"""GPU: the class search (archon_hip_fm_classes, _fm_classes_dev, _block_fm_classes; include/archon_hip.h) against the rule of
the header in Python (tests/fm_class_naive.py, pinned to brute force by test_fm_class_abi.py): hits in order, both work
counters and the largest width, a deep stack, the identity table against fm_count, the hits located and counted again, the
device form, the cap rule, the width bound and repeatability."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import fm_approx_naive as A
import fm_class_naive as C
import fm_naive
import fm_sampled_naive as M
import stride_util as G

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
NODE_BUDGET = 20_000_000        # expansions + steps one call may take at most (the Python rule predicts them first)
SMALL_ROUTE = {"ARCHON_FM_SUB_ROWS": "16", "ARCHON_FM_SUPER_ROWS": "256"}
WILD = 0xF7
NAMES = (0, 1, 2, 3, 7, 255)


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


def _small_table(archon):
    """0 -> {0}, 1 -> {0, 1}, 2 -> all bytes, 3 -> {1}, 7 -> empty, 255 -> {255} (the table of test_fm_class_abi.py)"""
    t = archon.classes_identity()
    for byte, accepted in ((1, [0, 1]), (2, range(256)), (3, [1]), (7, [])):
        t = archon.classes_set(t, byte, accepted)
    return t


def _tables(archon):
    ident = archon.classes_identity()
    pair, quad = ident.copy(), ident.copy()
    for b in range(256):
        pair = archon.classes_set(pair, b, [b, b ^ 1])
        quad = archon.classes_set(quad, b, [(b & ~3) + i for i in range(4)])
    return {"pair": pair, "quad": quad, "fold": archon.classes_fold_case(), "iupac": archon.classes_iupac(),
            "wild": archon.classes_set(ident, WILD, range(256))}


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


def _patterns(x, rng, sets, wild):
    """substrings of x; the same with some bytes replaced by another name of a class that holds them; with `wild`, substrings
    with 1 to 3 positions set to the wildcard; one random pattern, the empty pattern, one longer than the block.  A byte is
    replaced only while the pattern's width stays within the bound"""
    n = x.size
    here = set(np.unique(x).tolist())
    cost = [sum(c in here for c in s) - 1 for s in sets]        # what a pattern byte adds to the width
    names = {}          # byte -> the other pattern bytes whose class holds it

    def other(c):
        if c not in names:
            names[c] = [b for b in range(256) if b != c and c in sets[b]]
        return names[c]

    def put(p, i, b):
        if sum(cost[c] for c in p) - cost[p[i]] + cost[b] <= C.MAX_WIDTH:
            p[i] = b

    pats = []
    for m in (1, 2, 5, 12, 30, 70):
        if m > n:
            continue
        q = int(rng.integers(0, n - m + 1))
        p = x[q:q + m].copy()
        pats.append(p.tobytes())
        for _ in range(1 + m // 8):
            i = int(rng.integers(0, m))
            if other(int(p[i])):
                put(p, i, other(int(p[i]))[int(rng.integers(0, len(other(int(p[i])))))])
        pats.append(p.tobytes())
    if wild:
        for a, m in enumerate((2, 5, 12, 30)):
            if m > n:
                continue
            q = int(rng.integers(0, n - m + 1))
            p = x[q:q + m].copy()
            for i in rng.choice(m, min(1 + a % 3, m), replace=False):
                put(p, int(i), WILD)
            pats.append(p.tobytes())
    pats.append(rng.integers(0, 256, 6, dtype=np.uint8).tobytes())
    pats.append(b"")
    pats.append(np.resize(x, n + 1).tobytes())
    return pats


def _predict(rule, pats, table, sets):
    """the rule's (hits, expansions, steps) of every pattern and the largest width of the call, under the node budget"""
    want = [C.search(rule, p, table, sets) for p in pats]
    assert sum(e + s for _, e, s in want) < NODE_BUDGET
    width = max(C.width(rule, p, sets) for p in pats)
    assert width <= C.MAX_WIDTH
    return want, width


def _check_against_rule(archon, want, width, got, pats):
    nhits, nocc, h = got
    per = _per_pattern(nhits, h)
    for p, g, (w, _, _) in zip(pats, per, want):
        assert g == w, p
    assert (nocc == [sum(b - a for a, b, _ in w) for w, _, _ in want]).all()
    st = archon.fm_class_stats()
    assert st.expansions == sum(e for _, e, _ in want)
    assert st.steps == sum(s for _, _, s in want)
    assert st.hits == h.size and st.patterns == len(pats) and st.max_width == width
    assert st.occurrences == int(nocc.sum())


def test_tiny_exhaustive(archon):
    """every string of length <= 6 over {0, 1, 255}, every pattern of length <= 3 over the six class names, through a block and
    through a host-built index: the rule's hits in its order, its counters and the largest width"""
    table = _small_table(archon)
    sets = C.table_sets(table)
    patterns = [b""] + [bytes(p) for m in range(1, 4) for p in itertools.product(NAMES, repeat=m)]
    b = archon.Block()
    try:
        for n in range(1, 7):
            for tt in itertools.product((0, 1, 255), repeat=n):
                x = np.array(tt, np.uint8)
                _, bwt, base = M.a7_forward(bytes(tt))
                _, b0 = b.forward(x)
                assert b0 == base
                rule = A.Rule(bwt, base)
                want, width = _predict(rule, patterns, table, sets)
                _check_against_rule(archon, want, width, b.fm_classes(patterns, table), patterns)
                f = archon.FmIndex(np.frombuffer(bwt, np.uint8).copy(), base)
                _check_against_rule(archon, want, width, f.classes(patterns, table), patterns)
                f.close()
    finally:
        b.close()


@pytest.mark.parametrize("route", ["default", "small"])
@pytest.mark.parametrize("n", [4 * KiB, 64 * KiB])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_blocks_against_rule(archon, monkeypatch, shape, n, route):
    """blocks of every shape, the default table and 16-row sub-chunks / 256-row superblocks, under five class tables: hits in
    order, counters, the largest width; the block and a host-built index of its BWT agree; the calls leave the FM and the
    approximate statistics alone"""
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
        b.fm_approx([b"a"], 1)
        f = archon.FmIndex(bwt, base)
        for name, table in _tables(archon).items():
            sets = C.table_sets(table)
            pats = _patterns(x, rng, sets, name == "wild")
            want, width = _predict(rule, pats, table, sets)
            fm_before, fma_before = archon.fm_stats().asdict(), archon.fm_approx_stats().asdict()
            got = b.fm_classes(pats, table)
            _check_against_rule(archon, want, width, got, pats)
            g2 = f.classes(pats, table)
            assert (g2[0] == got[0]).all() and (g2[1] == got[1]).all() and (g2[2] == got[2]).all()
            assert archon.fm_stats().asdict() == fm_before and archon.fm_approx_stats().asdict() == fma_before
        f.close()
    finally:
        b.close()


def _de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence B(k, n) over 0 .. k - 1"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


@pytest.mark.parametrize("case", ["dna", "binary"])
def test_deep_stack(archon, case):
    """a de Bruijn sequence with its first symbols appended holds every string of the pattern's length once: 4096 hits of one
    row each in ascending order of their strings, every inner node an expansion, and 3 (or 1) frames left pending at every
    position"""
    if case == "dna":
        sigma, m, table, pat = b"ACGT", 6, archon.classes_iupac(), b"NNNNNN"
    else:
        sigma, m, pat = bytes([0x60, 0x61]), 12, bytes([0x60]) * 12
        table = archon.classes_set(archon.classes_set(archon.classes_identity(), 0x60, sigma), 0x61, sigma)
    seq = _de_bruijn(len(sigma), m)
    x = np.array([sigma[s] for s in seq + seq[:m - 1]], np.uint8)
    assert x.size == len(sigma) ** m + m - 1 and (case != "dna" or x.size == 4101)
    b = archon.Block()
    try:
        b.forward(x)
        nhits, nocc, h = b.fm_classes([pat], table)
        st = archon.fm_class_stats()
        assert nhits[0] == 4096 and nocc[0] == 4096 and h.size == 4096
        assert (h["hi"] - h["lo"] == 1).all()
        inner = sum(len(sigma) ** t for t in range(1, m))
        assert (st.expansions, st.steps, st.max_width) == (inner, 0, (len(sigma) - 1) * m)
        if case == "dna":
            assert (st.expansions, st.max_width) == (1364, 18)
        starts = b.fm_locate_hits([pat], h)
        words = [x[int(s[0]):int(s[0]) + m].tobytes() for s in starts]
        assert words == sorted(words) and len(set(words)) == 4096
        assert (h["mismatches"] == [sum(c != q for c, q in zip(w, pat)) for w in words]).all()
    finally:
        b.close()


def test_identity_is_count(archon):
    """under the identity table every pattern gives fm_count's range (or no hit) and fm_count's steps, with no expansion"""
    x = S.gen_text(64 * KiB)
    rng = np.random.default_rng(3)
    ident = archon.classes_identity()
    b = archon.Block()
    try:
        b.forward(x, want_sa=False)
        pats = []
        for m in (1, 4, 9, 40):
            for _ in range(4):
                q = int(rng.integers(0, x.size - m + 1))
                p = x[q:q + m].copy()
                if rng.integers(0, 2):
                    p[int(rng.integers(0, m))] = x[int(rng.integers(0, x.size))]     # (a byte of the block: no class is empty)
                pats.append(p.tobytes())
        pats += [b"", np.resize(x, x.size + 1).tobytes()]
        lo, hi = b.fm_count(pats)
        steps = archon.fm_stats().steps
        nhits, nocc, h = b.fm_classes(pats, ident)
        st = archon.fm_class_stats()
        assert st.steps == steps and st.expansions == 0 and st.max_width == 0
        for p, a, z, g in zip(pats, lo, hi, _per_pattern(nhits, h)):
            assert g == ([(int(a), int(z), 0)] if z > a else []), p
    finally:
        b.close()


def test_hits_are_counts_and_locate(archon):
    """64 KiB of text under the fold table: the block's SA and a sampled handle give identical starts for the hits; every hit's
    string lies in the classes, differs from the pattern in `mismatches` places and has the hit's rows under fm_count"""
    x = S.gen_text(64 * KiB)
    rng = np.random.default_rng(5)
    table = archon.classes_fold_case()
    sets = C.table_sets(table)
    b = archon.Block()
    try:
        b.forward(x)
        pats = []
        for m in (2, 3, 4, 6, 9):
            for _ in range(3):
                q = int(rng.integers(0, x.size - m + 1))
                pats.append(bytes(x[q:q + m]).swapcase())
        nhits, nocc, h = b.fm_classes(pats, table)
        assert h.size > len(pats) and (h["mismatches"] > 0).any()
        starts = b.fm_locate_hits(pats, h)
        f = b.fm_index(16)
        starts_s = f.locate_hits(pats, h)
        assert len(starts) == h.size and all((u == v).all() for u, v in zip(starts, starts_s))
        assert sum(u.size for u in starts) == int(nocc.sum())
        m = [len(pats[j]) for j in h["pattern"]]
        words = f.extract([int(s[0]) for s in starts], m)
        for w, j, d in zip(words, h["pattern"], h["mismatches"]):
            p = pats[j]
            assert all(c in sets[q] for c, q in zip(bytes(w), p))
            assert sum(c != q for c, q in zip(bytes(w), p)) == d
        clo, chi = b.fm_count(words)
        assert (clo == h["lo"]).all() and (chi == h["hi"]).all()
        f.close()
    finally:
        b.close()


def test_dev_form_cap_and_counting_only(archon):
    """the device form equals the host form; cap < total is ARCHON_E_ARG with counts and total written and the hits untouched;
    hits=False gives the same counts"""
    import torch
    import pyarchon
    x = S.gen_dna(64 * KiB)
    rng = np.random.default_rng(11)
    table = archon.classes_iupac()
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        f = archon.FmIndex(b.read_bwt(), base)
        pats = []
        for m in (6, 15, 40):
            for _ in range(3):
                q = int(rng.integers(0, x.size - m + 1))
                p = x[q:q + m].copy()
                p[rng.choice(m, 3, replace=False)] = np.frombuffer(b"NRY", np.uint8)
                pats.append(p.tobytes())
        pats += [b"", b"ACGNTT"]
        nhits, nocc, h = f.classes(pats, table)
        c_nhits, c_nocc, none = f.classes(pats, table, hits=False)
        assert none is None and (c_nhits == nhits).all() and (c_nocc == nocc).all()
        packed, off = fm_naive.pack(pats)
        pt = torch.tensor(packed, device="cuda:0")
        ot = torch.tensor(off.astype(np.int32), device="cuda:0")
        tt = torch.tensor(table.view(np.int32).ravel(), device="cuda:0")
        nt = torch.zeros(len(pats), dtype=torch.int32, device="cuda:0")
        ct = torch.zeros(len(pats), dtype=torch.int32, device="cuda:0")
        ht = torch.full((4 * h.size + 8,), -1, dtype=torch.int32, device="cuda:0")
        assert f.classes_dev(pt, ot, tt, nt, ct, ht) == h.size
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
        rc = L.archon_hip_fm_classes(f.h, pyarchon._p(packed), pyarchon._p(off), len(pats), pyarchon._p(table), pyarchon._p(nh2), pyarchon._p(no2),
                                     pyarchon._p(hits_small), h.size - 1, ctypes.cast(ctypes.byref(total), ctypes.c_void_p))
        assert rc == pyarchon.E_ARG and total.value == h.size
        assert (nh2 == nhits).all() and (no2 == nocc).all() and (hits_small["lo"] == 7).all()
        f.close()
    finally:
        b.close()


def test_width_bound(archon):
    """W = 1020 and W = 900 are accepted; W = 1275 is ARCHON_E_ARG with nothing written and max_width in the statistics; a
    pattern with an empty class gives no hits and no work and leaves the other patterns of the call alone"""
    import pyarchon
    x = S.gen_random(64 * KiB)
    assert np.unique(x).size == 256
    wild = archon.classes_set(archon.classes_identity(), WILD, range(256))
    q = 1000
    stem = x[q:q + 12].tobytes()
    assert WILD not in x[q:q + 16] and 7 not in stem
    b = archon.Block()
    try:
        b.forward(x, want_sa=False)
        lo, hi = b.fm_count([stem, x[q:q + 16].tobytes()])
        assert hi[0] - lo[0] == 1
        nhits, nocc, h = b.fm_classes([stem + bytes([WILD]) * 4], wild)
        st = archon.fm_class_stats()
        assert st.max_width == 1020
        # the stem is unique, so the one string behind it is the text's: four expansions, each with one child
        assert (int(nhits[0]), int(nocc[0])) == (1, 1) and _hits(h) == [(int(lo[1]), int(hi[1]), 4)]
        assert (st.expansions, st.steps) == (4, 11)
        # five wildcards: refused, nothing written
        L = pyarchon.lib()
        pats = [stem + bytes([WILD]) * 5, stem]
        packed, off = fm_naive.pack(pats)
        nh, no = np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
        hits = np.zeros(8, pyarchon.FM_HIT)
        hits["lo"] = 7
        total = ctypes.c_uint64(99)
        rc = L.archon_hip_block_fm_classes(b.h, pyarchon._p(packed), pyarchon._p(off), 2, pyarchon._p(wild), pyarchon._p(nh), pyarchon._p(no),
                                           pyarchon._p(hits), 8, ctypes.cast(ctypes.byref(total), ctypes.c_void_p))
        assert rc == pyarchon.E_ARG and total.value == 99
        assert (nh == 77).all() and (no == 77).all() and (hits["lo"] == 7).all()
        assert archon.fm_class_stats().max_width == 1275
        with pytest.raises(pyarchon.ArchonError):
            b.fm_classes(pats, wild)
        # an empty class: no hits, no work, the neighbours as they were
        none = archon.classes_set(wild, 7, [])
        alone = b.fm_classes([stem, stem[:5] + bytes([WILD])], none)
        alone_st = archon.fm_class_stats()
        both = b.fm_classes([stem, stem[:3] + bytes([7]) + stem[4:], stem[:5] + bytes([WILD]), bytes([7])], none)
        both_st = archon.fm_class_stats()
        assert list(both[0]) == [int(alone[0][0]), 0, int(alone[0][1]), 0] and list(both[1]) == [int(alone[1][0]), 0, int(alone[1][1]), 0]
        assert _hits(both[2]) == _hits(alone[2]) and list(both[2]["pattern"]) == [0 if j == 0 else 2 for j in alone[2]["pattern"]]
        assert (both_st.expansions, both_st.steps, both_st.max_width) == (alone_st.expansions, alone_st.steps, alone_st.max_width)
    finally:
        b.close()
    # DNA: 300 wildcards behind a unique 12-mer, W = 900
    y = S.gen_dna(64 * KiB)
    table = archon.classes_iupac()
    b = archon.Block()
    try:
        b.forward(y, want_sa=False)
        at = None
        for q in range(0, y.size - 312, 313):
            lo, hi = b.fm_count([y[q:q + 12].tobytes()])
            if hi[0] - lo[0] == 1:
                at = q
                break
        assert at is not None
        pat = y[at:at + 12].tobytes() + b"N" * 300
        nhits, nocc, h = b.fm_classes([pat], table)
        st = archon.fm_class_stats()
        lo, hi = b.fm_count([y[at:at + 312].tobytes()])
        assert st.max_width == 900 and len(pat) == 312
        assert int(nhits[0]) == 1 and _hits(h) == [(int(lo[0]), int(hi[0]), 300)]
        assert (st.expansions, st.steps) == (300, 11)
    finally:
        b.close()


def test_repeatable_and_two_threads(archon):
    """identical output on two runs, and from two threads on two contexts at once"""
    x = S.gen_text(256 * KiB)
    rng = np.random.default_rng(23)
    table = archon.classes_fold_case()
    b = archon.Block()
    try:
        _, base = b.forward(x, want_sa=False)
        bwt = b.read_bwt()
    finally:
        b.close()
    pats = []
    for m in (3, 5, 8, 20):
        for _ in range(8):
            q = int(rng.integers(0, x.size - m + 1))
            pats.append(bytes(x[q:q + m]).swapcase())
    f0 = archon.FmIndex(bwt, base)
    one = f0.classes(pats, table)
    two = f0.classes(pats, table)
    assert one[2].size > len(pats) and all((u == v).all() for u, v in zip(one, two))
    out = [None, None]

    def work(slot):
        archon.bind_context(slot)
        f = archon.FmIndex(bwt, base)
        out[slot] = f.classes(pats, table)
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
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID): the fold-case table on 64 KiB of text and the IUPAC table on 64 KiB of
    DNA with some seventy patterns each, so that every wave takes several; and on the de Bruijn block of test_deep_stack the
    pattern NNNNNN -- 4096 hits, 18 frames pending on the LDS stack -- directly ahead of plain six-byte patterns on the same
    wave (patterns j, j + 4 under one workgroup, j, j + 12 under three).  The rule's hits, counters and largest width from the
    count pass alone and with the emit pass, through a block and a host-built index, byte-equal to the same calls without
    the route, with their counters"""
    tables = _tables(archon)
    seq = _de_bruijn(4, 6)
    cases = [(_shape("text", 64 * KiB), "fold", None), (_shape("dna", 64 * KiB), "iupac", None),
             (np.array([b"ACGT"[s] for s in seq + seq[:5]], np.uint8), "iupac", b"NNNNNN")]
    for x, name, wide in cases:
        table = tables[name]
        sets = C.table_sets(table)
        rng = np.random.default_rng(x.size + len(name))
        b = archon.Block()
        try:
            _, base = b.forward(x, want_sa=False)
            bwt = b.read_bwt()
            rule = A.Rule(bwt, base)
            f = archon.FmIndex(bwt, base)
            b.fm_count([b"a"])
            f.count([b"a"])                  # (both tables built: `built` is 0 in every call below)
            if wide is None:
                pats = [p for _ in range(4) for p in _patterns(x, rng, sets, False)]
                assert len(pats) > 48
            else:
                narrow = [x[q:q + 6].tobytes() for q in rng.integers(0, x.size - 6, 8)]
                pats = [wide] * 4 + narrow[:4] + [wide] * 4 + narrow[4:]
            want, width = _predict(rule, pats, table, sets)
            if wide is not None:
                assert width == 18 and len(want[0][0]) == 4096 and all(len(want[j][0]) == 1 for j in (4, 5, 6, 7, 12, 13, 14, 15))

            def call():
                out, st = [], []
                for search in (b.fm_classes, f.classes):
                    nhits, nocc, none = search(pats, table, hits=False)
                    assert none is None
                    st.append(archon.fm_class_stats())
                    got = search(pats, table)
                    _check_against_rule(archon, want, width, got, pats)
                    assert (got[0] == nhits).all() and (got[1] == nocc).all()
                    st.append(archon.fm_class_stats())
                    out += [nhits, nocc, got[0], got[1], got[2]]
                return out, st
            G.same_under(monkeypatch, grid, call)
            f.close()
        finally:
            b.close()
