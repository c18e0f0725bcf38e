"""GPU: the sampled FM index (archon_hip_fm_sample, _block_fm_index, _fm_read_samples, _fm_locate, _fm_extract,
_fm_extract_dev; include/archon_hip.h) against the oracle's suffix array and the rule of the header
(tests/fm_sampled_naive.py, pinned to brute force by test_fm_sampled_abi.py): ISA samples by both routes, locate equal to
the resident block's locate with the exact LF steps, extract equal to slices of x, lifetime and limits."""
import numpy as np
import pytest

import archon_synth as S
import fm_sampled_naive as M
import stride_util as G

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SHAPES = ("random", "text", "dna", "prose", "a", "ab", "motif")
SIZES = (1, 2, 3, 63, 64, 65, 4099, MiB, 16 * MiB)
RATES = (1, 2, 32, 1024, 65536)
WALK_BUDGET = 1 << 21           # LF steps a test's locate call may take at most (patterns are dropped beyond it)


def _shape(shape, n):
    if shape == "prose":
        return S.gen_prose(n, S.SEED_BASE + 6)
    return S.gen_shape(shape, n)


def _patterns(x, rng):
    """substrings of lengths 1-32, random patterns, the empty pattern and one pattern longer than the block"""
    n = x.size
    pats = []
    for m in range(1, 33):
        if m <= n:
            for q in rng.integers(0, n - m + 1, 2):
                pats.append(x[q:q + m].tobytes())
    for m in rng.integers(1, 12, 16):
        pats.append(rng.integers(0, 256, m, dtype=np.uint8).tobytes())
    pats.append(b"")
    pats.append(np.resize(x, n + 1).tobytes())
    return pats


def _within_budget(f, pats, rate, n):
    """the patterns, in order, whose walks stay inside WALK_BUDGET LF steps (at most min(S, n) per occurrence)"""
    lo, hi = f.count(pats)
    out, used = [], 0
    for p, a, b in zip(pats, lo, hi):
        cost = int(b - a) * min(rate, n)
        if used + cost <= WALK_BUDGET:
            out.append(p)
            used += cost
    return out


def _budget_bytes(n, rate):
    return 8 * ((n + rate - 1) // rate) + n / 8 + n / 64 + 4096


def _check_samples(archon, f, exp, route, rate, n):
    got = f.samples()
    st = archon.fm_walk_stats()
    assert st.route == route and st.rate == rate and st.n == n
    assert st.samples == exp.size
    assert st.sample_bytes <= _budget_bytes(n, rate)
    assert got.dtype == np.uint32 and (got == exp).all()


def _check_locate(archon, f, b, sa, pats, rate):
    n = sa.size
    want = b.fm_locate(pats)
    lo, hi = b.fm_count(pats)
    got = f.locate(pats)
    assert len(got) == len(want)
    for p, g, w in zip(pats, got, want):
        assert g.dtype == np.uint32 and (g == w).all(), p
    st = archon.fm_walk_stats()
    rows = np.concatenate([np.arange(a, z, dtype=np.int64) for a, z in zip(lo, hi)] + [np.zeros(0, np.int64)])
    steps = M.locate_steps(sa, rows, rate)
    assert st.walks == rows.size
    assert st.lf_steps == int(steps.sum())
    assert st.max_walk == (int(steps.max()) if rows.size else 0)
    assert st.max_walk <= (rate - 1 if rate <= n else n - 1)


def _requests(n, rng):
    """random requests, length 0 (also at n), the last byte and the whole text"""
    starts, lengths = [], []
    for _ in range(24):
        a = int(rng.integers(0, n + 1))
        starts.append(a)
        lengths.append(int(rng.integers(0, min(n - a, 300) + 1)))
    starts += [0, n, n - 1, 0]
    lengths += [0, 0, 1, n]
    return starts, lengths


def _check_extract(archon, f, x, rate, rng):
    import torch
    n = x.size
    starts, lengths = _requests(n, rng)
    got = f.extract(starts, lengths)
    for a, L, g in zip(starts, lengths, got):
        assert g.tobytes() == x[a:a + L].tobytes(), (a, L)
    st = archon.fm_walk_stats()
    assert st.lf_steps == M.extract_steps(starts, lengths, rate)
    assert st.max_walk <= rate - 1
    # the device form, output at offsets that start past 0
    off = np.concatenate([[5], 5 + np.cumsum(lengths)]).astype(np.int32)
    starts_t = torch.tensor(np.array(starts, np.int32), device="cuda:0")
    off_t = torch.tensor(off, device="cuda:0")
    out_t = torch.full((int(off[-1]) + 7,), 0xEE, dtype=torch.uint8, device="cuda:0")
    f.extract_dev(starts_t, off_t, out_t)
    torch.cuda.synchronize()
    out = out_t.cpu().numpy()
    assert (out[:5] == 0xEE).all() and (out[int(off[-1]):] == 0xEE).all()
    for j, (a, L) in enumerate(zip(starts, lengths)):
        assert out[off[j]:off[j + 1]].tobytes() == x[a:a + L].tobytes(), (a, L)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_samples_locate_extract(archon, oracle, monkeypatch, shape, n):
    """every shape and size at every rate: samples from the BWT alone, from the block's SA and by the forced walk route all
    equal the oracle's inverse SA at the items kS; locate equals the block's locate; extract equals x"""
    x = _shape(shape, n)
    P, B, b0 = oracle.forward(x)
    rng = np.random.default_rng(n * 7 + len(shape))
    b = archon.Block()
    try:
        sa, base = b.forward(x)
        assert base == b0 and (sa == P).all()
        bwt = b.read_bwt()
        pats = _patterns(x, rng)
        for rate in RATES:
            exp = M.expected_isa(P, base, rate)
            f1 = archon.FmIndex(bwt, base).sample(rate)
            _check_samples(archon, f1, exp, 2, rate, n)
            f2 = b.fm_index(rate)
            _check_samples(archon, f2, exp, 1, rate, n)
            monkeypatch.setenv("ARCHON_FM_SAMPLE_WALK", "1")
            f3 = b.fm_index(rate)
            monkeypatch.delenv("ARCHON_FM_SAMPLE_WALK")
            _check_samples(archon, f3, exp, 2, rate, n)
            f3.close()
            some = _within_budget(f2, pats, rate, n)
            _check_locate(archon, f2, b, P, some, rate)
            _check_locate(archon, f1, b, P, some, rate)
            _check_extract(archon, f1, x, rate, rng)
            f1.close()
            f2.close()
    finally:
        b.close()


@pytest.mark.parametrize("routes", [{"INV_SBITS": "3"}, {"FM_SUB_ROWS": "16"}, {"INV_SBITS": "4", "FM_SUB_ROWS": "16", "FM_SUPER_ROWS": "64"}])
@pytest.mark.parametrize("shape,n", [("text", 65), ("dna", 4099), ("ab", 4099), ("text", MiB), ("random", MiB)])
def test_routes(archon, oracle, monkeypatch, routes, shape, n):
    """small chains of the walk route and small rank-table pieces change no sample, start or byte"""
    for k, v in routes.items():
        monkeypatch.setenv("ARCHON_" + k, v)
    x = _shape(shape, n)
    P, B, b0 = oracle.forward(x)
    rng = np.random.default_rng(n + 11)
    b = archon.Block()
    try:
        sa, base = b.forward(x)
        pats = _patterns(x, rng)
        for rate in (1, 32, 1024):
            exp = M.expected_isa(P, base, rate)
            f1 = archon.FmIndex(B, b0).sample(rate)
            _check_samples(archon, f1, exp, 2, rate, n)
            f2 = b.fm_index(rate)
            _check_samples(archon, f2, exp, 1, rate, n)
            _check_locate(archon, f1, b, P, _within_budget(f1, pats, rate, n), rate)
            _check_extract(archon, f2, x, rate, rng)
            f1.close()
            f2.close()
    finally:
        b.close()


def test_block_without_sa_takes_the_walk(archon, oracle):
    """a block forwarded without its SA samples by the walk, and its index locates without any SA"""
    x = _shape("text", 70000)
    P, B, b0 = oracle.forward(x)
    b = archon.Block()
    try:
        b.forward(x, want_sa=False)
        f = b.fm_index(32)
        _check_samples(archon, f, M.expected_isa(P, b0, 32), 2, 32, x.size)
        got = f.locate([x[100:108].tobytes()])
        assert sorted(got[0].tolist()) == sorted(int(P[r]) - 8 for r in range(P.size) if P[r] >= 8 and x[P[r] - 8:P[r]].tobytes() == x[100:108].tobytes())
    finally:
        b.close()


def test_lifetime(archon, oracle):
    """an index from Block.fm_index answers after the block forwards another text and after the block is closed"""
    x = _shape("text", 100000)
    y = _shape("dna", 50000)
    b = archon.Block()
    sa, base = b.forward(x)
    pats = [x[q:q + 6].tobytes() for q in (0, 17, 5000, 99990)]
    want = b.fm_locate(pats)
    f = b.fm_index(32)
    b.forward(y)
    for g, w in zip(f.locate(pats), want):
        assert (g == w).all()
    assert f.extract([123], [77])[0].tobytes() == x[123:200].tobytes()
    b.close()
    for g, w in zip(f.locate(pats), want):
        assert (g == w).all()
    assert f.extract([0, 99999], [100000, 1])[0].tobytes() == x.tobytes()
    f.close()


def test_limits_and_bad_input(archon, oracle):
    """a short cap, an unsampled handle, bad rates, out-of-range and decreasing requests in both forms, read_samples' cap"""
    import ctypes
    import torch
    L = archon.lib()
    E = archon.E_ARG
    x = _shape("text", 5000)
    P, B, b0 = oracle.forward(x)
    f = archon.FmIndex(B, b0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    pat = np.frombuffer(b"e", np.uint8).copy()
    off = np.array([0, 1], np.uint32)
    pos = np.zeros(8, np.uint32)
    total = ctypes.c_uint64(0)
    starts, roff, out = np.array([0], np.uint32), np.array([0, 4], np.uint32), np.zeros(8, np.uint8)
    # no samples yet: count works, locate / extract / read_samples refuse
    assert f.count([b"e"])[1][0] > 0
    assert L.archon_hip_fm_locate(f.h, p(pat), p(off), 1, p(pos), 8, ctypes.byref(total)) == E
    assert L.archon_hip_fm_extract(f.h, p(starts), p(roff), 1, p(out)) == E
    cnt = ctypes.c_uint32(0)
    assert L.archon_hip_fm_read_samples(f.h, p(pos), 8, ctypes.byref(cnt)) == E
    for rate in (0, 3, 48, 131072):
        assert L.archon_hip_fm_sample(f.h, rate) == E
    f.sample(64)
    # read_samples with a short cap sets the count
    assert L.archon_hip_fm_read_samples(f.h, p(pos), 8, ctypes.byref(cnt)) == E and cnt.value == (5000 + 63) // 64
    # locate with a short cap reports the total
    lo, hi = f.count([b"e"])
    want = int(hi[0] - lo[0])
    pos = np.zeros(want, np.uint32)
    assert L.archon_hip_fm_locate(f.h, p(pat), p(off), 1, p(pos), want - 1, ctypes.byref(total)) == E
    assert total.value == want
    assert L.archon_hip_fm_locate(f.h, p(pat), p(off), 1, p(pos), want, ctypes.byref(total)) == 0
    # requests out of range or with decreasing offsets: refused, nothing written
    for st, ro in (([4997], [0, 4]), ([5001], [0, 0]), ([0, 0], [0, 4, 2])):
        st, ro = np.array(st, np.uint32), np.array(ro, np.uint32)
        out[:] = 0xAB
        assert L.archon_hip_fm_extract(f.h, p(st), p(ro), st.size, p(out)) == E
        assert (out == 0xAB).all()
        st_t, ro_t = torch.tensor(st.astype(np.int64), device="cuda:0").int(), torch.tensor(ro.astype(np.int64), device="cuda:0").int()
        out_t = torch.full((8,), 0xAB, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(archon.ArchonError) as e:
            f.extract_dev(st_t, ro_t, out_t)
        assert e.value.code == E
        assert (out_t.cpu().numpy() == 0xAB).all()
    # the edge that is allowed: a request ending at n, and one of length 0 at n
    assert f.extract([4996, 5000], [4, 0])[0].tobytes() == x[4996:].tobytes()
    # k = 0 writes nothing
    assert L.archon_hip_fm_extract(f.h, p(starts), p(roff), 0, p(out)) == 0
    # a second sample replaces the first
    f.sample(2)
    assert (f.samples() == M.expected_isa(P, b0, 2)).all()
    f.close()


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text at 1 MiB, rate 32: locate through an index sampled from the BWT
    alone and through the block's (some eighty patterns and thousands of rows, so every wave walks row after row) with the
    exact LF steps, extract of 28 requests -- the whole text among them, 32 768 segments -- in both forms; byte-equal to the
    same calls without the route, with their counters"""
    n, rate = MiB, 32
    x = _shape("text", n)
    P, B, b0 = oracle.forward(x)
    b = archon.Block()
    try:
        sa, base = b.forward(x)
        assert base == b0 and (sa == P).all()
        f1 = archon.FmIndex(b.read_bwt(), base).sample(rate)
        f2 = b.fm_index(rate)
        b.fm_count([b"a"])                   # (the block's table built before the calls that are compared)
        some = _within_budget(f2, _patterns(x, np.random.default_rng(n + 5)), rate, n)
        assert len(some) > 40

        def call():
            out, stats = [], []
            for f in (f1, f2):
                _check_locate(archon, f, b, P, some, rate)
                stats.append(archon.fm_walk_stats())
                out += list(f.locate(some))
                _check_extract(archon, f, x, rate, np.random.default_rng(n + 6))
                stats.append(archon.fm_walk_stats())
                starts, lengths = _requests(n, np.random.default_rng(n + 6))
                out += list(f.extract(starts, lengths))
            return out, stats
        G.same_under(monkeypatch, grid, call)
        f1.close()
        f2.close()
    finally:
        b.close()
