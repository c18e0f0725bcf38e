"""GPU: the longest previous factors and the LZ77 parse of a block (archon_hip_lpf, lpf_dev, lz_parse, lz_parse_dev, block_lz;
include/archon_hip.h) against two stacks and a plain walk on the CPU (tests/lz_naive.c, pinned to the text by test_lz_abi.py):
content and order, the counters against numpy, the work bounds of the header, the cap rule, and bad input."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import lz_naive as Z
import stride_util as G

pytestmark = pytest.mark.gpu

MiB = 1 << 20
DEFAULT_FAN = 16                # lz.hiph kDefaultFan
DEFAULT_TILE = 256              # lz.hiph kDefaultTile


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return Z.build(tmp_path_factory.mktemp("lz_naive"))


@pytest.fixture(scope="module")
def tiny():
    """every string of length 1-7 over {0, 1, 255}: (sa, lcp) by the definition"""
    out = []
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            sa, lcp = Z.a7_arrays(bytes(t))
            out.append((np.array(sa, np.uint32), np.array(lcp, np.uint32)))
    return out


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _odd(t, by=1):
    """the same values `by` elements past an allocation's start"""
    import torch
    buf = torch.empty(t.numel() + by, dtype=t.dtype, device=t.device)
    buf[by:] = t
    return buf[by:]


def _parse_once(archon, rec):
    """archon_hip_lz_parse with room for n phrases: count and emit in one call"""
    out = np.zeros(rec.size, archon.PHRASE)
    total = ctypes.c_uint64(0)
    archon._check(archon.lib().archon_hip_lz_parse(archon._p(rec), rec.size, archon._p(out), out.size, ctypes.cast(ctypes.byref(total), ctypes.c_void_p), 0))
    return out[:total.value]


def _levels(n, base):
    k, c = 0, 1
    while c < n:
        c *= base
        k += 1
    return k


def _probe_bound(n, fan):
    """the header's bound on probes: 2 (2 F - 1) L n, L = ceil(log_F n)"""
    return 2 * (2 * fan - 1) * _levels(n, fan) * n


def _hop_bound(n, tile):
    """the header's bound on hops: ceil(n / T^(K-1)) + (K - 1) T, K = the least with T^K >= n (at least 1)"""
    K = max(_levels(n, tile), 1)
    top = tile ** (K - 1)
    return (n + top - 1) // top + (K - 1) * tile, K


def _check_parse_stats(st, n, phrases, tile):
    bound, K = _hop_bound(n, tile)
    assert (st.n, st.tile, st.parse_levels) == (n, tile, K)
    assert st.phrases == phrases.size and st.literals == int((phrases["len"] == 0).sum()) and st.longest == int(phrases["len"].max())
    assert 1 <= st.hops <= bound <= K * tile, (st.hops, bound)


@pytest.mark.parametrize("dir", [0, 1])
@pytest.mark.parametrize("fan,tile", [(2, 2), (0, 0), (2, 0), (0, 2)])
def test_exhaustive_tiny(archon, naive, tiny, fan, tile, dir, monkeypatch):
    """every string of length 1-7 over {0, 1, 255} through lpf, lpf_dev, lz_parse and lz_parse_dev (every other one at odd
    device addresses), with a fan-out of 2 or the default and a tile of 2 or the default (at 2 seven rows cross three levels),
    in all four combinations: the helper's records in the helper's order, nothing stored past them"""
    import torch
    if fan:
        monkeypatch.setenv("ARCHON_LZ_FAN", str(fan))
    if tile:
        monkeypatch.setenv("ARCHON_LZ_TILE", str(tile))
    for i, (sa, lcp) in enumerate(tiny):
        n = sa.size
        want = naive.lpf(sa, lcp, dir)
        phrases = naive.parse(want)
        got = archon.lpf(sa, lcp, dir)
        assert got.tolist() == want.tolist(), (sa, lcp)
        st = archon.lz_stats()
        assert (st.n, st.dir, st.fan, st.levels) == (n, dir, fan or DEFAULT_FAN, _levels(n, fan or DEFAULT_FAN))
        assert st.probes <= _probe_bound(n, fan or DEFAULT_FAN)
        assert _parse_once(archon, want).tolist() == phrases.tolist()
        _check_parse_stats(archon.lz_stats(), n, phrases, tile or DEFAULT_TILE)
        if tile == 2 and n == 7:
            assert archon.lz_stats().parse_levels == 3
        sa_t, lcp_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32))
        rec_t = torch.full((2 * n + 2,), -1, dtype=torch.int32, device="cuda:0")
        out_t = torch.full((3 * n + 1,), -1, dtype=torch.int32, device="cuda:0")
        if i % 2:
            sa_t, lcp_t = _odd(sa_t), _odd(lcp_t)
        archon.lpf_dev(sa_t, lcp_t, dir, rec_t[:2 * n])
        rec = rec_t.cpu().numpy().view(np.uint32)
        assert rec[:2 * n].view(archon.LPF).tolist() == want.tolist() and (rec[2 * n:] == 0xFFFFFFFF).all()
        lpf_t = _odd(rec_t[:2 * n]) if i % 2 else rec_t[:2 * n]         # (the parse reads records at any 4-byte address)
        total = archon.lz_parse_dev(lpf_t, out_t=out_t[1:])
        got = out_t[1:].cpu().numpy().view(np.uint32)
        assert total == phrases.size and (got[3 * total:] == 0xFFFFFFFF).all() and int(out_t[0]) == -1
        assert got[:3 * total].view(archon.PHRASE).tolist() == phrases.tolist(), (sa, lcp)


def _block_lz(archon, naive, x, dirs=(0, 1), tile=DEFAULT_TILE, fan=DEFAULT_FAN, keep=None):
    """x through Block.lz in the given directions against the helper; returns {dir: phrases} (keep: a list that takes the
    records, the phrases and the stats records of every call)"""
    n = x.size
    blk = archon.Block()
    sa, _ = blk.forward(x, want_sa=True)
    lcp = blk.lcp()
    out = {}
    for d in dirs:
        want = naive.lpf(sa, lcp, d)
        phrases = naive.parse(want)
        rec, got = blk.lz(d, want_lpf=True)
        st = archon.lz_stats()
        assert (rec == want).all(), d
        assert got.size == phrases.size and (got == phrases).all(), d
        assert int(np.maximum(got["len"], 1).astype(np.int64).sum()) == n
        assert (st.dir, st.fan, st.levels) == (d, fan, _levels(n, fan)) and st.probes <= _probe_bound(n, fan)
        _check_parse_stats(st, n, phrases, tile)
        assert st.ms_lcp > 0 and st.ms_lpf > 0 and st.ms_parse > 0 and st.ms_emit > 0
        assert blk.lz(d, count_only=True) == phrases.size and archon.lz_stats().ms_emit == 0
        out[d] = got
        if keep is not None:
            keep += [rec, got, st, archon.lz_stats()]
    blk.close()
    return out, sa


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65536, MiB + 3])
def test_shapes(archon, naive, shape, n, monkeypatch):
    """every synthetic shape through Block.lz in both directions: records and phrases equal the helper's, the phrase lengths
    sum to n, the counters equal numpy on the helper's output, probes and hops stay within the header's bounds; at 65536 once
    more with a tile of 16 (four parse levels) and a fan-out of 4"""
    x = S.gen_shape(shape, n)
    _block_lz(archon, naive, x)
    if n == 65536:
        monkeypatch.setenv("ARCHON_LZ_TILE", "16")
        monkeypatch.setenv("ARCHON_LZ_FAN", "4")
        _block_lz(archon, naive, x, tile=16, fan=4)
        assert archon.lz_stats().parse_levels == 4 and archon.lz_stats().levels == 8


def fibonacci(n):
    a, b = b"a", b"b"
    while len(a) < n:
        a, b = a + b, a
    return np.frombuffer(a[:n], np.uint8).copy()


def _check_long_copy(phrases, n):
    """the dir-0 parse of archon_synth.gen_random_copy, whose bytes [h, h + L) repeat [0, L) (h = n // 2, L = n // 8).  Every
    item e in (h, h + L] has the earlier item e - h with e - h equal bytes before both, so len(e) >= e - h.  The chain comes
    down from n through random bytes and need not stop at h + L itself: its first phrase end e <= h + L lies one step below
    an end e' > h + L, so e >= h + L + 1 - step(e'), and the phrase there has len >= e - h >= L + 1 - step(e').  step(e') is
    a repeat that holds a random byte past the copy: among n < 2^21 random positions a repeat of 8 bytes has a chance below
    2^42 / 2^64, so step(e') <= 8 for the fixed seed, and the copy comes out as one phrase of at least L - 7"""
    h, L = n // 2, n // 8
    i = int(np.argmax(phrases["end"] <= h + L))         # (ends descend: the first end inside or below the copy)
    assert i > 0
    e, step = int(phrases["end"][i]), max(int(phrases["len"][i - 1]), 1)
    assert step <= 8 and e == int(phrases["end"][i - 1]) - step and e >= h + L + 1 - step
    assert int(phrases["len"][i]) >= e - h >= L + 1 - step


@pytest.mark.parametrize("n", [65536, MiB + 3])
@pytest.mark.parametrize("kind", ["one_byte", "period2", "period1000", "fibonacci", "long_copy"])
def test_adversarial_blocks(archon, naive, kind, n):
    """chains at both ends of the scale: one phrase of n - 1 (sa descending, every dir-0 left search runs to row 0), periods,
    a Fibonacci word, a random block with a long copy"""
    x = {"one_byte": lambda: S.gen_shape("a", n), "period2": lambda: S.gen_shape("ab", n), "period1000": lambda: S.gen_shape("motif", n),
         "fibonacci": lambda: fibonacci(n), "long_copy": lambda: S.gen_shape("random_copy", n)}[kind]()
    got, sa = _block_lz(archon, naive, x)
    if kind == "one_byte":
        assert (sa == np.arange(n, 0, -1)).all()
        assert got[0].tolist() == [(n, n - 1, n - 1), (1, 0, 0)]
        assert got[1].tolist() == [(n, 0, 0), (n - 1, n - 1, n)]    # item n has no later item; the run before it ends again at n
    if kind == "period2":
        assert got[0].tolist() == [(n, n - 2, n - 2), (2, 0, 0), (1, 0, 0)]
    if kind == "long_copy":
        _check_long_copy(got[0], n)


def test_all_literals(archon, naive):
    """blocks without a repeat: 256 distinct bytes through Block.lz, and 65536 zero len words straight into lz_parse"""
    x = np.random.default_rng(5).permutation(256).astype(np.uint8)
    got, _ = _block_lz(archon, naive, x)
    for d in (0, 1):
        assert got[d].tolist() == [(e, 0, 0) for e in range(256, 0, -1)]
    n = 65536
    rec = np.zeros(n, archon.LPF)
    rec["src"] = 7
    got = archon.lz_parse(rec)
    assert (got["end"] == np.arange(n, 0, -1)).all() and not got["len"].any() and (got["src"] == 7).all()
    st = archon.lz_stats()
    assert st.phrases == st.literals == n and st.longest == 0 and st.hops <= _hop_bound(n, DEFAULT_TILE)[0]


@pytest.mark.parametrize("n", [65536, MiB + 3])
def test_every_item_on_the_chain(archon, naive, n):
    """len words of all ones: every item is a phrase end, every walk of the descent takes all its steps"""
    rec = np.ones(n, archon.LPF)
    got = archon.lz_parse(rec)
    assert (got == naive.parse(rec)).all() and got.size == n
    st = archon.lz_stats()
    bound, K = _hop_bound(n, DEFAULT_TILE)
    assert st.literals == 0 and st.longest == 1 and st.hops == bound and st.parse_levels == K


def _lz77_quadratic(z):
    """the textbook greedy LZ77 of z by comparing with every earlier start: (pos, len) pairs"""
    n, i, out = z.size, 0, []
    while i < n:
        cand, m = np.arange(i), 0
        while cand.size and i + m < n:
            cand = cand[z[cand + m] == z[i + m]]
            m += cand.size > 0
        out.append((i, int(m)))
        i += max(int(m), 1)
    return out


def _decode(phrases, z):
    """the text of (pos, len, src) phrases, literals taken from z"""
    out = np.zeros(z.size, np.uint8)
    for pos, m, src in phrases.tolist():
        if m == 0:
            out[pos] = z[pos]
        elif src + m <= pos:
            out[pos:pos + m] = out[src:src + m]
        else:                               # the copy overlaps what it writes: it repeats the pos - src bytes before pos
            out[pos:pos + m] = np.resize(out[src:pos], m)
    return out


@pytest.mark.parametrize("shape", ["text", "dna"])
def test_lz77_round_trip(archon, shape):
    """lz77(z): decoding the phrases on the CPU reproduces z (1 MiB); on 3000 bytes positions and lengths equal a quadratic
    CPU LZ77"""
    z = S.gen_shape(shape, MiB)
    ph = archon.lz77(z)
    assert ph["pos"][0] == 0 and (ph["pos"][1:] == ph["pos"][:-1] + np.maximum(ph["len"][:-1], 1)).all()
    assert int(ph["pos"][-1]) + max(int(ph["len"][-1]), 1) == z.size
    assert ((ph["src"] < ph["pos"]) | (ph["len"] == 0)).all()
    assert (_decode(ph, z) == z).all()
    small = z[:3000]
    ph = archon.lz77(small)
    assert list(zip(ph["pos"].tolist(), ph["len"].tolist())) == _lz77_quadratic(small)
    assert (_decode(ph, small) == small).all()


@pytest.fixture(scope="module")
def dna(archon):
    """dna at 65536: (x, sa, lcp)"""
    x = S.gen_shape("dna", 65536)
    sa, _, _ = archon.forward(x)
    return x, sa, archon.lcp(x, sa)


def test_cap_rule(archon, naive, dna):
    _, sa, lcp = dna
    L = archon.lib()
    rec = naive.lpf(sa, lcp, 0)
    want = naive.parse(rec)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    assert L.archon_hip_lz_parse(archon._p(rec), rec.size, None, 0, tp, 0) == 0
    assert total.value == want.size > 1
    out = np.zeros(want.size, archon.PHRASE)
    out.view(np.uint32)[:] = 0xABABABAB
    untouched = out.copy()
    total.value = 0
    assert L.archon_hip_lz_parse(archon._p(rec), rec.size, archon._p(out), want.size - 1, tp, 0) == archon.E_ARG
    assert total.value == want.size and (out == untouched).all()
    assert L.archon_hip_lz_parse(archon._p(rec), rec.size, archon._p(out), want.size, tp, 0) == 0
    assert total.value == want.size and (out == want).all()
    # the device form: the same rule, nothing stored past the phrases
    import torch
    rec_t = _cuda(rec.view(np.uint32).view(np.int32))
    out_t = torch.full((3 * want.size,), -1, dtype=torch.int32, device="cuda:0")
    assert archon.lz_parse_dev(rec_t) == want.size
    with pytest.raises(archon.ArchonError) as e:
        archon.lz_parse_dev(rec_t, out_t=out_t[:3 * (want.size - 1)])
    assert e.value.code == archon.E_ARG and (out_t == -1).all()
    assert archon.lz_parse_dev(rec_t, out_t=out_t) == want.size
    assert (out_t.cpu().numpy().view(np.uint32).view(archon.PHRASE) == want).all()
    # the block form
    x = dna[0]
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    total.value = 0
    assert L.archon_hip_block_lz(blk.h, 0, None, archon._p(out), want.size - 1, tp) == archon.E_ARG
    assert total.value == want.size
    blk.close()
    # one item: one literal
    one = archon.lpf(np.array([1], np.uint32), np.array([9], np.uint32))
    assert one.tolist() == [(0, 0)] and archon.lz_parse(one).tolist() == [(1, 0, 0)]
    st = archon.lz_stats()
    assert st.parse_levels == 1 and st.hops == 1 and st.phrases == st.literals == 1


def test_arrays_of_nothing(archon, naive, dna):
    """a garbage lcp with a true sa, and a random permutation as sa: ARCHON_OK, the rule is a rule about the arrays, so the
    helper says what comes out"""
    _, sa, lcp = dna
    n = sa.size
    rng = np.random.default_rng(11)
    garbage = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    perm = (rng.permutation(n) + 1).astype(np.uint32)
    for s, l in ((sa, garbage), (perm, lcp), (perm, garbage)):
        for d in (0, 1):
            got = archon.lpf(s, l, d)
            assert (got == naive.lpf(s, l, d)).all()
            assert archon.lz_stats().probes <= _probe_bound(n, DEFAULT_FAN)
            assert (got["src"] <= n).all()


@pytest.mark.parametrize("bad", [0, "n+1", 0xFFFFFFFF])
def test_sa_out_of_range(archon, dna, bad):
    """an sa holding 0, n + 1 or 2^32 - 1 is ARCHON_E_CORRUPT and leaves the output untouched, host and device form; so is
    the one-row block"""
    import torch
    _, sa, lcp = dna
    n = sa.size
    broken = sa.copy()
    broken[n // 3] = n + 1 if bad == "n+1" else bad
    out = np.zeros(n, archon.LPF)
    out.view(np.uint32)[:] = 0xABABABAB
    for d in (0, 1):
        assert archon.lib().archon_hip_lpf(archon._p(broken), archon._p(lcp), n, d, archon._p(out), 0) == archon.E_CORRUPT
        assert (out.view(np.uint32) == 0xABABABAB).all()
        rec_t = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda:0")
        with pytest.raises(archon.ArchonError) as e:
            archon.lpf_dev(_cuda(broken.view(np.int32)), _cuda(lcp.view(np.int32)), d, rec_t)
        assert e.value.code == archon.E_CORRUPT and (rec_t == -1).all()
    one = np.array([broken[n // 3]], np.uint32)
    assert archon.lib().archon_hip_lpf(archon._p(one), archon._p(one), 1, 0, archon._p(out), 0) == archon.E_CORRUPT
    assert (out.view(np.uint32) == 0xABABABAB).all()


@pytest.mark.parametrize("tile", [0, 2, 16, 4096])
def test_garbage_len_words(archon, naive, tile, monkeypatch):
    """random len words, most of them above e: the parse stays a rule about the array, at most n phrases"""
    if tile:
        monkeypatch.setenv("ARCHON_LZ_TILE", str(tile))
    rng = np.random.default_rng(13)
    n = 70001
    rec = np.zeros(n, archon.LPF)
    rec["src"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for top in (1 << 32, 2 * n, 40, 3):
        rec["len"] = rng.integers(0, top, n, dtype=np.uint64).astype(np.uint32)
        got = archon.lz_parse(rec)
        want = naive.parse(rec)
        assert got.size == want.size <= n and (got == want).all()
        _check_parse_stats(archon.lz_stats(), n, want, tile or DEFAULT_TILE)


def test_statistics_stay_apart(archon, naive, dna):
    x, sa, lcp = dna
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    blk.fm_count([b"ACGT"])
    archon.lcp(x, sa)
    archon.repeats(lcp, blk.read_bwt(), 0, kind=0, count_only=True)
    before = (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.repeat_stats()), bytes(archon.stats_raw()))
    rec = archon.lpf(sa, lcp, 1)
    st = archon.lz_stats()
    assert st.ms_lcp == 0 and st.ms_lpf > 0 and st.ms_parse == 0 and st.kernel_launches == 2 * st.levels + 1 and st.host_syncs == 2
    assert (st.tile, st.parse_levels, st.phrases, st.hops) == (0, 0, 0, 0)
    archon.lz_parse(rec, count_only=True)
    st = archon.lz_stats()
    assert st.ms_lpf == 0 and st.ms_parse > 0 and st.ms_emit == 0 and st.host_syncs == 1 and (st.fan, st.levels, st.probes) == (0, 0, 0)
    assert st.kernel_launches == 4 and st.parse_levels == 2         # F_1, the top walk, one level of the descent, the count
    assert before == (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.repeat_stats()), bytes(archon.stats_raw()))
    blk.lz()
    assert archon.lcp_stats().n == x.size
    assert before[1:] == (bytes(archon.fm_stats()), bytes(archon.repeat_stats()), bytes(archon.stats_raw()))
    blk.forward(x, want_sa=False)
    with pytest.raises(archon.ArchonError) as e:
        blk.lz()
    assert e.value.code == archon.E_ARG
    blk.close()


def test_two_contexts_concurrently(archon):
    blocks = [S.gen_shape("text", MiB + 1), S.gen_shape("motif_defects", MiB + 5)]
    solo = []
    for x in blocks:
        blk = archon.Block()
        blk.forward(x, want_sa=True)
        solo.append(blk.lz(0, want_lpf=True))
        blk.close()
    assert solo[0][1].size != solo[1][1].size
    got, stats, errors = [None, None], [None, None], []

    def run(k):
        try:
            archon.bind_context(k)
            blk = archon.Block()
            blk.forward(blocks[k], want_sa=True)
            for _ in range(3):
                got[k] = blk.lz(0, want_lpf=True)
                stats[k] = archon.lz_stats()
                assert (got[k][0] == solo[k][0]).all() and (got[k][1] == solo[k][1]).all()
            blk.close()
        except Exception as ex:          # noqa: BLE001 -- reported below
            errors.append(ex)

    threads = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in (0, 1):
        assert (got[k][1] == solo[k][1]).all()
        assert stats[k].n == blocks[k].size and stats[k].phrases == solo[k][1].size


def _decode_ends(phrases, x):
    """the text of (end, len, src) phrases of direction 0 in chain order (ends descending), literals taken from x: the len
    bytes before item end are the len bytes before the earlier item src"""
    out = np.zeros(x.size, np.uint8)
    for e, m, s in phrases[::-1].tolist():
        if m == 0:
            out[e - 1] = x[e - 1]
        elif s <= e - m:
            out[e - m:e] = out[s - m:s]
        else:                               # the copy overlaps what it writes: it repeats the e - s bytes before e - m
            out[e - m:e] = np.resize(out[s - m:e - m], m)
    return out


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, naive, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text and a random block with a long copy at 65 536 + 3 (33 tiles of
    the LPF pass, the last of 3 rows; 257 tiles of the parse): the LPF records in both directions, the parse counted and
    emitted through Block.lz against the helper, and lpf / lz_parse on host arrays, byte-equal to the same calls without the
    route, with their counters, launches and host waits"""
    for shape in ("text", "random_copy"):
        x = S.gen_shape(shape, 65536 + 3)

        def call():
            keep = []
            _, sa = _block_lz(archon, naive, x, keep=keep)
            rec = archon.lpf(sa, archon.lcp(x, sa), 1)
            keep += [rec, archon.lz_stats(), _parse_once(archon, rec), archon.lz_stats()]
            return [v for v in keep if isinstance(v, np.ndarray)], [v for v in keep if not isinstance(v, np.ndarray)]
        G.same_under(monkeypatch, grid, call)


@pytest.mark.parametrize("shape", ["a", "dna"])
def test_second_trip_at_the_product_grid(archon, naive, shape):
    """no route: 2048 * 2048 + 3 * 2048 + 5 rows are 2052 tiles of the LPF pass, so workgroups 0-3 of the 2048 take a second
    tile and the last tile has 5 rows (the parse's tiles of 256 items go round eight times).  One byte: two phrases.  DNA: the
    LPF records and the phrases against the helper, and decoding the phrases gives the block back"""
    n = G.N2
    x = S.gen_shape(shape, n)
    blk = archon.Block()
    try:
        sa, _ = blk.forward(x, want_sa=True)
        assert blk.validate() == 1
        rec, got = blk.lz(0, want_lpf=True)
        st = archon.lz_stats()
        if shape == "a":
            assert got.tolist() == [(n, n - 1, n - 1), (1, 0, 0)]
            assert (rec["len"] == np.arange(n)).all()
            assert blk.lz(1).tolist() == [(n, 0, 0), (n - 1, n - 1, n)]
        else:
            want = naive.lpf(sa, blk.lcp(), 0)
            phrases = naive.parse(want)
            assert (rec == want).all() and got.size == phrases.size and (got == phrases).all()
            assert (_decode_ends(got, x) == x).all()
            assert blk.lz(0, count_only=True) == phrases.size
        _check_parse_stats(st, n, got, DEFAULT_TILE)
        assert st.probes <= _probe_bound(n, DEFAULT_FAN)
    finally:
        blk.close()
