"""GPU: the minimal absent words of a block (archon_hip_maws*, archon_hip_block_maws; include/archon_hip.h) against the rule
over the arrays in plain Python (tests/maw_naive.model, pinned to the definition by test_maw_abi.py): record by record and counter
by counter through the host, device and block forms, at every size edge of the pass, of the direct/table threshold and of the
rank table; filters, the cap rule, bad input, determinism and the statistics.

`probes` depends on the fan-out as well as on the input; it is held to its bound -- every search reads at most 2F - 1 entries
per level, one left search per row, one right search per node and per child -- and to equality between the forms."""
import ctypes
import os

import numpy as np
import pytest

import archon_synth as S
import maw_naive as M
import repeats_naive as R
import stride_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_FAN = 16
DIRECT_ROWS = 64                # maw.hiph kDirectRows
TILE = 256                      # maw.hiph kTile: rows of a wave's tile
COUNTERS = ("intervals", "nodes", "children", "sets_direct", "sets_table", "words", "shortest", "longest", "absent_bytes")
_cases, _models = {}, {}


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")       # (a copy: the cases are read-only)


def _odd(t):
    """the same values one element past an allocation's start"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def _tp(total):
    return ctypes.cast(ctypes.byref(total), ctypes.c_void_p)


def _text(name):
    kind, _, arg = name.partition(":")
    if kind == "lit":
        return np.frombuffer(arg.encode("latin-1"), np.uint8)
    if kind == "rand":                      # rand:<letters>:<n>
        sigma, n = (int(v) for v in arg.split(":"))
        return (np.random.default_rng(1000 * sigma + n).integers(0, sigma, n).astype(np.uint8) + 97)
    if kind == "same":
        return np.full(int(arg), ord("c"), np.uint8)
    if kind == "fixed257":                  # the fixed byte first, then every byte followed by it: its node has INF and 256 bytes before it
        return np.concatenate(([7], np.stack((np.arange(256), np.full(256, 7)), 1).ravel())).astype(np.uint8)
    if kind == "perm256":                   # every byte once: the root has 256 children of one row, 255 words each
        return np.random.default_rng(256).permutation(256).astype(np.uint8)
    if kind == "lasttile":                  # 254 bytes that occur once, then 254 followed by one to three 255s, over and over
        rng = np.random.default_rng(7)
        tail = np.concatenate([[254] + [255] * int(k) for k in rng.integers(1, 4, 60)])
        return np.concatenate((np.arange(254), tail)).astype(np.uint8)
    if kind == "readme":
        return np.frombuffer(open(os.path.join(ROOT, "README.md"), "rb").read()[:int(arg)], np.uint8)
    if kind == "dna":
        return S.gen_dna(int(arg))
    raise KeyError(name)


def _case(archon, name):
    """(x, sa, lcp, bwt, base) of a named text, made once: by the definition up to 600 bytes, by the library above"""
    if name not in _cases:
        x = np.ascontiguousarray(_text(name))
        if x.size <= 600:
            sa, lcp, bwt, base = R.a7_arrays(x.tobytes())
            sa, lcp, bwt = np.array(sa, np.uint32), np.array(lcp, np.uint32), np.frombuffer(bwt, np.uint8).copy()
        else:
            sa, bwt, base = archon.forward(x)
            lcp = archon.lcp(x, sa)
        for a in (x, sa, lcp, bwt):
            a.setflags(write=False)
        _cases[name] = (x, sa, lcp, bwt, int(base))
    return _cases[name]


def _model(archon, name, min_len=2, max_len=0):
    key = (name, min_len, max_len)
    if key not in _models:
        _, sa, lcp, bwt, base = _case(archon, name)
        _models[key] = M.model(sa, lcp, bwt, base, min_len, max_len, DIRECT_ROWS)
    return _models[key]


def _levels(n, fan):
    levels, c = 0, 1
    while c < n:
        c *= fan
        levels += 1
    return levels


def _check_stats(st, n, c, min_len, max_len, fan, emitted, built=None):
    """the record of a call against the model's counters, the bound on probes, and the launches the header states"""
    got = {k: getattr(st, k) for k in COUNTERS}
    print("    n %d filter (%d, %d) fan %d: %s, probes %d, launches %d, waits %d" % (n, min_len, max_len, fan, got, st.probes, st.kernel_launches, st.host_syncs))
    assert got == {k: c[k] for k in COUNTERS}
    levels = _levels(n, fan)
    assert (st.n, st.min_len, st.max_len, st.fan, st.levels, st.direct_rows) == (n, min_len, max_len, fan, levels, DIRECT_ROWS)
    assert st.probes <= (2 * fan - 1) * max(levels, 1) * (n - 1 + c["nodes"] + c["children"])
    assert c["children"] <= 2 * n
    if built is not None:
        assert st.built == built
        assert st.kernel_launches == 1 + levels + 3 + 1 + (2 if emitted else 0) + (3 if built else 0)
    assert (st.ms_emit > 0) == bool(emitted) and st.ms_count > 0


def _host(archon, name, min_len=2, max_len=0, fan=DEFAULT_FAN):
    """archon_hip_maws: counting, then with room for exactly the words; sentinel words behind them"""
    _, sa, lcp, bwt, base = _case(archon, name)
    want, c = _model(archon, name, min_len, max_len)
    L, p, n = archon.lib(), archon._p, sa.size
    total = ctypes.c_uint64(77)
    archon._check(L.archon_hip_maws(p(sa), p(lcp), p(bwt), n, base, min_len, max_len, None, 0, _tp(total), 0))
    st = archon.maw_stats()
    assert total.value == want.size
    _check_stats(st, n, c, min_len, max_len, fan, False, built=1)
    assert st.host_syncs == 2                   # the table's, the count's
    probes = st.probes
    out = np.zeros(want.size + 1, archon.MAW)
    out.view(np.uint32)[:] = 0xA5A5A5A5
    archon._check(L.archon_hip_maws(p(sa), p(lcp), p(bwt), n, base, min_len, max_len, p(out), want.size, _tp(total), 0))
    assert total.value == want.size and out[:want.size].tolist() == want.tolist(), name
    assert (out[want.size:].view(np.uint32) == 0xA5A5A5A5).all()
    st = archon.maw_stats()
    _check_stats(st, n, c, min_len, max_len, fan, want.size > 0, built=1)
    assert st.host_syncs == 2 + (want.size > 0) and st.probes == probes
    return out[:want.size], st


def _dev(archon, name, min_len=2, max_len=0, fan=DEFAULT_FAN, odd=False):
    """archon_hip_maws_dev on torch tensors (odd: every array one element past an allocation's start)"""
    import torch
    _, sa, lcp, bwt, base = _case(archon, name)
    want, c = _model(archon, name, min_len, max_len)
    sa_t, lcp_t, bwt_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt)
    if odd:
        sa_t, lcp_t, bwt_t = _odd(sa_t), _odd(lcp_t), _odd(bwt_t)
    assert archon.maws_dev(sa_t, lcp_t, bwt_t, base, min_len, max_len) == want.size
    _check_stats(archon.maw_stats(), sa.size, c, min_len, max_len, fan, False, built=1)
    out_t = torch.full((5 * want.size + 2,), -1, dtype=torch.int32, device="cuda:0")
    assert archon.maws_dev(sa_t, lcp_t, bwt_t, base, min_len, max_len, out_t=out_t[1:5 * want.size + 1]) == want.size
    got = out_t.cpu().numpy().view(np.uint32)
    assert got[0] == got[-1] == 0xFFFFFFFF
    assert got[1:-1].view(archon.MAW).tolist() == want.tolist(), name
    st = archon.maw_stats()
    _check_stats(st, sa.size, c, min_len, max_len, fan, want.size > 0, built=1)
    return got[1:-1].view(archon.MAW), st


def _block(archon, name, min_len=2, max_len=0, fan=DEFAULT_FAN, fm_first=False):
    """Block.maws, counting and then emitting; fm_first: behind an FM call, so that the block's table is there already"""
    x, sa, _, _, base = _case(archon, name)
    want, c = _model(archon, name, min_len, max_len)
    blk = archon.Block()
    try:
        got_sa, got_base = blk.forward(x, want_sa=True)
        assert got_base == base and (got_sa == sa).all()
        if fm_first:
            blk.fm_count([x[:1].tobytes()])
        assert blk.maws(min_len, max_len, count_only=True) == want.size
        st = archon.maw_stats()
        _check_stats(st, x.size, c, min_len, max_len, fan, False, built=0 if fm_first else 1)
        assert st.ms_lcp > 0 and (st.ms_build > 0) == (not fm_first)
        got = blk.maws(min_len, max_len)
        assert got.tolist() == want.tolist(), name
        st = archon.maw_stats()
        _check_stats(st, x.size, c, min_len, max_len, fan, want.size > 0, built=0)     # (the first call's table was kept)
    finally:
        blk.close()
    return got, st


def _all_forms(archon, name, min_len=2, max_len=0, fan=DEFAULT_FAN):
    _, st_h = _host(archon, name, min_len, max_len, fan)
    _, st_d = _dev(archon, name, min_len, max_len, fan, odd=True)
    _, st_b = _block(archon, name, min_len, max_len, fan)
    _, st_f = _block(archon, name, min_len, max_len, fan, fm_first=True)
    assert st_h.probes == st_d.probes == st_b.probes == st_f.probes


@pytest.mark.parametrize("name", ["lit:a", "lit:ab", "lit:aa", "lit:aba", "lit:abc", "same:2", "same:65", "same:1025", "lit:banana", "lit:abracadabra"])
def test_smallest_and_examples(archon, name):
    """n = 1, 2, 3; one byte n times (one word of n + 1 bytes, the primary row a child of its own); the header's examples"""
    x = _case(archon, name)[0]
    want, c = _model(archon, name)
    if name.startswith("same"):
        assert want.tolist() == [(0, 1, x.size + 1, x.size, ord("c"))] and c["intervals"] == x.size - 1
    if name == "lit:banana":
        assert [M.word(x, r) for r in want] == [b"aa", b"ab", b"bb", b"bn", b"nb", b"nn", b"nanan"]
    if name == "lit:abracadabra":
        assert want.size == 25
    _all_forms(archon, name)


@pytest.mark.parametrize("name", ["fixed257", "perm256"])
def test_widest_nodes(archon, name):
    """a node with 257 children (INF and every byte before one fixed byte) and the root with 256; both emit more words from
    one node than a wave has lanes, and from one child up to 255"""
    x, sa, lcp, _, _ = _case(archon, name)
    want, c = _model(archon, name)
    if name == "fixed257":
        node = [v for v in M.intervals(lcp) if v[2] == 1 and int((lcp[v[0] + 1:v[1]] == 1).sum()) == 256]
        assert len(node) == 1 and sa[node[0][1] - 1] == 1 and c["absent_bytes"] == 0        # 257 children, the last one INF
    else:
        assert c["children"] == 256 and c["nodes"] == 1 and want.size == 256 * 255 + 1      # (the primary row's child misses all 256)
    assert np.bincount(want["lo"]).max() > 64
    _all_forms(archon, name)


@pytest.mark.parametrize("sigma", [2, 4])
@pytest.mark.parametrize("n", [63, 64, 65, 127, 129, 255, 256, 257, 512, 513])
def test_random_around_the_thresholds(archon, sigma, n):
    """random blocks over 2 and 4 letters around kDirectRows (nodes and children on both sides of the direct/table threshold)
    and just below, at and above one tile of the pass and two"""
    want, c = _model(archon, "rand:%d:%d" % (sigma, n))
    if n > 2 * DIRECT_ROWS:
        assert c["sets_direct"] and c["sets_table"]
    _all_forms(archon, "rand:%d:%d" % (sigma, n))


@pytest.mark.parametrize("rows", [(16, 16), (16, 64), (64, 64)])
@pytest.mark.parametrize("name", ["rand:2:129", "rand:4:513", "rand:2:4099", "rand:4:4099", "same:1025"])
def test_rank_table_boundaries(archon, name, rows, monkeypatch):
    """sub-chunks and superblocks of 16 and 64 rows: the long sets cross sub-chunk and superblock ends, and the primary row lies
    inside, below and above a partial chunk"""
    monkeypatch.setenv("ARCHON_FM_SUB_ROWS", str(rows[0]))
    monkeypatch.setenv("ARCHON_FM_SUPER_ROWS", str(rows[1]))
    _host(archon, name)
    _dev(archon, name)
    _block(archon, name)
    _block(archon, name, fm_first=True)


@pytest.mark.parametrize("name", ["rand:2:70001", "rand:4:70001"])
def test_many_tiles(archon, name, monkeypatch):
    """274 tiles, more than one superblock of the default table; once more with sub-chunks of 16 rows in superblocks of 64"""
    _all_forms(archon, name)
    monkeypatch.setenv("ARCHON_FM_SUB_ROWS", "16")
    monkeypatch.setenv("ARCHON_FM_SUPER_ROWS", "64")
    _host(archon, name)
    _block(archon, name)


def test_text(archon):
    """text-like input: 6000 bytes of the repository's README"""
    _all_forms(archon, "readme:6000")
    _host(archon, "readme:6000", 2, 4)


@pytest.mark.parametrize("fan", [2, 16, 64])
def test_fan(archon, fan, monkeypatch):
    """the hierarchy at fan-outs 2, 16 and 64: the same records, levels as the fan-out gives them"""
    monkeypatch.setenv("ARCHON_REP_FAN", str(fan))
    for name in ("lit:abracadabra", "rand:2:513", "same:1025", "rand:4:4099"):
        _host(archon, name, fan=fan)
    _dev(archon, "rand:2:513", fan=fan)
    _block(archon, "rand:4:4099", fan=fan)


def test_words_in_the_last_tile_only(archon):
    """254 bytes that occur once sort in front; with min_len 4 the root and the one-byte nodes are out, and every node left has
    its representative row in the second tile: the first tile's word is 0, the second's holds them all"""
    name = "lasttile"
    _, sa, lcp, _, _ = _case(archon, name)
    want, c = _model(archon, name, 4, 0)
    assert want.size > 0 and TILE < sa.size <= 2 * TILE
    assert all(k >= TILE for lo, hi, l, k in M.intervals(lcp) if l >= 2)
    _all_forms(archon, name, 4, 0)
    _all_forms(archon, name)


@pytest.mark.parametrize("name", ["rand:2:4099", "readme:6000"])
@pytest.mark.parametrize("window", [(2, 2), (3, 0), (4, 6), (40, 50), (0, 0), (1, 3)])
def test_filters(archon, window, name):
    """min_len <= len <= max_len; 0 and 1 behave as 2; a window that keeps nothing (no word of the text is that long, and no
    repeat of the random block); nodes and children drop with the window"""
    full, cf = _model(archon, name)
    lo, hi = window
    want, c = _model(archon, name, lo, hi)
    keep = (full["len"] >= max(lo, 2)) & (full["len"] <= (hi or 1 << 30))
    assert want.tolist() == full[keep].tolist()
    if window == (0, 0):
        assert c == cf
    else:
        assert c["nodes"] < cf["nodes"] and c["children"] < cf["children"] and c["intervals"] == cf["intervals"]
    if window == (40, 50):
        assert (want.size, c["shortest"], c["longest"]) == (0, 0, 0)
        if name == "rand:2:4099":
            assert (c["nodes"], c["children"], c["sets_direct"], c["sets_table"]) == (0, 0, 0, 0)
    elif name == "readme:6000" and window != (0, 0):
        assert 0 < want.size < full.size
    _host(archon, name, lo, hi)
    _dev(archon, name, lo, hi)
    _block(archon, name, lo, hi)


def test_cap_rule(archon):
    """cap = total - 1 is ARCHON_E_ARG with *total written and out untouched; cap = total is filled; no words and cap 0 is fine"""
    L, p = archon.lib(), archon._p
    _, sa, lcp, bwt, base = _case(archon, "lit:abracadabra")
    want, _ = _model(archon, "lit:abracadabra")
    total = ctypes.c_uint64(0)
    out = np.zeros(want.size, archon.MAW)
    assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), sa.size, base, 2, 0, p(out), want.size - 1, _tp(total), 0) == archon.E_ARG
    assert b"room for 24" in L.archon_hip_last_error() and total.value == 25 and not out.view(np.uint32).any()
    assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), sa.size, base, 2, 0, p(out), want.size, _tp(total), 0) == 0
    assert total.value == 25 and out.tolist() == want.tolist()
    total.value = 9
    assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), sa.size, base, 9, 12, p(out), 0, _tp(total), 0) == 0 and total.value == 0
    assert archon.maw_stats().ms_emit == 0
    import torch
    sa_t, lcp_t, bwt_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt)
    out_t = torch.full((5 * 24,), -1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(archon.ArchonError):
        archon.maws_dev(sa_t, lcp_t, bwt_t, base, out_t=out_t)
    assert (out_t.cpu().numpy() == -1).all()
    blk = archon.Block()
    blk.forward(_case(archon, "lit:abracadabra")[0], want_sa=True)
    out[:] = 0
    assert L.archon_hip_block_maws(blk.h, 2, 0, p(out), 24, _tp(total)) == archon.E_ARG and total.value == 25 and not out.view(np.uint32).any()
    blk.forward(_case(archon, "lit:banana")[0], want_sa=False)
    assert L.archon_hip_block_maws(blk.h, 2, 0, p(out), 25, _tp(total)) == archon.E_ARG and total.value == 0
    assert b"suffix array" in L.archon_hip_last_error()
    blk.close()


@pytest.mark.parametrize("bad", [0, "n+1"])
def test_corrupt_sa(archon, bad):
    """an sa value of 0 or n + 1 is ARCHON_E_CORRUPT through the host and the device form: *total 0, out untouched"""
    import torch
    L, p = archon.lib(), archon._p
    _, sa, lcp, bwt, base = _case(archon, "rand:4:513")
    sa = sa.copy()
    sa[300] = 0 if bad == 0 else sa.size + 1
    total = ctypes.c_uint64(5)
    out = np.zeros(4096, archon.MAW)
    assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), sa.size, base, 2, 0, p(out), out.size, _tp(total), 0) == archon.E_CORRUPT
    assert total.value == 0 and not out.view(np.uint32).any() and b"outside 1..513" in L.archon_hip_last_error()
    out_t = torch.full((5 * 4096,), -1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(archon.ArchonError) as e:
        archon.maws_dev(_cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(bwt), base, out_t=out_t)
    assert e.value.code == archon.E_CORRUPT and (out_t.cpu().numpy() == -1).all()


def test_arrays_of_nothing_stay_inside(archon):
    """arrays that are not the SA, LCP array or BWT of anything: ARCHON_OK, whatever comes out; records inside the cap, and the
    next good call is right"""
    rng = np.random.default_rng(5)
    n = 1000
    L, p = archon.lib(), archon._p
    for trial in range(4):
        sa = rng.integers(1, n + 1, n).astype(np.uint32)
        lcp = rng.integers(0, (2, 8, n, 1 << 32)[trial], n, dtype=np.uint64).astype(np.uint32)
        bwt = rng.integers(0, 256, n).astype(np.uint8)
        base = int(rng.integers(0, n))
        total = ctypes.c_uint64(0)
        assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), n, base, 2, 0, None, 0, _tp(total), 0) == 0
        words = total.value
        out = np.zeros(words + 1, archon.MAW)
        out[-1] = (9, 9, 9, 9, 9)
        assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), n, base, 2, 0, p(out), words, _tp(total), 0) == 0 and total.value == words
        assert out[-1].tolist() == (9, 9, 9, 9, 9)
        assert (out["hi"][:words] <= n).all() and (out["lo"][:words] < out["hi"][:words]).all() and (out["last"][:words] < 256).all()
    _host(archon, "lit:banana")


def test_deterministic(archon):
    """two emit runs give the same bytes"""
    a, _ = _host(archon, "rand:4:4099")
    b, _ = _host(archon, "rand:4:4099")
    assert a.tobytes() == b.tobytes()
    c, _ = _dev(archon, "rand:4:4099")
    assert a.tobytes() == c.tobytes()


def test_words_are_minimal_and_absent(archon):
    """every record of a 2000-byte DNA block, as bytes: the word is not in the block, both words with one end byte removed are"""
    x = _case(archon, "dna:2000")[0].tobytes()
    got, _ = _host(archon, "dna:2000")
    words = [archon.maw_bytes(x, r) for r in got]
    assert len(set(words)) == len(words) > 0
    for w in words:
        assert w not in x and w[:-1] in x and w[1:] in x
    assert all(len(w) == int(r["len"]) for w, r in zip(words, got))


def test_other_records_stay(archon):
    """a call of this family leaves the k-mer and the repeats record of the thread as they were"""
    _, sa, lcp, bwt, base = _case(archon, "rand:4:513")
    archon.kmers(sa, lcp, 3)
    archon.repeats(lcp, bwt, base)
    before = (archon.kmer_stats().asdict(), archon.repeat_stats().asdict())
    _host(archon, "rand:4:513")
    _dev(archon, "rand:4:513")
    assert (archon.kmer_stats().asdict(), archon.repeat_stats().asdict()) == before
    st = archon.maw_stats()
    assert st.n == 513 and archon.lib().archon_hip_maw_last_stats(0, None) == archon.E_ARG


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID; a wave takes a tile of 256 rows, so four and twelve waves share the 65
    tiles of 16 385 rows, 16 and 5 each, the last tile of one row): random blocks over 2 and 4 letters, one byte x 1025, the
    README under a length window, and the block whose words lie in the last tile only -- the model's records and counters
    through the host, device and block forms, byte-equal to the same calls without the route, with their counters, launches
    and host waits.  (The random blocks are 16 385 bytes, not the 70 001 of test_many_tiles: at 70 001 this test alone took as
    long as the rest of the file.)"""
    for name, lo, hi in (("rand:2:16385", 2, 0), ("rand:4:16385", 2, 0), ("same:1025", 2, 0), ("readme:6000", 2, 4), ("lasttile", 4, 0)):
        def call():
            got_h, st_h = _host(archon, name, lo, hi)
            got_d, st_d = _dev(archon, name, lo, hi, odd=True)
            got_b, st_b = _block(archon, name, lo, hi)
            assert st_h.probes == st_d.probes == st_b.probes
            return [got_h, got_d, got_b], [st_h, st_d, st_b]
        G.same_under(monkeypatch, grid, call)


def test_second_trip_at_the_product_grid_one_byte(archon):
    """no route: 8192 * 256 + 5 * 256 + 7 rows are 8198 tiles of 256, so waves 0-5 of the 2048 workgroups take a second tile
    and the last tile has 7 rows.  One byte: the one word of n + 1 bytes"""
    n = G.N_MAW
    blk = archon.Block()
    try:
        blk.forward(np.full(n, ord("c"), np.uint8), want_sa=True)
        assert blk.validate() == 1
        assert blk.maws().tolist() == [(0, 1, n + 1, n, ord("c"))]
        st = archon.maw_stats()
        assert (st.n, st.words, st.shortest, st.longest, st.absent_bytes, st.intervals) == (n, 1, n + 1, n + 1, 255, n - 1)
        assert blk.maws(count_only=True) == 1
    finally:
        blk.close()


def test_second_trip_at_the_product_grid_four_letters(archon):
    """no route, 8198 tiles: a random block over four letters with min_len = max_len = 11, 12, 13 (1.5, 1.4 and 0.5
    million words), as a set against the definition by the text (maw_naive.words_of_length, pinned by
    test_maw_abi.py): every word once, none missing"""
    n = G.N_MAW
    x = _text("rand:4:%d" % n)
    blk = archon.Block()
    try:
        blk.forward(x, want_sa=True)
        assert blk.validate() == 1
        for L in (11, 12, 13):
            got = blk.maws(L, L)
            want = M.words_of_length(x, L)
            codes = np.sort(M.record_codes(x, got, L))
            assert want.size > 10000 and got.size == want.size and (codes == want).all(), L
            st = archon.maw_stats()
            assert (st.n, st.min_len, st.max_len, st.words, st.shortest, st.longest) == (n, L, L, want.size, L, L)
            assert blk.maws(L, L, count_only=True) == want.size
    finally:
        blk.close()
