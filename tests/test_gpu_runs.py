"""GPU: the runs of a block and longest-common-extension queries (archon_hip_runs*, archon_hip_block_runs, archon_hip_lce*,
archon_hip_block_lce; include/archon_hip.h) against the rule in plain Python (tests/runs_naive.runs_rule, pinned to the
definition by test_runs_abi.py): record by record, in order, and counter by counter through the host, device and block forms,
on every tiny string, at the tile and hierarchy-level edges, under every filter; and independently of the rule, every record
checked as a run by slices and the short periods against a vectorised finder.

`probes` depends on the fan-out as well as on the input; it is held to its bound -- a left search reads at most 2F - 1 entries
per level -- and to equality between the forms."""
import ctypes
import itertools

import numpy as np
import pytest

import archon_synth as S
import repeats_naive as R
import runs_naive as N
import stride_util as G

pytestmark = pytest.mark.gpu

DEFAULT_FAN = 16
COUNTERS = ("candidates", "roots", "lce_queries", "runs", "emitted", "longest_period")
PARTS = 8
_cases, _rules, _tiny = {}, {}, []


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


def _levels(n, fan):
    levels, c = 0, 1
    while c < n:
        c *= fan
        levels += 1
    return levels


def _tiny_cases():
    """(x, sa, lcp, sa_c, records, counters) of every tiny string, by the definition, made once"""
    if not _tiny:
        for x in N.tiny_strings():
            sa, lcp = R.a7_arrays(x)[:2]
            sa_c = R.a7_arrays(bytes(255 - c for c in x))[0]
            recs, c = N.runs_rule(x)
            _tiny.append((np.frombuffer(x, np.uint8), np.array(sa, np.uint32), np.array(lcp, np.uint32), np.array(sa_c, np.uint32), recs, c))
    return _tiny


def _text(name):
    kind, _, arg = name.partition(":")
    n = int(arg)
    if kind == "binary":
        return np.random.default_rng(n).integers(0, 2, n).astype(np.uint8) + 97
    if kind == "dna":
        return S.gen_dna(n)
    if kind == "text":
        return S.gen_text(n)
    if kind == "motif7":                    # a 7-byte motif with a single-byte defect every few hundred bytes
        x = S.gen_repeat(n, b"abcabdc").copy()
        rng = np.random.default_rng(7 + n)
        x[rng.integers(0, n, max(n // 300, 1))] = ord("z")
        return x
    if kind == "mix":                       # random binary, then the motif with defects, then ab over and over
        return np.concatenate((_text("binary:%d" % (n // 2)), _text("motif7:%d" % (n // 4)), _text("ab:%d" % (n - n // 2 - n // 4))))
    if kind == "defects":                   # archon_synth's periodic block with defects
        return S.gen_motif_defects(n, motif_len=211, defects=7)
    if kind == "ab":
        return S.gen_repeat(n, b"ab").copy()
    if kind == "same":
        return np.full(n, ord("c"), np.uint8)
    if kind == "fib":                       # the Fibonacci string of length F(n)
        return np.frombuffer(N.fibonacci(n), np.uint8)
    raise KeyError(name)


def _case(archon, name):
    """(x, sa, lcp, sa_c) of a named block, made once: two forwards and one lcp of the library"""
    if name not in _cases:
        x = np.ascontiguousarray(_text(name))
        sa = archon.forward(x)[0]
        sa_c = archon.forward(255 - x)[0]
        lcp = archon.lcp(x, sa)
        for a in (x, sa, lcp, sa_c):
            a.setflags(write=False)
        _cases[name] = (x, sa, lcp, sa_c)
    return _cases[name]


def _rule(archon, name, filters=(0, 0, 2, 0)):
    """(records as a RUN array, counters) of the rule over the case's arrays, made once per filter"""
    key = (name,) + tuple(filters)
    if key not in _rules:
        x, sa, lcp, sa_c = _case(archon, name)
        n = x.size
        rank = []
        for a in (sa, sa_c):
            r = np.zeros(n + 1, np.int64)
            r[a] = np.arange(n)
            rank.append(r.tolist())
        recs, c = N.runs_rule(x.tobytes(), *filters, lce=N.SparseLce(sa, lcp).scalar(), rank=rank)
        _rules[key] = (np.array(recs, np.uint32).reshape(-1, 4).copy().view(N.RUN).ravel(), c)
    return _rules[key]


def _launches(n, fan, lcp_fan, emitted, block=False):
    """2 per inverse array, the levels of the two rank hierarchies over n + 1 entries and of the one over lcp, the count pass;
    the scan and the emit pass when something is emitted; the block form's complement kernel"""
    return 4 + 2 * _levels(n + 1, fan) + _levels(n, lcp_fan) + 1 + (2 if emitted else 0) + (1 if block else 0)


def _check_stats(st, n, c, filters, fan, lcp_fan, emit, block=False):
    got = {k: getattr(st, k) for k in COUNTERS}
    assert got == {k: c[k] for k in COUNTERS}, (got, c)
    assert (st.n, st.min_period, st.max_period, st.min_copies, st.min_len, st.what) == (n,) + tuple(filters) + (0,)
    assert (st.fan, st.lcp_fan, st.levels) == (fan, lcp_fan, _levels(n, lcp_fan))
    assert st.probes <= 2 * n * (2 * fan - 1) * _levels(n + 1, fan)
    assert c["candidates"] <= 2 * (n - 1) and c["emitted"] <= c["runs"] < max(n, 2)
    emitted = emit and c["emitted"] > 0
    assert st.kernel_launches == _launches(n, fan, lcp_fan, emitted, block)
    if block:
        assert st.host_syncs >= 3 + emitted and st.ms_forward > 0 and st.ms_lcp > 0
    else:
        assert st.host_syncs == 1 + emitted and st.ms_forward == 0 and st.ms_lcp == 0
    assert st.ms_build > 0 and st.ms_count > 0 and (st.ms_emit > 0) == bool(emitted)


def _host(archon, sa, lcp, sa_c, want, c, filters=(0, 0, 2, 0), fan=DEFAULT_FAN, lcp_fan=DEFAULT_FAN):
    """archon_hip_runs with room for exactly the records; a sentinel record behind them"""
    L, p, n = archon.lib(), archon._p, sa.size
    k = len(want)
    total = ctypes.c_uint64(77)
    out = np.zeros(k + 1, archon.RUN)
    out.view(np.uint32)[:] = 0xA5A5A5A5
    archon._check(L.archon_hip_runs(p(sa), p(lcp), p(sa_c), n, *filters, p(out), k, _tp(total), 0))
    assert total.value == k and out[:k].tolist() == [tuple(r) for r in want], (sa, filters)
    assert (out[k:].view(np.uint32) == 0xA5A5A5A5).all()
    st = archon.run_stats()
    _check_stats(st, n, c, filters, fan, lcp_fan, True)
    return out[:k], st


def _dev(archon, sa, lcp, sa_c, want, c, filters=(0, 0, 2, 0), fan=DEFAULT_FAN, lcp_fan=DEFAULT_FAN, odd=False):
    """archon_hip_runs_dev on torch tensors (odd: every array one element past an allocation's start)"""
    import torch
    k = len(want)
    ts = [_cuda(a.view(np.int32)) for a in (sa, lcp, sa_c)]
    if odd:
        ts = [_odd(t) for t in ts]
    out_t = torch.full((4 * k + 2,), -1, dtype=torch.int32, device="cuda:0")
    assert archon.runs_dev(*ts, *filters, out_t=out_t[1:4 * k + 1]) == k
    got = out_t.cpu().numpy().view(np.uint32)
    assert got[0] == got[-1] == 0xFFFFFFFF
    assert got[1:-1].view(archon.RUN).tolist() == [tuple(r) for r in want], (sa, filters)
    st = archon.run_stats()
    _check_stats(st, sa.size, c, filters, fan, lcp_fan, True)
    return got[1:-1].view(archon.RUN), st


def _block(archon, blk, x, sa, want, c, filters=(0, 0, 2, 0), fan=DEFAULT_FAN, lcp_fan=DEFAULT_FAN):
    """Block.forward, then archon_hip_block_runs with room for exactly the records"""
    L, p = archon.lib(), archon._p
    got_sa, _ = blk.forward(x, want_sa=True)
    assert (got_sa == sa).all()
    k = len(want)
    total = ctypes.c_uint64(77)
    out = np.zeros(k + 1, archon.RUN)
    out.view(np.uint32)[:] = 0xA5A5A5A5
    archon._check(L.archon_hip_block_runs(blk.h, *filters, p(out), k, _tp(total)))
    assert total.value == k and out[:k].tolist() == [tuple(r) for r in want], (x, filters)
    assert (out[k:].view(np.uint32) == 0xA5A5A5A5).all()
    st = archon.run_stats()
    _check_stats(st, x.size, c, filters, fan, lcp_fan, True, block=True)
    return out[:k], st


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("fan", [2, 0])
def test_exhaustive_tiny(archon, fan, part, monkeypatch):
    """every string of length 1-10 over {0, 1} and 1-7 over {0, 1, 255}, in parts, through the device form (every other string
    at odd device addresses), the host form and the block form, with fan-outs of 2 (ARCHON_LZ_FAN=2 ARCHON_REP_FAN=2: ten items
    cross four levels) and with the defaults: the rule's records in the rule's order, nothing stored past them, the rule's
    counters, the launches and the host waits"""
    if fan:
        monkeypatch.setenv("ARCHON_LZ_FAN", str(fan))
        monkeypatch.setenv("ARCHON_REP_FAN", str(fan))
    f = fan or DEFAULT_FAN
    blk = archon.Block()
    try:
        for i, (x, sa, lcp, sa_c, want, c) in enumerate(_tiny_cases()):
            if i % PARTS != part:
                continue
            _, st_d = _dev(archon, sa, lcp, sa_c, want, c, fan=f, lcp_fan=f, odd=bool((i // PARTS) % 2))
            _, st_h = _host(archon, sa, lcp, sa_c, want, c, fan=f, lcp_fan=f)
            _, st_b = _block(archon, blk, x, sa, want, c, fan=f, lcp_fan=f)
            assert st_d.probes == st_h.probes == st_b.probes
    finally:
        blk.close()


def test_header_examples(archon):
    """the header's four examples through pyarchon.runs_of, Block.runs and Block.lce, with their counters"""
    blk = archon.Block()
    try:
        for x, recs, counters in ((b"banana", [(1, 6, 2, 6)], (7, 1, 8)),
                                  (b"mississippi", [(2, 4, 1, 4), (5, 7, 1, 7), (1, 8, 3, 8), (8, 10, 1, 10)], (16, 6, 24)),
                                  (b"aaaa", [(0, 4, 1, 4)], (6, 2, 10)), (b"abracadabra", [], (18, 5, 26))):
            assert archon.runs_of(x).tolist() == recs
            st = archon.run_stats()
            assert (st.candidates, st.roots, st.lce_queries) == counters
            assert archon.runs_of(x, count_only=True) == len(recs) and archon.run_stats().ms_emit == 0
            blk.forward(np.frombuffer(x, np.uint8), want_sa=True)
            assert blk.runs().tolist() == recs and blk.runs(count_only=True) == len(recs)
            n, lce = len(x), N.plain_lce(x)
            s, t = (a.ravel() for a in np.meshgrid(np.arange(n + 1), np.arange(n + 1)))
            assert blk.lce(s, t).tolist() == [lce(int(a), int(b)) for a, b in zip(s, t)]
    finally:
        blk.close()


@pytest.mark.parametrize("fan", [2, 0])
def test_lce_every_pair_of_tiny_strings(archon, fan, monkeypatch):
    """every pair (s, t) in 0..n of a few tiny strings through the host and device forms (odd addresses) against the plain lce"""
    import torch
    if fan:
        monkeypatch.setenv("ARCHON_REP_FAN", str(fan))
    for x in (b"a", b"ab", b"aa", b"banana", b"mississippi", b"abracadabra", b"aaaaaaaaaaaaaaaaa", b"abababababababababa", bytes([0, 255, 0, 0, 255, 1, 0, 255])):
        sa, lcp = (np.array(a, np.uint32) for a in R.a7_arrays(x)[:2])
        n, lce = len(x), N.plain_lce(x)
        s, t = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(n + 1), np.arange(n + 1)))
        want = [lce(int(a), int(b)) for a, b in zip(s, t)]
        assert archon.lce(sa, lcp, s, t).tolist() == want, x
        st = archon.run_stats()
        assert (st.n, st.what, st.lce_queries, st.lcp_fan, st.levels) == (n, 1, s.size, fan or DEFAULT_FAN, _levels(n, fan or DEFAULT_FAN))
        assert st.kernel_launches == 2 + st.levels + 2 and st.host_syncs == 2
        out_t = torch.full((s.size + 2,), -1, dtype=torch.int32, device="cuda:0")
        archon.lce_dev(_odd(_cuda(sa.view(np.int32))), _odd(_cuda(lcp.view(np.int32))), _odd(_cuda(s.view(np.int32))), _odd(_cuda(t.view(np.int32))),
                       out_t[1:-1])
        got = out_t.cpu().numpy()
        assert got[1:-1].tolist() == want and got[0] == got[-1] == -1
        assert archon.run_stats().host_syncs == 1


@pytest.mark.parametrize("name", ["dna:5000", "text:33333", "defects:70000"])
def test_lce_random_pairs(archon, name):
    """4096 random pairs -- a quarter of them neighbours in the suffix array, a few equal or zero -- on DNA, text and a periodic
    block with defects, through the host, device and block forms, against the numpy lce over a sparse table"""
    import torch
    x, sa, lcp, _ = _case(archon, name)
    n = x.size
    rng = np.random.default_rng(n)
    s, t = rng.integers(0, n + 1, 4096).astype(np.uint32), rng.integers(0, n + 1, 4096).astype(np.uint32)
    rows = rng.integers(0, n - 1, 1024)
    s[:1024], t[:1024] = sa[rows], sa[rows + 1]
    s[1024:1040] = t[1024:1040]
    s[1040:1044], t[1044:1048] = 0, 0
    s[1048], t[1048] = n, n - 1
    want = N.SparseLce(sa, lcp).many(s, t)
    assert want[:1024].tolist() == lcp[rows + 1].tolist() and want[1024:1040].tolist() == t[1024:1040].tolist() and not want[1040:1048].any()
    assert archon.lce(sa, lcp, s, t).tolist() == want.tolist()
    out_t = torch.full((4096,), -1, dtype=torch.int32, device="cuda:0")
    archon.lce_dev(_cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(s.view(np.int32)), _cuda(t.view(np.int32)), out_t)
    assert out_t.cpu().numpy().tolist() == want.tolist()
    blk = archon.Block()
    try:
        blk.forward(x, want_sa=True)
        assert blk.lce(s, t).tolist() == want.tolist()
        assert archon.run_stats().ms_lcp > 0
    finally:
        blk.close()


def test_lce_refusals(archon):
    """an item above n is ARCHON_E_ARG with nothing written, found on the device by the device form; a bad sa is
    ARCHON_E_CORRUPT; k = 0 writes nothing; a block without its suffix array is ARCHON_E_ARG"""
    import torch
    sa, lcp = (np.array(a, np.uint32) for a in R.a7_arrays(b"banana")[:2])
    s, t = np.array([1, 2, 7], np.uint32), np.array([3, 6, 1], np.uint32)
    out_t = torch.full((3,), -1, dtype=torch.int32, device="cuda:0")
    ts = [_cuda(a.view(np.int32)) for a in (sa, lcp, s, t)]
    with pytest.raises(archon.ArchonError) as e:
        archon.lce_dev(*ts, out_t)
    assert e.value.code == archon.E_ARG and out_t.cpu().tolist() == [-1, -1, -1]
    with pytest.raises(archon.ArchonError) as e:
        archon.lce(sa, lcp, s, t)
    assert e.value.code == archon.E_ARG
    for bad in ([2, 4, 6, 1, 3, 3], [2, 4, 6, 1, 3, 7], [2, 4, 6, 1, 3, 0]):
        bad_t = _cuda(np.array(bad, np.int32))
        with pytest.raises(archon.ArchonError) as e:
            archon.lce_dev(bad_t, ts[1], _cuda(s[:2].view(np.int32)), _cuda(t[:2].view(np.int32)), out_t[:2])
        assert e.value.code == archon.E_CORRUPT and out_t.cpu().tolist() == [-1, -1, -1]
        with pytest.raises(archon.ArchonError) as e:
            archon.lce(np.array(bad, np.uint32), lcp, s[:2], t[:2])
        assert e.value.code == archon.E_CORRUPT
    archon.lce_dev(ts[0], ts[1], ts[2][:0], ts[3][:0], out_t[:0])
    assert archon.lce(sa, lcp, s[:0], t[:0]).size == 0 and out_t.cpu().tolist() == [-1, -1, -1]
    blk = archon.Block()
    try:
        blk.forward(np.frombuffer(b"banana", np.uint8), want_sa=False)
        for call in (lambda: blk.lce(s[:2], t[:2]), blk.runs):
            with pytest.raises(archon.ArchonError) as e:
                call()
            assert e.value.code == archon.E_ARG
    finally:
        blk.close()


def _independent(x, recs):
    """every record is a run by slices, none twice, in ascending root with start + period <= root <= end; the subset with
    period <= 64 is what the vectorised finder gives"""
    xb = x.tobytes()
    got = [(int(r["start"]), int(r["end"]), int(r["period"])) for r in recs]
    assert len(set(got)) == len(got)
    assert all(N.is_run_fast(xb, *r) for r in got)
    root = recs["root"].astype(np.int64)
    assert (np.diff(root) >= 0).all() and (recs["start"] + recs["period"] <= root).all() and (root <= recs["end"]).all()
    assert {r for r in got if r[2] <= 64} == N.runs_short(xb, 64)


@pytest.mark.parametrize("kind", ["binary", "dna", "motif7", "ab", "same"])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 16385, 65537])
def test_medium_blocks(archon, kind, n):
    """random binary, DNA, a 7-byte motif with single-byte defects, ab x n/2 and one byte at the tile edges (2047, 2048, 2049
    items) and the hierarchy-level edges (16^3 + 1 and 16^4 + 1 rows; the rank hierarchies hold n + 1 entries, so 65537 is past
    their edge as well): the records equal the rule's exactly through the host, device and block forms; independently every
    record is a run by slices and the periods up to 64 are those of the vectorised finder"""
    name = "%s:%d" % (kind, n)
    x, sa, lcp, sa_c = _case(archon, name)
    want, c = _rule(archon, name)
    got_h, st_h = _host(archon, sa, lcp, sa_c, want, c)
    got_d, st_d = _dev(archon, sa, lcp, sa_c, want, c, odd=True)
    blk = archon.Block()
    try:
        got_b, st_b = _block(archon, blk, x, sa, want, c)
    finally:
        blk.close()
    assert st_h.probes == st_d.probes == st_b.probes
    _independent(x, got_h)
    if kind == "same":
        assert got_h.tolist() == [(0, n, 1, n)] and st_h.roots == 2 and st_h.candidates == 2 * (n - 1)
    if kind == "ab":
        assert got_h.size == 1 and got_h[0].tolist()[:3] == (0, n, 2)
    if kind == "motif7":
        assert st_h.longest_period >= 7


FILTER_BLOCK = "mix:5000"


@pytest.mark.parametrize("min_period,max_period", [(0, 0), (1, 1), (2, 0), (0, 6), (7, 7), (8, 0), (3, 300)])
def test_filters(archon, min_period, max_period):
    """every combination of min_period, max_period, min_copies and min_len on one block: the records are those of the
    unfiltered list that pass, in its order; the counters are the rule's; counting only; a short cap"""
    x, sa, lcp, sa_c = _case(archon, FILTER_BLOCK)
    full, c_full = _rule(archon, FILTER_BLOCK)
    assert full.size > 20 and len(set(full["period"].tolist())) >= 3
    L, p, n = archon.lib(), archon._p, sa.size
    for min_copies, min_len in itertools.product((2, 3, 50), (0, 15, 1000)):
        filters = (min_period, max_period, min_copies, min_len)
        ln = full["end"].astype(np.int64) - full["start"]
        keep = (full["period"] >= min_period) & ((full["period"] <= max_period) | (max_period == 0)) & (ln >= min_copies * full["period"].astype(np.int64)) \
            & (ln >= min_len)
        want, c = _rule(archon, FILTER_BLOCK, filters)
        assert want.tolist() == full[keep].tolist(), filters
        got, st = _host(archon, sa, lcp, sa_c, want, c, filters)
        assert st.runs == int(((full["period"] >= min_period) & ((full["period"] <= max_period) | (max_period == 0))).sum())
        assert st.longest_period == (int(want["period"].max()) if want.size else 0)
        # counting only: no emit pass
        assert archon.runs(sa, lcp, sa_c, *filters, count_only=True) == want.size
        st = archon.run_stats()
        assert st.ms_emit == 0 and st.host_syncs == 1 and st.kernel_launches == _launches(n, DEFAULT_FAN, DEFAULT_FAN, False)
        if want.size:           # a short cap: *total written, out untouched
            total = ctypes.c_uint64(0)
            out = np.zeros(want.size, archon.RUN)
            assert L.archon_hip_runs(p(sa), p(lcp), p(sa_c), n, *filters, p(out), want.size - 1, _tp(total), 0) == archon.E_ARG
            assert total.value == want.size and not out.view(np.uint32).any()
    _dev(archon, sa, lcp, sa_c, *_rule(archon, FILTER_BLOCK, (min_period, max_period, 3, 15)), (min_period, max_period, 3, 15), odd=True)
    with pytest.raises(archon.ArchonError) as e:
        archon.runs(sa, lcp, sa_c, min_copies=1)
    assert e.value.code == archon.E_ARG


def test_fibonacci(archon):
    """the Fibonacci string of length F(k) has 2 F(k-2) - 3 runs: confirmed against the rule up to length 10 946, then used at
    length 317 811 (242 783 runs), where every record is verified by slices"""
    fib = [0, 1, 1]
    while len(fib) <= 28:
        fib.append(fib[-1] + fib[-2])
    for k in (5, 6, 9, 15, 21):
        name = "fib:%d" % k
        x, sa, lcp, sa_c = _case(archon, name)
        want, c = _rule(archon, name)
        assert x.size == fib[k] and want.size == 2 * fib[k - 2] - 3
        _host(archon, sa, lcp, sa_c, want, c)
    assert (fib[15], 2 * fib[13] - 3, fib[21]) == (610, 463, 10946)
    x, sa, lcp, sa_c = _case(archon, "fib:28")
    assert x.size == 317811
    got = archon.runs(sa, lcp, sa_c)
    assert got.size == 242783 == 2 * fib[26] - 3
    st = archon.run_stats()
    assert st.emitted == st.runs == got.size and st.longest_period == int(got["period"].max())
    xb = x.tobytes()
    assert all(N.is_run_fast(xb, s, e, p) for s, e, p in zip(got["start"].tolist(), got["end"].tolist(), got["period"].tolist()))
    assert len(set(zip(got["start"].tolist(), got["period"].tolist()))) == got.size and (np.diff(got["root"].astype(np.int64)) >= 0).all()


def test_one_byte(archon):
    """one byte x 2^20 gives exactly (0, n, 1, n) with two roots: every other candidate is dropped at step 3"""
    n = 1 << 20
    x = np.full(n, 7, np.uint8)
    blk = archon.Block()
    try:
        blk.forward(x, want_sa=True)
        assert blk.runs().tolist() == [(0, n, 1, n)]
        st = archon.run_stats()
        assert (st.roots, st.candidates, st.runs, st.emitted, st.longest_period) == (2, 2 * (n - 1), 1, 1, 1)
        assert st.lce_queries == 2 * (n - 1) + 2 * (n - 2)
        assert st.probes <= 2 * n * 31 * _levels(n + 1, DEFAULT_FAN)
    finally:
        blk.close()


def test_determinism_and_isolation(archon):
    """two calls on the same block give the same bytes; a runs call leaves archon_hip_stats, the LCP record and the k-mer record
    as they were (the block form keeps the LCP record of its own LCP step, as its siblings do)"""
    name = "binary:16385"
    x, sa, lcp, sa_c = _case(archon, name)
    archon.kmers(sa, lcp, 3, count_only=True)
    before = (archon.stats(), archon.lcp_stats().asdict(), archon.kmer_stats().asdict())
    a = archon.runs(sa, lcp, sa_c)
    b = archon.runs(sa, lcp, sa_c)
    assert a.tobytes() == b.tobytes() and a.size > 100
    assert archon.lce(sa, lcp, [5, 9], [7, 9]).tolist()[1] == 9
    assert (archon.stats(), archon.lcp_stats().asdict(), archon.kmer_stats().asdict()) == before
    blk = archon.Block()
    try:
        blk.forward(x, want_sa=True)
        before = (archon.stats(), archon.kmer_stats().asdict())
        c = blk.runs()
        assert c.tobytes() == a.tobytes() and blk.runs().tobytes() == a.tobytes()
        assert (archon.stats(), archon.kmer_stats().asdict()) == before
    finally:
        blk.close()


def test_corrupt_arrays(archon):
    """sa_c (or sa) with a value twice, with n + 1 or with 0 is ARCHON_E_CORRUPT with *total 0 and the output untouched, in the
    host and device forms; a permutation that is no suffix array, and an lcp of garbage, return ARCHON_OK with every access in
    bounds"""
    import torch
    x, sa, lcp, sa_c = _case(archon, "dna:5000")
    L, p, n = archon.lib(), archon._p, sa.size
    out = np.zeros(n, archon.RUN)
    for which in (0, 1):
        for value in (int(sa_c[17]), n + 1, 0):
            arrays = [sa.copy(), sa_c.copy()]
            arrays[which][4000] = arrays[which][17] if value == int(sa_c[17]) else value
            total = ctypes.c_uint64(5)
            assert L.archon_hip_runs(p(arrays[0]), p(lcp), p(arrays[1]), n, 0, 0, 2, 0, p(out), n, _tp(total), 0) == archon.E_CORRUPT
            assert total.value == 0 and not out.view(np.uint32).any()
            assert ("sa_c" if which else "sa is") in L.archon_hip_last_error().decode()
            out_t = torch.full((4 * n,), -1, dtype=torch.int32, device="cuda:0")
            with pytest.raises(archon.ArchonError) as e:
                archon.runs_dev(_cuda(arrays[0].view(np.int32)), _cuda(lcp.view(np.int32)), _cuda(arrays[1].view(np.int32)), out_t=out_t)
            assert e.value.code == archon.E_CORRUPT and int(out_t.max()) == -1
    rng = np.random.default_rng(5)
    garbage = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for a, b, c in ((rng.permutation(n).astype(np.uint32) + 1, lcp, sa_c), (sa, lcp, rng.permutation(n).astype(np.uint32) + 1), (sa, garbage, sa_c),
                    (sa_c, garbage, sa)):
        got = archon.runs(a, b, c)
        assert got.size < 2 * n
        if got.size:
            assert int(got["end"].max()) <= n and (got["start"] <= got["end"]).all() and int(got["root"].max()) <= n


def test_resident_block_survives(archon):
    """Block.runs after Block.forward leaves the resident block valid: validate() is 1 afterwards and read_bwt unchanged -- the
    second forward, on the complemented copy, has not disturbed it; and a later FM call still answers from it"""
    name = "text:33333"
    x, sa, lcp, sa_c = _case(archon, name)
    want, c = _rule(archon, name)
    blk = archon.Block()
    try:
        got_sa, base = blk.forward(x, want_sa=True)
        bwt = blk.read_bwt().copy()
        got = blk.runs()
        assert got.tolist() == want.tolist()
        assert blk.validate() == 1 and (blk.read_bwt() == bwt).all()
        assert (blk.lcp() == lcp).all()
        lo, hi = blk.fm_count([x[100:104].tobytes()])
        assert hi[0] > lo[0]
        assert blk.runs(min_period=2).tolist() == want[want["period"] >= 2].tolist()
    finally:
        blk.close()
    _independent(x, got)


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID): random binary at 16^3 + 1 (9 tiles), the Fibonacci string of length
    10 946 (6 tiles, the last one ragged), text under period, copies and length filters (17 tiles) and 70 000 LCE queries
    (274 workgroups by themselves) -- the rule's records and counters through the host and device forms, byte-equal to the same
    call without the route, with its counters, launches and host waits"""
    for name, filters in (("binary:16385", (0, 0, 2, 0)), ("fib:21", (0, 0, 2, 0)), ("text:33333", (2, 40, 2, 4))):
        x, sa, lcp, sa_c = _case(archon, name)
        want, c = _rule(archon, name, filters)
        assert want.size > 50

        def call():
            got_h, st_h = _host(archon, sa, lcp, sa_c, want, c, filters)
            got_d, st_d = _dev(archon, sa, lcp, sa_c, want, c, filters, odd=True)
            count = archon.runs(sa, lcp, sa_c, *filters, count_only=True)
            return (got_h, got_d, count), (st_h, st_d, archon.run_stats())
        got = G.same_under(monkeypatch, grid, call)
        assert all(N.is_run_fast(x.tobytes(), int(r["start"]), int(r["end"]), int(r["period"])) for r in got[0])
    x, sa, lcp, _ = _case(archon, "defects:70000")
    n = x.size
    rng = np.random.default_rng(70000)
    s, t = rng.integers(0, n + 1, 70000).astype(np.uint32), rng.integers(0, n + 1, 70000).astype(np.uint32)
    rows = rng.integers(0, n - 1, 20000)
    s[:20000], t[:20000] = sa[rows], sa[rows + 1]
    want = N.SparseLce(sa, lcp).many(s, t)

    def lce():
        got = archon.lce(sa, lcp, s, t)
        assert got.tolist() == want.tolist()
        return got, archon.run_stats()
    G.same_under(monkeypatch, grid, lce)


@pytest.mark.parametrize("shape", ["same", "dna"])
def test_second_trip_at_the_product_grid(archon, shape):
    """no route: 2048 * 2048 + 3 * 2048 + 5 items are 2052 tiles, so workgroups 0-3 of the 2048 take a second tile in the count
    and the emit pass and the last tile has 5 items.  One byte: the single record and the exact counters of test_one_byte.
    DNA with max_period 8: a million records, as a set those of the vectorised finder, in ascending root, and a sample of
    10 000 checked as runs by slices"""
    n = G.N2
    x = np.ascontiguousarray(_text("%s:%d" % (shape, n)))
    blk = archon.Block()
    try:
        blk.forward(x, want_sa=True)
        assert blk.validate() == 1
        if shape == "same":
            assert blk.runs().tolist() == [(0, n, 1, n)]
            st = archon.run_stats()
            assert (st.roots, st.candidates, st.runs, st.emitted, st.longest_period) == (2, 2 * (n - 1), 1, 1, 1)
            assert st.lce_queries == 2 * (n - 1) + 2 * (n - 2)
            assert st.probes <= 2 * n * 31 * _levels(n + 1, DEFAULT_FAN)
        else:
            got = blk.runs(max_period=8)
            st = archon.run_stats()
            xb = x.tobytes()
            want = N.runs_short(xb, 8)
            triples = set(zip(got["start"].tolist(), got["end"].tolist(), got["period"].tolist()))
            assert got.size == len(triples) == len(want) > 500000 and triples == want
            assert st.emitted == st.runs == got.size and st.longest_period == int(got["period"].max()) == 8
            root = got["root"].astype(np.int64)
            assert (np.diff(root) >= 0).all() and (got["start"] + got["period"] <= root).all() and (root <= got["end"]).all()
            for i in np.random.default_rng(n).integers(0, got.size, 10000).tolist():
                assert N.is_run_fast(xb, int(got["start"][i]), int(got["end"][i]), int(got["period"][i]))
            assert blk.runs(max_period=8, count_only=True) == got.size
    finally:
        blk.close()
