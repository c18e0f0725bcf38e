"""GPU: the repeats of a block (archon_hip_repeats, repeats_dev, block_repeats; include/archon_hip.h) against the stack
enumeration on the CPU (tests/repeats_naive.c, pinned to the definition by test_repeats_abi.py): content and order, the
call's counters against numpy on the LCP array, the work bound of the header, the cap rule, locating, and bad input."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import repeats_naive as R
import stride_util as G

pytestmark = pytest.mark.gpu

MiB = 1 << 20
DEFAULT_FAN = 16                # repeats.hiph kDefaultFan: F when no test route names one


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("repeats_naive"))


@pytest.fixture(scope="module")
def tiny(archon, oracle):
    """every string of length 1-7 over {0, 1, 255}: (lcp, bwt, base), SA and BWT from the oracle, lcp from archon.lcp"""
    out = []
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = np.array(t, np.uint8)
            sa, bwt, base = oracle.forward(x)
            out.append((archon.lcp(x, sa), np.ascontiguousarray(bwt, np.uint8), int(base)))
    return out


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _odd(t):
    """the same values at an odd device address (one element past an allocation's start)"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def _host_once(archon, lcp, bwt, base, kind, min_len=1, min_occ=2):
    """archon_hip_repeats with room for n records: count and emit in one call"""
    out = np.zeros(bwt.size, archon.REPEAT)
    total = ctypes.c_uint64(0)
    archon._check(archon.lib().archon_hip_repeats(archon._p(lcp), archon._p(bwt), bwt.size, base, kind, min_len, min_occ, archon._p(out), out.size,
                                                  ctypes.cast(ctypes.byref(total), ctypes.c_void_p), 0))
    return out[:total.value]


def _bound(n, fan):
    """the header's bound on probes: 2 (2 F - 1) L (n - 1), L = ceil(log_F n)"""
    levels, c = 0, 1
    while c < n:
        c *= fan
        levels += 1
    return 2 * (2 * fan - 1) * levels * (n - 1), levels


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("fan", [2, 0])
def test_exhaustive_tiny(archon, naive, tiny, fan, kind, monkeypatch):
    """every string of length 1-7 over {0, 1, 255} through repeats and repeats_dev (every other one at odd device addresses),
    with a fan-out of 2 (seven rows cross three levels) and the default: the helper's records in the helper's order"""
    import torch
    if fan:
        monkeypatch.setenv("ARCHON_REP_FAN", str(fan))
    for i, (lcp, bwt, base) in enumerate(tiny):
        want = naive(lcp, bwt, base, kind)[0]
        got = _host_once(archon, lcp, bwt, base, kind)
        assert got.tolist() == want.tolist(), (bwt, base, lcp)
        st = archon.repeat_stats()
        assert st.fan == (fan or DEFAULT_FAN) and st.repeats == want.size and st.n == bwt.size
        lcp_t, bwt_t = _cuda(lcp.view(np.int32)), _cuda(bwt)
        out_t = torch.full((4 * bwt.size + 1,), -1, dtype=torch.int32, device="cuda:0")
        if i % 2:
            lcp_t, bwt_t = _odd(lcp_t), _odd(bwt_t)
        total = archon.repeats_dev(lcp_t, bwt_t, base, kind, out_t=out_t[1:])
        got = out_t[1:].cpu().numpy().view(np.uint32)
        assert total == want.size and (got[4 * total:] == 0xFFFFFFFF).all()
        assert got[:4 * total].view(archon.REPEAT).tolist() == want.tolist(), (bwt, base, lcp)


def _numpy_counters(lcp):
    """(intervals, sum_lcp) from the LCP array alone: a row opens an interval when no row between it and its nearest smaller
    value to the left holds the same value -- counted as the distinct (lo, value) pairs by a stack over numpy's array"""
    v = lcp.astype(np.int64)
    v[0] = 0
    intervals, stack = 0, [0]
    for cur in v[1:].tolist():
        while stack[-1] > cur:
            stack.pop()
        if stack[-1] < cur:
            stack.append(cur)
            intervals += 1
    return intervals, int(v[1:].sum())


def _check_kinds(archon, naive, blk, lcp, bwt, base, kinds):
    """Block.repeats of the given kinds with both filters against the helper, the counters against numpy on the LCP array;
    returns the records and the stats records of every call"""
    n = bwt.size
    intervals, sum_lcp = _numpy_counters(lcp)
    out, stats = [], []
    for kind in kinds:
        for min_len in (1, 8):
            for min_occ in (2, 3):
                want, w_int, w_occ, w_long = naive(lcp, bwt, base, kind, min_len, min_occ)
                got = blk.repeats(kind, min_len, min_occ)
                st = archon.repeat_stats()
                assert got.size == want.size and (got == want).all(), (kind, min_len, min_occ)
                assert (st.n, st.kind, st.min_len, st.min_occ) == (n, kind, min_len, min_occ)
                assert st.intervals == intervals == w_int and st.sum_lcp == sum_lcp
                assert st.distinct_substrings == n * (n + 1) // 2 - sum_lcp
                assert st.repeats == want.size and st.occurrences == w_occ == int((want["hi"].astype(np.int64) - want["lo"]).sum())
                assert st.longest == w_long == (int(want["len"].max()) if want.size else 0)
                assert st.probes <= _bound(n, DEFAULT_FAN)[0] and st.levels == _bound(n, DEFAULT_FAN)[1]
                assert blk.repeats(kind, min_len, min_occ, count_only=True) == want.size
                assert archon.repeat_stats().ms_emit == 0 and archon.repeat_stats().ms_lcp > 0
                out.append(got)
                stats += [st, archon.repeat_stats()]
    return out, stats


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65536, MiB + 3])
def test_shapes(archon, naive, shape, n, monkeypatch):
    """every synthetic shape through Block.repeats, kinds 1 and 2 with both filters, against the helper; the counters against
    numpy on the LCP array; at 65536 once more with a fan-out of 4"""
    x = S.gen_shape(shape, n)
    blk = archon.Block()
    _, base = blk.forward(x, want_sa=True)
    lcp, bwt = blk.lcp(), blk.read_bwt()
    _check_kinds(archon, naive, blk, lcp, bwt, base, (1, 2))
    if n == 65536:
        monkeypatch.setenv("ARCHON_REP_FAN", "4")
        want = naive(lcp, bwt, base, 1)[0]
        got = blk.repeats(1)
        st = archon.repeat_stats()
        assert st.fan == 4 and st.levels == 8 and (got == want).all() and st.probes <= _bound(n, 4)[0]
    blk.close()


def fibonacci(least):
    a, b = b"a", b"b"
    while len(a) < least:
        a, b = a + b, a
    return np.frombuffer(a, np.uint8).copy()


@pytest.mark.parametrize("shape", ["a", "ab", "fibonacci"])
def test_worst_case_depth(archon, naive, shape):
    """counting only, where the nearest smaller value is far: a block of one byte (every left search ends at row 0), of two
    alternating bytes, and a Fibonacci string -- totals, and the probes within the header's bound"""
    n = 16 * MiB
    x = fibonacci(MiB) if shape == "fibonacci" else S.gen_shape(shape, n)
    n = x.size
    blk = archon.Block()
    _, base = blk.forward(x, want_sa=True)
    bound, levels = _bound(n, DEFAULT_FAN)
    if shape == "a":
        for kind, want in ((0, n - 1), (1, n - 1), (2, 1)):
            assert blk.repeats(kind, count_only=True) == want
            st = archon.repeat_stats()
            assert st.intervals == n - 1 and st.probes <= bound and st.levels == levels and st.longest == n - 1
            assert st.sum_lcp == n * (n - 1) // 2 and st.distinct_substrings == n
        out = np.zeros(1, archon.REPEAT)
        total = ctypes.c_uint64(0)
        archon._check(archon.lib().archon_hip_block_repeats(blk.h, 2, 1, 2, archon._p(out), 1, ctypes.cast(ctypes.byref(total), ctypes.c_void_p)))
        assert total.value == 1 and out[0].tolist() == (0, 2, n - 1, 1)
    else:
        lcp, bwt = blk.lcp(), blk.read_bwt()
        for kind in (0, 1, 2):
            want, w_int, w_occ, w_long = naive(lcp, bwt, base, kind, count_only=True)
            assert blk.repeats(kind, count_only=True) == want
            st = archon.repeat_stats()
            assert (st.intervals, st.occurrences, st.longest) == (w_int, w_occ, w_long)
            assert st.probes <= bound and st.levels == levels
            assert st.distinct_substrings == n * (n + 1) // 2 - int(lcp[1:].astype(np.int64).sum())
    blk.close()


@pytest.fixture(scope="module")
def dna(archon):
    """dna at 65536: (x, sa, lcp, bwt, base)"""
    x = S.gen_shape("dna", 65536)
    sa, bwt, base = archon.forward(x)
    return x, sa, archon.lcp(x, sa), bwt, base


def test_cap_rule(archon, naive, dna):
    _, _, lcp, bwt, base = dna
    L = archon.lib()
    want = naive(lcp, bwt, base, 1)[0]
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    assert L.archon_hip_repeats(archon._p(lcp), archon._p(bwt), bwt.size, base, 1, 1, 2, None, 0, tp, 0) == 0
    assert total.value == want.size > 1
    out = np.zeros(want.size, archon.REPEAT)
    out.view(np.uint32)[:] = 0xABABABAB
    untouched = out.copy()
    total.value = 0
    assert L.archon_hip_repeats(archon._p(lcp), archon._p(bwt), bwt.size, base, 1, 1, 2, archon._p(out), want.size - 1, tp, 0) == archon.E_ARG
    assert total.value == want.size and (out == untouched).all()
    assert L.archon_hip_repeats(archon._p(lcp), archon._p(bwt), bwt.size, base, 1, 1, 2, archon._p(out), want.size, tp, 0) == 0
    assert total.value == want.size and (out == want).all()
    # the device form: the same rule, nothing stored past the records
    import torch
    lcp_t, bwt_t = _cuda(lcp.view(np.int32)), _cuda(bwt)
    out_t = torch.full((4 * want.size,), -1, dtype=torch.int32, device="cuda:0")
    assert archon.repeats_dev(lcp_t, bwt_t, base, 1) == want.size
    with pytest.raises(archon.ArchonError) as e:
        archon.repeats_dev(lcp_t, bwt_t, base, 1, out_t=out_t[:4 * (want.size - 1)])
    assert e.value.code == archon.E_ARG and (out_t == -1).all()
    assert archon.repeats_dev(lcp_t, bwt_t, base, 1, out_t=out_t) == want.size
    assert (out_t.cpu().numpy().view(np.uint32).view(archon.REPEAT) == want).all()
    # one row: nothing to ask
    assert archon.repeats(np.zeros(1, np.uint32), np.zeros(1, np.uint8), 0).size == 0


def test_location_round_trip(archon, dna):
    """the starts of a repeat's occurrences are sa[lo:hi] - len, and what fm_locate finds for the repeat's own bytes; the same
    from a sampled index of the block"""
    x, sa, _, _, _ = dna
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    reps = blk.repeats(kind=1, min_len=9)
    assert 10 < reps.size < 20000
    want = [sa[r["lo"]:r["hi"]] - r["len"] for r in reps]
    got = blk.locate_repeats(reps)
    assert all((g == w).all() for g, w in zip(got, want))
    starts = [int(w[0]) for w in want]
    by_search = blk.fm_locate([x[s:s + int(r["len"])] for s, r in zip(starts, reps)])
    assert all(g.size == w.size and (g == w).all() for g, w in zip(by_search, want))
    f = blk.fm_index(32)
    got = f.locate_repeats(reps)
    assert all((g == w).all() for g, w in zip(got, want))
    supers = blk.repeats(kind=2)
    assert supers.size and set(map(tuple, supers.tolist())) <= set(map(tuple, blk.repeats(kind=1).tolist()))
    f.close()
    blk.close()


def test_statistics_stay_apart(archon, dna):
    x, sa, lcp, bwt, base = dna
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    blk.fm_count([b"ACGT"])
    archon.lcp(x, sa)
    before = (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.stats_raw()))
    archon.repeats(lcp, bwt, base, kind=2)
    st = archon.repeat_stats()
    assert st.ms_lcp == 0 and st.ms_count > 0 and st.ms_emit > 0 and st.kernel_launches == st.levels + 3 and st.host_syncs == 2
    archon.repeats(lcp, bwt, base, kind=1, count_only=True)
    st = archon.repeat_stats()
    assert st.kernel_launches == st.levels + 4 and st.host_syncs == 1 and st.ms_emit == 0
    assert before == (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.stats_raw()))
    blk.repeats()
    assert archon.lcp_stats().n == x.size and bytes(archon.fm_stats()) == before[1] and bytes(archon.stats_raw()) == before[2]
    blk.forward(x, want_sa=False)
    with pytest.raises(archon.ArchonError) as e:
        blk.repeats()
    assert e.value.code == archon.E_ARG
    blk.close()


def test_two_contexts_concurrently(archon, naive):
    blocks = [S.gen_shape("text", MiB + 1), S.gen_shape("motif_defects", MiB + 5)]
    solo = []
    for x in blocks:
        blk = archon.Block()
        blk.forward(x, want_sa=True)
        solo.append(blk.repeats(kind=1, min_len=4))
        blk.close()
    assert solo[0].size != solo[1].size
    got, stats, errors = [None, None], [None, None], []

    def run(k):
        try:
            archon.bind_context(k)
            blk = archon.Block()
            blk.forward(blocks[k], want_sa=True)
            for _ in range(3):
                got[k] = blk.repeats(kind=1, min_len=4)
                stats[k] = archon.repeat_stats()
                assert (got[k] == solo[k]).all()
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
        assert (got[k] == solo[k]).all()
        assert stats[k].n == blocks[k].size and stats[k].repeats == solo[k].size


def test_garbage_lcp(archon, naive):
    """random words are the LCP array of nothing: ARCHON_OK, every record inside the block, at most n - 1 of them.  (The rule
    is a rule about the array, so the helper still says which.)"""
    n = 65536
    rng = np.random.default_rng(11)
    lcp = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    bwt = rng.integers(0, 4, n, dtype=np.uint8)
    for kind in (0, 1, 2):
        got = archon.repeats(lcp, bwt, 12345, kind)
        assert got.size <= n - 1
        assert (got["lo"] < got["row"]).all() and (got["row"] < got["hi"]).all() and (got["hi"] <= n).all()
        assert (got == naive(lcp, bwt, 12345, kind)[0]).all()
        assert archon.repeat_stats().probes <= _bound(n, DEFAULT_FAN)[0]


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, naive, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text and motif_defects at 65 536 (32 tiles: 32 and 11, 11, 10 trips):
    kinds 0, 1, 2 with both filters through Block.repeats against the helper, counting only and with the emit pass, byte-equal
    to the same calls without the route, with their counters, launches and host waits"""
    for shape in ("text", "motif_defects"):
        x = S.gen_shape(shape, 65536)
        blk = archon.Block()
        try:
            _, base = blk.forward(x, want_sa=True)
            lcp, bwt = blk.lcp(), blk.read_bwt()
            G.same_under(monkeypatch, grid, lambda: _check_kinds(archon, naive, blk, lcp, bwt, base, (0, 1, 2)))
        finally:
            blk.close()


@pytest.mark.parametrize("shape", ["a", "dna"])
def test_second_trip_at_the_product_grid(archon, naive, shape):
    """no route: 2048 * 2048 + 3 * 2048 + 5 rows are 2052 tiles, so workgroups 0-3 of the 2048 take a second tile and the
    last tile has 5 rows.  One byte: the counts of the three kinds and the one supermaximal record, as in
    test_worst_case_depth.  DNA: the maximal repeats emitted, against the helper, with its counters"""
    n = G.N2
    x = S.gen_shape(shape, n)
    blk = archon.Block()
    try:
        _, base = blk.forward(x, want_sa=True)
        assert blk.validate() == 1
        bound, levels = _bound(n, DEFAULT_FAN)
        if shape == "a":
            for kind, want in ((0, n - 1), (1, n - 1), (2, 1)):
                assert blk.repeats(kind, count_only=True) == want
                st = archon.repeat_stats()
                assert st.intervals == n - 1 and st.probes <= bound and st.levels == levels and st.longest == n - 1
                assert st.sum_lcp == n * (n - 1) // 2 and st.distinct_substrings == n
            assert blk.repeats(2).tolist() == [(0, 2, n - 1, 1)]
        else:
            lcp, bwt = blk.lcp(), blk.read_bwt()
            want, w_int, w_occ, w_long = naive(lcp, bwt, base, 1)
            got = blk.repeats(1)
            assert got.size == want.size > n // 8 and (got == want).all()
            st = archon.repeat_stats()
            assert (st.intervals, st.repeats, st.occurrences, st.longest) == (w_int, want.size, w_occ, w_long)
            assert st.probes <= bound and st.levels == levels
            assert st.distinct_substrings == n * (n + 1) // 2 - int(lcp[1:].astype(np.int64).sum())
    finally:
        blk.close()
