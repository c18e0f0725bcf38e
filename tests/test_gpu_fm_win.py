"""GPU: the windows of a row range in text order (include/archon_hip.h, archon_hip_fm_attach_wm, _block_fm_attach_wm,
_fm_win_count*, _select*, _list*) against tests/fm_win_naive.py, the definition in numpy: every count, item, record and
counter is equal to the model's.  The suffix array comes from the device forward (Block.fm_index(wm=True)) and, in a second
run, from the CPU oracle through attach_sa."""
import ctypes
import os

import numpy as np
import pytest

import archon_synth as S
import fm_win_naive as W
import stride_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 32
# L changes at a power of two, b = n + 1 = 2^L (63, 255, 511, 4095), a ragged last word, a ragged last 256-bit block, exact multiples
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4097, 70001)
KINDS = ("random", "a", "ab")
BIG = 70001
U32 = 0xFFFFFFFF


def _block(kind, n):
    if kind == "readme":
        return np.frombuffer(open(os.path.join(ROOT, "README.md"), "rb").read()[:6000], np.uint8).copy()
    return S.gen_shape(kind, n)


_refs = {}


def _reference(oracle, kind, n):
    """(x, sa, bwt, base) of the CPU oracle: computed once, shared, left unchanged"""
    if (kind, n) not in _refs:
        x = _block(kind, n)
        sa, bwt, base = oracle.forward(x)
        for a in (x, sa, bwt):
            a.setflags(write=False)
        _refs[kind, n] = (x, sa, bwt, int(base))
    return _refs[kind, n]


def _queries(n, seed):
    """(lo, hi, a, b) as uint32 arrays.  n <= 65: every (lo, hi) with every window a <= b drawn from {0, 1, n, n + 1} and two
    random ones.  Otherwise 4096 random queries of 1 to 4096 rows, one in 256 of up to all rows, and the edges: lo = hi, [0, n),
    single rows, a = b, windows below and above every item, lo and hi at multiples of 64 and 256 and one to either side"""
    rng = np.random.default_rng(seed)
    q = []
    if n <= 65:
        fixed = sorted({0, 1, n, n + 1})
        wins = [(a, b) for a in fixed for b in fixed if a <= b]
        for lo in range(n + 1):
            for hi in range(lo, n + 1):
                a, b = sorted(int(v) for v in rng.integers(0, n + 2, 2))
                c, d = sorted(int(v) for v in rng.integers(0, n + 2, 2))
                q += [(lo, hi, a_, b_) for a_, b_ in wins + [(a, b), (c, d)]]
    else:
        for j in range(4096):
            lo = int(rng.integers(0, n))
            hi = lo + int(min(n - lo, np.exp(rng.uniform(0, np.log(n if j % 256 == 0 else min(n, 4096))))))
            a, b = sorted(int(v) for v in rng.integers(0, n + 2, 2))
            if rng.integers(0, 8) == 0:
                a = 0
            if rng.integers(0, 8) == 0:
                b = n + 1
            q.append((lo, hi, a, b))
        q += [(0, 0, 0, n + 1), (n, n, 0, n + 1), (n // 2, n // 2, 1, n), (0, n, 0, n + 1), (0, n, 1, n), (0, n, n // 3, 2 * n // 3)]
        q += [(r, r + 1, 0, n + 1) for r in (0, 1, n // 2, n - 1)] + [(r, r + 1, 3, n - 2) for r in (0, 63, 64, 255, 256, n - 1)]
        q += [(0, n, v, v) for v in (0, 1, n // 2, n, n + 1)] + [(5, n - 5, 0, 0), (5, n - 5, n + 1, n + 1), (5, n - 5, 0, 1), (5, n - 5, n, n + 1)]
        edges = sorted({v + d for m in (64, 256) for v in range(m, min(n, 4 * m) + 1, m) for d in (-1, 0, 1)} |
                       {v + d for v in (n // 256 * 256, n // 64 * 64) for d in (-1, 0, 1)})
        edges = [e for e in edges if 0 <= e <= n]
        near, far = [e for e in edges if e <= 1025], [e for e in edges if e > 1025]
        q += [(lo, hi, 2, n - 1) for lo in near for hi in near if lo <= hi] + [(lo, hi, 2, n - 1) for lo in far for hi in far if lo <= hi]
        q += [(lo, hi, 2, n - 1) for lo in near[:3] for hi in far]
    q = [v for v in q if W.valid(n, *v)]            # (at 255 and 257 some of the fixed edges lie past n)
    lo, hi, a, b = (np.array(v, np.uint32) for v in zip(*q))
    return lo, hi, a, b


def _idx(cnt, seed):
    """select indices: 0, count - 1, count, 2^32 - 1 and a random one below the count, in turn"""
    rng = np.random.default_rng(seed)
    c = cnt.astype(np.int64)
    pick = np.stack([np.zeros_like(c), c - 1, c, np.full_like(c, U32), (rng.random(c.size) * c).astype(np.int64)])
    return (pick[np.arange(c.size) % 5, np.arange(c.size)] & U32).astype(np.uint32)


def _dev(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _zeros(n):
    import torch
    return torch.zeros(max(n, 1), dtype=torch.int32, device="cuda:0")


def _host(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def _stats(archon, n, k, most, c, attached=0):
    """the record of the last window call against the model's counters"""
    st = archon.fm_win_stats()
    got = {key: getattr(st, key) for key in ("n", "levels", "ranges", "most", "attached", "rows", "in_window", "listed", "walks", "wm_bytes")}
    want = dict(n=n, levels=W.levels(n), ranges=k, most=most, attached=attached, rows=c["rows"], in_window=c["in_window"], listed=c["listed"],
                walks=c["walks"], wm_bytes=W.wm_bytes(n))
    assert got == want
    return st


def _same_recs(got, want):
    assert got.size == want.size
    assert (got["range"] == want["range"]).all() and (got["item"] == want["item"]).all()


def _model(sa, q, idx_seed):
    """what every call of _check_handle must give: computed once per block and query set"""
    lo, hi, a, b = q
    n = len(sa)
    wins = W.windows(sa, lo, hi, a, b)
    cnt, cc = W.count(sa, lo, hi, a, b, wins=wins)
    idx = _idx(cnt, idx_seed)
    return {"count": (cnt, cc), "idx": idx, "select": W.select(sa, lo, hi, idx, a, b, wins=wins), "whole": W.listing(sa, lo, hi, None, None, 2),
            "lists": {most: W.listing(sa, lo, hi, a, b, most, wins=wins) for most in (0, 1, 3, n + 5)},
            "noemit": W.listing(sa, lo, hi, a, b, 3, emit=False, wins=wins)}


def _check_handle(archon, f, n, q, m, dev_forms):
    lo, hi, a, b = q
    k = lo.size
    cnt, cc = m["count"]
    assert (f.win_count(lo, hi, a, b) == cnt).all()
    _stats(archon, n, k, 0, cc)
    item, cs = m["select"]
    assert (f.win_select(lo, hi, m["idx"], a, b) == item).all()
    _stats(archon, n, k, 0, cs)
    for most, (wc, wr, wl) in m["lists"].items():
        gc, gr = f.win_list(lo, hi, a, b, most=most)
        assert (gc == wc).all()
        _same_recs(gr, wr)
        _stats(archon, n, k, most, wl)
    wc, _, wl = m["noemit"]
    gc, none = f.win_list(lo, hi, a, b, most=3, emit=False)
    assert none is None and (gc == wc).all()
    _stats(archon, n, k, 3, wl)
    # no window: the whole block
    wc, wr, wl = m["whole"]
    gc, gr = f.win_list(lo, hi, most=2)
    assert (gc == wc).all() and (f.win_count(lo, hi) == wc).all()
    _same_recs(gr, wr)
    if not dev_forms:
        return
    lo_t, hi_t, a_t, b_t, idx_t = _dev(lo), _dev(hi), _dev(a), _dev(b), _dev(m["idx"])
    out_t = _zeros(k)
    f.win_count_dev(lo_t, hi_t, out_t, a_t, b_t)
    assert (_host(out_t, k) == cnt).all()
    _stats(archon, n, k, 0, cc)
    out_t.zero_()
    f.win_select_dev(lo_t, hi_t, idx_t, out_t, a_t, b_t)
    assert (_host(out_t, k) == item).all()
    _stats(archon, n, k, 0, cs)
    wc, wr, wl = m["lists"][3]
    rec_t = _zeros(2 * wr.size)
    out_t.zero_()
    assert f.win_list_dev(lo_t, hi_t, out_t, rec_t, a_t, b_t, most=3) == wr.size
    assert (_host(out_t, k) == wc).all()
    _same_recs(_host(rec_t, 2 * wr.size).view(archon.FM_WIN), wr)
    _stats(archon, n, k, 3, wl)
    out_t.zero_()
    assert f.win_list_dev(lo_t, hi_t, out_t, None, a_t, b_t, most=3) == wr.size
    assert (_host(out_t, k) == wc).all()
    _stats(archon, n, k, 3, m["noemit"][2])
    wc, wr, wl = m["whole"]
    rec_t = _zeros(2 * wr.size)
    assert f.win_list_dev(lo_t, hi_t, out_t, rec_t, most=2) == wr.size
    _same_recs(_host(rec_t, 2 * wr.size).view(archon.FM_WIN), wr)


_ZERO = dict(rows=0, in_window=0, listed=0, walks=0)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(archon, oracle, n):
    """random bytes, one byte repeated and `ab` repeated at every size: the matrix from the device forward's suffix array (the
    block form), then from the oracle's through attach_sa; host forms on every block, device forms on the random one"""
    for kind in KINDS:
        x, sa, bwt, base = _reference(oracle, kind, n)
        q = _queries(n, n + len(kind))
        m = _model(sa, q, n)
        blk = archon.Block()
        try:
            got_sa, got_base = blk.forward(x)
            assert (got_sa == sa).all() and got_base == base
            f = blk.fm_index(RATE, wm=True)
            _stats(archon, n, 0, 0, _ZERO, attached=1)
            _check_handle(archon, f, n, q, m, dev_forms=kind == "random")
            f.close()
        finally:
            blk.close()
        f = archon.FmIndex(bwt, base).attach_sa(sa).attach_wm()
        try:
            _stats(archon, n, 0, 0, _ZERO, attached=1)
            _check_handle(archon, f, n, q, m, dev_forms=False)
        finally:
            f.close()


def test_readme_and_pattern_conveniences(archon, oracle):
    """6000 bytes of the README: the queries, then first() and locate_sorted() against sorted(fm_locate) for patterns that occur
    once, often and never"""
    x, sa, bwt, base = _reference(oracle, "readme", 6000)
    n = x.size
    q = _queries(n, 17)
    blk = archon.Block()
    try:
        blk.forward(x)
        f = blk.fm_index(RATE, wm=True)
        _check_handle(archon, f, n, q, _model(sa, q, 17), dev_forms=True)
        rng = np.random.default_rng(6000)
        pats = [b"e", b" ", b"th", b"the ", b"\n", x[:40].tobytes(), x[n - 9:].tobytes(), b"\x01\x02", b"zzzzqzzzz"]
        pats += [x[s:s + m].tobytes() for s, m in zip(rng.integers(0, n - 12, 12), rng.integers(1, 12, 12))]
        want = [np.sort(p) for p in blk.fm_locate(pats)]
        assert min(w.size for w in want) == 0 and max(w.size for w in want) > 100
        for most in (0, 1, 10):
            got = f.locate_sorted(pats, most=most)
            for g, w in zip(got, want):
                assert g.dtype == np.uint32 and (g == (w[:most] if most else w)).all()
        for after in (0, 1, 777, n - 20, n):
            got = f.first(pats, after=after)
            assert got.tolist() == [int(w[w >= after][0]) if (w >= after).any() else -1 for w in want]
        f.close()
    finally:
        blk.close()


def test_refusals(archon, oracle):
    """lo > hi, hi > n, a > b, b > n + 1, one of a and b NULL, a cap too small with out untouched, a handle without a matrix,
    an attach without a suffix array, a second attach in place of the first: ARCHON_E_ARG each time, on the host forms before
    anything runs and on the device forms from the kernel's flag, and the handle answers as before afterwards"""
    n = 513
    x, sa, bwt, base = _reference(oracle, "random", n)
    L = archon.lib()
    E = archon.E_ARG
    p = lambda v: ctypes.c_void_p(v.ctypes.data)       # noqa: E731
    tp = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    u = lambda *v: np.array(v, np.uint32)              # noqa: E731
    good = (u(0, 5, 100), u(n, 300, 101), u(0, 7, 0), u(n + 1, 400, n + 1))
    want_cnt, want_recs, _ = W.listing(sa, *good)
    f = archon.FmIndex(bwt, base)
    try:
        cnt = np.full(3, 9, np.uint32)
        assert L.archon_hip_fm_win_count(f.h, p(good[0]), p(good[1]), p(good[2]), p(good[3]), 3, p(cnt)) == E
        assert b"no wavelet matrix" in L.archon_hip_last_error()
        assert L.archon_hip_fm_attach_wm(f.h) == E and b"no suffix array" in L.archon_hip_last_error()
        f.attach_sa(sa)
        assert (f.count([x[:3].tobytes()])[1] > 0).all()         # the handle without a matrix behaves as before
        f.attach_wm()

        def still_fine():
            gc, gr = f.win_list(*good)
            assert (gc == want_cnt).all()
            _same_recs(gr, want_recs)

        still_fine()
        # a refused attach leaves the earlier matrix in place: the block form with a handle that is not of the block
        other = archon.Block()
        try:
            other.forward(_reference(oracle, "random", 512)[0])
            assert L.archon_hip_block_fm_attach_wm(other.h, f.h) == E and b"is not of this block" in L.archon_hip_last_error()
            assert L.archon_hip_block_fm_attach_wm(None, f.h) == E
        finally:
            other.close()
        still_fine()
        bad = [(u(6), u(5), u(0), u(9)), (u(0), u(n + 1), u(0), u(9)), (u(0), u(5), u(9), u(8)), (u(0), u(5), u(0), u(n + 2))]
        total = ctypes.c_uint64(7)
        tot = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
        recs = np.zeros(8, archon.FM_WIN)
        for lo, hi, a, b in bad:
            # the bad query last of three, so that the good ones in front of it would have answered
            lo3, hi3, a3, b3 = (np.concatenate([g[:2], v]) for g, v in zip(good, (lo, hi, a, b)))
            cnt[:] = 9
            assert L.archon_hip_fm_win_count(f.h, p(lo3), p(hi3), p(a3), p(b3), 3, p(cnt)) == E
            assert L.archon_hip_fm_win_select(f.h, p(lo3), p(hi3), p(a3), p(b3), p(lo3), 3, p(cnt)) == E
            total.value = 7
            assert L.archon_hip_fm_win_list(f.h, p(lo3), p(hi3), p(a3), p(b3), 3, 0, p(cnt), p(recs), 8, tot) == E and total.value == 0
            assert (cnt == 9).all() and not recs.view(np.uint32).any()
            t = [_dev(v) for v in (lo3, hi3, a3, b3)]
            out_t, rec_t = _zeros(3), _zeros(16)
            s = archon._stream_ptr()
            assert L.archon_hip_fm_win_count_dev(f.h, tp(t[0]), tp(t[1]), tp(t[2]), tp(t[3]), 3, tp(out_t), s) == E
            assert b"a query is not lo <= hi <= 513, a <= b <= 514" in L.archon_hip_last_error()
            assert L.archon_hip_fm_win_select_dev(f.h, tp(t[0]), tp(t[1]), tp(t[2]), tp(t[3]), tp(t[0]), 3, tp(out_t), s) == E
            total.value = 7
            assert L.archon_hip_fm_win_list_dev(f.h, tp(t[0]), tp(t[1]), tp(t[2]), tp(t[3]), 3, 0, tp(out_t), tp(rec_t), 8, tot, s) == E
            assert total.value == 0 and not _host(rec_t, 16).any()
            still_fine()
        # one of a and b alone
        for a_, b_ in ((p(good[2]), None), (None, p(good[3]))):
            assert L.archon_hip_fm_win_count(f.h, p(good[0]), p(good[1]), a_, b_, 3, p(cnt)) == E
            assert L.archon_hip_fm_win_select(f.h, p(good[0]), p(good[1]), a_, b_, p(good[0]), 3, p(cnt)) == E
            total.value = 7
            assert L.archon_hip_fm_win_list(f.h, p(good[0]), p(good[1]), a_, b_, 3, 0, p(cnt), p(recs), 8, tot) == E and total.value == 0
            assert b"both given or both null" in L.archon_hip_last_error()
        # the cap rule: too small with records asked for is ARCHON_E_ARG with *total and count written and out untouched;
        # NULL is counts only; k = 0 writes *total = 0 and nothing else
        big = np.zeros(want_recs.size, archon.FM_WIN)
        assert L.archon_hip_fm_win_list(f.h, p(good[0]), p(good[1]), p(good[2]), p(good[3]), 3, 0, p(cnt), p(big), want_recs.size - 1, tot) == E
        assert total.value == want_recs.size and (cnt == want_cnt).all() and not big.view(np.uint32).any()
        big_t = _zeros(2 * want_recs.size)
        t = [_dev(v) for v in good]
        assert L.archon_hip_fm_win_list_dev(f.h, tp(t[0]), tp(t[1]), tp(t[2]), tp(t[3]), 3, 0, tp(out_t), tp(big_t), want_recs.size - 1, tot,
                                            archon._stream_ptr()) == E
        assert total.value == want_recs.size and not _host(big_t, 2 * want_recs.size).any()
        total.value = 7
        assert L.archon_hip_fm_win_list(f.h, p(good[0]), p(good[1]), p(good[2]), p(good[3]), 3, 0, p(cnt), None, 0, tot) == 0
        assert total.value == want_recs.size
        cnt[:] = 9
        total.value = 7
        assert L.archon_hip_fm_win_list(f.h, p(good[0]), p(good[1]), p(good[2]), p(good[3]), 0, 0, p(cnt), p(big), 0, tot) == 0
        assert total.value == 0 and (cnt == 9).all()
        still_fine()
        # a second attach replaces the first: the matrix of another array of the same size answers for that array
        sa2 = np.roll(sa, 7)
        f.attach_sa(sa2)
        still_fine()                                    # the matrix keeps what it made
        f.attach_wm()
        _stats(archon, n, 0, 0, _ZERO, attached=1)
        gc, gr = f.win_list(*good)
        wc, wr, _ = W.listing(sa2, *good)
        assert (gc == wc).all() and wr.tobytes() != want_recs.tobytes()
        _same_recs(gr, wr)
    finally:
        f.close()


def _big_case(oracle):
    x, sa, bwt, base = _reference(oracle, "random", BIG)
    q = _queries(BIG, 5)
    if "big" not in _refs:
        _refs["big"] = _model(sa, q, 5)
    return x, sa, bwt, base, q, _refs["big"]


@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, oracle, grid, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) over the 70 001-byte case: the attach is inside the call, so the build
    kernels take their later trips too (274 blocks on 1 or 3 workgroups), as do the queries; byte-equal to the same calls without
    the route, with their counters"""
    x, sa, bwt, base, q, m = _big_case(oracle)
    lo, hi, a, b = q
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    try:
        def call():
            f.attach_wm()
            stats = [archon.fm_win_stats()]
            cnt = f.win_count(lo, hi, a, b)
            stats.append(archon.fm_win_stats())
            item = f.win_select(lo, hi, m["idx"], a, b)
            stats.append(archon.fm_win_stats())
            lc, recs = f.win_list(lo, hi, a, b, most=3)
            stats.append(archon.fm_win_stats())
            assert (cnt == m["count"][0]).all() and (item == m["select"][0]).all() and (lc == cnt).all()
            _same_recs(recs, m["lists"][3][1])
            return [cnt, item, lc, recs], stats

        G.same_under(monkeypatch, grid, call)
    finally:
        f.close()


def test_second_trip_at_the_product_grid(archon, oracle):
    """no route.  The build at stride_util.N2 rows: 16 409 blocks of 256, so workgroups 0 .. 24 of the 2048 take a ninth block;
    2048 random queries against numpy.  The queries at 2048 * 256 + 3 * 256 + 5 of them on the 70 001-byte block: lanes of the
    first workgroups take a second query, the last workgroup has 5; they are the case's query set over and over, so the model
    answers once"""
    n = G.N2
    x = S.gen_shape("dna", n)
    blk = archon.Block()
    try:
        sa, _ = blk.forward(x)
        f = blk.fm_index(RATE, wm=True)
        st = _stats(archon, n, 0, 0, _ZERO, attached=1)
        assert st.levels == 23
        rng = np.random.default_rng(n)
        lo = rng.integers(0, n - 70000, 2048).astype(np.uint32)
        hi = (lo + np.exp(rng.uniform(0, np.log(60000), 2048)).astype(np.uint32)).astype(np.uint32)
        lo[:2], hi[:2] = (0, n // 2), (n, n)
        ab = np.sort(rng.integers(0, n + 2, (2, 2048)), axis=0).astype(np.uint32)
        cnt, cc = W.count(sa, lo, hi, ab[0], ab[1])
        assert (f.win_count(lo, hi, ab[0], ab[1]) == cnt).all()
        _stats(archon, n, 2048, 0, cc)
        idx = _idx(cnt, 3)
        item, cs = W.select(sa, lo, hi, idx, ab[0], ab[1])
        assert (f.win_select(lo, hi, idx, ab[0], ab[1]) == item).all() and item.any()
        _stats(archon, n, 2048, 0, cs)
        f.close()
    finally:
        blk.close()
    K = 2048 * 256 + 3 * 256 + 5
    x, sa, bwt, base, q, m = _big_case(oracle)
    k0 = q[0].size
    rep = lambda v: np.resize(v, K)         # noqa: E731
    lo, hi, a, b = (rep(v) for v in q)
    f = archon.FmIndex(bwt, base).attach_sa(sa).attach_wm()
    try:
        # the counters of the K queries: the per-query terms of the model's, each as often as its query is repeated -- what every
        # wave posts after its lanes' trips
        per = {"rows": q[1].astype(np.int64) - q[0], "in_window": m["count"][0].astype(np.int64),
               "walks": np.array([W.bound_walks(BIG, *(int(v[j]) for v in q)) for j in range(k0)], np.int64)}
        cc = {key: int(rep(v).sum()) for key, v in per.items()}
        assert (f.win_count(lo, hi, a, b) == rep(m["count"][0])).all()
        _stats(archon, BIG, K, 0, dict(cc, listed=0))
        assert (f.win_select(lo, hi, rep(m["idx"]), a, b) == rep(m["select"][0])).all()
        _stats(archon, BIG, K, 0, dict(cc, listed=0, walks=cc["walks"] + int(np.count_nonzero(rep(m["select"][0])))))
        wc, wr, _ = m["lists"][1]
        gc, gr = f.win_list(lo, hi, a, b, most=1)
        listed = int(np.minimum(rep(wc), 1).sum())
        assert (gc == rep(wc)).all() and gr.size == listed
        _stats(archon, BIG, K, 1, dict(cc, listed=listed, walks=cc["walks"] + listed))
        full, part = divmod(K, k0)
        first = wr["range"] < part
        assert (gr["item"] == np.concatenate([np.tile(wr["item"], full), wr["item"][first]])).all()
        assert (gr["range"] == np.flatnonzero(rep(wc))).all()
    finally:
        f.close()


def test_calls(archon, oracle):
    """kernel launches and host waits of attach, count, select and list as functions of L alone, equal on two runs.  A wait is
    one host wait for the call's stream; the arena holds each call without growing after the first run.  Step by step
    (fm_host.hiph):
      fmwin_attach_run   per level the bits kernel and the scan of the block popcounts (1 + 3), and but for the last level the
                         scatter (1): 5 L - 1 launches; one wait at the end
      fmwin_run          count or select: the kernel (1); one wait for the counters, with which a host form's answers travel
                         list: the count kernel and the scan of min(count, most) (1 + 3); one wait for the counters and the
                         total; with records that fit the emit kernel (1) and one wait for them"""
    x, sa, bwt, base, q, m = _big_case(oracle)
    lo, hi, a, b = q
    L = W.levels(BIG)
    assert L == 17
    f = archon.FmIndex(bwt, base).attach_sa(sa)
    lw = lambda: (archon.fm_win_stats().kernel_launches, archon.fm_win_stats().host_syncs)       # noqa: E731
    try:
        lo_t, hi_t, a_t, b_t, idx_t = (_dev(v) for v in (lo, hi, a, b, m["idx"]))
        out_t, rec_t = _zeros(lo.size), _zeros(2 * m["lists"][3][1].size)
        seen = []
        for run in range(3):
            got = []
            f.attach_wm()
            got.append(lw())
            f.win_count(lo, hi, a, b)
            got.append(lw())
            f.win_count_dev(lo_t, hi_t, out_t, a_t, b_t)
            got.append(lw())
            f.win_select(lo, hi, m["idx"], a, b)
            got.append(lw())
            f.win_select_dev(lo_t, hi_t, idx_t, out_t, a_t, b_t)
            got.append(lw())
            f.win_list(lo, hi, a, b, most=3, emit=False)
            got.append(lw())
            f.win_list_dev(lo_t, hi_t, out_t, None, a_t, b_t, most=3)
            got.append(lw())
            recs = np.zeros(m["lists"][3][1].size, archon.FM_WIN)
            total = ctypes.c_uint64(0)
            cnt = np.zeros(lo.size, np.uint32)
            p = lambda v: ctypes.c_void_p(v.ctypes.data)       # noqa: E731
            assert archon.lib().archon_hip_fm_win_list(f.h, p(lo), p(hi), p(a), p(b), lo.size, 3, p(cnt), p(recs), recs.size,
                                                       ctypes.cast(ctypes.byref(total), ctypes.c_void_p)) == 0
            got.append(lw())
            f.win_list_dev(lo_t, hi_t, out_t, rec_t, a_t, b_t, most=3)
            got.append(lw())
            if run:                                     # (the first run grows the arena where it has to)
                seen.append(got)
        want = [(5 * L - 1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (4, 1), (4, 1), (5, 2), (5, 2)]
        assert seen[0] == want and seen[1] == want
        g = None
        blk = archon.Block()
        try:
            blk.forward(x)
            g = blk.fm_index(RATE, wm=True)
            assert lw() == (5 * L - 1, 1)
        finally:
            if g:
                g.close()
            blk.close()
    finally:
        f.close()


def _snapshot(archon):
    """the counters of the calling thread's last call of every other family: every *_stats getter pyarchon has but the windows'
    own, and stats() of the transforms; a family with no record gives its refusal text"""
    names = sorted(k for k in dir(archon) if k.endswith("_stats") and not k.startswith("_") and k != "fm_win_stats" and callable(getattr(archon, k)))
    snap = {}
    for name in names + ["stats"]:
        try:
            snap[name] = G.counters(getattr(archon, name)())
        except archon.ArchonError as e:
            snap[name] = str(e)
    return snap


def test_other_families_are_left_alone(archon, oracle):
    """one small call of every other family on this thread, then the window calls of every form on a handle that also holds a
    mirror, an LCP array, a suffix array and documents: the record of every other family is what it was, and the other parts
    of the handle answer as before"""
    n = 4097
    x, sa, bwt, base = _reference(oracle, "random", n)
    lo, hi, a, b = _queries(n, 9)
    bounds = np.array([0, 1000, 3000, n], np.uint32)
    pats = [x[100:124].tobytes(), x[2000:2024].tobytes(), x[7:10].tobytes()]
    text = np.concatenate([x[300:700], x[50:90]])
    blk = archon.Block()
    try:
        blk.forward(x)
        blk.lcp()
        blk.fm_count(pats)
        f = blk.fm_index(RATE, mirror=True, sa=True, docs=bounds, lcp=True)
        f.approx(pats, 1)
        f.classes(pats, archon.classes_identity())
        f.edit(pats[:2], 1)
        f.locate(pats)
        blk.repeats()
        blk.lz()
        blk.kmers(4)
        blk.maws()
        blk.entropy([0, 1])
        blk.runs()

        def parts():
            plo, phi = f.count(pats)
            return [plo, phi] + list(f.smems(pats)) + list(f.ms(pats)) + list(f.ms_text(text)) + list(f.docs(pats))

        answers = parts()
        before = _snapshot(archon)
        assert all(isinstance(v, dict) for v in before.values()), [k for k, v in before.items() if not isinstance(v, dict)]
        assert len(before) >= 17
        assert archon.lib().archon_hip_block_fm_attach_wm(blk.h, f.h) == 0
        f.attach_wm()
        cnt = f.win_count(lo, hi, a, b)
        idx = np.zeros(lo.size, np.uint32)
        f.win_select(lo, hi, idx, a, b)
        f.win_list(lo, hi, a, b, most=3)
        f.win_list(lo, hi, a, b, most=3, emit=False)
        lo_t, hi_t, a_t, b_t, idx_t, out_t = _dev(lo), _dev(hi), _dev(a), _dev(b), _dev(idx), _zeros(lo.size)
        f.win_count_dev(lo_t, hi_t, out_t, a_t, b_t)
        f.win_select_dev(lo_t, hi_t, idx_t, out_t, a_t, b_t)
        f.win_list_dev(lo_t, hi_t, out_t, _zeros(6 * lo.size), a_t, b_t, most=3)
        assert (cnt == W.count(sa, lo, hi, a, b)[0]).all()
        assert _snapshot(archon) == before
        again = parts()
        assert len(again) == len(answers) and all(G._bytes(u) == G._bytes(v) for u, v in zip(again, answers))
        f.close()
    finally:
        blk.close()


def test_memory_returns(archon):
    """the device memory of the matrix is back after destroy.  The library keeps no account of what it owns that a caller can
    read, so this compares the device's free memory (torch.cuda.mem_get_info): at 4 MiB the matrix is 13.6 MiB, and after the
    handle is destroyed the free figure is within a quarter of that of what it was before the handle was made -- a quarter of
    what a leak of the matrix would take, and wide enough for an allocator that rounds; after a second attach the handle holds
    at most one and a half matrices more than without one.  The arena has grown to what
    the attach takes before the first figure is read"""
    import torch
    n = 4 << 20
    slack = W.wm_bytes(n) // 4
    blk = archon.Block()
    try:
        blk.forward(S.gen_shape("random", n), want_sa=True)
        blk.fm_index(RATE, wm=True).close()
        free0 = torch.cuda.mem_get_info()[0]
        f = blk.fm_index(RATE)
        bare = free0 - torch.cuda.mem_get_info()[0]
        attach = lambda: archon._check(archon.lib().archon_hip_block_fm_attach_wm(blk.h, f.h))      # noqa: E731
        attach()
        assert archon.fm_win_stats().wm_bytes == W.wm_bytes(n)
        attach()                                        # replaces: the first matrix is freed
        held = free0 - torch.cuda.mem_get_info()[0] - bare
        f.close()
        back = free0 - torch.cuda.mem_get_info()[0]
        print("    free before %d; the handle %d, its matrix %d (wm_bytes %d); short after destroy %d" % (free0, bare, held, W.wm_bytes(n), back))
        assert held <= W.wm_bytes(n) + 2 * slack        # one matrix, not two
        assert back <= slack
    finally:
        blk.close()
