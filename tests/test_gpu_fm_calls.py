"""GPU: how many kernels every FM entry point launches and how often it waits for its stream (kernel_launches and
host_syncs of the statistics record the call keeps: fm_stats, fm_walk_stats, fm_approx_stats; include/archon_hip.h).  The
other FM tests pin results, order and work counters; this one pins the shape of each call, so that a change to the host
layer cannot add a launch or a wait unnoticed.  A wait is one host wait for the call's stream; the device-wide wait of an
arena that grows is not counted.

A record describes the last C call only, and Block.fm_locate, FmIndex.locate and approx(hits=True) may make two: the
cases that need one particular C call go through pyarchon.lib()."""
import ctypes

import numpy as np
import pytest

import archon_synth as S

pytestmark = pytest.mark.gpu

N = 256 << 10
RATE = 32
# FmIndex.sample by the LF walk over this block: 3 (LF table) + 2 (walk, rank init) + 8 (rank jumps over 32769 chains)
# + 1 (samples) + 6 (marks, directory, scan, SA samples): the figure the library reported for this block at the commit
# before the one that added this test
WALK_SAMPLE_LAUNCHES = 20


@pytest.fixture(scope="module")
def text():
    """the block, patterns that occur (24-byte substrings), and patterns that do not"""
    x = S.gen_prose(N, S.SEED_BASE + 6)
    rng = np.random.default_rng(11)
    found = [x[q:q + 24].tobytes() for q in rng.integers(0, N - 24, 6)]
    absent = [bytes([1, 2, 3, 254, 255, 0, 7, 9]), bytes(range(200, 216))]
    return x, found, absent


def _lw(st):
    print("   ", type(st).__name__, st.asdict())
    return st.kernel_launches, st.host_syncs


def _forward(archon, x, want_sa=True):
    b = archon.Block()
    _, base = b.forward(x, want_sa=want_sa)
    return b, base


def _raw(archon, pats):
    packed, off = archon._pack_patterns(pats)
    return packed, off, off.size - 1


def _total():
    t = ctypes.c_uint64(0)
    return t, ctypes.cast(ctypes.byref(t), ctypes.c_void_p)


def test_create_and_count(archon, text):
    import torch
    x, found, absent = text
    pats = found + absent
    b, base = _forward(archon, x, want_sa=False)
    bwt = b.read_bwt()
    b.close()
    f = archon.FmIndex(bwt, base)
    st = archon.fm_stats()
    assert _lw(st) == (3, 1) and st.built == 1
    lo, hi = f.count(pats)
    assert (hi[:len(found)] > lo[:len(found)]).all() and (hi[len(found):] == lo[len(found):]).all()
    st = archon.fm_stats()
    assert _lw(st) == (1, 2) and st.built == 0
    packed, off, k = _raw(archon, pats)
    p_t = torch.from_numpy(packed).to("cuda:0")
    o_t = torch.from_numpy(off.view(np.int32)).to("cuda:0")
    lo_t = torch.zeros(k, dtype=torch.int32, device="cuda:0")
    hi_t = torch.zeros(k, dtype=torch.int32, device="cuda:0")
    f.count_dev(p_t, o_t, lo_t, hi_t)
    assert _lw(archon.fm_stats()) == (1, 1)
    assert (lo_t.cpu().numpy().view(np.uint32) == lo).all() and (hi_t.cpu().numpy().view(np.uint32) == hi).all()
    f.close()


def test_block_count_and_locate(archon, text):
    x, found, absent = text
    b, _ = _forward(archon, x)
    try:
        lo, hi = b.fm_count(found)
        st = archon.fm_stats()
        assert _lw(st) == (4, 3) and st.built == 1
        b.fm_count(found)
        st = archon.fm_stats()
        assert _lw(st) == (1, 2) and st.built == 0
        pos = b.fm_locate(found)
        assert sum(p.size for p in pos) == int((hi - lo).sum()) > 0
        assert _lw(archon.fm_stats()) == (2, 3)
        pos = b.fm_locate(absent)
        assert sum(p.size for p in pos) == 0
        assert _lw(archon.fm_stats()) == (1, 3)
        # room for one start fewer than there are: the call ends after the count, with the total set
        packed, off, k = _raw(archon, found)
        want = int((hi - lo).sum())
        out = np.zeros(want, np.uint32)
        t, tp = _total()
        rc = archon.lib().archon_hip_block_fm_locate(b.h, archon._p(packed), archon._p(off), k, archon._p(out), want - 1, tp)
        assert rc == archon.E_ARG and t.value == want
        assert _lw(archon.fm_stats()) == (1, 2)
    finally:
        b.close()


def test_sample_locate_extract(archon, text):
    import torch
    x, found, absent = text
    b, base = _forward(archon, x)
    try:
        f = b.fm_index(RATE)
        st, wst = archon.fm_stats(), archon.fm_walk_stats()
        assert _lw(st) == (3, 1) and st.built == 1
        assert _lw(wst) == (7, 1) and wst.route == 1
        want = b.fm_locate(found + absent)
        bwt = b.read_bwt()
    finally:
        b.close()
    got = f.locate(found + absent)
    total = sum(p.size for p in want)
    assert total > 0 and all((g == w).all() for g, w in zip(got, want))
    st, wst = archon.fm_stats(), archon.fm_walk_stats()
    assert _lw(st) == (2, 3)
    assert _lw(wst) == (1, 3) and wst.walks == total
    starts, lengths = [0, 1000, N - 50, 77], [40, 1, 50, 0]
    out = f.extract(starts, lengths)
    assert all((o == x[a:a + m]).all() for o, a, m in zip(out, starts, lengths))
    assert _lw(archon.fm_walk_stats()) == (5, 2)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    out_t = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda:0")
    f.extract_dev(torch.tensor(np.array(starts, np.int32), device="cuda:0"), torch.tensor(off, device="cuda:0"), out_t)
    assert _lw(archon.fm_walk_stats()) == (5, 1)
    assert (out_t.cpu().numpy() == np.concatenate(out)).all()
    f.close()
    # the samples by the LF walk over the handle's own BWT
    g = archon.FmIndex(bwt, base)
    g.sample(RATE)
    wst = archon.fm_walk_stats()
    assert _lw(wst) == (WALK_SAMPLE_LAUNCHES, 2) and wst.route == 2
    g.close()


def test_approx(archon, text):
    import torch
    x, found, absent = text
    pats = found + absent
    b, base = _forward(archon, x)
    try:
        # the first FM call on the block: the table's build is this call's, and the FM record stays as it was
        archon.FmIndex(np.zeros(8, np.uint8), 0).close()
        before = archon.fm_stats().asdict()
        packed, off, k = _raw(archon, pats)
        nh, no = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        t, tp = _total()
        assert archon.lib().archon_hip_block_fm_approx(b.h, archon._p(packed), archon._p(off), k, 1, archon._p(nh), archon._p(no), None, 0, tp) == 0
        st = archon.fm_approx_stats()
        assert _lw(st) == (4, 2) and st.built == 1
        assert archon.fm_stats().asdict() == before
        f = b.fm_index(RATE)
        c_nh, c_no, none = f.approx(pats, 1, hits=False)
        st = archon.fm_approx_stats()
        assert none is None and (c_nh == nh).all() and _lw(st) == (1, 1) and st.built == 0
        nhits, nocc, h = f.approx(pats, 1)
        assert 0 < h.size <= 4 * k, "the wrapper's first guess holds the hits: one C call"
        assert _lw(archon.fm_approx_stats()) == (2, 3)
        nt = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        ct = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        ht = torch.zeros(4 * h.size, dtype=torch.int32, device="cuda:0")
        assert f.approx_dev(torch.tensor(packed, device="cuda:0"), torch.tensor(off.astype(np.int32), device="cuda:0"), 1, nt, ct, ht) == h.size
        assert _lw(archon.fm_approx_stats()) == (2, 2)
        via_sa = b.fm_locate_hits(pats, h)
        assert _lw(archon.fm_approx_stats()) == (1, 1)
        via_samples = f.locate_hits(pats, h)
        assert _lw(archon.fm_approx_stats()) == (1, 1)
        assert sum(p.size for p in via_sa) == int(nocc.sum()) and all((u == v).all() for u, v in zip(via_sa, via_samples))
        # hits without rows, and no hits at all: nothing to launch and nothing to wait for
        empty = h[:2].copy()
        empty["hi"] = empty["lo"]
        for hits in (empty, h[:0]):
            assert sum(p.size for p in b.fm_locate_hits(pats, hits)) == 0
            assert _lw(archon.fm_approx_stats()) == (0, 0)
            assert sum(p.size for p in f.locate_hits(pats, hits)) == 0
            assert _lw(archon.fm_approx_stats()) == (0, 0)
        f.close()
    finally:
        b.close()
