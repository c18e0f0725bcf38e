"""GPU: the k-mers of a block, the count of the k-mer at every position and the shortest unique substrings (archon_hip_kmers*,
archon_hip_kmer_occ*, archon_hip_sus*; include/archon_hip.h) against answers made from the text alone (tests/kmers_naive.py,
pinned by test_kmers_abi.py): records and order, the histogram, the counters and their invariants, stores that stay inside the
outputs, the cap rule, locating and document frequency through the existing calls, the statistics, and bad input."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import kmers_naive as K
import repeats_naive as R
import stride_util as G

pytestmark = pytest.mark.gpu

MiB = 1 << 20
DEFAULT_TILE = 2048             # kmers.hiph kDefaultTile: T when no test route names one
SENT = 0xA5A5A5A5
PARTS = 8


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _odd(t):
    """the same values at an odd device address (one element past an allocation's start)"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def _tp(total):
    return ctypes.cast(ctypes.byref(total), ctypes.c_void_p)


@pytest.fixture(scope="module")
def tiny():
    """every string of length 1-7 over {0, 1, 255}: (x, sa, lcp, sus, {k: (records, occ)} for k in 1 .. n+1), all from the
    text (the arrays by the definition, tests/repeats_naive.a7_arrays)"""
    out = []
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            sa, lcp, _, _ = R.a7_arrays(x)
            per_k = {k: (K.kmers_text(x, k, sa)[0], K.occ_text(x, k)) for k in range(1, n + 2)}
            out.append((x, np.array(sa, np.uint32), np.array(lcp, np.uint32), K.sus_text(x), per_k))
    return out


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("tile", [4, 0])
def test_exhaustive_tiny(archon, tiny, tile, part, monkeypatch):
    """every string of length 1-7 over {0, 1, 255} (in eight parts), every k in 1 .. n+1, through the host forms and the _dev
    forms (every other string at odd device addresses), with tiles of 4 rows (seven rows cross a tile boundary) and the default:
    records and order, occ, sus, the histogram with 2 and 5 bins (one through each form), and sentinel words behind every output"""
    import torch
    if tile:
        monkeypatch.setenv("ARCHON_KMER_TILE", str(tile))
    L = archon.lib()
    p = archon._p
    total = ctypes.c_uint64(0)
    for i, (x, sa, lcp, sus, per_k) in enumerate(tiny):
        if i % PARTS != part:
            continue
        n = len(x)
        sa_t, lcp_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32))
        if i % 2:
            sa_t, lcp_t = _odd(sa_t), _odd(lcp_t)
        # sus: host, then device
        buf = np.full(n + 1, SENT, np.uint32)
        archon._check(L.archon_hip_sus(p(sa), p(lcp), n, p(buf), 0))
        assert buf[:n].tolist() == sus.tolist() and buf[n] == SENT, x
        st = archon.kmer_stats()
        assert (st.what, st.n, st.tile) == (2, n, tile or DEFAULT_TILE)
        buf_t = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda:0")
        archon.sus_dev(sa_t, lcp_t, buf_t[1:n + 1])
        got = buf_t.cpu().numpy().view(np.uint32)
        assert got[1:n + 1].tolist() == sus.tolist() and got[0] == got[n + 1] == 0xFFFFFFFF, x
        for k in range(1, n + 2):
            want, occ = per_k[k]
            sizes = want["hi"].astype(np.int64) - want["lo"]
            words = max(n - k + 1, 0)
            bins_h, bins_d = (5, 2) if (i + k) % 2 else (2, 5)
            # host forms: count and emit in one call with room for n records
            out = np.zeros(n + 1, archon.KMER)
            out.view(np.uint32)[:] = SENT
            hist = np.full(bins_h + 1, SENT, np.uint32)
            archon._check(L.archon_hip_kmers(p(sa), p(lcp), n, k, 1, 0, p(out), n, _tp(total), p(hist), bins_h, 0))
            assert total.value == want.size and out[:want.size].tolist() == want.tolist(), (x, k)
            assert (out[want.size:].view(np.uint32) == SENT).all()
            assert hist[:bins_h].tolist() == K.hist_of(sizes, bins_h).tolist() and hist[bins_h] == SENT, (x, k)
            st = archon.kmer_stats()
            assert (st.what, st.k, st.kmers, st.distinct, st.short_rows, st.groups) == (0, k, want.size, want.size, min(k - 1, n), want.size + min(k - 1, n))
            buf = np.full(words + 1, SENT, np.uint32)
            archon._check(L.archon_hip_kmer_occ(p(sa), p(lcp), n, k, p(buf), 0))
            assert buf[:words].tolist() == occ.tolist() and buf[words] == SENT, (x, k)
            # device forms: records | word | histogram | word | occ | word in one sentinel-filled tensor
            a, b = 3 * n + 1, 3 * n + 1 + bins_d + 1
            buf_t = torch.full((b + words + 1,), -1, dtype=torch.int32, device="cuda:0")
            got_total = archon.kmers_dev(sa_t, lcp_t, k, out_t=buf_t[:3 * n], hist_t=buf_t[a:a + bins_d])
            archon.kmer_occ_dev(sa_t, lcp_t, k, buf_t[b:b + max(words, 1)])       # (k = n + 1: the sentinel word itself, not written)
            got = buf_t.cpu().numpy().view(np.uint32)
            assert got_total == want.size and got[:3 * want.size].view(archon.KMER).tolist() == want.tolist(), (x, k)
            assert (got[3 * want.size:a] == 0xFFFFFFFF).all() and got[a + bins_d] == 0xFFFFFFFF and got[b + words] == 0xFFFFFFFF
            assert got[a:a + bins_d].tolist() == K.hist_of(sizes, bins_d).tolist(), (x, k)
            assert got[b:b + words].tolist() == occ.tolist(), (x, k)


def _check_block(archon, x, ks, sample=24, tile=DEFAULT_TILE, keep=None):
    """Block.kmers, Block.kmer_occ and Block.sus of x against the text: records, histogram, counters and their invariants,
    filters, count_only, occ, sus (the rule in numpy, and the identity "least L with count 1" on a sample of items).  keep: a
    list that takes every output and the stats record of every call"""
    n = x.size
    blk = archon.Block()
    sa, _ = blk.forward(x, want_sa=True)
    lcp = blk.lcp()
    sus = blk.sus()
    st0 = st = archon.kmer_stats()
    assert (st.what, st.n, st.ms_lcp > 0, st.ms_scatter > 0) == (2, n, True, True)
    assert (sus == K.sus_arrays(sa, lcp)).all()
    rng = np.random.default_rng(n)
    K.check_sus_sample(x.tobytes(), sus, [1, n] + [int(e) for e in rng.integers(1, n + 1, sample)])
    for k in ks:
        want, nshort = K.kmers_windows(x, k, sa)
        by_rule, groups, shorts = K.kmers_arrays(sa, lcp, k)
        assert (by_rule == want).all() and shorts == nshort
        sizes = want["hi"].astype(np.int64) - want["lo"]
        got, hist = blk.kmers(k, bins=16)
        st = archon.kmer_stats()
        assert got.size == want.size and (got == want).all(), k
        assert (st.what, st.n, st.k, st.bins, st.tile) == (0, n, k, 16, tile) and st.ms_lcp > 0 and st.ms_count > 0
        # the three invariants of the header
        assert st.distinct + st.short_rows == st.groups == groups and st.short_rows == min(k - 1, n)
        assert int(sizes.sum()) == max(n - k + 1, 0) == st.occurrences
        assert int(hist.sum()) == st.distinct == want.size and (hist == K.hist_of(sizes, 16)).all() and hist[0] == 0
        assert st.kmers == want.size and st.unique == int((sizes == 1).sum()) and st.most == (int(sizes.max()) if sizes.size else 0)
        # filters and counting
        twice = blk.kmers(k, min_occ=2)
        assert twice.size == int((sizes >= 2).sum()) and (twice == want[sizes >= 2]).all()
        st2 = archon.kmer_stats()
        assert st2.kmers == twice.size and st2.occurrences == int(sizes[sizes >= 2].sum()) and st2.distinct == want.size
        once = blk.kmers(k, max_occ=1)
        assert once.size == st.unique and (once == want[sizes == 1]).all()
        assert blk.kmers(k, min_occ=2, max_occ=3, count_only=True) == int(((sizes >= 2) & (sizes <= 3)).sum())
        assert archon.kmer_stats().ms_emit == 0
        # occ, and unique k-mers through sus
        occ = blk.kmer_occ(k)
        st3 = archon.kmer_stats()
        assert (st3.what, st3.k, st3.groups) == (1, k, groups) and st3.ms_scatter > 0
        assert occ.size == max(n - k + 1, 0) and (occ == K.occ_windows(x, k)).all(), k
        assert ((occ == 1) == ((sus[k - 1:] > 0) & (sus[k - 1:] <= k))).all(), k
        if keep is not None:
            keep += [got, hist, twice, once, occ, st, st2, archon.kmer_stats(), st3]
    if keep is not None:
        keep += [sus, st0]
    return blk, sa, lcp


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65536])
def test_shapes(archon, shape, n, monkeypatch):
    """every synthetic shape through Block.kmers, Block.kmer_occ and Block.sus at k = 1, 2, 8, 31; at 65536 once more with
    tiles of 16 rows (4096 tile words: four per lane of the scan)"""
    x = S.gen_shape(shape, n)
    blk, sa, lcp = _check_block(archon, x, (1, 2, 8, 31))
    if n == 65536:
        monkeypatch.setenv("ARCHON_KMER_TILE", "16")
        for k in (2, 8):
            want, _ = K.kmers_windows(x, k, sa)
            got, hist = blk.kmers(k, bins=4096)
            sizes = want["hi"].astype(np.int64) - want["lo"]
            assert archon.kmer_stats().tile == 16 and (got == want).all() and (hist == K.hist_of(sizes, 4096)).all()
            assert (blk.kmers(k, min_occ=3) == want[sizes >= 3]).all()
            assert (blk.kmer_occ(k) == K.occ_windows(x, k)).all()
        assert (blk.sus() == K.sus_arrays(sa, lcp)).all()
    blk.close()


@pytest.mark.parametrize("shape", ["dna", "text", "a"])
def test_shapes_large(archon, shape):
    """513 tiles and a ragged last one: MiB + 3 at k = 12"""
    blk, _, _ = _check_block(archon, S.gen_shape(shape, MiB + 3), (12,))
    blk.close()


@pytest.mark.parametrize("shape", ["a", "ab"])
def test_one_group_over_every_tile(archon, shape):
    """a block of one byte at MiB + 3 with k = 5 is ONE group of n - 4 rows behind which four short rows follow: every tile but
    the first and the last has no boundary; `ab` has two such groups"""
    n = MiB + 3
    x = S.gen_shape(shape, n)
    blk, sa, _ = _check_block(archon, x, (5,), sample=4)
    got = blk.kmers(5)
    st = archon.kmer_stats()
    if shape == "a":
        assert got.tolist() == [(0, n - 4, n)] and (st.groups, st.short_rows, st.distinct, st.most, st.unique) == (5, 4, 1, n - 4, 0)
        assert (blk.kmer_occ(5) == n - 4).all()
        sus = blk.sus()
        assert sus[n - 1] == n and not sus[:n - 1].any()
    else:
        assert sorted((got["hi"] - got["lo"]).tolist()) == [(n - 4) // 2, (n - 3) // 2] and st.most == (n - 3) // 2 and st.short_rows == 4
    blk.close()


def test_k_at_the_block_size(archon):
    """k = n is the block itself, once; k = n + 1 is nothing; one byte is one 1-mer"""
    x = b"abracadabra"
    n = len(x)
    sa, lcp, _, _ = R.a7_arrays(x)
    got = archon.kmers(sa, lcp, n)
    assert got.tolist() == [(sa.index(n), sa.index(n) + 1, n)] == K.kmers_text(x, n, sa)[0].tolist()
    assert archon.kmer_occ(sa, lcp, n).tolist() == [1]
    st = archon.kmer_stats()
    assert (st.what, st.groups) == (1, n)
    got, hist = archon.kmers(sa, lcp, n + 1, bins=3)
    st = archon.kmer_stats()
    assert got.size == 0 and not hist.any() and (st.groups, st.short_rows, st.distinct, st.most) == (n, n, 0, 0)
    assert archon.kmer_occ(sa, lcp, n + 1).size == 0 and archon.kmers(sa, lcp, 1000000, count_only=True) == 0
    assert archon.sus(sa, lcp).tolist() == K.sus_text(x).tolist()
    one = (np.array([1], np.uint32), np.array([0], np.uint32))
    assert archon.kmers(*one, 1).tolist() == [(0, 1, 1)] and archon.kmers(*one, 2).size == 0
    assert archon.kmer_occ(*one, 1).tolist() == [1] and archon.kmer_occ(*one, 2).size == 0 and archon.sus(*one).tolist() == [1]


LAYOUTS = [
    # (text, k, the rows that start a group, the short rows among them)
    (b"aacaacab", 4, [0, 1, 2, 4, 5, 6, 7], [1, 4, 7]),     # group [2, 4) ends on the tile edge; row 4 is short and first in its tile, row 7 short and last
    (b"aaaababa", 2, [0, 3, 5, 6], [5]),                    # group [3, 5) lies across the tile edge
    (b"aaaaaa", 4, [0, 3, 4, 5], [3, 4, 5]),                # group [0, 3) leaves one row of its tile to a short row; the next tile is short rows only
]


@pytest.mark.parametrize("x,k,starts,shorts", LAYOUTS)
def test_tile_edges(archon, oracle, x, k, starts, shorts, monkeypatch):
    """with tiles of 4 rows: a group that ends exactly on a tile edge, a short row first and last in a tile, a group across an
    edge -- the layout asserted from the oracle's suffix array, the answers from the text"""
    monkeypatch.setenv("ARCHON_KMER_TILE", "4")
    xa = np.frombuffer(x, np.uint8).copy()
    sa, _, _ = oracle.forward(xa)
    sa = np.asarray(sa, np.uint32)
    lcp = archon.lcp(xa, sa)
    assert sa.tolist() == R.a7_arrays(x)[0]
    below = lcp < k
    below[0] = True
    assert np.flatnonzero(below).tolist() == starts and [r for r in starts if sa[r] < k] == shorts
    want = K.kmers_text(x, k, sa)[0]
    got, hist = archon.kmers(sa, lcp, k, bins=4)
    st = archon.kmer_stats()
    assert st.tile == 4 and got.tolist() == want.tolist() and (st.groups, st.short_rows) == (len(starts), len(shorts))
    assert hist.tolist() == K.hist_of(want["hi"].astype(np.int64) - want["lo"], 4).tolist()
    assert archon.kmers(sa, lcp, k, min_occ=2).tolist() == [r for r in want.tolist() if r[1] - r[0] >= 2]
    assert archon.kmer_occ(sa, lcp, k).tolist() == K.occ_text(x, k).tolist()
    assert archon.sus(sa, lcp).tolist() == K.sus_text(x).tolist()


@pytest.fixture(scope="module")
def dna(archon):
    """dna at 65536: (x, sa, lcp)"""
    x = S.gen_shape("dna", 65536)
    sa, _, _ = archon.forward(x)
    return x, sa, archon.lcp(x, sa)


def test_cap_rule(archon, dna):
    """host and device forms: a short cap is ARCHON_E_ARG with *total set and out untouched"""
    import torch
    x, sa, lcp = dna
    k, n = 8, x.size
    L = archon.lib()
    p = archon._p
    want = K.kmers_windows(x, k, sa)[0]
    total = ctypes.c_uint64(0)
    assert L.archon_hip_kmers(p(sa), p(lcp), n, k, 1, 0, None, 0, _tp(total), None, 0, 0) == 0
    assert total.value == want.size > 1
    out = np.zeros(want.size, archon.KMER)
    out.view(np.uint32)[:] = 0xABABABAB
    untouched = out.copy()
    total.value = 0
    assert L.archon_hip_kmers(p(sa), p(lcp), n, k, 1, 0, p(out), want.size - 1, _tp(total), None, 0, 0) == archon.E_ARG
    assert total.value == want.size and (out == untouched).all()
    assert L.archon_hip_kmers(p(sa), p(lcp), n, k, 1, 0, p(out), want.size, _tp(total), None, 0, 0) == 0
    assert total.value == want.size and (out == want).all()
    sa_t, lcp_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32))
    out_t = torch.full((3 * want.size,), -1, dtype=torch.int32, device="cuda:0")
    assert archon.kmers_dev(sa_t, lcp_t, k) == want.size
    with pytest.raises(archon.ArchonError) as e:
        archon.kmers_dev(sa_t, lcp_t, k, out_t=out_t[:3 * (want.size - 1)])
    assert e.value.code == archon.E_ARG and (out_t == -1).all()
    assert archon.kmers_dev(sa_t, lcp_t, k, out_t=out_t) == want.size
    assert (out_t.cpu().numpy().view(np.uint32).view(archon.KMER) == want).all()
    # a filter that keeps nothing: no emit pass, out untouched
    out_t.fill_(-1)
    assert archon.kmers_dev(sa_t, lcp_t, k, min_occ=n, out_t=out_t) == 0 and (out_t == -1).all()


def test_location_and_documents(archon, dna):
    """the starts of a k-mer's occurrences are sa[lo:hi] - k, and what fm_locate finds for the k-mer's own bytes; the same from a
    sampled index of the block; docs_ranges over lo and hi gives every k-mer the number of documents a count over the text gives"""
    x, sa, _ = dna
    k, n = 10, x.size
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    recs = blk.kmers(k)
    want_recs = K.kmers_windows(x, k, sa)[0]
    assert (recs == want_recs).all()
    sizes = recs["hi"].astype(np.int64) - recs["lo"]
    pick = np.concatenate([np.arange(min(1500, recs.size)), np.flatnonzero(sizes >= 2)[:1500]])
    some = recs[pick]
    want = [sa[r["lo"]:r["hi"]] - k for r in some]
    got = blk.locate_kmers(some, k)
    assert all(g.size == w.size and (g == w).all() for g, w in zip(got, want))
    words = archon.kmer_bytes(x, some, k)
    assert all((words[j] == x[int(w[0]):int(w[0]) + k]).all() for j, w in enumerate(want))
    by_search = blk.fm_locate([w.tobytes() for w in words])
    assert all(g.size == w.size and (g == w).all() for g, w in zip(by_search, want))
    bounds = np.arange(0, n + 1, n // 8, dtype=np.uint32)
    f = blk.fm_index(32, docs=bounds)
    got = f.locate_kmers(some, k)
    assert all(g.size == w.size and (g == w).all() for g, w in zip(got, want))
    # document frequency from the text: an occurrence at p belongs to the document that holds its last byte, p + k - 1
    ndocs, _ = f.docs_ranges(recs["lo"], recs["hi"], emit=False)
    _, inv = np.unique(K._void_rows(np.lib.stride_tricks.sliding_window_view(x, k)), return_inverse=True)
    inv = inv.ravel()
    doc = (np.arange(n - k + 1, dtype=np.int64) + k - 1) // (n // 8)
    pairs = np.unique(inv.astype(np.int64) * 8 + doc)
    df_by_window = np.bincount(pairs // 8)
    window_of_rec = inv[recs["item"].astype(np.int64) - k]
    assert (ndocs == df_by_window[window_of_rec]).all() and int(ndocs.max()) > 1
    f.close()
    blk.close()


def test_statistics_stay_apart(archon, dna):
    """the launch and wait counts the header states; ms_emit == 0 when counting; the records of lcp, fm and forward stay
    byte-equal across the family's calls; a forward without its suffix array is refused"""
    import torch
    x, sa, lcp = dna
    n = x.size
    blk = archon.Block()
    blk.forward(x, want_sa=True)
    blk.fm_count([b"ACGT"])
    archon.lcp(x, sa)
    before = (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.stats_raw()))
    sa_t, lcp_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32))
    out_t = torch.empty(3 * n, dtype=torch.int32, device="cuda:0")
    hist_t = torch.empty(8, dtype=torch.int32, device="cuda:0")

    def counts():
        st = archon.kmer_stats()
        return st.kernel_launches, st.host_syncs

    # kmers: 4 launches counting, 6 with the emit pass; 1 wait, 2 with a histogram or the emit pass
    archon.kmers_dev(sa_t, lcp_t, 8)
    assert counts() == (4, 1) and archon.kmer_stats().ms_emit == 0 and archon.kmer_stats().ms_count > 0
    archon.kmers_dev(sa_t, lcp_t, 8, hist_t=hist_t)
    assert counts() == (4, 2) and archon.kmer_stats().ms_emit == 0
    archon.kmers_dev(sa_t, lcp_t, 8, out_t=out_t)
    assert counts() == (6, 2) and archon.kmer_stats().ms_emit > 0
    archon.kmers_dev(sa_t, lcp_t, 8, out_t=out_t, hist_t=hist_t)
    assert counts() == (6, 2)
    total = ctypes.c_uint64(0)
    out = np.zeros(n, archon.KMER)
    hist = np.zeros(8, np.uint32)
    L, p = archon.lib(), archon._p
    archon._check(L.archon_hip_kmers(p(sa), p(lcp), n, 8, 1, 0, None, 0, _tp(total), None, 0, 0))
    assert counts() == (4, 1) and archon.kmer_stats().ms_emit == 0
    archon._check(L.archon_hip_kmers(p(sa), p(lcp), n, 8, 1, 0, p(out), n, _tp(total), p(hist), 8, 0))
    assert counts() == (6, 2) and (hist == hist_t.cpu().numpy().view(np.uint32)).all()
    # kmer_occ: 4 launches; sus: 2; 1 wait on the device, 2 through host buffers
    archon.kmer_occ_dev(sa_t, lcp_t, 8, out_t[:n - 7])
    assert counts() == (4, 1) and archon.kmer_stats().ms_emit == 0
    archon.kmer_occ(sa, lcp, 8)
    assert counts() == (4, 2)
    archon.sus_dev(sa_t, lcp_t, out_t[:n])
    assert counts() == (2, 1)
    archon.sus(sa, lcp)
    assert counts() == (2, 2) and archon.kmer_stats().ms_lcp == 0
    assert before == (bytes(archon.lcp_stats()), bytes(archon.fm_stats()), bytes(archon.stats_raw()))
    # the block forms: the same launches, the waits of the LCP step on top, and its record kept
    for call, launches, waits in ((lambda: blk.kmers(8, count_only=True), 4, 1), (lambda: blk.kmer_occ(8), 4, 2), (blk.sus, 2, 2)):
        call()
        assert archon.lcp_stats().n == n and counts() == (launches, waits + archon.lcp_stats().host_syncs)
        assert archon.kmer_stats().ms_lcp > 0
    assert bytes(archon.fm_stats()) == before[1] and bytes(archon.stats_raw()) == before[2]
    blk.forward(x, want_sa=False)
    for call in (lambda: blk.kmers(8), lambda: blk.kmer_occ(8), blk.sus):
        with pytest.raises(archon.ArchonError) as e:
            call()
        assert e.value.code == archon.E_ARG
    blk.close()


def test_two_contexts_concurrently(archon):
    blocks = [S.gen_shape("text", MiB + 1), S.gen_shape("dna", MiB + 1)]
    solo = []
    for x in blocks:
        blk = archon.Block()
        blk.forward(x, want_sa=True)
        solo.append((blk.kmers(9, min_occ=2), blk.kmer_occ(9), blk.sus()))
        blk.close()
    assert solo[0][0].size != solo[1][0].size
    stats, errors = [None, None], []

    def run(j):
        try:
            archon.bind_context(j)
            blk = archon.Block()
            blk.forward(blocks[j], want_sa=True)
            for _ in range(3):
                got = blk.kmers(9, min_occ=2)
                stats[j] = archon.kmer_stats()
                assert (got == solo[j][0]).all() and (blk.kmer_occ(9) == solo[j][1]).all() and (blk.sus() == solo[j][2]).all()
            blk.close()
        except Exception as ex:          # noqa: BLE001 -- reported below
            errors.append(ex)

    threads = [threading.Thread(target=run, args=(j,)) for j in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for j in (0, 1):
        assert stats[j].n == blocks[j].size and stats[j].kmers == solo[j][0].size and stats[j].what == 0


def test_garbage_lcp(archon, dna):
    """random words are the LCP array of nothing: ARCHON_OK, every record lo < hi <= n, and the rule is a rule about the arrays,
    so the array helper still says which"""
    _, sa, _ = dna
    n = sa.size
    lcp = np.random.default_rng(12).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for k in (1, 3, 1 << 31):
        got, hist = archon.kmers(sa, lcp, k, bins=7)
        want, groups, shorts = K.kmers_arrays(sa, lcp, k)
        assert (got["lo"] < got["hi"]).all() and (got["hi"] <= n).all()
        assert (got == want).all() and int(hist.sum()) == want.size
        st = archon.kmer_stats()
        assert (st.groups, st.short_rows) == (groups, shorts)
        assert (archon.kmer_occ(sa, lcp, k) == K.occ_arrays(sa, lcp, k)).all()
    assert (archon.sus(sa, lcp) == K.sus_arrays(sa, lcp)).all()


@pytest.mark.parametrize("bad", ["zero", "past"])
def test_bad_sa_is_corrupt(archon, dna, bad):
    """an sa value outside 1..n is never used as an index: ARCHON_E_CORRUPT from every form, the outputs untouched"""
    import torch
    _, sa, lcp = dna
    n = sa.size
    sa = sa.copy()
    sa[n // 3] = 0 if bad == "zero" else n + 1
    L, p = archon.lib(), archon._p
    out = np.zeros(n, archon.KMER)
    out.view(np.uint32)[:] = SENT
    hist = np.full(8, SENT, np.uint32)
    words = np.full(n, SENT, np.uint32)
    total = ctypes.c_uint64(5)
    assert L.archon_hip_kmers(p(sa), p(lcp), n, 4, 1, 0, p(out), n, _tp(total), p(hist), 8, 0) == archon.E_CORRUPT
    assert total.value == 0 and (out.view(np.uint32) == SENT).all() and (hist == SENT).all()
    assert L.archon_hip_kmer_occ(p(sa), p(lcp), n, 4, p(words), 0) == archon.E_CORRUPT and (words == SENT).all()
    assert L.archon_hip_sus(p(sa), p(lcp), n, p(words), 0) == archon.E_CORRUPT and (words == SENT).all()
    sa_t, lcp_t = _cuda(sa.view(np.int32)), _cuda(lcp.view(np.int32))
    buf_t = torch.full((3 * n + 8 + n,), -1, dtype=torch.int32, device="cuda:0")
    for call in (lambda: archon.kmers_dev(sa_t, lcp_t, 4, out_t=buf_t[:3 * n], hist_t=buf_t[3 * n:3 * n + 8]),
                 lambda: archon.kmer_occ_dev(sa_t, lcp_t, 4, buf_t[3 * n + 8:]), lambda: archon.sus_dev(sa_t, lcp_t, buf_t[3 * n + 8:])):
        with pytest.raises(archon.ArchonError) as e:
            call()
        assert e.value.code == archon.E_CORRUPT
    assert (buf_t == -1).all()


@pytest.mark.parametrize("tile", [0, 16])
@pytest.mark.parametrize("grid", G.GRIDS)
def test_stride_grid(archon, grid, tile, monkeypatch):
    """at most 1 and 3 workgroups (ARCHON_STRIDE_GRID) on text and dna at 65 536 + 3, with the default tile (33 tiles, the last
    of 3 rows) and with tiles of 16 rows (4097 tiles; 17 words of the tile scan): kmers with the histogram and the filters,
    kmer_occ and sus at k = 2 and 12 against the text, byte-equal to the same calls without the route, with their counters,
    launches and host waits"""
    if tile:
        monkeypatch.setenv("ARCHON_KMER_TILE", str(tile))
    for shape in ("text", "dna"):
        x = S.gen_shape(shape, 65536 + 3)

        def call():
            keep = []
            _check_block(archon, x, (2, 12), sample=4, tile=tile or DEFAULT_TILE, keep=keep)[0].close()
            return [v for v in keep if isinstance(v, np.ndarray)], [v for v in keep if not isinstance(v, np.ndarray)]
        G.same_under(monkeypatch, grid, call)


@pytest.mark.parametrize("shape", ["a", "dna"])
def test_second_trip_at_the_product_grid(archon, shape):
    """no route: 2048 * 2048 + 3 * 2048 + 5 rows are 2052 tiles, so workgroups 0-3 of the 2048 take a second tile in every pass
    and the last tile has 5 rows.  One byte at k = 5: one group of n - 4 rows.  DNA at k = 12 against the text"""
    n = G.N2
    x = S.gen_shape(shape, n)
    blk, _, _ = _check_block(archon, x, (5,) if shape == "a" else (12,), sample=4)
    try:
        assert blk.validate() == 1
        if shape == "a":
            got = blk.kmers(5)
            st = archon.kmer_stats()
            assert got.tolist() == [(0, n - 4, n)] and (st.groups, st.short_rows, st.distinct, st.most, st.unique) == (5, 4, 1, n - 4, 0)
            assert (blk.kmer_occ(5) == n - 4).all()
            sus = blk.sus()
            assert sus[n - 1] == n and not sus[:n - 1].any()
    finally:
        blk.close()
