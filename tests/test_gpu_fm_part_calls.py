"""GPU: how many kernels the entry points of the handle's attached parts launch and how often they wait for their stream
(kernel_launches and host_syncs of fm_ms_stats, fm_text_stats, fm_doc_stats and fm_edit_stats), in the manner of
test_gpu_fm_calls.py and test_gpu_fm_mem_calls.py, for the calls those two do not reach: attach_lcp and ms, attach_sa, ms_text
and rlz, attach_docs, docs, docs_ranges and doc_of, and the edit-distance search.  A wait is one host wait for the call's
stream; the device-wide wait of an arena that grows is not counted, and every test runs a forward of the block first, after
which the arena holds each of these calls without growing.  A record describes the last C call only; the wrappers that may
make two (docs, docs_ranges and edit with records, rlz with phrases) end with the call that ran to its end.

Every call's answer is checked too, against the references the other FM tests use.  The figures are the ones the library
reported at the commit before the one that added this test (profiles/fm/fm_part_calls_parent.txt)."""
import numpy as np
import pytest

import archon_synth as S
import fm_doc_naive as D
import fm_edit_naive as E
import fm_ms_naive
import lcp_kasai

pytestmark = pytest.mark.gpu

N = 256 << 10
RATE = 32
FAN = 16
# The drivers, step by step (fm_host.hiph), as (launches, waits):
#   fms_attach_run   the guard and one level kernel per level of the minimum hierarchy; one wait for the guard's flag
LEVELS = 5                              # 256 Ki entries at F = 16: 16 Ki, 1 Ki, 64, 4, 1
ATTACH_LCP = (1 + LEVELS, 1)
#   fms_host / _dev  the search; one wait for the records (host) or the counters (device), rows or not
MS = (1, 1)
#   fmt_attach_run   the kernel that checks sa and scatters isa; one wait for its flag
ATTACH_SA = (1, 1)
#   fmt_host / _dev  chunk offsets, the walk, the sweep, the fix; one wait
MS_TEXT = (4, 1)
#   fmt_rlz          those four and the kernel that makes the parse's items, then the parse: its launches and waits are the ones
#                    lz_parse reports for the same items (the parse waits, fmt_rlz itself does not)
RLZ_OWN_LAUNCHES = 4 + 1
#   fmd_attach_run   bounds check (a wait for its flag), pairs, [digit counts (a wait for them), one launch per sort byte], link;
#                    a wait at the end
ATTACH_DOCS_NO_SORT = (3, 2)            # D = 1: no byte of D - 1 can differ


def attach_docs_shape(sort_passes):
    return (3 + 1 + sort_passes, 3) if sort_passes else ATTACH_DOCS_NO_SORT


#   fmd_run          tiles and their scan (1 + 3; a wait for the tile total), then -- unless every range is empty -- the count, its
#                    scan and the per-range counts (1 + 3 + 1; a wait for the record total), then the emit pass (1; a wait)
#   fmd_ranges_*     fmd_run; with every range empty the device form waits once more for the zeros it writes
DOCS_RANGES = {False: (9, 2), True: (10, 3)}
DOCS_RANGES_EMPTY = {"host": (4, 1), "dev": (4, 2)}
#   fmd_host         fm_count_host before it: 1 launch, a wait for the counters and one for the ranges
DOCS_HOST = {False: (10, 4), True: (11, 5)}
#   fmd_dev          the count kernel inside the run, with no wait of its own
DOCS_DEV = {False: (10, 2), True: (11, 3)}
#   fmd_doc_of       the check of the items (a wait for its flag), then the lookup (a wait for the stream)
DOC_OF = (2, 2)


def edit_shape(batches, windows, emit, form):
    """fme_run over batches of (seed rows, marked pairs, hits): the pieces (1; a wait for the flag), their count (1; a wait) and
    its ranges (a wait); per batch tcount and its scan (1 + 3; a wait for the pairs) and nhits (1; a wait for the hits), with
    seed rows the locate and the marks (2), with pairs the list (1) and the count pass with its scan (1 + 3), on a handle also
    the windows and their scan (1 + 3) and the extract (5; a wait); the emit pass (1; a wait) at once with one batch, else in a
    second round over every batch when there are hits.  The host forms wait once more for the results, the device form once
    at the start for the offsets"""
    launches, waits = 2, 3
    rounds = [(b, emit and len(batches) == 1) for b in batches]
    if emit and len(batches) > 1 and sum(b[2] for b in batches):
        rounds += [(b, True) for b in batches]
    for (rows, pairs, hits), with_emit in rounds:
        launches += 4 + 1
        waits += 2
        if rows:
            launches += 2
        if pairs:
            launches += 1 + 4
            if windows:
                launches += 4 + 5
                waits += 1
        if with_emit and hits:
            launches += 1
            waits += 1
    return launches, waits + (1 if form in ("host", "dev") else 0)


@pytest.fixture(scope="module")
def block(oracle, tmp_path_factory):
    """the block with its oracle arrays, patterns that occur (24-byte substrings) and patterns that do not, and a text of
    4500 bytes cut from the block with two bytes changed: computed once, shared, left unchanged"""
    x = S.gen_prose(N, S.SEED_BASE + 6)
    sa, bwt, base = oracle.forward(x)
    lcp = lcp_kasai.build(tmp_path_factory.mktemp("fm_part_kasai"))(x, sa)
    rng = np.random.default_rng(11)
    found = [x[q:q + 24].tobytes() for q in rng.integers(0, N - 24, 6)]
    absent = [bytes([1, 2, 3, 254, 255, 0, 7, 9]), bytes(range(200, 216))]
    text = np.concatenate([x[100000:103000], x[5000:6500]])
    text[700] ^= 1
    text[3900] ^= 1
    naive = fm_ms_naive.build(tmp_path_factory.mktemp("fm_part_naive"))
    pats = found + absent
    ms_want = naive(x, sa, lcp, pats)[:4]
    text_want = naive(x, sa, lcp, [text.tobytes()])[:3]
    for a in (x, sa, bwt, lcp, text) + tuple(ms_want) + tuple(text_want):
        a.setflags(write=False)
    return {"x": x, "sa": sa, "bwt": bwt, "base": base, "lcp": lcp, "found": found, "absent": absent, "pats": pats, "text": text,
            "ms": ms_want, "ms_text": text_want}


def _lw(st):
    print("   ", type(st).__name__, st.asdict())
    return st.kernel_launches, st.host_syncs


def _dev(a):
    import torch
    a = np.array(a)              # (a copy: the shared arrays are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _zeros(n):
    import torch
    return torch.zeros(max(n, 1), dtype=torch.int32, device="cuda:0")


def _host(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def _resident(archon, block):
    b = archon.Block()
    b.forward(block["x"])
    return b


def _same_ms(got, want):
    for g, w in zip(got, want):
        assert (np.asarray(g) == w).all()


def test_attach_lcp_and_ms(archon, block):
    pats, want = block["pats"], block["ms"]
    packed, off = archon._pack_patterns(pats)
    total = int(off[-1])
    b = _resident(archon, block)
    try:
        f = archon.FmIndex(block["bwt"], block["base"])
        f.attach_lcp(block["lcp"])
        st = archon.fm_ms_stats()
        assert _lw(st) == ATTACH_LCP and (st.levels, st.fan, st.attached) == (LEVELS, FAN, 1)
        _same_ms(f.ms(pats), want)
        assert _lw(archon.fm_ms_stats()) == MS
        assert (f.ms(pats, rows=False)[0] == want[0]).all()
        assert _lw(archon.fm_ms_stats()) == MS
        f.attach_lcp_dev(_dev(block["lcp"]))
        st = archon.fm_ms_stats()
        assert _lw(st) == ATTACH_LCP and st.attached == 1
        p_t, o_t = _dev(packed), _dev(off)
        len_t, lo_t, hi_t = _zeros(total), _zeros(total), _zeros(total)
        f.ms_dev(p_t, o_t, len_t, lo_t, hi_t)
        assert _lw(archon.fm_ms_stats()) == MS
        _same_ms((_host(len_t, total), _host(lo_t, total), _host(hi_t, total)), want)
        len_t.zero_()
        f.ms_dev(p_t, o_t, len_t)
        assert _lw(archon.fm_ms_stats()) == MS
        assert (_host(len_t, total) == want[0]).all()
        f.close()
        # the block form: the LCP array is made on the device first, with the waits its own record counts
        g = b.fm_index(RATE, lcp=True)
        st = archon.fm_ms_stats()
        assert _lw(st) == (1 + LEVELS, archon.lcp_stats().host_syncs + 1) and st.attached == 1
        _same_ms(g.ms(pats), want)
        g.close()
    finally:
        b.close()


def test_attach_sa_ms_text_and_rlz(archon, block):
    import torch
    x, sa, text, want = block["x"], block["sa"], block["text"], block["ms_text"]
    m = text.size
    rec = np.zeros(m, archon.LPF)
    rec["len"] = want[0]
    rec["src"] = np.where(want[0] > 0, sa[np.minimum(want[1], N - 1)], 0)
    b = _resident(archon, block)
    try:
        phrases = archon.lz_parse(rec)
        parse_emit = _lw(archon.lz_stats())
        assert archon.lz_parse(rec, count_only=True) == phrases.size
        parse_count = _lw(archon.lz_stats())
        assert archon.lz_parse_dev(_dev(rec.view(np.uint32))) == phrases.size
        parse_dev = _lw(archon.lz_stats())
        f = archon.FmIndex(block["bwt"], block["base"]).attach_lcp(block["lcp"])
        for attach in (lambda: f.attach_sa(sa), lambda: f.attach_sa_dev(_dev(sa))):
            attach()
            st = archon.fm_text_stats()
            assert _lw(st) == ATTACH_SA and st.sa_bytes == 4 * N + 4 * (N + 1)
            _same_ms(f.ms_text(text), want)
            assert _lw(archon.fm_text_stats()) == MS_TEXT
        assert (f.ms_text(text, rows=False)[0] == want[0]).all()
        assert _lw(archon.fm_text_stats()) == MS_TEXT
        t_t = _dev(np.concatenate([text, np.zeros(1, np.uint8)]))[:m]
        len_t, lo_t, hi_t = _zeros(m), _zeros(m), _zeros(m)
        f.ms_text_dev(t_t, len_t, lo_t, hi_t)
        assert _lw(archon.fm_text_stats()) == MS_TEXT
        _same_ms((_host(len_t, m), _host(lo_t, m), _host(hi_t, m)), want)
        len_t.zero_()
        f.ms_text_dev(t_t, len_t)
        assert _lw(archon.fm_text_stats()) == MS_TEXT
        assert (_host(len_t, m) == want[0]).all()
        assert f.rlz(text, count_only=True) == phrases.size
        assert _lw(archon.fm_text_stats()) == (RLZ_OWN_LAUNCHES + parse_count[0], parse_count[1])
        got = f.rlz(text)
        assert _lw(archon.fm_text_stats()) == (RLZ_OWN_LAUNCHES + parse_emit[0], parse_emit[1])
        assert (got == phrases).all()
        lit = got["len"] == 0
        assert (archon.rlz_decode(x, got, m, text[got["end"][lit] - 1]) == text).all()
        assert f.rlz_dev(t_t) == phrases.size
        assert _lw(archon.fm_text_stats()) == (RLZ_OWN_LAUNCHES + parse_dev[0], parse_dev[1])
        out_t = torch.zeros(3 * phrases.size, dtype=torch.int32, device="cuda:0")
        assert f.rlz_dev(t_t, out_t) == phrases.size
        assert (out_t.cpu().numpy().view(np.uint32).view(archon.PHRASE) == phrases).all()
        f.close()
        g = b.fm_index(RATE, lcp=True, sa=True)
        assert _lw(archon.fm_text_stats()) == ATTACH_SA
        _same_ms(g.ms_text(text), want)
        g.close()
    finally:
        b.close()


def _same_docs(got, want):
    assert got.size == want.size
    for key in ("range", "row", "doc", "tf"):
        assert (got[key] == want[key]).all(), key


@pytest.mark.parametrize("ndocs", [1, 300])
def test_documents(archon, block, ndocs):
    x, sa, pats = block["x"], block["sa"], block["pats"]
    rng = np.random.default_rng(ndocs)
    cuts = np.sort(rng.choice(np.arange(1, N), ndocs - 1, replace=False))
    bounds = np.concatenate([[0], cuts, [N]]).astype(np.uint32)
    sort_passes = {1: 0, 300: 2}[ndocs]
    packed, off = archon._pack_patterns(pats)
    k = len(pats)
    b = _resident(archon, block)
    try:
        f = archon.FmIndex(block["bwt"], block["base"]).attach_sa(sa)
        lo, hi = f.count(pats)
        ranges = [(int(a), int(c)) if a < c else (0, 0) for a, c in zip(lo, hi)]
        T = D.DEFAULT_TILE
        want, wnd, ctr = D.listing(sa, bounds, ranges, T)
        assert want.size >= len(block["found"])
        for attach in (lambda: f.attach_docs(bounds), lambda: f.attach_docs_dev(_dev(bounds))):
            attach()
            st = archon.fm_doc_stats()
            assert _lw(st) == attach_docs_shape(sort_passes) and (st.attached, st.sort_passes, st.docs) == (1, sort_passes, ndocs)
            nd, got = f.docs(pats)
            _same_docs(got, want)
            assert (nd == wnd).all()
            assert _lw(archon.fm_doc_stats()) == DOCS_HOST[True]
        nd, none = f.docs(pats, emit=False)
        assert none is None and (nd == wnd).all()
        assert _lw(archon.fm_doc_stats()) == DOCS_HOST[False]
        # the ranges of the same patterns, as a count gives them (an absent pattern's range is empty wherever it lies)
        nd, got = f.docs_ranges(lo, hi)
        _same_docs(got, want)
        assert _lw(archon.fm_doc_stats()) == DOCS_RANGES[True]
        nd, none = f.docs_ranges(lo, hi, emit=False)
        assert (nd == wnd).all()
        assert _lw(archon.fm_doc_stats()) == DOCS_RANGES[False]
        nd, got = f.docs_ranges(lo[-2:], hi[-2:])
        assert got.size == 0 and not nd.any()
        assert _lw(archon.fm_doc_stats()) == DOCS_RANGES_EMPTY["host"]
        p_t, o_t, lo_t, hi_t = _dev(packed), _dev(off), _dev(lo), _dev(hi)
        nd_t, rec_t = _zeros(k), _zeros(4 * want.size)
        for call, shape in ((lambda r: f.docs_dev(p_t, o_t, nd_t, r), DOCS_DEV), (lambda r: f.docs_ranges_dev(lo_t, hi_t, nd_t, r), DOCS_RANGES)):
            nd_t.zero_()
            assert call(None) == want.size
            assert _lw(archon.fm_doc_stats()) == shape[False]
            assert (_host(nd_t, k) == wnd).all()
            rec_t.zero_()
            assert call(rec_t) == want.size
            assert _lw(archon.fm_doc_stats()) == shape[True]
            _same_docs(_host(rec_t, 4 * want.size).view(archon.FM_DOC), want)
        nd_t.fill_(7)
        assert f.docs_ranges_dev(lo_t[-2:], hi_t[-2:], nd_t[:2], rec_t) == 0
        assert _lw(archon.fm_doc_stats()) == DOCS_RANGES_EMPTY["dev"]
        assert not _host(nd_t, 2).any()
        # doc_of over the ends of the first pattern's occurrences
        items = np.sort(sa[lo[0]:hi[0]])
        doc, offs = f.doc_of(items)
        assert _lw(archon.fm_doc_stats()) == DOC_OF
        assert (doc == D.doc_of_items(bounds, items)).all() and (offs == items - 1 - bounds[doc]).all()
        doc, none = f.doc_of(items, offsets=False)
        assert none is None and (doc == D.doc_of_items(bounds, items)).all()
        assert _lw(archon.fm_doc_stats()) == DOC_OF
        d_t, f_t = _zeros(items.size), _zeros(items.size)
        L = archon.lib()
        vp = lambda t: archon.ctypes.c_void_p(t.data_ptr())      # noqa: E731
        assert L.archon_hip_fm_doc_of_dev(f.h, vp(_dev(items)), items.size, vp(d_t), vp(f_t), archon._stream_ptr()) == 0
        assert _lw(archon.fm_doc_stats()) == DOC_OF
        assert (_host(d_t, items.size) == doc).all() and (_host(f_t, items.size) == offs).all()
        f.close()
        g = b.fm_index(RATE, docs=bounds)
        st = archon.fm_doc_stats()
        assert _lw(st) == attach_docs_shape(sort_passes) and st.attached == 1
        nd, got = g.docs(pats)
        _same_docs(got, want)
        g.close()
    finally:
        b.close()


@pytest.mark.parametrize("per_batch", [0, 1])
def test_edit(archon, block, monkeypatch, per_batch):
    """K = 1 on a handle (the seeds located by walks, the text extracted), on the device form and on the resident block; once
    more with one pattern per batch, so that the hits are emitted in a second round over the batches"""
    x, pats = block["x"], block["pats"]
    K = 1
    if per_batch:
        monkeypatch.setenv("ARCHON_EDIT_BATCH", str(per_batch))
    cells = [E.rule_cells(x, p) for p in pats]
    ends = [np.flatnonzero(d <= K) for d, _ in cells]
    want_n = np.array([e.size for e in ends], np.uint32)
    want = np.zeros(int(want_n.sum()), archon.FM_EDIT)
    at = 0
    for j, ((d, s), e) in enumerate(zip(cells, ends)):
        part = want[at:at + e.size]
        part["start"], part["end"], part["distance"], part["pattern"] = s[e], e, d[e], j
        at += e.size
    assert (want_n[:len(block["found"])] >= 1).all() and not want_n[len(block["found"]):].any()
    packed, off = archon._pack_patterns(pats)
    k = len(pats)
    b = _resident(archon, block)
    try:
        b.fm_count(pats[:1])        # the block's table: built here, not by the edit call
        f = b.fm_index(RATE)
        W = None
        for form in ("host", "dev", "block"):
            for emit in (False, True):
                if form == "host":
                    nh, got = f.edit(pats, K, emit=emit)
                elif form == "block":
                    nh, got = b.fm_edit(pats, K, emit=emit)
                else:
                    nh_t, rec_t = _zeros(k), _zeros(4 * want.size)
                    assert f.edit_dev(_dev(packed), _dev(off), K, nh_t, rec_t if emit else None) == want.size
                    nh, got = _host(nh_t, k), (_host(rec_t, 4 * want.size).view(archon.FM_EDIT) if emit else None)
                st = archon.fm_edit_stats()
                assert (nh == want_n).all() and (got is None) == (not emit)
                if emit:
                    assert (got == want).all()
                if W is None:
                    # what each pattern marks at this tile, from the model of the search: seed rows, marked tiles, hits
                    W = st.tile
                    per = []
                    for p, e in zip(pats, ends):
                        tiles, rows = E.marked_tiles(x, p, K, W)
                        per.append((rows, len(tiles), e.size))
                    groups = [per] if not per_batch else [per[i:i + per_batch] for i in range(0, k, per_batch)]
                    batches = [tuple(sum(v[i] for v in g) for i in range(3)) for g in groups]
                assert st.batches == len(batches) and st.built == 0
                assert (st.seed_rows, st.tiles) == (sum(v[0] for v in per), sum(v[1] for v in per))
                assert _lw(st) == edit_shape(batches, form != "block", emit, form if form != "block" else "host")
        f.close()
    finally:
        b.close()
