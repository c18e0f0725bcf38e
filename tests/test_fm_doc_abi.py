"""CPU: the document listing (include/archon_hip.h: archon_hip_fm_attach_docs, _fm_attach_docs_dev, _block_fm_attach_docs, _fm_docs,
_fm_docs_dev, _fm_docs_ranges, _fm_docs_ranges_dev, _fm_doc_of, _fm_doc_of_dev, _get_fm_doc_stats) is declared, exported and bound;
the record and the statistics mirror have the C layout; bad arguments are refused and, without a GPU, the calls fail loudly.  And
the model of the listing over a suffix array (fm_doc_naive.listing) is pinned to the DEFINITION from the text alone
(fm_doc_naive.definition) on every short block, boundary set and pattern."""
import ctypes
import inspect
import itertools
import re

import numpy as np
import pytest

from fm_abi_util import ROOT, declared as _declared, layout as _layout, p as _p
import fm_doc_naive as N

FUNCTIONS = ["archon_hip_fm_attach_docs", "archon_hip_fm_attach_docs_dev", "archon_hip_block_fm_attach_docs", "archon_hip_fm_docs",
             "archon_hip_fm_docs_dev", "archon_hip_fm_docs_ranges", "archon_hip_fm_docs_ranges_dev", "archon_hip_fm_doc_of",
             "archon_hip_fm_doc_of_dev", "archon_hip_get_fm_doc_stats"]
FIELDS = ["n", "docs", "ranges", "tile", "attached", "sort_passes", "longest_tf", "reserved0", "pattern_bytes", "rows", "tiles", "listed",
          "probes", "doc_bytes", "kernel_launches", "host_syncs", "ms_attach", "ms_search", "ms_count", "ms_emit"]
RECORD = ["doc", "tf", "row", "range"]


def test_doc_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmDocStats", "fm_doc_stats", "FM_DOC"):
        assert hasattr(pyarchon, name), name
    for name in ("attach_docs", "attach_docs_dev", "docs", "docs_dev", "docs_ranges", "docs_ranges_dev", "doc_of"):
        assert hasattr(pyarchon.FmIndex, name), name
    assert inspect.signature(pyarchon.Block.fm_index).parameters["docs"].default is None
    assert inspect.signature(pyarchon.FmIndex.docs).parameters["emit"].default is True
    assert inspect.signature(pyarchon.FmIndex.docs_ranges).parameters["emit"].default is True
    assert pyarchon.FM_DOC == N.FM_DOC
    assert "DOC_TILE" in pyarchon._ROUTE_NAMES
    assert "DOC_TILE" in open(ROOT + "/include/archon_hip_test.h").read()


def test_fm_doc_struct_layouts(tmp_path):
    """the header declares archon_hip_fm_doc_stats with the fields of the issue, in its order, 8-byte fields on 8-byte offsets, and
    the ctypes mirror has the size and the field offsets the C compiler gives it; the record is four words and FM_DOC is it"""
    import pyarchon
    src = open(ROOT + "/include/archon_hip.h").read()
    body = re.search(r"typedef struct archon_hip_fm_doc_stats \{(.*?)\} archon_hip_fm_doc_stats;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    names = [k for k, _ in pyarchon.FmDocStats._fields_]
    assert names == FIELDS
    got = _layout(tmp_path, "archon_hip_fm_doc_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmDocStats)
    assert got[1:] == [getattr(pyarchon.FmDocStats, k).offset for k in names]
    for k, t in pyarchon.FmDocStats._fields_:
        if ctypes.sizeof(t) == 8:
            assert getattr(pyarchon.FmDocStats, k).offset % 8 == 0, k
    rec = _layout(tmp_path, "archon_hip_fm_doc", RECORD)
    assert rec == [16, 0, 4, 8, 12]
    assert pyarchon.FM_DOC.itemsize == 16 and [pyarchon.FM_DOC.fields[k][1] for k in RECORD] == rec[1:]


def test_doc_tile_route():
    import pyarchon
    L = pyarchon.lib()
    for bad in (1, 63, 65, (1 << 20) + 64, -64):
        assert L.archon_hip_test_route(b"DOC_TILE", bad) == pyarchon.E_ARG, bad
        assert b"DOC_TILE" in L.archon_hip_last_error()
    for good in (64, 128, 4096, 1 << 20, 0):
        assert L.archon_hip_test_route(b"DOC_TILE", good) == 0, good
    assert L.archon_hip_test_route(b"DOC_TILE", 64) == 0 and L.archon_hip_test_route(b"RESET", 0) == 0


def test_doc_bad_arguments():
    """null pointers and bad bounds are ARCHON_E_ARG with or without a device: they are refused before the handle is read (a
    stand-in handle is never used); *total is written 0 before a refusal"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    stand_in = _p(np.zeros(64, np.uint8))
    good = np.array([0, 3, 6], np.uint32)
    a, b, nd = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.full(8, 9, np.uint32)
    rec = np.zeros(8, pyarchon.FM_DOC)
    total = ctypes.c_uint64(5)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    # attach: null pointers, then what bounds say by themselves
    assert L.archon_hip_fm_attach_docs(None, _p(good), 2) == E
    assert L.archon_hip_fm_attach_docs(stand_in, None, 2) == E
    assert L.archon_hip_fm_attach_docs_dev(None, _p(good), 2, None) == E
    assert L.archon_hip_fm_attach_docs_dev(stand_in, None, 2, None) == E
    assert L.archon_hip_fm_attach_docs_dev(stand_in, _p(good), 0, None) == E
    assert L.archon_hip_block_fm_attach_docs(None, stand_in, _p(good), 2) == E
    assert L.archon_hip_block_fm_attach_docs(stand_in, None, _p(good), 2) == E
    assert L.archon_hip_block_fm_attach_docs(stand_in, stand_in, None, 2) == E
    for bad, D in (([0, 3, 6], 0), ([1, 3, 6], 2), ([0, 3, 3], 2), ([0, 4, 3], 2), ([0, 0, 6], 2)):
        bb = np.array(bad, np.uint32)
        assert L.archon_hip_fm_attach_docs(stand_in, _p(bb), D) == E, bad
        assert L.archon_hip_block_fm_attach_docs(stand_in, stand_in, _p(bb), D) == E, bad
    # the listings: every pointer but the records, *total 0 whenever it is given
    for fn, dev in ((L.archon_hip_fm_docs, False), (L.archon_hip_fm_docs_ranges, False), (L.archon_hip_fm_docs_dev, True),
                    (L.archon_hip_fm_docs_ranges_dev, True)):
        tail = (None,) if dev else ()
        for args in ((None, _p(a), _p(b), 8, _p(nd), _p(rec), 8, tp), (stand_in, None, _p(b), 8, _p(nd), _p(rec), 8, tp),
                     (stand_in, _p(a), None, 8, _p(nd), _p(rec), 8, tp), (stand_in, _p(a), _p(b), 8, None, _p(rec), 8, tp)):
            total.value = 5
            assert fn(*args, *tail) == E
            assert total.value == 0
        assert fn(stand_in, _p(a), _p(b), 8, _p(nd), _p(rec), 8, None, *tail) == E
    assert (nd == 9).all() and not rec.view(np.uint32).any()
    # doc_of
    assert L.archon_hip_fm_doc_of(None, _p(a), 8, _p(b), None) == E
    assert L.archon_hip_fm_doc_of(stand_in, None, 8, _p(b), None) == E
    assert L.archon_hip_fm_doc_of(stand_in, _p(a), 8, None, None) == E
    assert L.archon_hip_fm_doc_of_dev(None, _p(a), 8, _p(b), None, None) == E
    assert L.archon_hip_fm_doc_of_dev(stand_in, None, 8, _p(b), None, None) == E
    assert L.archon_hip_fm_doc_of_dev(stand_in, _p(a), 8, None, None, None) == E
    assert L.archon_hip_fm_doc_of_dev(stand_in, _p(a), 1 << 32, _p(b), None, None) == E
    assert L.archon_hip_get_fm_doc_stats(0, None) == E
    if pyarchon.device_count() == 0:
        assert L.archon_hip_get_fm_doc_stats(0, ctypes.byref(pyarchon.FmDocStats())) == E


def test_doc_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).attach_sa(np.array([2, 4, 6, 1, 3, 5], np.uint32)).attach_docs([0, 3, 6])
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_index(32, docs=[0, 3, 6])


def test_model_header_examples(oracle):
    """the worked example of the header, literally: "banana" cut into "ban" and "ana" """
    x, bounds = b"banana", [0, 3, 6]
    sa = oracle.sa(x)
    assert list(sa) == [2, 4, 6, 1, 3, 5]
    assert list(N.row_docs(sa, bounds)) == [0, 1, 1, 0, 0, 1]
    want = {b"an": ((4, 6), [(0, 1, 4), (1, 1, 5)]), b"a": ((0, 3), [(0, 1, 0), (1, 2, 1)]), b"na": ((1, 3), [(1, 2, 1)])}
    for P, (rows, recs) in want.items():
        assert N.pattern_rows(x, sa, P) == rows, P
        got, ndocs, ctr = N.listing(sa, bounds, [rows], 64)
        assert [(int(r["doc"]), int(r["tf"]), int(r["row"])) for r in got] == recs, P
        assert list(ndocs) == [len(recs)] and ctr == {"rows": rows[1] - rows[0], "tiles": 1, "listed": len(recs)}
        assert N.definition(x, bounds, P) == {d: tf for d, tf, _ in recs}, P
    assert N.definition(x, bounds, b"na") == {1: 2}, "x[2 .. 4) starts in document 0 and counts for document 1"


def test_model_against_the_definition(oracle):
    """every block of <= 8 bytes over two symbols, every boundary set, every pattern of 1 .. 3 bytes over those symbols: the (doc, tf)
    of the model's records over the oracle's suffix array are the definition's; records ascend by row, their tf sum to the rows"""
    patterns = [bytes(p) for m in (1, 2, 3) for p in itertools.product((0, 1), repeat=m)]
    cases = crossing = 0
    for n in range(1, 9):
        for tt in itertools.product((0, 1), repeat=n):
            x = bytes(tt)
            sa = oracle.sa(x)
            ranges = [N.pattern_rows(x, sa, P) for P in patterns]
            for bounds in N.boundary_sets(n):
                rec, ndocs, ctr = N.listing(sa, bounds, ranges, 64)
                assert ctr["rows"] == sum(hi - lo for lo, hi in ranges) == int(rec["tf"].sum())
                at = 0
                for j, P in enumerate(patterns):
                    mine = rec[at:at + int(ndocs[j])]
                    at += int(ndocs[j])
                    assert (mine["range"] == j).all()
                    assert (np.diff(mine["row"].astype(np.int64)) > 0).all()
                    want = N.definition(x, bounds, P)
                    assert {int(r["doc"]): int(r["tf"]) for r in mine} == want, (x, bounds, P)
                    cases += 1
                    crossing += len(P) > 1 and len(bounds) > 2 and bool(want)
                assert at == rec.size
    assert cases == sum((1 << n) * (1 << (n - 1)) for n in range(1, 9)) * 14 and crossing > 10000
