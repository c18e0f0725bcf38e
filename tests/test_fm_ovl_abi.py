"""CPU: the suffix-prefix overlaps (include/archon_hip.h: archon_hip_fm_attach_ends, _fm_attach_ends_dev, _block_fm_attach_ends,
_fm_overlaps, _fm_overlaps_dev, _fm_ovl_last_stats, and the record archon_hip_fm_ovl) are declared, exported and bound; the record
and the statistics mirror have the C layout; bad arguments are refused and, without a GPU, the calls fail loudly.  And the model of
the search over a suffix array (fm_ovl_naive.model) is pinned to the DEFINITION from the text alone (fm_ovl_naive.definition) on
every short block, set of ends and query; the host helpers of pyarchon are held to plain loops."""
import ctypes
import inspect
import itertools
import re

import numpy as np
import pytest

from fm_abi_util import ROOT, declared as _declared, layout as _layout, p as _p
import fm_ovl_naive as N

FUNCTIONS = ["archon_hip_fm_attach_ends", "archon_hip_fm_attach_ends_dev", "archon_hip_block_fm_attach_ends", "archon_hip_fm_overlaps",
             "archon_hip_fm_overlaps_dev", "archon_hip_fm_ovl_last_stats"]
FIELDS = ["n", "docs", "queries", "min_len", "attached", "longest", "pattern_bytes", "steps", "tested", "hit", "overlaps", "emitted",
          "end_bytes", "kernel_launches", "host_syncs", "ms_attach", "ms_count", "ms_emit", "reserved0"]
RECORD = ["query", "doc", "len", "row"]


def test_ovl_functions_declared_exported_and_bound():
    """the six functions and the record: seven symbols of the header, each exported by the library and bound by pyarchon"""
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"\}\s*archon_hip_fm_ovl;", open(ROOT + "/include/archon_hip.h").read())
    for name in ("FmOvlStats", "fm_ovl_stats", "FM_OVL", "ends_from_bounds", "best_overlaps", "drop_self"):
        assert hasattr(pyarchon, name), name
    for name in ("attach_ends", "attach_ends_dev", "overlaps", "overlaps_dev"):
        assert hasattr(pyarchon.FmIndex, name), name
    params = inspect.signature(pyarchon.Block.fm_index).parameters
    assert params["ends"].default is None and list(params)[-1] == "lcp"
    assert inspect.signature(pyarchon.FmIndex.overlaps).parameters["emit"].default is True
    assert pyarchon.FM_OVL == N.FM_OVL


def test_fm_ovl_struct_layouts(tmp_path):
    """sizeof(archon_hip_fm_ovl) == 16, four words in the order of the rule, and FM_OVL is it; the statistics record has the
    fields of the header in its order, 8-byte fields on 8-byte offsets, and the ctypes mirror the C compiler's offsets"""
    import pyarchon
    rec = _layout(tmp_path, "archon_hip_fm_ovl", RECORD)
    assert rec == [16, 0, 4, 8, 12]
    assert pyarchon.FM_OVL.itemsize == 16 and [pyarchon.FM_OVL.fields[k][1] for k in RECORD] == rec[1:]
    src = open(ROOT + "/include/archon_hip.h").read()
    body = re.search(r"typedef struct archon_hip_fm_ovl_stats \{(.*?)\} archon_hip_fm_ovl_stats;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    names = [k for k, _ in pyarchon.FmOvlStats._fields_]
    assert names == FIELDS
    got = _layout(tmp_path, "archon_hip_fm_ovl_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmOvlStats)
    assert got[1:] == [getattr(pyarchon.FmOvlStats, k).offset for k in names]
    for k, t in pyarchon.FmOvlStats._fields_:
        if ctypes.sizeof(t) == 8:
            assert getattr(pyarchon.FmOvlStats, k).offset % 8 == 0, k


def test_ovl_bad_arguments():
    """a NULL handle, NULL ends, ndocs = 0, ends that do not increase from 1, min_len = 0 and a NULL total are ARCHON_E_ARG with or
    without a device: they are refused before the handle is read (a stand-in handle is never used); *total is written 0 before a
    refusal, and nothing else is written"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    stand_in = _p(np.zeros(64, np.uint8))
    good = np.array([3, 6], np.uint32)
    pat, off = np.frombuffer(b"anab", np.uint8).copy(), np.array([0, 3, 4], np.uint32)
    novl = np.full(8, 9, np.uint32)
    rec = np.zeros(8, pyarchon.FM_OVL)
    total = ctypes.c_uint64(5)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    assert L.archon_hip_fm_attach_ends(None, _p(good), 2) == E
    assert L.archon_hip_fm_attach_ends(stand_in, None, 2) == E
    assert L.archon_hip_fm_attach_ends(stand_in, _p(good), 0) == E
    assert L.archon_hip_fm_attach_ends_dev(None, _p(good), 2, None) == E
    assert L.archon_hip_fm_attach_ends_dev(stand_in, None, 2, None) == E
    assert L.archon_hip_fm_attach_ends_dev(stand_in, _p(good), 0, None) == E
    assert L.archon_hip_block_fm_attach_ends(None, stand_in, _p(good), 2) == E
    assert L.archon_hip_block_fm_attach_ends(stand_in, None, _p(good), 2) == E
    assert L.archon_hip_block_fm_attach_ends(stand_in, stand_in, None, 2) == E
    assert L.archon_hip_block_fm_attach_ends(stand_in, stand_in, _p(good), 0) == E
    for bad in ([0, 3], [3, 3], [4, 3], [0], [2, 5, 5]):
        bb = np.array(bad, np.uint32)
        assert L.archon_hip_fm_attach_ends(stand_in, _p(bb), bb.size) == E, bad
        assert b"FM attach ends" in L.archon_hip_last_error()
        assert L.archon_hip_block_fm_attach_ends(stand_in, stand_in, _p(bb), bb.size) == E, bad
    for fn, tail in ((L.archon_hip_fm_overlaps, ()), (L.archon_hip_fm_overlaps_dev, (None,))):
        for args in ((None, _p(pat), _p(off), 2, 1, _p(novl), _p(rec), 8, tp), (stand_in, None, _p(off), 2, 1, _p(novl), _p(rec), 8, tp),
                     (stand_in, _p(pat), None, 2, 1, _p(novl), _p(rec), 8, tp), (stand_in, _p(pat), _p(off), 2, 1, None, _p(rec), 8, tp),
                     (stand_in, _p(pat), _p(off), 2, 0, _p(novl), _p(rec), 8, tp), (stand_in, _p(pat), _p(off), 2, 0, _p(novl), None, 0, tp)):
            total.value = 5
            assert fn(*args, *tail) == E
            assert total.value == 0
        assert b"min_len = 0" in L.archon_hip_last_error()
        assert fn(stand_in, _p(pat), _p(off), 2, 1, _p(novl), _p(rec), 8, None, *tail) == E
    assert (novl == 9).all() and not rec.view(np.uint32).any()
    assert L.archon_hip_fm_ovl_last_stats(0, None) == E
    if pyarchon.device_count() == 0:
        assert L.archon_hip_fm_ovl_last_stats(0, ctypes.byref(pyarchon.FmOvlStats())) == E


def test_ovl_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).attach_sa(np.array([2, 4, 6, 1, 3, 5], np.uint32)).attach_ends([3, 6])
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_index(32, ends=[3, 6])


def test_model_header_examples(oracle):
    """the worked example of the header, literally: "banana" whose documents "ban" and "ana" end at items 3 and 6"""
    x, ends = b"banana", [3, 6]
    sa = oracle.sa(x)
    assert list(sa) == [2, 4, 6, 1, 3, 5]
    w = N.Walker(x, sa)
    assert N.end_rows(w, ends) == ([2, 4], [1, 0])
    assert w.walk(b"ana") == ([(0, 3), (4, 6), (1, 3)], 2) and w.walk(b"nab") == ([(4, 6), (1, 3)], 2)
    rec, novl, ctr = N.model(w, ends, [b"ana", b"nab"], 1)
    assert [tuple(int(v) for v in r) for r in rec] == [(0, 1, 1, 2), (0, 0, 2, 4), (0, 1, 3, 2), (1, 0, 1, 4), (1, 1, 2, 2)]
    assert list(novl) == [3, 2] and ctr == {"steps": 4, "tested": 5, "hit": 5, "overlaps": 5, "longest": 3}
    assert N.definition(x, ends, [b"ana", b"nab"], 1) == {(0, 1, 1), (0, 0, 2), (0, 1, 3), (1, 0, 1), (1, 1, 2)}
    assert N.definition(x, ends, [b"ana"], 3) == {(0, 1, 3)}
    # a query longer than the block is walked as its first n bytes; the whole query as a suffix of a document is an overlap
    rec, novl, ctr = N.model(w, [6], [b"bananas", b"banana", b""], 6)
    assert [tuple(int(v) for v in r) for r in rec] == [(0, 0, 6, 2), (1, 0, 6, 2)] and list(novl) == [1, 1, 0]
    assert ctr == {"steps": 10, "tested": 2, "hit": 2, "overlaps": 2, "longest": 6}
    assert N.end_bytes(6, 2) == 512 and N.end_bytes(1 << 24, 4096) == 49152 + 2359552


def _queries(alphabet, most):
    """every string of 1 .. most bytes over the alphabet: the largest prefix-closed set of queries.  A query's records depend on
    no other query, so every prefix-closed set is a sub-list of these (test_queries_do_not_depend_on_each_other)"""
    return [bytes(p) for m in range(1, most + 1) for p in itertools.product(alphabet, repeat=m)]


def _end_sets(n):
    """every non-empty subset of 1 .. n, ascending"""
    for mask in range(1, 1 << n):
        yield [e for e in range(1, n + 1) if mask >> (e - 1) & 1]


def _check_block(oracle, x, queries, tally):
    """model == definition on block x with every set of ends and min_len 1 and 2; the records come in the stated order, their row
    is the document's end row, novl and the counters are the records' and the text's"""
    sa = oracle.sa(x)
    w = N.Walker(x, sa)
    walks = [w.walk(Q) for Q in queries]
    isa = w.isa
    for min_len in (1, 2):
        steps, tested = N.text_counters(x, queries, min_len)
        for ends in _end_sets(len(x)):
            rec, novl, ctr = N.model(w, ends, queries, min_len, walks=walks)
            triples = [(int(r["query"]), int(r["doc"]), int(r["len"])) for r in rec]
            assert set(triples) == N.definition(x, ends, queries, min_len) and len(set(triples)) == len(triples), (x, ends, min_len)
            keys = [(int(r["query"]), int(r["len"]), int(r["row"])) for r in rec]
            assert keys == sorted(keys) and len(set(keys)) == len(keys), (x, ends, min_len)
            assert all(int(r["row"]) == isa[ends[int(r["doc"])]] for r in rec)
            assert novl.tolist() == np.bincount(rec["query"], minlength=len(queries)).tolist()
            assert ctr == {"steps": steps, "tested": tested, "hit": len({(q, l) for q, _, l in triples}), "overlaps": len(triples),
                           "longest": max((l for _, _, l in triples), default=0)}, (x, ends, min_len)
            tally["cases"] += 1
            tally["overlaps"] += len(triples)
            tally["primary"] += ends[-1] == len(x) and any(int(r["row"]) == isa[len(x)] for r in rec)
            tally["whole"] += any(l == len(queries[q]) for q, _, l in triples)
            tally["before"] += any(l > ends[d] - (ends[d - 1] if d else 0) for _, d, l in triples)


def test_model_against_the_definition_two_letters(oracle):
    """every block of 1 .. 7 bytes over {a, b}, every non-empty subset of 1 .. n as ends, every query of 1 .. 4 bytes over {a, b}
    (the prefix-closed sets: see _queries), min_len 1 and 2.  Among them: ends[D-1] = n with the primary row as an end row that
    overlaps, whole queries as suffixes, pieces that begin before their document does"""
    queries = _queries(b"ab", 4)
    assert len(queries) == 30
    tally = dict(cases=0, overlaps=0, primary=0, whole=0, before=0)
    for n in range(1, 8):
        for tt in itertools.product(b"ab", repeat=n):
            _check_block(oracle, bytes(tt), queries, tally)
    assert tally["cases"] == 2 * sum((1 << n) * ((1 << n) - 1) for n in range(1, 8))
    assert tally["overlaps"] > 100000 and tally["primary"] > 1000 and tally["whole"] > 1000 and tally["before"] > 1000


def test_model_against_the_definition_three_letters(oracle):
    """three blocks of up to 5 bytes over {a, b, c}, every set of ends, every query of 1 .. 4 bytes over {a, b, c}"""
    queries = _queries(b"abc", 4)
    assert len(queries) == 120
    tally = dict(cases=0, overlaps=0, primary=0, whole=0, before=0)
    for x in (b"abcab", b"cbac", b"bccbc"):
        _check_block(oracle, x, queries, tally)
    assert tally["cases"] == 2 * (31 + 15 + 31) and tally["overlaps"] > 500


def test_queries_do_not_depend_on_each_other(oracle):
    """the records of a prefix-closed set of queries are those of the same queries inside the set of all of them: random
    prefix-closed sets, drawn by closing random picks under prefixes"""
    queries = _queries(b"ab", 4)
    rng = np.random.default_rng(7)
    for x, ends in ((b"abbabab", [2, 5, 7]), (b"aabab", [1, 2, 3, 4, 5]), (b"bbbbbb", [3, 6])):
        w = N.Walker(x, oracle.sa(x))
        rec, novl, _ = N.model(w, ends, queries, 1)
        for _ in range(40):
            picks = {queries[i] for i in rng.integers(0, len(queries), int(rng.integers(1, 6)))}
            closed = sorted({Q[:l] for Q in picks for l in range(1, len(Q) + 1)}, key=queries.index)
            sub, sub_novl, _ = N.model(w, ends, closed, 1)
            idx = [queries.index(Q) for Q in closed]
            assert sub_novl.tolist() == novl[idx].tolist()
            want = np.concatenate([rec[rec["query"] == i] for i in idx])
            assert [tuple(r)[1:] for r in sub.tolist()] == [tuple(r)[1:] for r in want.tolist()]


def test_host_helpers_against_plain_loops():
    """ends_from_bounds, best_overlaps and drop_self of pyarchon against loops, on records in the order of the rule"""
    import pyarchon
    assert pyarchon.ends_from_bounds([0, 3, 6]).tolist() == [3, 6] and pyarchon.ends_from_bounds([0, 3, 6]).dtype == np.uint32
    assert pyarchon.ends_from_bounds([0, 3, 6, 10], trim=1).tolist() == [2, 5, 9]
    assert pyarchon.ends_from_bounds([0, 3, 6, 10], trim=2).tolist() == [1, 4, 8]
    for bounds, trim in (([0, 3, 6, 10], 3), ([0, 1, 5], 1), ([0, 4, 4], 0), ([0], 0), ([0, 3], -1)):
        with pytest.raises(ValueError):
            pyarchon.ends_from_bounds(bounds, trim=trim)
    rng = np.random.default_rng(11)
    for size in (0, 1, 2, 50, 3000):
        rec = np.zeros(size, pyarchon.FM_OVL)
        rec["query"], rec["doc"] = rng.integers(0, 9, size), rng.integers(0, 7, size)
        rec["len"], rec["row"] = rng.integers(1, 30, size), rng.integers(0, 1000, size)
        rec = rec[np.lexsort((rec["row"], rec["len"], rec["query"]))]           # the order of the rule
        _, first = np.unique(rec[["query", "doc", "len"]], return_index=True)   # a pair has one record per length
        rec = rec[np.sort(first)]
        best = pyarchon.best_overlaps(rec)
        assert best.tobytes() == N.best_loop(rec).tobytes()
        assert len({(int(r["query"]), int(r["doc"])) for r in best}) == best.size
        own = rng.integers(0, 7, 9)
        kept = pyarchon.drop_self(rec, own)
        loop = [r for r in rec.tolist() if own[r[0]] != r[1]]
        assert kept.tolist() == loop
        assert pyarchon.drop_self(best, own).tobytes() == pyarchon.best_overlaps(kept).tobytes()
