"""CPU: the class search entry points (include/archon_hip.h, archon_hip_fm_classes, _fm_classes_dev, _block_fm_classes,
_get_fm_class_stats) are declared, exported and bound; the statistics mirror has the C layout; the table builders give the
classes they name; bad arguments are refused and, without a GPU, the calls fail loudly.  And the rule of the header
(fm_class_naive.search) is pinned to brute force on every short string: hit sets, starts, mismatches, the order and both work
counters."""
import ctypes
import itertools

import numpy as np
import pytest

from fm_abi_util import declared as _declared, layout as _layout, p as _p
import fm_approx_naive as A
import fm_class_naive as C
import fm_sampled_naive as M

FUNCTIONS = ["archon_hip_fm_classes", "archon_hip_fm_classes_dev", "archon_hip_block_fm_classes", "archon_hip_get_fm_class_stats"]


def small_table():
    """the six class names of the exhaustive checks: 0 -> {0}, 1 -> {0, 1}, 2 -> all bytes, 3 -> {1} (a class without its own
    byte), 7 -> empty, 255 -> {255}; every other byte is itself"""
    import pyarchon
    t = pyarchon.classes_identity()
    t = pyarchon.classes_set(t, 1, [0, 1])
    t = pyarchon.classes_set(t, 2, range(256))
    t = pyarchon.classes_set(t, 3, [1])
    t = pyarchon.classes_set(t, 7, [])
    return t


NAMES = (0, 1, 2, 3, 7, 255)


def test_class_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmClassStats", "fm_class_stats", "classes_identity", "classes_fold_case", "classes_iupac", "classes_set"):
        assert hasattr(pyarchon, name), name
    for name in ("classes", "classes_dev"):
        assert hasattr(pyarchon.FmIndex, name), name
    assert hasattr(pyarchon.Block, "fm_classes")


def test_fm_class_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_fm_class_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.FmClassStats._fields_]
    assert names == ["n", "patterns", "max_width", "built", "pattern_bytes", "expansions", "steps", "hits", "occurrences", "kernel_launches",
                     "host_syncs", "ms_build", "ms_width", "ms_count", "ms_emit"]
    got = _layout(tmp_path, "archon_hip_fm_class_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmClassStats)
    assert got[1:] == [getattr(pyarchon.FmClassStats, k).offset for k in names]


def test_table_builders():
    import pyarchon
    ident = pyarchon.classes_identity()
    assert ident.shape == (256, 8) and ident.dtype == np.uint32
    assert C.table_sets(ident) == [[b] for b in range(256)]
    fold = C.table_sets(pyarchon.classes_fold_case())
    for b in range(256):
        if chr(b).isascii() and chr(b).isalpha():
            assert fold[b] == sorted({ord(chr(b).lower()), ord(chr(b).upper())}), b
        else:
            assert fold[b] == [b], b
    assert fold[ord("a")] == [ord("A"), ord("a")] and fold[ord("A")] == [ord("A"), ord("a")]
    assert fold[ord("@")] == [ord("@")] and fold[ord("[")] == [ord("[")] and fold[ord("1")] == [ord("1")]
    iupac = C.table_sets(pyarchon.classes_iupac())
    assert iupac[ord("N")] == sorted(b"ACGT") and ord("N") not in iupac[ord("N")]
    want = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
    for b in range(256):
        assert iupac[b] == (sorted(want[chr(b)].encode()) if chr(b) in want else [b]), b
    one = pyarchon.classes_set(ident, b"?", b"xyz")
    assert C.table_sets(one)[ord("?")] == sorted(b"xyz") and (ident == pyarchon.classes_identity()).all()
    small = C.table_sets(small_table())
    assert [small[b] for b in NAMES] == [[0], [0, 1], list(range(256)), [1], [], [255]]


def test_class_bad_arguments():
    """null pointers, a null table and decreasing offsets are ARCHON_E_ARG with or without a device: they are refused before the
    handle is used (a stand-in handle is never read)"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    pat = np.zeros(8, np.uint8)
    off, bad_off = np.array([0, 2, 4], np.uint32), np.array([0, 3, 2], np.uint32)
    nh, no = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    hits = np.zeros(4, pyarchon.FM_HIT)
    table = pyarchon.classes_identity()
    total = ctypes.c_uint64(0)
    tp = ctypes.byref(total)
    stand_in = _p(np.zeros(64, np.uint8))
    for fn in (L.archon_hip_fm_classes, L.archon_hip_block_fm_classes):
        assert fn(None, _p(pat), _p(off), 2, _p(table), _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, None, _p(off), 2, _p(table), _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), None, 2, _p(table), _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, None, _p(nh), _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, _p(table), None, _p(no), _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, _p(table), _p(nh), None, _p(hits), 4, tp) == E
        assert fn(stand_in, _p(pat), _p(off), 2, _p(table), _p(nh), _p(no), _p(hits), 4, None) == E
        assert fn(stand_in, _p(pat), _p(bad_off), 2, _p(table), _p(nh), _p(no), _p(hits), 4, tp) == E
    dv = L.archon_hip_fm_classes_dev
    assert dv(None, _p(pat), _p(off), 2, _p(table), _p(nh), _p(no), None, 0, tp, None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, None, _p(nh), _p(no), None, 0, tp, None) == E
    assert dv(stand_in, _p(pat), _p(off), 2, _p(table), _p(nh), _p(no), None, 0, None, None) == E
    assert L.archon_hip_get_fm_class_stats(0, None) == E
    if pyarchon.device_count() == 0:
        # a thread that ran no class call has no statistics
        assert L.archon_hip_get_fm_class_stats(0, ctypes.byref(pyarchon.FmClassStats())) == E
    with pytest.raises(ValueError):
        pyarchon._class_table(np.zeros(255 * 8, np.uint32))


def test_class_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).classes([b"?a"], pyarchon.classes_identity())
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_classes([b"?a"], pyarchon.classes_identity())


def test_rule_banana():
    """the worked example of the header"""
    import pyarchon
    sa, bwt, base = M.a7_forward(b"banana")
    assert (bwt, base) == (b"nnbaaa", 2) and list(sa) == [2, 4, 6, 1, 3, 5]
    r = A.Rule(bwt, base)
    table = pyarchon.classes_set(pyarchon.classes_identity(), b"?", range(256))
    sets = C.table_sets(table)
    assert C.search(r, b"?a", table) == ([(0, 1, 1), (1, 3, 1)], 0, 3)
    assert C.width(r, b"?a", sets) == 2
    assert r.search(b"ba", 0)[0] == [(0, 1, 0)] and r.search(b"na", 0)[0] == [(1, 3, 0)]
    assert sa[0] - 2 == 0 and sorted(sa[q] - 2 for q in range(1, 3)) == [2, 4]
    assert C.search(r, b"", table) == ([(0, 6, 0)], 0, 0)
    assert C.search(r, b"???????", table) == ([], 0, 0)
    assert C.search(r, b"b?n?n?", table) == ([(2, 3, 3)], 3, 2)


def test_rule_against_brute_force():
    """every string of length <= 6 over {0, 1, 255}, every pattern of length <= 3 over the six class names of small_table():
    the hits are the distinct strings in the classes with their starts and mismatches, in ascending order of the strings, with
    the rows archon_hip_fm_count gives them; the counters equal the closed forms"""
    table = small_table()
    sets = C.table_sets(table)
    patterns = [bytes(p) for m in range(1, 4) for p in itertools.product(NAMES, repeat=m)]
    cases = 0
    for n in range(1, 7):
        for tt in itertools.product((0, 1, 255), repeat=n):
            x = bytes(tt)
            sa, bwt, base = M.a7_forward(x)
            r = A.Rule(bwt, base)
            for P in patterns:
                m = len(P)
                hits, ex, st = C.search(r, P, table, sets)
                if m > n:
                    assert (hits, ex, st) == ([], 0, 0)
                    continue
                cases += 1
                want, wex, wst = C.brute(x, P, sets)
                assert (ex, st) == (wex, wst), (x, P)
                got, order = {}, []
                for lo, hi, d in hits:
                    starts = sorted(sa[q] - m for q in range(lo, hi))
                    w = x[starts[0]:starts[0] + m]
                    got[w] = (d, starts)
                    order.append(w)
                    assert r.search(w, 0)[0] == [(lo, hi, 0)], (x, P, w)
                assert len(got) == len(hits)
                assert got == want, (x, P)
                assert order == sorted(order), (x, P)
                assert C.search.pending <= C.width(r, P, sets), (x, P)
    assert cases == 279036
