"""CPU: the minimal-absent-words entry points (include/archon_hip.h, archon_hip_maws*) are declared, exported and bound; the
record and the statistics mirror have the C layout; they refuse bad arguments and, without a GPU, fail loudly; the getter
refuses as its siblings do.  And the expected answers of the GPU tests, tests/maw_naive.py: the header's examples record by
record, and the rule over the arrays pinned to the definition by the text."""
import ctypes
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import maw_naive as M
import repeats_naive as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["archon_hip_maws", "archon_hip_maws_dev", "archon_hip_block_maws", "archon_hip_maw_last_stats"]
FIELDS = ["n", "min_len", "max_len", "fan", "levels", "direct_rows", "built", "kernel_launches", "host_syncs", "absent_bytes", "shortest",
          "longest", "intervals", "nodes", "children", "sets_direct", "sets_table", "words", "probes", "ms_lcp", "ms_build", "ms_count",
          "ms_emit"]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(archon_[a-z0-9_]+)\s*\(", src))


def test_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
    for name in ("MAW", "MawStats", "maws", "maws_dev", "maw_stats", "maw_bytes"):
        assert hasattr(pyarchon, name), name
    assert hasattr(pyarchon.Block, "maws")
    assert [k for k, _ in pyarchon.MawStats._fields_] == FIELDS


def test_struct_layouts(tmp_path):
    """archon_hip_maw is 20 bytes with its words at 0, 4, 8, 12, 16, in the order of the numpy dtype; the ctypes mirror of
    archon_hip_maw_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    fields = ["lo", "hi", "len", "item", "last"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%zu", sizeof(archon_hip_maw_stats));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_maw_stats, %s));' % k for k in FIELDS)
                   + 'printf(" %zu", sizeof(archon_hip_maw));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_maw, %s));' % k for k in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = len(FIELDS)
    assert got[0] == ctypes.sizeof(pyarchon.MawStats)
    assert got[1:1 + k] == [getattr(pyarchon.MawStats, f).offset for f in FIELDS]
    assert got[1 + k] == 20 == pyarchon.MAW.itemsize == M.MAW.itemsize
    assert got[2 + k:] == [pyarchon.MAW.fields[f][1] for f in fields] == [0, 4, 8, 12, 16]
    assert pyarchon.MAW == M.MAW


def _banana():
    return (np.array([2, 4, 6, 1, 3, 5], np.uint32), np.array([0, 1, 3, 0, 0, 2], np.uint32), np.frombuffer(b"nnbaaa", np.uint8).copy(), 2)


def test_bad_arguments():
    """null pointers, n = 0, base_id >= n and min_len > max_len != 0 are ARCHON_E_ARG, with or without a device, and *total is
    written 0; the output stays untouched"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp, bwt, base = _banana()
    out = np.zeros(8, pyarchon.MAW)
    total = ctypes.c_uint64(7)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    E = pyarchon.E_ARG
    for fn, tail in ((L.archon_hip_maws, (0,)), (L.archon_hip_maws_dev, (0, None))):
        assert fn(p(sa), p(lcp), p(bwt), 6, base, 2, 0, p(out), 8, None, *tail) == E
        for a, b, c, n, bid, lo, hi in ((None, p(lcp), p(bwt), 6, base, 2, 0), (p(sa), None, p(bwt), 6, base, 2, 0), (p(sa), p(lcp), None, 6, base, 2, 0),
                                        (p(sa), p(lcp), p(bwt), 0, 0, 2, 0), (p(sa), p(lcp), p(bwt), 6, 6, 2, 0), (p(sa), p(lcp), p(bwt), 6, 7, 2, 0),
                                        (p(sa), p(lcp), p(bwt), 6, base, 3, 2), (p(sa), p(lcp), p(bwt), 6, base, 9, 1)):
            total.value = 7
            assert fn(a, b, c, n, bid, lo, hi, p(out), 8, tp, *tail) == E, (n, bid, lo, hi)
            assert total.value == 0
    total.value = 7
    assert L.archon_hip_block_maws(None, 2, 0, p(out), 8, tp) == E and total.value == 0
    assert L.archon_hip_block_maws(None, 2, 0, p(out), 8, None) == E
    assert not out.view(np.uint32).any()


def test_getter_refusals():
    """a null out is "null pointer"; a thread that has run no such call is told so, with the device's number"""
    import pyarchon
    L = pyarchon.lib()
    got = {}

    def ask():
        st = pyarchon.MawStats()
        got["null"] = (L.archon_hip_maw_last_stats(0, None), L.archon_hip_last_error())
        got["none"] = (L.archon_hip_maw_last_stats(3, ctypes.byref(st)), L.archon_hip_last_error())

    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got["null"] == (pyarchon.E_ARG, b"null pointer")
    assert got["none"] == (pyarchon.E_ARG, b"the calling thread has run no minimal-absent-words call on device 3")


def test_without_a_device():
    """no CPU fallback: without a GPU a good call is ARCHON_E_NODEVICE (with one, the host form answers the header's example)"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp, bwt, base = _banana()
    out = np.zeros(8, pyarchon.MAW)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    if pyarchon.device_count() > 0:
        assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), 6, base, 2, 0, p(out), 8, tp, 0) == 0
        assert total.value == 7 and out[:7].tolist() == BANANA
        return
    N = pyarchon.E_NODEVICE
    assert L.archon_hip_maws(p(sa), p(lcp), p(bwt), 6, base, 2, 0, p(out), 8, tp, 0) == N
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_maws_dev(p(sa), p(lcp), p(bwt), 6, base, 2, 0, p(out), 8, tp, 0, None) == N
    for call in (lambda: pyarchon.maws(sa, lcp, bwt, base), lambda: pyarchon.maws(sa, lcp, bwt, base, count_only=True), pyarchon.maw_stats):
        with pytest.raises(pyarchon.ArchonError):
            call()
    assert not out.view(np.uint32).any()


A, B, N_ = ord("a"), ord("b"), ord("n")
BANANA = [(0, 3, 2, 2, A), (0, 3, 2, 2, B), (3, 4, 2, 1, B), (3, 4, 2, 1, N_), (4, 6, 2, 3, B), (4, 6, 2, 3, N_), (2, 3, 5, 6, N_)]


def test_worked_examples():
    """the header's examples through the rule, record by record, and pyarchon.maw_bytes"""
    import pyarchon
    x = b"banana"
    sa, lcp, bwt, base = R.a7_arrays(x)
    assert (sa, lcp, bwt, base) == ([2, 4, 6, 1, 3, 5], [0, 1, 3, 0, 0, 2], b"nnbaaa", 2)
    recs, c = M.model(sa, lcp, bwt, base)
    assert recs.tolist() == BANANA
    assert [pyarchon.maw_bytes(x, r) for r in recs] == [M.word(x, r) for r in recs] == [b"aa", b"ab", b"bb", b"bn", b"nb", b"nn", b"nanan"]
    # the root (three children), "a" (0,3,1,1) and "ana" (1,3,3,2) (two each); "an" (4,6,2,5) is right-uniform.  One set per node
    # and one per child: none of banana's children is INF
    assert c == dict(intervals=3, nodes=3, children=7, sets_direct=10, sets_table=0, words=7, shortest=2, longest=5, absent_bytes=253)

    x = b"abracadabra"
    sa, lcp, bwt, base = R.a7_arrays(x)
    recs, c = M.model(sa, lcp, bwt, base)
    words = [M.word(x, r) for r in recs]
    assert len(words) == 25 and sum(len(w) == 2 for w in words) == 18 and words[:18] == [w for w in words if len(w) == 2]
    assert words[18:] == [b"cab", b"cac", b"dac", b"dad", b"rab", b"rad", b"dabrac"]
    # the node (0,5,1,1) "a": children [0,1) c, [1,2) d, [2,4) r, the INF row 4 of item 1; the node (2,4,4,3) "abra"
    assert (sa[4], lcp[4]) == (1, 1)
    assert recs[18:].tolist() == [(0, 1, 3, 6, ord("b")), (0, 1, 3, 6, ord("c")), (1, 2, 3, 8, ord("c")), (1, 2, 3, 8, ord("d")),
                                  (2, 4, 3, 11, ord("b")), (2, 4, 3, 11, ord("d")), (2, 3, 6, 11, ord("c"))]
    assert (c["nodes"], c["children"], c["intervals"], c["absent_bytes"]) == (3, 11, 4, 251)
    assert set(words) == M.definition(x)

    for n in (1, 2, 7):
        x = b"c" * n
        sa, lcp, bwt, base = R.a7_arrays(x)
        recs, c = M.model(sa, lcp, bwt, base)
        assert [M.word(x, r) for r in recs] == [b"c" * (n + 1)] and base == 0
        assert recs.tolist() == [(0, 1, n + 1, n, ord("c"))]
        assert (c["words"], c["shortest"], c["longest"], c["absent_bytes"], c["intervals"]) == (1, n + 1, n + 1, 255, n - 1)


def test_filters_of_the_model():
    """the filters keep min_len <= len <= max_len, 0 and 1 behave as 2, and a node outside does no work"""
    x = b"abracadabra"
    sa, lcp, bwt, base = R.a7_arrays(x)
    full, c = M.model(sa, lcp, bwt, base)
    for lo, hi in ((0, 0), (1, 0), (2, 2), (3, 0), (4, 6), (7, 9), (3, 3)):
        got, cf = M.model(sa, lcp, bwt, base, lo, hi)
        keep = (full["len"] >= max(lo, 2)) & (full["len"] <= (hi or 1 << 30))
        assert got.tolist() == full[keep].tolist(), (lo, hi)
        assert cf["intervals"] == c["intervals"] and cf["absent_bytes"] == c["absent_bytes"]
        assert cf["nodes"] <= c["nodes"] and cf["children"] <= c["children"]
    assert M.model(sa, lcp, bwt, base, 7, 9)[1]["nodes"] == 0


def test_model_is_the_definition():
    """the rule over the arrays against the definition by the text, on 360 random strings of length 1 to 24 over 2, 3 and 4
    letters: the same set of words, no word twice"""
    rng = np.random.default_rng(20261020)
    for sigma in (2, 3, 4):
        for i in range(120):
            n = 1 + i % 24
            x = bytes(rng.integers(0, sigma, n).astype(np.uint8) + 97)
            sa, lcp, bwt, base = R.a7_arrays(x)
            recs, c = M.model(sa, lcp, bwt, base, direct_rows=4)
            words = [M.word(x, r) for r in recs]
            assert len(set(words)) == len(words), x
            assert set(words) == M.definition(x), x
            assert c["absent_bytes"] == 256 - len(set(x)) and c["children"] <= 2 * n
            for r, w in zip(recs, words):
                assert w not in x and w[:-1] in x and w[1:] in x


def test_bitmap_helper_is_the_definition():
    """words_of_length (presence bitmaps of 2-bit codes, what the GPU test at two million rows compares with) against the
    definition by the text on the random strings over 2, 3 and 4 letters, at every length from 2 to n + 1; record_codes gives
    the codes of the model's records"""
    rng = np.random.default_rng(20261021)
    for sigma in (2, 3, 4):
        for i in range(90):
            n = 1 + i % 18
            x = bytes(rng.integers(0, sigma, n).astype(np.uint8) + 97)
            xa = np.frombuffer(x, np.uint8)
            words = M.definition(x)
            recs = M.model(*R.a7_arrays(x))[0]
            seen = 0
            for L in range(2, min(n + 2, 12)):
                codes = M.words_of_length(xa, L)
                assert {M.code_bytes(c, L) for c in codes.tolist()} == {w for w in words if len(w) == L}, (x, L)
                assert (np.diff(codes) > 0).all()
                assert sorted(M.record_codes(xa, recs[recs["len"] == L], L).tolist()) == codes.tolist(), (x, L)
                seen += codes.size
            assert seen == sum(len(w) < 12 for w in words)
