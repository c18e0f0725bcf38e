"""CPU: the repeats entry points (include/archon_hip.h, archon_hip_repeats*) are declared, exported and bound; the record and
the statistics mirror have the C layout; they refuse bad arguments and, without a GPU, fail loudly.  And the expected answer
of the GPU tests, tests/repeats_naive.c, is pinned to the definition in terms of the text."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import repeats_naive as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["archon_hip_repeats", "archon_hip_repeats_dev", "archon_hip_block_repeats", "archon_hip_get_repeat_stats"]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(archon_[a-z0-9_]+)\s*\(", src))


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("repeats_naive"))


def test_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
    assert "REP_FAN" in pyarchon._ROUTE_NAMES
    assert "REP_FAN" in open(os.path.join(ROOT, "include", "archon_hip_test.h")).read()
    for name in ("repeats", "repeats_dev", "repeat_stats", "REPEAT", "RepeatStats"):
        assert hasattr(pyarchon, name), name
    for name in ("repeats", "locate_repeats"):
        assert hasattr(pyarchon.Block, name), name
    assert hasattr(pyarchon.FmIndex, "locate_repeats")


def test_struct_layouts(tmp_path):
    """archon_hip_repeat is 16 bytes in the order of the numpy dtype; the ctypes mirror of archon_hip_repeat_stats has the size
    and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.RepeatStats._fields_]
    fields = ["lo", "hi", "len", "row"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%zu", sizeof(archon_hip_repeat_stats));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_repeat_stats, %s));' % k for k in names)
                   + 'printf(" %zu", sizeof(archon_hip_repeat));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_repeat, %s));' % k for k in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = len(names)
    assert got[0] == ctypes.sizeof(pyarchon.RepeatStats)
    assert got[1:1 + k] == [getattr(pyarchon.RepeatStats, f).offset for f in names]
    assert got[1 + k] == 16 == pyarchon.REPEAT.itemsize == R.REPEAT.itemsize
    assert got[2 + k:] == [pyarchon.REPEAT.fields[f][1] for f in fields] == [0, 4, 8, 12]
    assert pyarchon.REPEAT == R.REPEAT


def _banana():
    lcp = np.array([0, 1, 3, 0, 0, 2], np.uint32)
    bwt = np.frombuffer(b"nnbaaa", np.uint8).copy()
    return lcp, bwt, 2


def test_bad_arguments():
    """null pointers, n = 0, a primary row past the block and kind 3 are ARCHON_E_ARG, with or without a device; so is a
    fan-out that is no power of two in [2, 64]"""
    import pyarchon
    L = pyarchon.lib()
    lcp, bwt, base = _banana()
    out = np.zeros(8, pyarchon.REPEAT)
    total = ctypes.c_uint64(7)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    for fn, tail in ((L.archon_hip_repeats, (0,)), (L.archon_hip_repeats_dev, (0, None))):
        assert fn(None, p(bwt), 6, base, 1, 1, 2, p(out), 8, tp, *tail) == pyarchon.E_ARG
        assert fn(p(lcp), None, 6, base, 1, 1, 2, p(out), 8, tp, *tail) == pyarchon.E_ARG
        assert fn(p(lcp), p(bwt), 6, base, 1, 1, 2, p(out), 8, None, *tail) == pyarchon.E_ARG
        assert fn(p(lcp), p(bwt), 0, 0, 1, 1, 2, p(out), 8, tp, *tail) == pyarchon.E_ARG
        assert fn(p(lcp), p(bwt), 6, 6, 1, 1, 2, p(out), 8, tp, *tail) == pyarchon.E_ARG
        assert fn(p(lcp), p(bwt), 6, base, 3, 1, 2, p(out), 8, tp, *tail) == pyarchon.E_ARG
    assert L.archon_hip_block_repeats(None, 1, 1, 2, p(out), 8, tp) == pyarchon.E_ARG
    assert L.archon_hip_get_repeat_stats(0, None) == pyarchon.E_ARG
    assert not out.view(np.uint32).any()
    for bad in (3, 128, 1, -2, 48):
        assert L.archon_hip_test_route(b"REP_FAN", bad) == pyarchon.E_ARG, bad
    for good in (2, 4, 8, 16, 32, 64, 0):
        assert L.archon_hip_test_route(b"REP_FAN", good) == 0, good
    assert L.archon_hip_test_route(b"RESET", 0) == 0


def test_without_a_device():
    """no CPU fallback: without a GPU every repeats entry point is ARCHON_E_NODEVICE (with one, the host form answers)"""
    import pyarchon
    L = pyarchon.lib()
    lcp, bwt, base = _banana()
    out = np.zeros(8, pyarchon.REPEAT)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    if pyarchon.device_count() > 0:
        assert L.archon_hip_repeats(p(lcp), p(bwt), 6, base, 0, 1, 2, p(out), 8, tp, 0) == 0
        assert total.value == 3 and out[:3].tolist() == [(0, 3, 1, 1), (1, 3, 3, 2), (4, 6, 2, 5)]
        return
    assert L.archon_hip_repeats(p(lcp), p(bwt), 6, base, 1, 1, 2, p(out), 8, tp, 0) == pyarchon.E_NODEVICE
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_repeats_dev(p(lcp), p(bwt), 6, base, 1, 1, 2, p(out), 8, tp, 0, None) == pyarchon.E_NODEVICE
    assert L.archon_hip_repeats(p(lcp), p(bwt), 1, 0, 1, 1, 2, None, 0, tp, 0) == pyarchon.E_NODEVICE
    h = ctypes.c_void_p(None)
    assert L.archon_hip_block_create(0, ctypes.byref(h)) == pyarchon.E_NODEVICE     # so no handle reaches block_repeats
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.repeats(lcp, bwt, base)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.repeats(lcp, bwt, base, kind=2, count_only=True)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.repeat_stats()


EXAMPLES = [
    (b"banana", 0, [(0, 3, 1, 1), (1, 3, 3, 2), (4, 6, 2, 5)]),
    (b"banana", 1, [(0, 3, 1, 1), (1, 3, 3, 2)]),
    (b"banana", 2, [(1, 3, 3, 2)]),
    (b"abracadabra", 1, [(0, 5, 1, 1), (2, 4, 4, 3)]),
    (b"abracadabra", 2, [(2, 4, 4, 3)]),
]


@pytest.mark.parametrize("x,kind,want", EXAMPLES)
def test_worked_examples(naive, x, kind, want):
    """the examples of the header, through the definition and through the helper"""
    sa, lcp, bwt, base = R.a7_arrays(x)
    if x == b"banana":
        assert (sa, lcp, bwt, base) == ([2, 4, 6, 1, 3, 5], [0, 1, 3, 0, 0, 2], b"nnbaaa", 2)
    picked, _ = R.definition(x, kind)
    assert sorted((R.rows_of(x, sa, lcp, u, ps) for u, ps in picked.items()), key=lambda r: r[3]) == want
    got = naive(lcp, np.frombuffer(bwt, np.uint8), base, kind)[0]
    assert got.tolist() == want
    if x == b"abracadabra":
        assert {u for u in picked} == ({b"a", b"abra"} if kind == 1 else {b"abra"})


def test_naive_helper_is_the_definition(naive):
    """tests/repeats_naive.c against the definition on every string of length 1-7 over {0, 1, 255}: all three kinds, min_len
    1-3, min_occ 2-3; rows, order, starts, the counters, and distinct substrings = n (n + 1) / 2 - sum of lcp"""
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            sa, lcp, bwt, base = R.a7_arrays(x)
            bwt_a = np.frombuffer(bwt, np.uint8)
            nsub = None
            all_intervals = len(R.definition(x, 0)[0])
            for kind in (0, 1, 2):
                for min_len in (1, 2, 3):
                    for min_occ in (2, 3):
                        picked, nsub = R.definition(x, kind, min_len, min_occ)
                        want = sorted((R.rows_of(x, sa, lcp, u, ps) for u, ps in picked.items()), key=lambda r: r[3])
                        got, intervals, occurrences, longest = naive(lcp, bwt_a, base, kind, min_len, min_occ)
                        assert got.tolist() == want, (x, kind, min_len, min_occ)
                        assert occurrences == sum(len(ps) for ps in picked.values())
                        assert longest == max([len(u) for u in picked], default=0)
                        assert intervals == all_intervals, x
                        assert naive(lcp, bwt_a, base, kind, min_len, min_occ, count_only=True)[0] == len(want)
                        for (lo, hi, m, _), u in zip(want, sorted(picked, key=lambda u: R.rows_of(x, sa, lcp, u, picked[u])[3])):
                            assert sorted(sa[r] - m for r in range(lo, hi)) == picked[u]
                            assert all(x[sa[r] - m:sa[r]] == u for r in range(lo, hi))
            assert nsub == n * (n + 1) // 2 - sum(lcp), x
            # filters given as 0 / 1 behave as 1 and 2
            assert naive(lcp, bwt_a, base, 1, 0, 0)[0].tolist() == naive(lcp, bwt_a, base, 1, 1, 2)[0].tolist()
