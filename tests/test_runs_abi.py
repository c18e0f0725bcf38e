"""CPU: the runs and LCE entry points (include/archon_hip.h, archon_hip_runs*, archon_hip_lce*) are declared, exported and bound;
the record and the statistics mirror have the C layout; they refuse bad arguments and, without a GPU, fail loudly; the getter
refuses as its siblings do.  And the expected answers of the GPU tests, tests/runs_naive.py: the header's four examples with
their counters, and the rule and the short-period finder pinned to the definition on every tiny string."""
import ctypes
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import repeats_naive as R
import runs_naive as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["archon_hip_lce", "archon_hip_lce_dev", "archon_hip_block_lce", "archon_hip_runs", "archon_hip_runs_dev", "archon_hip_block_runs",
             "archon_hip_runs_last_stats"]
FIELDS = ["n", "min_period", "max_period", "min_copies", "min_len", "what", "fan", "lcp_fan", "levels", "longest_period", "kernel_launches",
          "host_syncs", "candidates", "roots", "lce_queries", "probes", "runs", "emitted", "ms_forward", "ms_lcp", "ms_build", "ms_count",
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
    for name in ("RUN", "RunStats", "lce", "lce_dev", "runs", "runs_dev", "runs_of", "run_stats"):
        assert hasattr(pyarchon, name), name
    assert hasattr(pyarchon.Block, "lce") and hasattr(pyarchon.Block, "runs")
    assert [k for k, _ in pyarchon.RunStats._fields_] == FIELDS


def test_struct_layouts(tmp_path):
    """archon_hip_run is 16 bytes with its words at 0, 4, 8, 12, in the order of the numpy dtype; the ctypes mirror of
    archon_hip_run_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    fields = ["start", "end", "period", "root"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%zu", sizeof(archon_hip_run_stats));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_run_stats, %s));' % k for k in FIELDS)
                   + 'printf(" %zu", sizeof(archon_hip_run));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_run, %s));' % k for k in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = len(FIELDS)
    assert got[0] == ctypes.sizeof(pyarchon.RunStats)
    assert got[1:1 + k] == [getattr(pyarchon.RunStats, f).offset for f in FIELDS]
    assert got[1 + k] == 16 == pyarchon.RUN.itemsize == N.RUN.itemsize
    assert got[2 + k:] == [pyarchon.RUN.fields[f][1] for f in fields] == [0, 4, 8, 12]
    assert pyarchon.RUN == N.RUN


def _banana():
    sa, lcp = R.a7_arrays(b"banana")[:2]
    sa_c = R.a7_arrays(bytes(255 - c for c in b"banana"))[0]
    return np.array(sa, np.uint32), np.array(lcp, np.uint32), np.array(sa_c, np.uint32)


def test_bad_arguments():
    """null pointers, n = 0, min_copies < 2 and min_period > max_period != 0 are ARCHON_E_ARG, with or without a device, and
    *total is written 0; the output stays untouched.  An LCE call refuses null pointers, n = 0 and, in the host form, an item
    above n before any device is asked for"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp, sa_c = _banana()
    out = np.zeros(8, pyarchon.RUN)
    total = ctypes.c_uint64(7)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    E = pyarchon.E_ARG
    for fn, tail in ((L.archon_hip_runs, (0,)), (L.archon_hip_runs_dev, (0, None))):
        assert fn(p(sa), p(lcp), p(sa_c), 6, 0, 0, 2, 0, p(out), 8, None, *tail) == E
        for a, b, c, n, lo, hi, copies in ((None, p(lcp), p(sa_c), 6, 0, 0, 2), (p(sa), None, p(sa_c), 6, 0, 0, 2), (p(sa), p(lcp), None, 6, 0, 0, 2),
                                           (p(sa), p(lcp), p(sa_c), 0, 0, 0, 2), (p(sa), p(lcp), p(sa_c), 6, 0, 0, 1), (p(sa), p(lcp), p(sa_c), 6, 0, 0, 0),
                                           (p(sa), p(lcp), p(sa_c), 6, 3, 2, 2), (p(sa), p(lcp), p(sa_c), 6, 9, 1, 2)):
            total.value = 7
            assert fn(a, b, c, n, lo, hi, copies, 0, p(out), 8, tp, *tail) == E, (n, lo, hi, copies)
            assert total.value == 0
    total.value = 7
    assert L.archon_hip_block_runs(None, 0, 0, 2, 0, p(out), 8, tp) == E and total.value == 0
    assert L.archon_hip_block_runs(None, 0, 0, 2, 0, p(out), 8, None) == E
    assert not out.view(np.uint32).any()

    s, t, res = np.array([1, 7], np.uint32), np.array([2, 3], np.uint32), np.full(2, 99, np.uint32)
    for fn, tail in ((L.archon_hip_lce, (0,)), (L.archon_hip_lce_dev, (0, None))):
        assert fn(None, p(lcp), 6, p(s), p(t), 1, p(res), *tail) == E
        assert fn(p(sa), None, 6, p(s), p(t), 1, p(res), *tail) == E
        assert fn(p(sa), p(lcp), 6, None, p(t), 1, p(res), *tail) == E
        assert fn(p(sa), p(lcp), 6, p(s), None, 1, p(res), *tail) == E
        assert fn(p(sa), p(lcp), 6, p(s), p(t), 1, None, *tail) == E
        assert fn(p(sa), p(lcp), 0, p(s), p(t), 1, p(res), *tail) == E
        assert fn(p(sa), p(lcp), 6, None, None, 0, None, *tail) == 0          # k = 0 writes nothing
    assert L.archon_hip_lce(p(sa), p(lcp), 6, p(s), p(t), 2, p(res), 0) == E
    assert b"(7, 3), an item above 6" in L.archon_hip_last_error()
    assert L.archon_hip_block_lce(None, p(s), p(t), 1, p(res)) == E
    assert res.tolist() == [99, 99]


def test_getter_refusals():
    """a null out is "null pointer"; a thread that has run no such call is told so, with the device's number"""
    import pyarchon
    L = pyarchon.lib()
    got = {}

    def ask():
        st = pyarchon.RunStats()
        got["null"] = (L.archon_hip_runs_last_stats(0, None), L.archon_hip_last_error())
        got["none"] = (L.archon_hip_runs_last_stats(3, ctypes.byref(st)), L.archon_hip_last_error())

    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got["null"] == (pyarchon.E_ARG, b"null pointer")
    assert got["none"] == (pyarchon.E_ARG, b"the calling thread has run no runs or LCE call on device 3")


BANANA = [(1, 6, 2, 6)]


def test_without_a_device():
    """no CPU fallback: without a GPU a good call is ARCHON_E_NODEVICE (with one, the host forms answer the header's example)"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp, sa_c = _banana()
    out = np.zeros(8, pyarchon.RUN)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    s, t, res = np.array([6, 3], np.uint32), np.array([4, 3], np.uint32), np.full(2, 99, np.uint32)
    if pyarchon.device_count() > 0:
        assert L.archon_hip_runs(p(sa), p(lcp), p(sa_c), 6, 0, 0, 2, 0, p(out), 8, tp, 0) == 0
        assert total.value == 1 and out[:1].tolist() == BANANA
        assert L.archon_hip_lce(p(sa), p(lcp), 6, p(s), p(t), 2, p(res), 0) == 0 and res.tolist() == [3, 3]
        return
    NO = pyarchon.E_NODEVICE
    assert L.archon_hip_runs(p(sa), p(lcp), p(sa_c), 6, 0, 0, 2, 0, p(out), 8, tp, 0) == NO
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_runs_dev(p(sa), p(lcp), p(sa_c), 6, 0, 0, 2, 0, p(out), 8, tp, 0, None) == NO
    assert L.archon_hip_lce(p(sa), p(lcp), 6, p(s), p(t), 2, p(res), 0) == NO
    assert L.archon_hip_lce_dev(p(sa), p(lcp), 6, p(s), p(t), 2, p(res), 0, None) == NO
    for call in (lambda: pyarchon.runs(sa, lcp, sa_c), lambda: pyarchon.runs(sa, lcp, sa_c, count_only=True), lambda: pyarchon.lce(sa, lcp, s, t),
                 lambda: pyarchon.runs_of(b"banana"), pyarchon.run_stats):
        with pytest.raises(pyarchon.ArchonError):
            call()
    assert not out.view(np.uint32).any() and res.tolist() == [99, 99]


def test_worked_examples():
    """the header's four examples through the rule: the records, then candidates / roots / lce_queries"""
    for x, recs, counters in ((b"banana", BANANA, (7, 1, 8)),
                              (b"mississippi", [(2, 4, 1, 4), (5, 7, 1, 7), (1, 8, 3, 8), (8, 10, 1, 10)], (16, 6, 24)),
                              (b"aaaa", [(0, 4, 1, 4)], (6, 2, 10)),
                              (b"abracadabra", [], (18, 5, 26))):
        got, c = N.runs_rule(x)
        assert got == recs, x
        assert (c["candidates"], c["roots"], c["lce_queries"]) == counters, x
        assert c["runs"] == c["emitted"] == len(recs)
        assert {r[:3] for r in recs} == N.runs_text(x) == N.runs_short(x, len(x))
        assert all(N.is_run(x, *r[:3]) for r in recs)
    # a block of one byte drops every candidate but the last at step 3
    got, c = N.runs_rule(b"c" * 40)
    assert got == [(0, 40, 1, 40)] and (c["candidates"], c["roots"]) == (78, 2)
    # the plain lce is the header's: the longest common suffix of two prefixes
    lce = N.plain_lce(b"banana")
    assert [lce(6, 4), lce(4, 2), lce(6, 2), lce(5, 3), lce(3, 3), lce(0, 5), lce(1, 4)] == [3, 1, 1, 2, 3, 0, 0]


def test_filters_of_the_rule():
    """the period filter acts on candidates, the copies and length filters on the runs found"""
    x = b"aabaabaabbbbabababaab"
    full, c = N.runs_rule(x)
    assert {r[:3] for r in full} == N.runs_text(x)
    for lo, hi, copies, ln in ((0, 0, 2, 0), (2, 0, 2, 0), (0, 1, 2, 0), (2, 3, 2, 0), (0, 0, 3, 0), (0, 0, 2, 5), (1, 2, 3, 7)):
        got, cf = N.runs_rule(x, lo, hi, copies, ln)
        keep = [r for r in full if r[2] >= lo and (not hi or r[2] <= hi) and r[1] - r[0] >= copies * r[2] and r[1] - r[0] >= ln]
        assert got == keep, (lo, hi, copies, ln)
        assert cf["emitted"] == len(keep) and cf["candidates"] <= c["candidates"]
        assert cf["runs"] == sum(1 for r in full if r[2] >= lo and (not hi or r[2] <= hi))


def test_rule_and_short_finder_are_the_definition():
    """on every string of length 1-10 over {0, 1} and 1-7 over {0, 1, 255}: the rule gives the set of the definition with no
    run twice and in ascending root, and so does the short-period finder; every record is a run by slices"""
    count = 0
    for x in N.tiny_strings():
        want = N.runs_text(x)
        recs, c = N.runs_rule(x)
        got = [r[:3] for r in recs]
        assert len(set(got)) == len(got) and set(got) == want, x
        roots = [r[3] for r in recs]
        assert roots == sorted(roots), x
        assert all(r[0] + r[2] <= r[3] <= r[1] for r in recs), x
        assert N.runs_short(x, len(x)) == want, x
        assert all(N.is_run(x, *r) for r in want), x
        assert len(want) < len(x) and c["roots"] <= c["candidates"] <= 2 * (len(x) - 1)
        count += 1
    assert count == 2046 + 3279


def test_fast_arrays_are_the_definition():
    """the numpy arrays and the sparse-table lce the GPU tests use on long blocks, against the plain ones"""
    rng = np.random.default_rng(20261021)
    for i in range(60):
        n = 1 + i % 30
        x = bytes(rng.choice(np.array([97, 98, 255], np.uint8), n))
        sa, lcp = N.a7_fast(x)
        sa2, lcp2 = R.a7_arrays(x)[:2]
        assert sa.tolist() == sa2 and lcp.tolist()[1:] == lcp2[1:], x
        sp, pl = N.SparseLce(sa, lcp), N.plain_lce(x)
        s, t = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
        assert sp.many(s.ravel(), t.ravel()).tolist() == [pl(int(a), int(b)) for a, b in zip(s.ravel(), t.ravel())], x
        assert N.ranks_fast(x) == N.ranks(x)
        assert N.runs_rule(x, lce=sp, rank=N.ranks_fast(x)) == N.runs_rule(x)
    # the Fibonacci strings: 2 F(k-2) - 3 runs in the string of length F(k)
    for k, runs in ((5, 1), (8, 13), (15, 463)):
        x = N.fibonacci(k)
        sa, lcp = N.a7_fast(x)
        assert len(N.runs_rule(x, lce=N.SparseLce(sa, lcp), rank=N.ranks_fast(x))[0]) == runs
    assert len(N.fibonacci(15)) == 610
