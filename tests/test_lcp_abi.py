"""CPU: the LCP entry points (include/archon_hip.h, archon_hip_lcp*) are declared, exported and bound; their statistics
mirror has the C layout; they refuse bad arguments and, without a GPU, fail loudly.  And the expected answer of the GPU
tests, tests/lcp_kasai.c, is pinned to the definition."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import lcp_kasai

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LCP_FUNCTIONS = ["archon_hip_lcp", "archon_hip_lcp_dev", "archon_hip_block_lcp", "archon_hip_lcp_keep", "archon_hip_get_lcp_stats"]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(archon_[a-z0-9_]+)\s*\(", src))


def test_lcp_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in LCP_FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
    assert "LCP_CAP" in pyarchon._ROUTE_NAMES and "LCP_WINDOW" in pyarchon._ROUTE_NAMES


def test_lcp_stats_struct_layout(tmp_path):
    """the ctypes mirror of archon_hip_lcp_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.LcpStats._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%zu", sizeof(archon_hip_lcp_stats));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_lcp_stats, %s));' % k for k in names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(pyarchon.LcpStats)
    assert got[1:] == [getattr(pyarchon.LcpStats, k).offset for k in names]


def test_lcp_bad_arguments():
    """null pointers and n = 0 are ARCHON_E_ARG, with or without a device; so is a test route out of range"""
    import pyarchon
    L = pyarchon.lib()
    x = np.frombuffer(b"banana", np.uint8).copy()
    sa = np.array([2, 4, 6, 1, 3, 5], np.uint32)
    out = np.zeros(6, np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    assert L.archon_hip_lcp(None, 6, p(sa), p(out), 0) == pyarchon.E_ARG
    assert L.archon_hip_lcp(p(x), 6, None, p(out), 0) == pyarchon.E_ARG
    assert L.archon_hip_lcp(p(x), 6, p(sa), None, 0) == pyarchon.E_ARG
    assert L.archon_hip_lcp(p(x), 0, p(sa), p(out), 0) == pyarchon.E_ARG
    assert L.archon_hip_lcp_dev(None, 6, p(sa), p(out), 0, None) == pyarchon.E_ARG
    assert L.archon_hip_lcp_dev(p(x), 6, None, p(out), 0, None) == pyarchon.E_ARG
    assert L.archon_hip_lcp_dev(p(x), 6, p(sa), None, 0, None) == pyarchon.E_ARG
    assert L.archon_hip_lcp_dev(p(x), 0, p(sa), p(out), 0, None) == pyarchon.E_ARG
    assert L.archon_hip_block_lcp(None, p(out)) == pyarchon.E_ARG
    assert L.archon_hip_lcp_keep(0, None) == pyarchon.E_ARG
    assert L.archon_hip_get_lcp_stats(0, None) == pyarchon.E_ARG
    assert L.archon_hip_test_route(b"LCP_CAP", 4097) == pyarchon.E_ARG
    assert L.archon_hip_test_route(b"LCP_WINDOW", (1 << 30) + 1) == pyarchon.E_ARG
    assert L.archon_hip_test_route(b"LCP_CAP", 1) == 0 and L.archon_hip_test_route(b"LCP_WINDOW", 64) == 0
    assert L.archon_hip_test_route(b"RESET", 0) == 0


def test_lcp_without_a_device():
    """no CPU fallback: without a GPU every LCP entry point is ARCHON_E_NODEVICE (with one, the host form answers)"""
    import pyarchon
    L = pyarchon.lib()
    x = np.frombuffer(b"banana", np.uint8).copy()
    sa = np.array([2, 4, 6, 1, 3, 5], np.uint32)          # a7 order of "banana" (test_abi.py: BWT nnbaaa, primary row 2)
    out = np.zeros(6, np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    if pyarchon.device_count() > 0:
        assert L.archon_hip_lcp(p(x), 6, p(sa), p(out), 0) == 0
        assert out.tolist() == _brute_lcp(x.tobytes(), sa.tolist()) == [0, 1, 3, 0, 0, 2]
        return
    assert L.archon_hip_lcp(p(x), 6, p(sa), p(out), 0) == pyarchon.E_NODEVICE
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_lcp_dev(p(x), 6, p(sa), p(out), 0, None) == pyarchon.E_NODEVICE
    assert L.archon_hip_lcp_keep(0, p(out)) == pyarchon.E_NODEVICE
    h = ctypes.c_void_p(None)
    assert L.archon_hip_block_create(0, ctypes.byref(h)) == pyarchon.E_NODEVICE    # so no handle reaches block_lcp
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.lcp(x, sa)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.lcp_stats()


def _key(x, s):
    """the key of item s in a7 order, INF as 256"""
    return [x[s - 1 - j] for j in range(s)] + [256]


def _brute_lcp(x, sa):
    out = [0]
    for i in range(1, len(sa)):
        a, b = _key(x, sa[i - 1]), _key(x, sa[i])
        L = 0
        while a[L] == b[L] and a[L] != 256:
            L += 1
        out.append(L)
    return out


def test_kasai_helper_is_the_definition(oracle, tmp_path):
    """tests/lcp_kasai.c against the definition on every string of length 1-6 over {0, 1, 255}: keys compared directly.
    The same strings check the orientation the header states: for z[k] = 255 - x[n-1-k], sa[i] = n - SA_z[n-1-i] and
    lcp[i] = LCP_z[n-i] (textbook suffix and LCP arrays of z)."""
    kasai = lcp_kasai.build(tmp_path)
    for n in range(1, 7):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            xa = np.frombuffer(x, np.uint8)
            sa = oracle.sa(xa)
            keys = sorted(range(1, n + 1), key=lambda s: _key(x, s))
            assert sa.tolist() == keys, x
            want = _brute_lcp(x, keys)
            assert kasai(xa, sa).tolist() == want, x
            z = bytes(255 - x[n - 1 - k] for k in range(n))
            sa_z = sorted(range(n), key=lambda k: z[k:])
            lcp_z = [0] + [len(os.path.commonprefix([z[sa_z[k - 1]:], z[sa_z[k]:]])) for k in range(1, n)]
            assert [n - sa_z[n - 1 - i] for i in range(n)] == keys
            assert [0] + [lcp_z[n - i] for i in range(1, n)] == want


def test_irreducible_rule_counts_row_zero_and_runs():
    """the numpy count the GPU work-bound test compares with: 'banana' in a7 order has BWT nnbaaa, primary row 2"""
    x = np.frombuffer(b"banana", np.uint8)
    sa = np.array([2, 4, 6, 1, 3, 5], np.uint32)
    assert lcp_kasai.irreducible_rows(x, sa).tolist() == [True, False, True, True, False, False]
