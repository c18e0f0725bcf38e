"""CPU: the LZ entry points (include/archon_hip.h, archon_hip_lpf*, archon_hip_lz_parse*, archon_hip_block_lz) are declared,
exported and bound; the records and the statistics mirror have the C layout; they refuse bad arguments and, without a GPU, fail
loudly.  And the expected answer of the GPU tests, tests/lz_naive.c, is pinned to the definitions in terms of the text."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import lz_naive as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["archon_hip_lpf", "archon_hip_lpf_dev", "archon_hip_lz_parse", "archon_hip_lz_parse_dev", "archon_hip_block_lz", "archon_hip_get_lz_stats"]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(archon_[a-z0-9_]+)\s*\(", src))


@pytest.fixture(scope="module")
def naive(tmp_path_factory):
    return Z.build(tmp_path_factory.mktemp("lz_naive"))


def test_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
    test_h = open(os.path.join(ROOT, "include", "archon_hip_test.h")).read()
    for route in ("LZ_FAN", "LZ_TILE"):
        assert route in pyarchon._ROUTE_NAMES and route in test_h
    for name in ("LPF", "PHRASE", "LzStats", "lz_stats", "lpf", "lpf_dev", "lz_parse", "lz_parse_dev", "lz77"):
        assert hasattr(pyarchon, name), name
    assert hasattr(pyarchon.Block, "lz")


def test_struct_layouts(tmp_path):
    """struct archon_hip_lpf is 8 bytes and archon_hip_phrase 12 in the order of the numpy dtypes; the ctypes mirror of
    archon_hip_lz_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    names = [k for k, _ in pyarchon.LzStats._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%zu", sizeof(archon_hip_lz_stats));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_lz_stats, %s));' % k for k in names)
                   + 'printf(" %zu %zu", sizeof(struct archon_hip_lpf), sizeof(archon_hip_lpf_rec));'
                   + "".join('printf(" %%zu", offsetof(struct archon_hip_lpf, %s));' % k for k in ("len", "src"))
                   + 'printf(" %zu", sizeof(archon_hip_phrase));'
                   + "".join('printf(" %%zu", offsetof(archon_hip_phrase, %s));' % k for k in ("end", "len", "src")) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = len(names)
    assert got[0] == ctypes.sizeof(pyarchon.LzStats)
    assert got[1:1 + k] == [getattr(pyarchon.LzStats, f).offset for f in names]
    assert got[1 + k:] == [8, 8, 0, 4, 12, 0, 4, 8]
    assert pyarchon.LPF.itemsize == 8 and [pyarchon.LPF.fields[f][1] for f in ("len", "src")] == [0, 4]
    assert pyarchon.PHRASE.itemsize == 12 and [pyarchon.PHRASE.fields[f][1] for f in ("end", "len", "src")] == [0, 4, 8]
    assert pyarchon.LPF == Z.LPF and pyarchon.PHRASE == Z.PHRASE


def _banana():
    return np.array([2, 4, 6, 1, 3, 5], np.uint32), np.array([0, 1, 3, 0, 0, 2], np.uint32)


def test_bad_arguments():
    """null pointers, n = 0 and dir 2 are ARCHON_E_ARG, with or without a device; so are a fan-out that is no power of two in
    [2, 64] and a tile that is none in [2, 4096]"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp = _banana()
    rec = np.zeros(6, pyarchon.LPF)
    out = np.zeros(8, pyarchon.PHRASE)
    total = ctypes.c_uint64(7)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    for fn, tail in ((L.archon_hip_lpf, (0,)), (L.archon_hip_lpf_dev, (0, None))):
        assert fn(None, p(lcp), 6, 0, p(rec), *tail) == pyarchon.E_ARG
        assert fn(p(sa), None, 6, 0, p(rec), *tail) == pyarchon.E_ARG
        assert fn(p(sa), p(lcp), 6, 0, None, *tail) == pyarchon.E_ARG
        assert fn(p(sa), p(lcp), 0, 0, p(rec), *tail) == pyarchon.E_ARG
        assert fn(p(sa), p(lcp), 6, 2, p(rec), *tail) == pyarchon.E_ARG
    for fn, tail in ((L.archon_hip_lz_parse, (0,)), (L.archon_hip_lz_parse_dev, (0, None))):
        assert fn(None, 6, p(out), 8, tp, *tail) == pyarchon.E_ARG
        assert fn(p(rec), 6, p(out), 8, None, *tail) == pyarchon.E_ARG
        assert fn(p(rec), 0, p(out), 8, tp, *tail) == pyarchon.E_ARG
    assert L.archon_hip_block_lz(None, 0, p(rec), p(out), 8, tp) == pyarchon.E_ARG
    assert L.archon_hip_get_lz_stats(0, None) == pyarchon.E_ARG
    assert not out.view(np.uint32).any() and not rec.view(np.uint32).any()
    for bad in (3, 128, 1, -2, 48):
        assert L.archon_hip_test_route(b"LZ_FAN", bad) == pyarchon.E_ARG, bad
    for good in (2, 4, 8, 16, 32, 64, 0):
        assert L.archon_hip_test_route(b"LZ_FAN", good) == 0, good
    for bad in (3, 8192, 1, -2, 48):
        assert L.archon_hip_test_route(b"LZ_TILE", bad) == pyarchon.E_ARG, bad
    for good in (2, 16, 256, 4096, 0):
        assert L.archon_hip_test_route(b"LZ_TILE", good) == 0, good
    assert L.archon_hip_test_route(b"RESET", 0) == 0


def test_without_a_device():
    """no CPU fallback: without a GPU every LZ entry point is ARCHON_E_NODEVICE (with one, the host forms answer)"""
    import pyarchon
    L = pyarchon.lib()
    sa, lcp = _banana()
    rec = np.zeros(6, pyarchon.LPF)
    out = np.zeros(8, pyarchon.PHRASE)
    total = ctypes.c_uint64(0)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    if pyarchon.device_count() > 0:
        assert L.archon_hip_lpf(p(sa), p(lcp), 6, 0, p(rec), 0) == 0
        assert rec.tolist() == BANANA[0][0]
        assert L.archon_hip_lz_parse(p(rec), 6, p(out), 8, tp, 0) == 0
        assert total.value == 4 and out[:4].tolist() == BANANA[0][1]
        return
    assert L.archon_hip_lpf(p(sa), p(lcp), 6, 0, p(rec), 0) == pyarchon.E_NODEVICE
    assert b"no CPU fallback" in L.archon_hip_last_error()
    assert L.archon_hip_lpf_dev(p(sa), p(lcp), 6, 1, p(rec), 0, None) == pyarchon.E_NODEVICE
    assert L.archon_hip_lz_parse(p(rec), 6, p(out), 8, tp, 0) == pyarchon.E_NODEVICE
    assert L.archon_hip_lz_parse_dev(p(rec), 6, None, 0, tp, 0, None) == pyarchon.E_NODEVICE
    h = ctypes.c_void_p(None)
    assert L.archon_hip_block_create(0, ctypes.byref(h)) == pyarchon.E_NODEVICE     # so no handle reaches block_lz
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.lpf(sa, lcp)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.lz_parse(rec, count_only=True)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.lz77(b"banana")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.lz_stats()


# the header's examples: {dir: (records of items 1..n, phrases)}
BANANA = {
    0: ([(0, 0), (0, 0), (0, 0), (1, 2), (2, 3), (3, 4)], [(6, 3, 4), (3, 0, 0), (2, 0, 0), (1, 0, 0)]),
    1: ([(0, 0), (1, 4), (2, 5), (3, 6), (0, 0), (0, 0)], [(6, 0, 0), (5, 0, 0), (4, 3, 6), (1, 0, 0)]),
}
ABRACADABRA = [(11, 4, 4), (7, 0, 0), (6, 1, 4), (5, 0, 0), (4, 1, 1), (3, 0, 0), (2, 0, 0), (1, 0, 0)]


def test_worked_examples(naive):
    """the examples of the header through the helper, and their text in include/archon_hip.h"""
    sa, lcp = Z.a7_arrays(b"banana")
    assert (sa, lcp) == ([2, 4, 6, 1, 3, 5], [0, 1, 3, 0, 0, 2])
    header = " ".join(open(os.path.join(ROOT, "include", "archon_hip.h")).read().replace("*", " ").split())
    for d in (0, 1):
        rec = naive.lpf(sa, lcp, d)
        assert rec.tolist() == BANANA[d][0]
        assert naive.parse(rec).tolist() == BANANA[d][1]
        for quoted in BANANA[d]:
            assert " ".join("(%s)" % ",".join(str(v) for v in t) for t in quoted) in header
    sa, lcp = Z.a7_arrays(b"abracadabra")
    assert naive.parse(naive.lpf(sa, lcp, 0)).tolist() == ABRACADABRA
    assert " ".join("(%d,%d,%d)" % t for t in ABRACADABRA) in header


def test_naive_helper_is_the_definition(naive):
    """tests/lz_naive.c against the text on every string of length 1-7 over {0, 1, 255}, both directions: len is the longest
    common suffix with an admissible item, src is admissible and its bytes match, the phrase lengths sum to n, and the dir-1
    chain on reverse(z) is the textbook greedy LZ77 of z in positions and lengths"""
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = bytes(t)
            sa, lcp = Z.a7_arrays(x)
            for d in (0, 1):
                rec = naive.lpf(sa, lcp, d)
                assert rec["len"].tolist() == Z.lpf_by_text(x, d), (x, d)
                for s, (m, src) in enumerate(rec.tolist(), 1):
                    if m == 0:
                        assert src == 0
                        continue
                    assert (src < s if d == 0 else src > s) and 1 <= src <= n, (x, d, s)
                    assert m <= min(s, src) and x[s - m:s] == x[src - m:src], (x, d, s)
                ph = naive.parse(rec)
                assert ph["end"][0] == n and int(np.maximum(ph["len"], 1).sum()) == n
                assert (ph["end"][1:] == ph["end"][:-1] - np.maximum(ph["len"][:-1], 1)).all()
                assert all((e, m, src) == (e,) + tuple(rec[e - 1].tolist()) for e, m, src in ph.tolist())
                if d == 1:
                    z = x[::-1]
                    assert [(n - e, m) for e, m, _ in ph.tolist()] == Z.lz77_by_text(z), z
                    for e, m, src in ph.tolist():
                        pos, at = n - e, n - src
                        assert m == 0 or (at < pos and all(z[at + k] == z[pos + k] for k in range(m)))


def test_naive_parse_of_any_words(naive):
    """the parse is a rule about the len words of any array: values above e step by e, never more than n phrases"""
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 100):
        rec = np.zeros(n, Z.LPF)
        rec["len"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        rec["src"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        ph = naive.parse(rec)
        assert 1 <= ph.size <= n and ph["end"][0] == n
        e = n
        for end, m, src in ph.tolist():
            assert end == e and (m, src) == tuple(rec[e - 1].tolist())
            e -= min(max(1, m), e)
        assert e == 0
