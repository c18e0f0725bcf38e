"""CPU: the window entry points (include/archon_hip.h, archon_hip_fm_attach_wm, _block_fm_attach_wm, _fm_win_count*, _select*,
_list*) are declared, exported and bound; the record and the statistics mirror have the C layout; the getter refuses as its
siblings do; without a GPU every compute entry point fails loudly.  And the expected answers of the GPU tests,
tests/fm_win_naive.py: the header's examples read back out of its text, and the model pinned to brute force on every
permutation of 1 .. n for n <= 5 with every (lo, hi, a, b)."""
import ctypes
import itertools
import os
import re
import threading

import numpy as np
import pytest

import fm_abi_util as U
import fm_win_naive as W

FUNCTIONS = ["archon_hip_fm_attach_wm", "archon_hip_block_fm_attach_wm", "archon_hip_fm_win_count", "archon_hip_fm_win_count_dev",
             "archon_hip_fm_win_select", "archon_hip_fm_win_select_dev", "archon_hip_fm_win_list", "archon_hip_fm_win_list_dev",
             "archon_hip_fm_win_last_stats"]
FIELDS = ["n", "levels", "ranges", "most", "attached", "reserved0", "rows", "in_window", "listed", "walks", "wm_bytes", "kernel_launches",
          "host_syncs", "ms_attach", "ms_count", "ms_emit"]
BANANA_SA = [2, 4, 6, 1, 3, 5]


def test_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = U.declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
    for name in ("FM_WIN", "FmWinStats", "fm_win_stats"):
        assert hasattr(pyarchon, name), name
    for name in ("attach_wm", "win_count", "win_count_dev", "win_select", "win_select_dev", "win_list", "win_list_dev", "first", "locate_sorted"):
        assert hasattr(pyarchon.FmIndex, name), name
    assert [k for k, _ in pyarchon.FmWinStats._fields_] == FIELDS
    # no new statistics getter of the archon_hip_get_*_stats family, no new test route
    assert not [f for f in declared if re.fullmatch(r"archon_hip_get_\w*win\w*_stats", f)]


def test_struct_layouts(tmp_path):
    """archon_hip_fm_win is 8 bytes with item at 0 and range at 4, as the numpy dtypes; the ctypes mirror of
    archon_hip_fm_win_stats has the size and the field offsets the C header gives it"""
    import pyarchon
    got = U.layout(tmp_path, "archon_hip_fm_win_stats", FIELDS)
    assert got[0] == ctypes.sizeof(pyarchon.FmWinStats)
    assert got[1:] == [getattr(pyarchon.FmWinStats, f).offset for f in FIELDS]
    assert U.layout(tmp_path, "archon_hip_fm_win", ["item", "range"]) == [8, 0, 4]
    assert pyarchon.FM_WIN.itemsize == 8 and [pyarchon.FM_WIN.fields[f][1] for f in ("item", "range")] == [0, 4]
    assert pyarchon.FM_WIN == W.FM_WIN


_EXAMPLE = re.compile(r"rows \[(\d+), (\d+)\)[^,]*, (?:no window|window \[(\d+), (\d+)\))(?:, most (\d+))?: count (\d+)(.*)")


def header_examples():
    """the example lines of the windows section of include/archon_hip.h:
    (lo, hi, a, b, most, count, listed items or None, [(idx, item)])"""
    text = open(os.path.join(U.ROOT, "include", "archon_hip.h")).read()
    section = text[text.index("windows: count, select and list"):text.index("} archon_hip_fm_win;")]
    assert '"banana", sa = ' + " ".join(map(str, BANANA_SA)) in section
    out = []
    for line in section.splitlines():
        m = _EXAMPLE.search(line)
        if not m:
            continue
        lo, hi = int(m.group(1)), int(m.group(2))
        a, b = (None, None) if m.group(3) is None else (int(m.group(3)), int(m.group(4)))
        rest = m.group(7)
        lm = re.search(r"list ((?:\d+ ?)+|nothing)", rest)
        listed = None if not lm else ([] if lm.group(1) == "nothing" else [int(t) for t in lm.group(1).split()])
        selects = [(int(i), int(v)) for i, v in re.findall(r"select (\d+) -> (\d+)", rest)]
        out.append((lo, hi, a, b, int(m.group(5) or 0), int(m.group(6)), listed, selects))
    return out


def test_header_examples():
    """the five examples of the header, parsed from its text, through the naive model"""
    ex = header_examples()
    assert len(ex) == 5
    assert sum(e[6] is not None for e in ex) == 4 and sum(len(e[7]) for e in ex) == 4
    for lo, hi, a, b, most, count, listed, selects in ex:
        A, B = (None, None) if a is None else ([a], [b])
        cnt, recs, _ = W.listing(BANANA_SA, [lo], [hi], A, B, most)
        assert cnt.tolist() == [count]
        if listed is not None:
            assert recs["item"].tolist() == listed and not recs["range"].any()
        for idx, item in selects:
            assert W.select(BANANA_SA, [lo], [hi], [idx], A, B)[0].tolist() == [item]
    # the counters of the second example: n = 6 has L = 3, so both bounds of [3, 7) walk; two selects of three return an item
    _, c = W.select(BANANA_SA, [0, 0, 0], [3, 3, 3], [0, 1, 2], [3, 3, 3], [7, 7, 7])
    assert c == {"rows": 9, "in_window": 6, "walks": 6 + 2, "listed": 0}


def test_memory_formula():
    """wm_bytes from n alone: L = bits(n) levels of 36 B + 4 bytes rounded up to 256; 4.1 n at 2^28, 3.5 n at 16 MiB"""
    assert [W.levels(n) for n in (1, 2, 3, 4, 255, 256, 65535, 65536)] == [1, 2, 2, 3, 8, 9, 16, 17]
    assert W.wm_bytes(1) == 256 and W.wm_bytes(256) == 9 * 256 and W.wm_bytes(257) == 9 * 256 and W.wm_bytes(70001) == 17 * 9984      # B = 274: 9868 bytes a level
    assert 4.0 < W.wm_bytes(1 << 28) / (1 << 28) < 4.1 and 3.5 < W.wm_bytes(1 << 24) / (1 << 24) < 3.6


def test_getter_refusals():
    """a null out is "null pointer"; a thread that has run no window call is told so, with the device's number"""
    import pyarchon
    L = pyarchon.lib()
    got = {}

    def ask():
        st = pyarchon.FmWinStats()
        got["null"] = (L.archon_hip_fm_win_last_stats(0, None), L.archon_hip_last_error())
        got["none"] = (L.archon_hip_fm_win_last_stats(3, ctypes.byref(st)), L.archon_hip_last_error())
        got["far"] = (L.archon_hip_fm_win_last_stats(64, ctypes.byref(st)), L.archon_hip_last_error())

    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got["null"] == (pyarchon.E_ARG, b"null pointer")
    assert got["none"] == (pyarchon.E_ARG, b"the calling thread has run no window call on device 3")
    assert got["far"] == (pyarchon.E_ARG, b"the calling thread has run no window call on device 64")


def test_bad_arguments_and_no_device():
    """a null handle is ARCHON_E_ARG everywhere and a list writes *total = 0 first; no CPU fallback: without a GPU no handle can be
    made (archon_hip_fm_create is ARCHON_E_NODEVICE), so no window call gets past its handle, and the Python calls raise"""
    import pyarchon
    L = pyarchon.lib()
    p = U.p
    lo, hi = np.array([0], np.uint32), np.array([3], np.uint32)
    out = np.zeros(2, np.uint32)
    recs = np.zeros(4, pyarchon.FM_WIN)
    total = ctypes.c_uint64(7)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    E = pyarchon.E_ARG
    assert L.archon_hip_fm_attach_wm(None) == E
    assert L.archon_hip_block_fm_attach_wm(None, None) == E
    assert L.archon_hip_fm_win_count(None, p(lo), p(hi), None, None, 1, p(out)) == E
    assert L.archon_hip_fm_win_count_dev(None, p(lo), p(hi), None, None, 1, p(out), None) == E
    assert L.archon_hip_fm_win_select(None, p(lo), p(hi), None, None, p(lo), 1, p(out)) == E
    assert L.archon_hip_fm_win_select_dev(None, p(lo), p(hi), None, None, p(lo), 1, p(out), None) == E
    assert L.archon_hip_fm_win_list(None, p(lo), p(hi), None, None, 1, 0, p(out), p(recs), 4, tp) == E and total.value == 0
    total.value = 7
    assert L.archon_hip_fm_win_list_dev(None, p(lo), p(hi), None, None, 1, 0, p(out), p(recs), 4, tp, None) == E and total.value == 0
    assert L.archon_hip_fm_win_list(None, p(lo), p(hi), None, None, 1, 0, p(out), p(recs), 4, None) == E
    assert not out.any() and not recs.view(np.uint32).any()
    if pyarchon.device_count() > 0:
        return
    bwt = np.frombuffer(b"nnbaaa", np.uint8).copy()
    h = ctypes.c_void_p(None)
    assert L.archon_hip_fm_create(p(bwt), 6, 2, 0, ctypes.byref(h)) == pyarchon.E_NODEVICE and not h.value
    assert b"no CPU fallback" in L.archon_hip_last_error()
    b = ctypes.c_void_p(None)
    assert L.archon_hip_block_create(0, ctypes.byref(b)) == pyarchon.E_NODEVICE and not b.value
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(bwt, 2)
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.fm_win_stats()


def test_naive_model_is_brute_force():
    """count, select and list of the model against plain Python on every permutation of 1 .. n, n <= 5, with every (lo, hi, a, b):
    the window is the sorted list of the values in range, select indexes it, the list takes its first `most`; and the walks
    rule bound by bound"""
    for n in range(1, 6):
        top = 1 << max(n.bit_length(), 1)
        for perm in itertools.permutations(range(1, n + 1)):
            sa = list(perm)
            qs = [(lo, hi, a, b) for lo in range(n + 1) for hi in range(lo, n + 1) for a in range(n + 2) for b in range(a, n + 2)]
            lo, hi, a, b = (np.array(v, np.uint32) for v in zip(*qs))
            cnt, c = W.count(sa, lo, hi, a, b)
            wins = [sorted(v for v in sa[q[0]:q[1]] if q[2] <= v < q[3]) for q in qs]
            assert cnt.tolist() == [len(w) for w in wins]
            assert c["rows"] == sum(q[1] - q[0] for q in qs) and c["in_window"] == sum(len(w) for w in wins)
            assert c["walks"] == sum((0 < q[2] < top) + (0 < q[3] < top) for q in qs if q[0] < q[1])
            for idx in (0, 1, n - 1, n, 0xFFFFFFFF):
                item, cs = W.select(sa, lo, hi, np.full(len(qs), idx, np.uint32), a, b)
                want = [w[idx] if idx < len(w) else 0 for w in wins]
                assert item.tolist() == want
                assert cs["walks"] == c["walks"] + sum(v > 0 for v in want)
            for most in (0, 1, 2):
                cl, recs, cc = W.listing(sa, lo, hi, a, b, most)
                want = [(v, j) for j, w in enumerate(wins) for v in (w[:most] if most else w)]
                assert cl.tolist() == cnt.tolist() and recs.tolist() == want
                assert cc["listed"] == len(want) and cc["walks"] == c["walks"] + len(want)
            if n <= 3:
                # no window is the whole block
                c0, r0, _ = W.listing(sa, lo, hi)
                c1, r1, _ = W.listing(sa, lo, hi, np.zeros(len(qs), np.uint32), np.full(len(qs), n + 1, np.uint32))
                assert c0.tolist() == c1.tolist() and r0.tolist() == r1.tolist()
