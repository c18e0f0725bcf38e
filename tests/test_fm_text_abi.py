"""CPU: the attached suffix array, the matching statistics of a long text and its relative LZ parse (include/archon_hip.h:
archon_hip_fm_attach_sa, _fm_attach_sa_dev, _block_fm_attach_sa, _fm_ms_text, _fm_ms_text_dev, _fm_rlz, _fm_rlz_dev,
_get_fm_text_stats) are declared, exported and bound; the statistics mirror has the C layout; bad arguments are refused and,
without a GPU, the calls fail loudly.  And the walk, sweep and fix of the header (fm_text_naive.Model) are pinned to the
DEFINITION from the text alone (fm_ms_naive.definition) on every short block, text and chunk."""
import ctypes
import inspect
import itertools
import re

import numpy as np
import pytest

from fm_abi_util import ROOT, declared as _declared, layout as _layout, p as _p
import fm_ms_naive as N
import fm_text_naive as T

FUNCTIONS = ["archon_hip_fm_attach_sa", "archon_hip_fm_attach_sa_dev", "archon_hip_block_fm_attach_sa", "archon_hip_fm_ms_text",
             "archon_hip_fm_ms_text_dev", "archon_hip_fm_rlz", "archon_hip_fm_rlz_dev", "archon_hip_get_fm_text_stats"]
FIELDS = ["n", "m", "chunk", "chunks", "fan", "levels", "saturated", "full_chunks", "runs", "longest_run", "sa_probes", "lcp_probes",
          "matched", "longest", "phrases", "sa_bytes", "kernel_launches", "host_syncs", "ms_walk", "ms_sweep", "ms_fix", "ms_parse"]


def test_text_functions_declared_exported_and_bound():
    import pyarchon
    lib = pyarchon.lib()
    declared = _declared("archon_hip.h")
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in pyarchon.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("FmTextStats", "fm_text_stats", "rlz_decode"):
        assert hasattr(pyarchon, name), name
    for name in ("attach_sa", "attach_sa_dev", "ms_text", "ms_text_dev", "rlz", "rlz_dev"):
        assert hasattr(pyarchon.FmIndex, name), name
    params = inspect.signature(pyarchon.Block.fm_index).parameters
    assert params["sa"].default is False and params["lcp"].default is False and params["mirror"].default is False
    assert list(inspect.signature(pyarchon.rlz_decode).parameters)[:3] == ["x", "phrases", "m"]
    assert inspect.signature(pyarchon.FmIndex.ms_text).parameters["rows"].default is True
    assert "MS_CHUNK" in pyarchon._ROUTE_NAMES
    assert "MS_CHUNK" in open(ROOT + "/include/archon_hip_test.h").read()


def test_fm_text_stats_struct_layout(tmp_path):
    """the header declares archon_hip_fm_text_stats with the fields of the issue, in its order, and the ctypes mirror has the
    size and the field offsets the C compiler gives it"""
    import pyarchon
    src = open(ROOT + "/include/archon_hip.h").read()
    body = re.search(r"typedef struct archon_hip_fm_text_stats \{(.*?)\} archon_hip_fm_text_stats;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*;", body) == FIELDS
    names = [k for k, _ in pyarchon.FmTextStats._fields_]
    assert names == FIELDS
    got = _layout(tmp_path, "archon_hip_fm_text_stats", names)
    assert got[0] == ctypes.sizeof(pyarchon.FmTextStats)
    assert got[1:] == [getattr(pyarchon.FmTextStats, k).offset for k in names]


def test_text_bad_arguments():
    """null pointers and lo without hi are ARCHON_E_ARG with or without a device: they are refused before the handle is used (a
    stand-in handle is never read); *total is written 0 before a refusal; an unknown chunk is refused by the test route"""
    import pyarchon
    L = pyarchon.lib()
    E = pyarchon.E_ARG
    text = np.zeros(8, np.uint8)
    ln, lo, hi = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    sa = np.arange(1, 9, dtype=np.uint32)
    stand_in = _p(np.zeros(64, np.uint8))
    fn = L.archon_hip_fm_ms_text
    assert fn(None, _p(text), 8, _p(ln), _p(lo), _p(hi)) == E
    assert fn(stand_in, None, 8, _p(ln), _p(lo), _p(hi)) == E
    assert fn(stand_in, _p(text), 8, None, _p(lo), _p(hi)) == E
    assert fn(stand_in, _p(text), 8, _p(ln), _p(lo), None) == E
    assert fn(stand_in, _p(text), 8, _p(ln), None, _p(hi)) == E
    dv = L.archon_hip_fm_ms_text_dev
    assert dv(None, _p(text), 8, _p(ln), _p(lo), _p(hi), None) == E
    assert dv(stand_in, None, 8, _p(ln), _p(lo), _p(hi), None) == E
    assert dv(stand_in, _p(text), 8, None, _p(lo), _p(hi), None) == E
    assert dv(stand_in, _p(text), 8, _p(ln), _p(lo), None, None) == E
    assert dv(stand_in, _p(text), 8, _p(ln), None, _p(hi), None) == E
    total = ctypes.c_uint64(5)
    tp = ctypes.cast(ctypes.byref(total), ctypes.c_void_p)
    assert L.archon_hip_fm_rlz(None, _p(text), 8, None, 0, tp) == E and total.value == 0
    total.value = 5
    assert L.archon_hip_fm_rlz(stand_in, None, 8, None, 0, tp) == E and total.value == 0
    assert L.archon_hip_fm_rlz(stand_in, _p(text), 8, None, 0, None) == E
    total.value = 5
    assert L.archon_hip_fm_rlz_dev(None, _p(text), 8, None, 0, tp, None) == E and total.value == 0
    assert L.archon_hip_fm_rlz_dev(stand_in, None, 8, None, 0, tp, None) == E
    assert L.archon_hip_fm_rlz_dev(stand_in, _p(text), 8, None, 0, None, None) == E
    assert L.archon_hip_fm_attach_sa(None, _p(sa)) == E
    assert L.archon_hip_fm_attach_sa(stand_in, None) == E
    assert L.archon_hip_fm_attach_sa_dev(None, _p(sa), None) == E
    assert L.archon_hip_fm_attach_sa_dev(stand_in, None, None) == E
    assert L.archon_hip_block_fm_attach_sa(None, stand_in) == E
    assert L.archon_hip_block_fm_attach_sa(stand_in, None) == E
    assert L.archon_hip_get_fm_text_stats(0, None) == E
    assert (ln == 0).all() and (lo == 0).all() and (hi == 0).all()
    assert L.archon_hip_test_route(b"MS_CHUNK", -1) == E
    assert L.archon_hip_test_route(b"MS_CHUNK", 1 << 32) == E
    assert L.archon_hip_test_route(b"MS_CHUNK", 7) == 0 and L.archon_hip_test_route(b"MS_CHUNK", 0) == 0
    if pyarchon.device_count() == 0:
        assert L.archon_hip_get_fm_text_stats(0, ctypes.byref(pyarchon.FmTextStats())) == E


def test_text_no_gpu_fails_loudly():
    """without a device the index cannot be made: ArchonError, no CPU fallback"""
    import pyarchon
    if pyarchon.device_count() > 0:
        pytest.skip("a GPU is present (the GPU suite covers the calls)")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.FmIndex(np.frombuffer(b"nnbaaa", np.uint8).copy(), 2).attach_sa(np.array([2, 4, 6, 1, 3, 5], np.uint32)).ms_text(b"nanan")
    with pytest.raises(pyarchon.ArchonError):
        pyarchon.Block().fm_index(32, lcp=True, sa=True)


def test_model_header_example():
    """the worked example of the header, literally: "banana", the text "nanan", C = 2"""
    M = T.Model(b"banana")
    assert (M.sa, M.isa[1:], M.rule.lcp) == ([2, 4, 6, 1, 3, 5], [3, 0, 4, 1, 5, 2], [0, 1, 3, 0, 0, 2])
    assert M.walk(b"nanan", 2) == [(1, 4, 6), (2, 1, 3), (1, 4, 6), (2, 1, 3), (1, 4, 6)]
    assert M.join((2, 1, 3), 2, 1, 3) == (4, 2, 3)
    assert M.join((2, 1, 3), 1, 4, 6) == (3, 5, 6)
    assert M.join((4, 2, 3), 1, 4, 6) == (4, 5, 6)
    records, ctr = M.run(b"nanan", 2)
    assert records == [(1, 4, 6), (2, 1, 3), (3, 5, 6), (4, 2, 3), (4, 5, 6)] == N.definition(b"banana", b"nanan")
    assert ctr == {"chunks": 3, "saturated": 3, "full_chunks": 3, "runs": 1, "longest_run": 1}
    assert T.chain(T.rlz_records(records, M.sa)) == T.chain([(1, 3), (2, 4), (3, 3), (4, 4), (4, 5)]) == [(5, 4, 5), (1, 1, 3)]


def test_model_against_the_definition():
    """every block of <= 6 bytes over two symbols, every text of <= 6 bytes over those symbols and an absent one, every chunk of
    1 .. 4 bytes: the model's records are the definition's, whatever the chunk; its counters are those the exact lengths give"""
    texts = [bytes(p) for m in range(0, 7) for p in itertools.product((0, 1, 7), repeat=m)]
    cases = joins = 0
    for n in range(1, 7):
        for tt in itertools.product((0, 1), repeat=n):
            x = bytes(tt)
            M = T.Model(x)
            for P in texts:
                want = N.definition(x, P)
                exact = [r[0] for r in want]
                for C in (1, 2, 3, 4):
                    got, ctr = M.run(P, C)
                    assert got == want, (x, P, C)
                    assert ctr == T.counters(T.walk_len_of(exact, C), C), (x, P, C)
                    cases += 1
            joins += M.joins
    assert cases == 126 * 1093 * 4 and joins > 100000


def test_counters_of_the_worst_case():
    """a text that occurs entire in the block: every chunk full, one run of chunks - 2 joins"""
    for m, C in ((64, 8), (65, 8), (1000, 1), (7, 8), (16, 8)):
        k = (m + C - 1) // C
        got = T.counters(T.walk_len_of(np.arange(1, m + 1), C), C)
        assert got == {"chunks": k, "saturated": max(m - C, 0), "full_chunks": k, "runs": int(k > 2), "longest_run": max(k - 2, 0)}
