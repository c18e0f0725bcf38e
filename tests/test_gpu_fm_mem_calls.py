"""GPU: how many kernels every mirror / SMEM entry point launches and how often it waits for its stream (kernel_launches and
host_syncs of archon_hip_fm_mem_stats), in the manner of test_gpu_fm_calls.py: the other SMEM tests pin results, order and
work counters; this one pins the shape of each call.  A wait is one host wait for the call's stream; the device-wide wait of an
arena that grows is not counted.  A record describes the last C call only, so the cases that need one particular C call go
through pyarchon.lib()."""
import ctypes

import numpy as np
import pytest

import archon_synth as S

pytestmark = pytest.mark.gpu

N = 256 << 10
RATE = 32
# The drivers, step by step (fm_host.hiph):
#   fm_search_count   the count pass: 1 launch; one wait for the counters, nmems and nocc
#   fm_search_emit    the emit pass: 1 launch; one wait for it
#   fm_search_host    the count, then (SMEMs wanted and found, cap large enough) the emit and one wait more for the SMEMs' copy
#   fm_search_dev     the count, then the emit: the SMEMs stay on the device
#   fmm_locate   1 launch (the gather or the walks), one wait for the starts
COUNT_ONLY = (1, 1)
HOST_WITH_MEMS = (2, 3)
DEV_WITH_MEMS = (2, 2)
LOCATE = (1, 1)
# A mirror build: the nested transforms' launches are whatever those transforms report for the same input (read from their
# own statistics below), plus 1 (the reverse kernel), plus 3 (the table: fm_build), plus 1 when the caller's text is guarded
# by its byte counts.  Its waits: those of the nested forward (its statistics say), one for the mirror's primary row, one
# inside fm_build, one at the end for the events; the inverse's single wait is not a counted one (inverse_run), the guard's
# read-back is.
MIRROR_EXTRA_LAUNCHES = 1 + 3
MIRROR_EXTRA_WAITS = 3


@pytest.fixture(scope="module")
def text():
    x = S.gen_prose(N, S.SEED_BASE + 6)
    rng = np.random.default_rng(11)
    found = [x[q:q + 24].tobytes() for q in rng.integers(0, N - 24, 6)]
    chimera = [found[0] + found[1], found[2][:10] + bytes([1, 2, 3]) + found[3]]
    absent = [bytes([1, 2, 3, 254, 255, 0, 7, 9])]
    return x, found + chimera, absent


def _lw(st):
    print("   ", type(st).__name__, st.asdict())
    return st.kernel_launches, st.host_syncs


def _total():
    t = ctypes.c_uint64(0)
    return t, ctypes.cast(ctypes.byref(t), ctypes.c_void_p)


def test_mirror_builds(archon, text):
    import torch
    x, _, _ = text
    xr = x[::-1].copy()
    b = archon.Block()
    try:
        _, base = b.forward(x)
        bwt = b.read_bwt()
        # what the nested transforms launch and wait for on these inputs, by their own records
        archon.inverse(bwt, base)
        inv_launches = archon.stats()["kernel_launches"]
        archon.forward(xr, want_sa=False)
        fwd = archon.stats()
        f = archon.FmIndex(bwt, base)
        f.mirror()
        st = archon.fm_mem_stats()
        assert _lw(st) == (inv_launches + fwd["kernel_launches"] + MIRROR_EXTRA_LAUNCHES, fwd["host_syncs"] + MIRROR_EXTRA_WAITS)
        assert st.built == 1 and st.ms_mirror > 0
        x_t = torch.from_numpy(x).to("cuda:0")
        f.mirror(x_t)
        st = archon.fm_mem_stats()
        assert _lw(st) == (fwd["kernel_launches"] + MIRROR_EXTRA_LAUNCHES + 1, fwd["host_syncs"] + MIRROR_EXTRA_WAITS + 1)
        f.close()
        g = b.fm_index(RATE, mirror=True)
        st = archon.fm_mem_stats()
        assert _lw(st) == (fwd["kernel_launches"] + MIRROR_EXTRA_LAUNCHES, fwd["host_syncs"] + MIRROR_EXTRA_WAITS)
        g.close()
    finally:
        b.close()


def test_smems_and_locate(archon, text):
    import torch
    x, found, absent = text
    pats = found + absent
    b = archon.Block()
    try:
        b.forward(x)
        f = b.fm_index(RATE, mirror=True)
        L = archon.lib()
        packed, off = archon._pack_patterns(pats)
        k = off.size - 1
        nm, no = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        t, tp = _total()
        assert L.archon_hip_fm_smems(f.h, archon._p(packed), archon._p(off), k, 1, archon._p(nm), archon._p(no), None, 0, tp) == 0
        st = archon.fm_mem_stats()
        assert _lw(st) == COUNT_ONLY and st.built == 0
        total = t.value
        assert total >= len(found)
        mems = np.zeros(total, archon.FM_MEM)
        assert L.archon_hip_fm_smems(f.h, archon._p(packed), archon._p(off), k, 1, archon._p(nm), archon._p(no), archon._p(mems), total, tp) == 0
        assert _lw(archon.fm_mem_stats()) == HOST_WITH_MEMS
        # room for one SMEM fewer than there are: the call ends after the count, with the total set
        assert L.archon_hip_fm_smems(f.h, archon._p(packed), archon._p(off), k, 1, archon._p(nm), archon._p(no), archon._p(mems), total - 1,
                                     tp) == archon.E_ARG
        assert t.value == total and _lw(archon.fm_mem_stats()) == COUNT_ONLY
        # no SMEM at all: no emit pass
        a_packed, a_off = archon._pack_patterns(absent)
        assert L.archon_hip_fm_smems(f.h, archon._p(a_packed), archon._p(a_off), 1, 1, archon._p(nm), archon._p(no), archon._p(mems), total, tp) == 0
        assert t.value == 0 and _lw(archon.fm_mem_stats()) == COUNT_ONLY
        nt = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        ct = torch.zeros(k, dtype=torch.int32, device="cuda:0")
        mt = torch.zeros(6 * total, dtype=torch.int32, device="cuda:0")
        assert f.smems_dev(torch.tensor(packed, device="cuda:0"), torch.tensor(off.astype(np.int32), device="cuda:0"), 1, nt, ct, mt) == total
        assert _lw(archon.fm_mem_stats()) == DEV_WITH_MEMS
        assert (mt.cpu().numpy().view(np.uint32).view(archon.FM_MEM) == mems).all()
        via_samples = f.locate_mems(mems)
        assert _lw(archon.fm_mem_stats()) == LOCATE
        via_sa = b.fm_locate_mems(mems)
        assert _lw(archon.fm_mem_stats()) == LOCATE
        assert sum(p.size for p in via_sa) == int((mems["hi"] - mems["lo"]).sum()) > 0
        assert all((u == v).all() for u, v in zip(via_sa, via_samples))
        # SMEMs without rows, and none at all: nothing to launch and nothing to wait for
        empty = mems[:2].copy()
        empty["hi"] = empty["lo"]
        for q in (empty, mems[:0]):
            assert sum(p.size for p in b.fm_locate_mems(q)) == 0
            assert _lw(archon.fm_mem_stats()) == (0, 0)
            assert sum(p.size for p in f.locate_mems(q)) == 0
            assert _lw(archon.fm_mem_stats()) == (0, 0)
        f.close()
    finally:
        b.close()
