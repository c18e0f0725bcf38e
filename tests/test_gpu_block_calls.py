"""GPU: the resident LCP step of a block -- the LCP array into staging buffer 1, its record kept for the thread, its time into
the caller's ms_lcp -- through its four callers: Block.lcp, Block.repeats, Block.lz and Block.fm_index(..., lcp=True) (which
makes archon_hip_block_fm_attach_lcp), in the manner of test_gpu_fm_part_calls.py and on its block.  After each caller the
thread's lcp_stats describe this block with the launches and waits of a plain Block.lcp, the caller's own record has its
ms_lcp and the launches and waits pinned below, and the answer is right.  A block without its suffix array refuses all four
and leaves lcp_stats as they were.

The pinned figures are the ones the library reported at the commit before the one that added this test
(profiles/block/block_calls_parent.txt)."""
import numpy as np
import pytest

import archon_synth as S
import lcp_kasai
import lz_naive
import repeats_naive

pytestmark = pytest.mark.gpu

N = 256 << 10
RATE = 32
LEVELS = 5                              # 256 Ki entries at F = 16: 16 Ki, 1 Ki, 64, 4, 1
# (kernel_launches, host_syncs) of each caller's own record; a wait is one host wait for the call's stream
LCP = (20, 10)                          # lcp_stats of a plain Block.lcp of this block (7 long rounds): every caller leaves the same
# A caller's record counts its own launches and, as host_syncs, every wait of the call: the LCP step's ten and its own
#   repeats   count only: one wait for the counters; with the repeats: the last C call, one wait for the counters, one for the records
#             (two until the listing calls got one ending, analysis.hiph: the emit pass and the copy home had a wait each)
REPEATS = {"count": (9, LCP[1] + 1), "emit": (11, LCP[1] + 2)}
#   lz        the LPF pass and the parse, count only / with the phrases (the last C call of the wrapper's two; one wait for the
#             phrases, as for the repeats)
LZ = {"count": (272, LCP[1] + 2), "emit": (274, LCP[1] + 3)}
#   attach    the guard and one kernel per level; one wait for the guard's flag
ATTACH_LCP = (1 + LEVELS, LCP[1] + 1)


@pytest.fixture(scope="module")
def block(oracle, tmp_path_factory):
    """the block with its oracle arrays and what the CPU helpers make of them: computed once, shared, left unchanged"""
    x = S.gen_prose(N, S.SEED_BASE + 6)
    sa, bwt, base = oracle.forward(x)
    lcp = lcp_kasai.build(tmp_path_factory.mktemp("block_kasai"))(x, sa)
    repeats = repeats_naive.build(tmp_path_factory.mktemp("block_repeats"))(lcp, bwt, base, 1)[0]
    lz = lz_naive.build(tmp_path_factory.mktemp("block_lz"))
    phrases = lz.parse(lz.lpf(sa, lcp, 0))
    for a in (x, sa, bwt, lcp, repeats, phrases):
        a.setflags(write=False)
    return {"x": x, "sa": sa, "bwt": bwt, "base": base, "lcp": lcp, "repeats": repeats, "phrases": phrases}


def _lw(st):
    print("   ", type(st).__name__, st.asdict())
    return st.kernel_launches, st.host_syncs


def _lcp_step(archon):
    """the thread's LCP record after a caller: this block's, with the launches and waits of a plain Block.lcp"""
    st = archon.lcp_stats()
    assert st.n == N and _lw(st) == LCP
    return st


def test_lcp_step_of_every_caller(archon, block):
    b = archon.Block()
    try:
        b.forward(block["x"])
        assert (b.lcp() == block["lcp"]).all()
        _lcp_step(archon)

        want = block["repeats"]
        for key in ("count", "emit"):
            got = b.repeats(1, count_only=key == "count")
            _lcp_step(archon)
            st = archon.repeat_stats()
            assert st.ms_lcp > 0 and _lw(st) == REPEATS[key]
            assert (got == want.size) if key == "count" else (got.size == want.size and (got == want).all())

        want = block["phrases"]
        for key in ("count", "emit"):
            got = b.lz(0, count_only=key == "count")
            _lcp_step(archon)
            st = archon.lz_stats()
            assert st.ms_lcp > 0 and _lw(st) == LZ[key]
            assert (got == want.size) if key == "count" else (got.size == want.size and (got == want).all())

        f = b.fm_index(RATE, lcp=True)
        _lcp_step(archon)
        st = archon.fm_ms_stats()
        assert st.ms_lcp > 0 and _lw(st) == ATTACH_LCP and (st.levels, st.attached) == (LEVELS, 1)
        # the attached array is the block's: matching statistics as from a handle that was given the CPU's LCP array
        g = archon.FmIndex(block["bwt"], block["base"]).attach_lcp(block["lcp"])
        pats = [block["x"][777:777 + 40].tobytes(), bytes([1, 2, 3, 254, 255, 0, 7, 9])]
        for got, want in zip(f.ms(pats), g.ms(pats)):
            assert (np.asarray(got) == np.asarray(want)).all()
        g.close()
        f.close()
    finally:
        b.close()


def test_refusal_without_the_suffix_array(archon, block):
    b, other = archon.Block(), archon.Block()
    try:
        b.forward(block["x"])
        f = b.fm_index(RATE)
        # the thread's last LCP record is another, smaller block's: a refused call must leave exactly that
        other.forward(block["x"][:4096])
        other.lcp()
        before = archon.lcp_stats().asdict()
        assert before["n"] == 4096
        b.forward(block["x"], want_sa=False)
        L = archon.lib()
        calls = {"lcp": b.lcp, "repeats": lambda: b.repeats(1, count_only=True), "lz": lambda: b.lz(0, count_only=True),
                 "attach_lcp": lambda: archon._check(L.archon_hip_block_fm_attach_lcp(b.h, f.h))}
        for name, call in calls.items():
            with pytest.raises(archon.ArchonError, match="no resident block with its suffix array"):
                call()
            assert archon.lcp_stats().asdict() == before, name
        f.close()
    finally:
        b.close()
        other.close()
