"""GPU: the device memory a resident block and a compute context own.  One block through forwards that grow its text and BWT,
grow its suffix array and then reuse all three while smaller; two blocks on two threads whose forwards interleave; and
archon_hip_release between two forwards, after which the contexts and the one-shot scratch of hist256 and radix_scatter are
made again.  Every answer is checked against the CPU oracle or numpy."""
import threading

import numpy as np
import pytest

import archon_synth as S

pytestmark = pytest.mark.gpu

KiB = 1 << 10


def _count(bwt, base, p):
    """(lo, hi) of pattern p by the rule of include/archon_hip.h over the oracle's BWT: P[0] first, occ leaves the primary row out"""
    R = np.concatenate([[0], np.cumsum(np.bincount(bwt, minlength=256))])

    def occ(c, i):
        return int(np.count_nonzero(bwt[:i] == c)) - int(base < i and bwt[base] == c)

    lo, hi = int(R[p[0]]), int(R[p[0] + 1])
    for c in p[1:]:
        if lo >= hi:
            break
        lo, hi = int(R[c]) + occ(c, lo), int(R[c]) + occ(c, hi)
    return lo, hi


def test_one_block_grows_and_shrinks(archon, oracle):
    """4 KiB without SA, 64 KiB with, 1 KiB with, 256 KiB without: x and bwt grow, sa grows, all three are reused while smaller,
    x and bwt grow again beside an sa that stays; the block's own FM handle is rebuilt after each forward"""
    b = archon.Block()
    try:
        for i, (n, want_sa) in enumerate([(4 * KiB, False), (64 * KiB, True), (1 * KiB, True), (256 * KiB, False)]):
            x = S.gen_prose(n, S.SEED_BASE + 20 + i)
            P, B, b0 = oracle.forward(x)
            sa, base = b.forward(x, want_sa=want_sa)
            assert base == b0 and (b.read_bwt() == B).all()
            assert (b.read_bwt(n // 3, n // 2) == B[n // 3:n // 3 + n // 2]).all()
            if want_sa:
                assert (sa == P).all() and b.validate() is True
            pats = [x[q:q + m].tobytes() for q, m in ((0, 3), (n // 2, 9), (n - 20, 20))]
            lo, hi = b.fm_count(pats)
            assert archon.fm_stats().built == 1
            for j, p in enumerate(pats):
                assert (int(lo[j]), int(hi[j])) == _count(B, b0, p) and hi[j] > lo[j], (n, p)
        with pytest.raises(archon.ArchonError, match="no resident block with its suffix array"):
            b.lcp()
    finally:
        b.close()


def test_two_blocks_on_two_threads(archon, oracle):
    """two blocks, a thread each, forwards of 16 KiB and 48 KiB taken in turn: one grows while the other is reused smaller, and
    each reads back its own BWT (test_gpu_cli.py's six objects are of equal size: none of their buffers is ever replaced)"""
    sizes = (16 * KiB, 48 * KiB)
    xs = [[S.gen_prose(n, S.SEED_BASE + 30 + 2 * t + k) for k, n in enumerate(sizes[::1 - 2 * t])] for t in (0, 1)]
    want = [[oracle.forward(x) for x in row] for row in xs]
    barrier = threading.Barrier(2)
    errs = []

    def work(t):
        try:
            b = archon.Block()
            for x, (P, B, b0) in zip(xs[t], want[t]):
                barrier.wait(60)
                sa, base = b.forward(x)
                barrier.wait(60)                      # both have computed before either reads back
                assert base == b0 and (sa == P).all() and (b.read_bwt() == B).all() and b.validate() is True
            b.close()
        except Exception as e:      # noqa: BLE001
            errs.append((t, repr(e)))
            barrier.abort()

    ts = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs


def test_release_then_again(archon, oracle):
    """archon_hip_release(0) frees every context of the device; the next call makes its context again and computes the same"""
    x = S.gen_prose(64 * KiB, S.SEED_BASE + 40)
    P, B, b0 = oracle.forward(x)
    rng = np.random.default_rng(40)
    small = {n: rng.integers(0, 256, n, dtype=np.uint8) for n in (1, 4097, 70000)}

    def run():
        sa, bwt, base = archon.forward(x)
        assert (sa == P).all() and (bwt == B).all() and base == b0
        for n in (1, 4097):
            assert (archon.hist256(small[n]) == np.bincount(small[n], minlength=256)).all(), n
        for n in (1, 70000):
            assert (archon.radix_scatter(small[n]) == np.sort(small[n])).all(), n

    run()
    assert archon.lib().archon_hip_release(0) == 0
    run()
    assert archon.reserve(x.size) > 0
