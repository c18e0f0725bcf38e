"""GPU: the LCP array of a suffix array (archon_hip_lcp, lcp_dev, block_lcp; include/archon_hip.h) against Kasai's pass on
the CPU (tests/lcp_kasai.c, pinned to the definition by test_lcp_abi.py), its work bounds from the call's statistics, the
entry points against each other, and bad input."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import archon_synth as S
import lcp_kasai

pytestmark = pytest.mark.gpu

MiB = 1 << 20
DEFAULT_WINDOW = 256            # lcp.hiph kDefaultWindow: W_0 when no test route names one


@pytest.fixture(scope="module")
def kasai(tmp_path_factory):
    return lcp_kasai.build(tmp_path_factory.mktemp("kasai"))


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _odd(t):
    """the same values at an odd device address (one element past an allocation's start)"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def _lcp_dev(archon, x, sa, odd=False):
    import torch
    x_t, sa_t = _cuda(x), _cuda(sa.view(np.int32))
    out = torch.full((x.size + (1 if odd else 0),), -1, dtype=torch.int32, device="cuda:0")
    if odd:
        x_t, sa_t, out = _odd(x_t), _odd(sa_t), out[1:]
    archon.lcp_dev(x_t, sa_t, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _bound_ok(x, sa, lcp, st, window):
    """compared_bytes <= 2 * sum over irreducible rows of (lcp + 1) + long_items * W_0, and the irreducible count"""
    irr = lcp_kasai.irreducible_rows(x, sa)
    assert st.irreducible == int(irr.sum())
    assert st.compared_bytes <= 2 * int((lcp[irr].astype(np.int64) + 1).sum()) + st.long_items * window
    assert st.max_lcp == int(lcp.max())


def test_exhaustive_tiny(archon, oracle, kasai):
    """every string of length 1-7 over {0, 1, 255}, SA from the oracle, through lcp and lcp_dev"""
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = np.array(t, np.uint8)
            sa = oracle.sa(x)
            want = kasai(x, sa)
            assert (archon.lcp(x, sa) == want).all(), x
            assert (_lcp_dev(archon, x, sa) == want).all(), x


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65536, MiB + 3])
def test_shapes(archon, kasai, shape, n, monkeypatch):
    """every synthetic shape, SA from the GPU forward; once more with a per-lane cap of 1 byte and a first window of 64, so
    that nearly every irreducible row goes through the long comparisons and their rounds"""
    x = S.gen_shape(shape, n)
    sa, _, _ = archon.forward(x)
    want = kasai(x, sa)
    got = archon.lcp(x, sa)
    assert (got == want).all()
    _bound_ok(x, sa, want, archon.lcp_stats(), DEFAULT_WINDOW)
    monkeypatch.setenv("ARCHON_LCP_CAP", "1")
    monkeypatch.setenv("ARCHON_LCP_WINDOW", "64")
    got = archon.lcp(x, sa)
    st = archon.lcp_stats()
    assert (got == want).all()
    _bound_ok(x, sa, want, st, 64)
    if want.max() > 1:
        assert st.long_items > 0 and st.long_rounds > 0


@pytest.mark.parametrize("shape,n", [("random", 256 * MiB), ("prose", 256 * MiB), ("a", 256 * MiB),
                                     ("text", 64 * MiB), ("dna", 64 * MiB), ("ab", 64 * MiB), ("motif", 64 * MiB),
                                     ("motif_defects", 64 * MiB), ("random_copy", 64 * MiB)])
def test_at_scale(archon, kasai, shape, n):
    x = S.gen_shape(shape, n)
    sa, _, _ = archon.forward(x)
    assert archon.validate(x, sa)
    got = archon.lcp(x, sa)
    st = archon.lcp_stats()
    if shape == "a":
        assert got[0] == 0 and (got[1:] == np.arange(n - 1, 0, -1, dtype=np.uint32)).all()
        assert st.max_lcp == n - 1
    else:
        assert (got == kasai(x, sa)).all()
    assert st.long_rounds <= 24


def test_work_bounds(archon):
    """exact, machine-independent work of the two extreme shapes at 16 MiB"""
    n = 16 * MiB
    x = S.gen_shape("a", n)
    sa, _, _ = archon.forward(x)
    lcp = archon.lcp(x, sa)
    st = archon.lcp_stats()
    assert lcp[1] == n - 1
    assert st.irreducible <= 3 and st.long_items >= 1 and st.max_lcp == n - 1 and st.compared_bytes <= 3 * n
    assert st.n == n and st.host_syncs == 3 + st.long_rounds and st.kernel_launches == 6 + 2 * st.long_rounds
    x = S.gen_shape("random", n)
    sa, _, _ = archon.forward(x)
    archon.lcp(x, sa)
    st = archon.lcp_stats()
    assert st.long_items == 0 and st.long_rounds == 0
    assert st.irreducible == int(lcp_kasai.irreducible_rows(x, sa).sum())


def test_entry_points_agree(archon, kasai):
    import torch
    n = MiB + 17
    x = S.gen_shape("prose", n)
    blk = archon.Block()
    sa, _ = blk.forward(x, want_sa=True)
    via_block = blk.lcp()
    want = kasai(x, sa)
    assert (via_block == want).all()
    assert (archon.lcp(x, sa) == want).all()
    assert (_lcp_dev(archon, x, sa) == want).all()
    # the resident form through the thread's default block
    base = ctypes.c_uint32(0)
    L = archon.lib()
    assert L.archon_hip_forward_keep(ctypes.c_void_p(x.ctypes.data), n, ctypes.c_void_p(sa.ctypes.data), ctypes.cast(ctypes.byref(base), ctypes.c_void_p), 0) == 0
    out = np.zeros(n, np.uint32)
    assert L.archon_hip_lcp_keep(0, ctypes.c_void_p(out.ctypes.data)) == 0
    assert (out == want).all()
    # lcp_dev on a side stream, behind a pending kernel that writes the suffix array
    side = torch.cuda.Stream()
    x_t = _cuda(x)
    sa_src = _cuda(sa.view(np.int32))
    sa_t = torch.zeros_like(sa_src)
    out_t = torch.empty_like(sa_src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)
        sa_t.copy_(sa_src)
        archon.lcp_dev(x_t, sa_t, out_t)
    side.synchronize()
    assert (out_t.cpu().numpy().view(np.uint32) == want).all()
    # no suffix array kept: no LCP
    blk.forward(x, want_sa=False)
    with pytest.raises(archon.ArchonError) as e:
        blk.lcp()
    assert e.value.code == archon.E_ARG
    blk.close()


def test_two_contexts_concurrently(archon):
    blocks = [S.gen_shape("text", 4 * MiB + 1), S.gen_shape("motif_defects", 4 * MiB + 5)]
    sas = [archon.forward(x)[0] for x in blocks]
    solo = [archon.lcp(x, sa) for x, sa in zip(blocks, sas)]
    got, errors = [None, None], []

    def run(k):
        try:
            archon.bind_context(k)
            for _ in range(3):
                got[k] = archon.lcp(blocks[k], sas[k])
                assert (got[k] == solo[k]).all()
        except Exception as ex:          # noqa: BLE001 -- reported below
            errors.append(ex)

    threads = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all((g == s).all() for g, s in zip(got, solo))


def test_edges(archon, oracle, kasai):
    for x in (b"q", b"\xff\x00", b"aba", b"\x00\xff\x00\xff\x01"):
        x = np.frombuffer(x, np.uint8).copy()
        sa = oracle.sa(x)
        assert (archon.lcp(x, sa) == kasai(x, sa)).all()
    # a block of 0xFF bytes: INF lies above 255, so the shorter key sorts last and lcp[i] = n - i
    n = 5000
    x = np.full(n, 255, np.uint8)
    sa = oracle.sa(x)
    got = archon.lcp(x, sa)
    assert got[0] == 0 and (got[1:] == np.arange(n - 1, 0, -1)).all()
    # text and suffix array (and the result) at odd device addresses
    x = S.gen_shape("random_copy", 300001)
    sa, _, _ = archon.forward(x)
    assert (_lcp_dev(archon, x, sa, odd=True) == kasai(x, sa)).all()


def test_bad_input(archon, kasai):
    n = 100003
    x = S.gen_shape("text", n)
    sa, _, _ = archon.forward(x)
    for bad in ("zero", "n+1", "twice"):
        b = sa.copy()
        if bad == "zero":
            b[n // 2] = 0
        elif bad == "n+1":
            b[7] = n + 1
        else:
            b[n - 1] = b[0]
        with pytest.raises(archon.ArchonError) as e:
            archon.lcp(x, b)
        assert e.value.code == archon.E_CORRUPT
    rng = np.random.default_rng(5)
    perm = rng.permutation(np.arange(1, n + 1, dtype=np.uint32))
    out = archon.lcp(x, perm)                        # not the suffix array: ARCHON_OK, contents unspecified
    assert out.size == n
    out = archon.lcp(x, sa[::-1].copy())
    assert out.size == n
    assert (archon.lcp(x, sa) == kasai(x, sa)).all()
