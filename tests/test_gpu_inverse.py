"""GPU parity: inverse BWT (lf_build + lf_walk) vs the CPU oracle, and round trips."""
import numpy as np
import pytest

import archon_synth as S
import inv_chain_model as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1, 2, 9, 1000, 65536, 1 << 20])
def test_inverse_vs_oracle(archon, oracle, shape, n):
    x = S.gen_shape(shape, n)
    _, B, base = oracle.forward(x)
    out = archon.inverse(B, base)
    assert (out == x).all()


def test_round_trip_gpu_only(archon):
    """encode -> decode on the GPU: a size-independent property (no oracle involved)."""
    for shape in S.SHAPES:
        x = S.gen_shape(shape, (1 << 21) + 7)
        _, bwt, base = archon.forward(x, want_sa=False)
        assert (archon.inverse(bwt, base) == x).all(), shape


def test_inverse_rejects_non_bwt(archon, oracle):
    """a byte string that is not a BWT: the LF walk does not close over all rows (the oracle's walk says so too)"""
    bad = np.frombuffer(b"abab", np.uint8)   # LF permutation of "abab" with base 0 has two cycles
    import ctypes
    assert oracle.inverse(bad, 0)[0] != 0
    out = np.empty(4, np.uint8)
    rc = archon.lib().archon_hip_inverse(ctypes.c_void_p(bad.ctypes.data), 4, 0, ctypes.c_void_p(out.ctypes.data), 0)
    assert rc == archon.E_CORRUPT
    rc = archon.lib().archon_hip_inverse(ctypes.c_void_p(bad.ctypes.data), 4, 7, ctypes.c_void_p(out.ctypes.data), 0)
    assert rc == archon.E_ARG


@pytest.mark.parametrize("slab", ["16", "64"])
def test_inverse_long_chain_route(archon, oracle, slab, monkeypatch):
    """the single walk stores each sub-chain in a slab; chains that outgrow it are walked again (k_walk_emit).
    Tiny slabs make that route carry most of the block."""
    monkeypatch.setenv("ARCHON_INV_SLAB", slab)
    for shape, n in (("random", 300001), ("text", 1 << 20), ("a", 70000), ("dna", 123457)):
        x = S.gen_shape(shape, n)
        _, B, base = oracle.forward(x)
        assert (archon.inverse(B, base) == x).all(), (shape, n)


@pytest.mark.parametrize("rows", ["0", "1", "2"])
def test_inverse_walk_variants(archon, oracle, rows, monkeypatch):
    """the walk writes its slabs by quads through LDS rows (k_walk_rows: 128-byte rows = 1, the product's choice above 128 MiB; 64-byte rows = 2)
    or lane by lane (k_walk_queue = 0)"""
    monkeypatch.setenv("ARCHON_INV_ROWS", rows)
    for slab in ("0", "128", "192"):          # (192: a multiple of 64 only -- the 128-byte rows fall back to 64-byte ones)
        monkeypatch.setenv("ARCHON_INV_SLAB", slab)
        for shape, n in (("random", 300001), ("text", (1 << 21) + 5), ("dna", 400000), ("a", 140000)):
            x = S.gen_shape(shape, n)
            _, B, base = oracle.forward(x)
            assert (archon.inverse(B, base) == x).all(), (shape, n, slab)


def test_inverse_unaligned_device_buffers(archon, oracle):
    """chain copies start at any byte offset; so may the caller's buffers"""
    import torch
    x = S.gen_shape("text", 500003)
    _, B, base = oracle.forward(x)
    buf = torch.zeros(x.size + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(x.size + 64, dtype=torch.uint8, device="cuda")
    for off_in, off_out in ((0, 0), (1, 3), (7, 2), (16, 5)):
        buf[off_in:off_in + x.size] = torch.from_numpy(B).cuda()
        archon.inverse_dev(buf[off_in:off_in + x.size], base, out[off_out:off_out + x.size])
        assert (out[off_out:off_out + x.size].cpu().numpy() == x).all(), (off_in, off_out)


# ---------------------------------------------------------------- the walk at every chain geometry the product uses
# tests/inv_chain_model.py holds the table of (input, geometry, edges) and the model that says which kernel a case runs
# and which chain lengths its input holds there; tests/test_inv_chain_model.py proves the edges on the CPU.

@pytest.fixture(scope="module")
def chain_inputs(oracle):
    """name -> (x, B, base) of every input of the table, from the oracle, computed once"""
    out = {}
    for name in M.INPUTS:
        x = M.gen_input(name)
        _, B, base = oracle.forward(x)
        out[name] = (x, B, base)
    return out


def _run_case(archon, case, x, B, base, monkeypatch):
    """inverse under the case's routes = x, with the chains of the model and the launches of one closed cut"""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sbits, _ = M.route_of_env(x.size, case.env)
    out = archon.inverse(B, base)
    st = archon.stats()
    bad = np.flatnonzero(out != x)
    assert bad.size == 0, (case.id, "first wrong byte at", int(bad[0]), "of", x.size, "wrong bytes:", bad.size)
    nchains = M.nchains_of(x.size, sbits)
    assert st["walk_chains"] == nchains, (case.id, st["walk_chains"], nchains)
    assert st["kernel_launches"] == 3 + 1 + M.rank_rounds(nchains) + 3, (case.id, st["kernel_launches"], nchains)


@pytest.mark.parametrize("case", M.cases("geometry"), ids=[c.id for c in M.cases("geometry")])
def test_inverse_chain_geometries(archon, chain_inputs, case, monkeypatch):
    """each row of the table: sbits 4..6 on the queue walk, several rows per slab and exactly full slabs on both rows
    kernels, 64-byte rows where 128 do not divide the slab, 0 / 1 / 2 walk workgroups per CU, few long chains on a small
    block.  walk_chains shows that INV_SBITS took effect, the launch count that the first cut closed"""
    _run_case(archon, case, *chain_inputs[case.input], monkeypatch)


@pytest.mark.parametrize("case", M.cases("base"), ids=[c.id for c in M.cases("base")])
def test_inverse_base_edges(archon, chain_inputs, case, monkeypatch):
    """row `base` on a regular head (the unused slot of the extra chain), base == 0, base == n - 1, the last region's cut row
    clamped to n - 1, the chain from `base` filling the last slab: on k_walk_store, k_walk_queue and both k_walk_rows"""
    _run_case(archon, case, *chain_inputs[case.input], monkeypatch)


@pytest.mark.parametrize("geometry", ["rows128_s5", "rows64_s4_slab64"])
def test_inverse_unaligned_under_rows(archon, chain_inputs, geometry, monkeypatch):
    """the caller's buffers at any byte offset while the slabs are written through LDS rows: the block comes back, and not a
    byte in front of it or behind it changes"""
    import torch
    cs = [c for c in M.cases("unaligned") if c.id.startswith("unaligned_" + geometry)]
    assert [(c.in_offset, c.out_offset) for c in cs] == list(M.OFFSETS)
    x, B, base = chain_inputs[cs[0].input]
    for k, v in cs[0].env.items():
        monkeypatch.setenv(k, v)
    n, pad, sentinel = x.size, 64, 0xA5
    B_t = torch.from_numpy(B).cuda()
    buf = torch.zeros(n + pad, dtype=torch.uint8, device="cuda")
    out = torch.empty(n + pad, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0          # (the census took the output's alignment from the offset)
    sbits, _ = M.route_of_env(n, cs[0].env)
    for c in cs:
        oi, oo = c.in_offset, c.out_offset
        buf[oi:oi + n] = B_t
        out.fill_(sentinel)
        archon.inverse_dev(buf[oi:oi + n], base, out[oo:oo + n])
        got = out.cpu().numpy()
        assert (got[oo:oo + n] == x).all(), c.id
        assert (got[:oo] == sentinel).all() and (got[oo + n:] == sentinel).all(), c.id
        assert archon.stats()["walk_chains"] == M.nchains_of(n, sbits), c.id


@pytest.mark.parametrize("shape,n", [(s, n) for n in ((4 << 20) + 1, (8 << 20) + 3, (16 << 20) + 5) for s in ("text", "dna")])
def test_round_trip_product_geometry(archon, shape, n):
    """forward -> inverse on the GPU with nothing forced: the product's own sbits 4, 5 and 6 (no oracle involved)"""
    x = S.gen_shape(shape, n)
    _, bwt, base = archon.forward(x, want_sa=False)
    out = archon.inverse(bwt, base)
    st = archon.stats()
    assert (out == x).all()
    sbits = M.inv_sbits(n)
    assert sbits == {4 << 20: 4, 8 << 20: 5, 16 << 20: 6}[n & ~0xFF]
    assert st["walk_chains"] == M.nchains_of(n, sbits)
    assert st["kernel_launches"] == M.inverse_launches(st["walk_chains"])
