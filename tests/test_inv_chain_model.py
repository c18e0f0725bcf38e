"""CPU: the model of the inverse's cut (tests/inv_chain_model.py) against the oracle, and the edge census of the table of
cases that tests/test_gpu_inverse.py runs on the GPU.

The census is what keeps the GPU cases from passing vacuously: a case listed for "a chain of exactly slab_bytes symbols"
is only worth its GPU time while its input holds such a chain at its geometry.  A change to the hash, the slab rule or the
row flush that drops an edge out of an input fails here, on a machine without a GPU.
"""
import itertools

import numpy as np
import pytest

import archon_synth as S
import inv_chain_model as M


# ---------------------------------------------------------------- the model against the oracle
def test_emit_exhaustive_tiny(oracle):
    """every string of length 1..7 over {0, 1, 255}: the model's walk gives the oracle's inverse, which is the input"""
    cases = 0
    for n in range(1, 8):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = np.array(t, np.uint8)
            _, B, base = oracle.forward(x)
            rc, want = oracle.inverse(B, base)
            got = M.emit(B, base)
            assert rc == 0 and (got == want).all() and (got == x).all(), t
            assert (M.lf_table(B, base) == oracle.lf_build(B, base)).all(), t
            cases += 1
    assert cases == sum(3 ** n for n in range(1, 8))


def _check_chains(ch, n, base, sbits, salt=0):
    used = np.flatnonzero(ch.len > 0)
    assert ch.nchains == M.nchains_of(n, sbits) == ch.len.size
    assert ch.len.sum() == n
    assert used.size == ch.nchains - ch.base_on_head
    # `next` is one cycle over the used ids, and `start` follows from the lengths along it
    j = M.head_id(base, n, base, sbits, salt)
    assert j == (base >> sbits if ch.base_on_head else ch.nreg)
    seen, at = 0, 0
    for _ in range(used.size):
        assert ch.len[j] > 0 and ch.start[j] == at
        at += int(ch.len[j])
        j = int(ch.next[j])
        seen += 1
    assert seen == used.size and at == n and j == M.head_id(base, n, base, sbits, salt)
    assert np.unique(ch.next[used]).size == used.size


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", [1000, 65537])
def test_model_on_shapes(oracle, shape, n):
    """emit = oracle.inverse = the input on every shape; chain lengths sum to n and `next` is one cycle, for sbits 3, 5, 12"""
    x = S.gen_shape(shape, n)
    _, B, base = oracle.forward(x)
    rc, want = oracle.inverse(B, base)
    got = M.emit(B, base)
    assert rc == 0 and (got == want).all() and (got == x).all()
    order = M.walk_order(M.lf_table(B, base), base)
    for sbits in (3, 5, 12):
        _check_chains(M.chains(B, base, sbits, 0, order), n, base, sbits)
    _check_chains(M.chains(B, base, 5, M.salt_of(1), order), n, base, 5, M.salt_of(1))        # the second cut's salt


def test_cut_row_by_hand():
    """the hash in plain Python integers, the clamp, and the two helpers built on it"""
    def plain(j, n, sbits, salt):
        h = ((j ^ salt) * 0x9E3779B1) & 0xFFFFFFFF
        h ^= h >> 15
        return min((j << sbits) + (h & ((1 << sbits) - 1)), n - 1)
    for n, sbits in ((1, 3), (9, 3), (1000, 3), (1000, 5), (65537, 12), ((1 << 20) + 5, 5), (0x3FFFFF00, 8)):
        nreg = -(-n >> sbits)
        for salt in (0, 0x85EBCA6B):
            js = sorted({0, 1, nreg // 2, nreg - 1})
            assert [M.cut_row(j, n, sbits, salt) for j in js] == [plain(j, n, sbits, salt) for j in js]
            assert list(M.cut_row(np.array(js), n, sbits, salt)) == [plain(j, n, sbits, salt) for j in js]
    assert M.salt_of(0) == 0 and M.salt_of(1) == 0x85EBCA6B and M.salt_of(3) == (3 * 0x85EBCA6B) % (1 << 32)
    # a last region of one row: whatever the hash says, its head is row n - 1
    assert M.cut_row(2, 17, 3) == 16 and M.head_id(16, 17, 5, 3) == 2 and M.head_row(2, 17, 5, 3) == 16
    assert M.head_row(3, 17, 5, 3) == 5 and M.head_id(5, 17, 5, 3) == 3 and M.head_id(6, 17, 5, 3) == M.NIL
    assert M.cut_row(0, 1, 3) == 0 and M.nchains_of(1, 3) == 2


def test_route_by_hand():
    """the driver's rule on cases worked out from inverse_run by hand"""
    cu = M.num_cu()
    assert cu == 256
    big = (1 << 20) + 51
    R = M.Route
    assert M.route(big, 5, num_cu=cu) == R("walk_queue", 512, 3)
    assert M.route(big, 5, inv_rows=0, num_cu=cu) == R("walk_queue", 512, 3)
    assert M.route(big, 5, inv_rows=1, num_cu=cu) == R("walk_rows128", 512, 2)           # three per CU capped at two
    assert M.route(big, 5, inv_rows=1, walk_wgs=1, num_cu=cu) == R("walk_rows128", 512, 1)
    assert M.route(big, 5, inv_rows=1, inv_slab=192, num_cu=cu) == R("walk_rows64", 192, 3)
    assert M.route(big, 5, inv_rows=1, inv_slab=200, num_cu=cu) == R("walk_rows64", 192, 3)  # slabs are cut to 16 bytes
    assert M.route(big, 5, inv_rows=1, inv_slab=16, num_cu=cu) == R("walk_queue", 16, 3)     # no row fits
    assert M.route(big, 5, inv_rows=1, inv_slab=512, num_cu=cu) == R("walk_rows128", 512, 2) # not below the default: ignored
    assert M.route(big, 4, inv_rows=2, inv_slab=64, num_cu=cu) == R("walk_rows64", 64, 3)
    assert M.route(big, 5, inv_rows=2, num_cu=cu) == R("walk_rows64", 512, 3)
    assert M.route(big, 5, inv_rows=1, walk_wgs=0, num_cu=cu) == R("walk_store", 512, 0)
    assert M.route(big, 7, inv_rows=1, num_cu=cu) == R("walk_store", 2048, 0)              # 8194 chains: below 64 per CU
    assert M.route(big, 6, inv_rows=0, num_cu=cu) == R("walk_queue", 1024, 3)              # 16386 chains
    assert M.route(100003, 3, inv_rows=1, num_cu=cu) == R("walk_store", 128, 0)
    assert M.route((128 << 20) + 4099, 7, num_cu=cu) == R("walk_rows128", 2048, 2)         # the product above 128 MiB
    assert M.route(128 << 20, 7, num_cu=cu) == R("walk_queue", 2048, 3)
    # the product's sbits (inverse.hiph: 3 up to 2 MiB, 4 at 4 MiB, 5 at 8, 6 at 16 and 32, 7 at 64 and 128, 8 at 256) and the clamp
    assert [M.inv_sbits(m << 20) for m in (1, 2, 4, 8, 16, 32, 64, 128, 256)] == [3, 3, 4, 5, 6, 6, 7, 7, 8]
    assert M.inv_sbits((4 << 20) - 1) == 3 and M.inv_sbits(1) == 3 and M.inv_sbits(0x3FFFFF00) == 8
    assert [M.inv_sbits(1 << 20, f) for f in (0, 2, 3, 9, 12, 13, 40)] == [3, 3, 3, 9, 12, 12, 12]
    assert [M.rank_rounds(c) for c in (1, 2, 4, 5, 16, 17, 16386, 32771, 65541)] == [0, 1, 1, 2, 2, 3, 8, 8, 9]
    assert M.inverse_launches(32771) == 15


# ---------------------------------------------------------------- the census
@pytest.fixture(scope="module")
def walks(oracle):
    """name -> (x, bwt, base, walk order) of every input of the table, computed once"""
    out = {}
    for name in M.INPUTS:
        x = M.gen_input(name)
        _, B, base = oracle.forward(x)
        out[name] = (x, B, base, M.walk_order(M.lf_table(B, base), base))
    return out


def test_inputs_are_few_and_sized():
    """two inputs of 2^20 + small odd rows for the kernels that need 16384 chains; the rest have 2^17 rows or fewer"""
    sizes = sorted(spec[1] for spec in M.INPUTS.values())
    assert len(sizes) <= 5
    assert all((1 << 20) < n < (1 << 20) + 64 and n % 2 for n in sizes[-2:]) and all(n <= (1 << 17) for n in sizes[:-2])


def test_model_inverts_the_inputs(walks):
    for name, (x, B, base, order) in walks.items():
        assert (np.searchsorted(M.bucket_starts(B), order, side="right") - 1 == x).all(), name


def test_table_ids_are_unique_and_cover_the_issue():
    ids = [c.id for c in M.CASES]
    assert len(set(ids)) == len(ids)
    assert {c.group for c in M.CASES} == {"geometry", "base", "unaligned"}
    geo = {(c.kernel, c.env.get("ARCHON_INV_SBITS"), c.env.get("ARCHON_INV_ROWS"), c.env.get("ARCHON_INV_SLAB"), c.env.get("ARCHON_INV_WALK_WGS"))
           for c in M.cases("geometry")}
    for want in [("walk_queue", "4", "0", None, None), ("walk_queue", "5", "0", None, None), ("walk_queue", "6", "0", None, None),
                 ("walk_rows128", "5", "1", None, None), ("walk_rows128", "6", "1", None, None), ("walk_rows128", "5", "1", "128", None),
                 ("walk_rows64", "4", "2", "64", None), ("walk_rows64", "5", "1", "192", None),
                 ("walk_store", "8", None, None, None), ("walk_store", "12", None, None, None)]:
        assert want in geo, want
    for kernel in ("walk_queue", "walk_rows64", "walk_rows128"):
        assert {c.env.get("ARCHON_INV_WALK_WGS") for c in M.cases("geometry") if c.kernel == kernel} >= {None, "1", "2"}, kernel
    assert sum(c.env.get("ARCHON_INV_WALK_WGS") == "0" and c.kernel == "walk_store" for c in M.cases("geometry")) >= 3
    # each kernel has its exact-slab, slab-plus-one, several-stores and base-coincidence case
    for kernel in M.STORE_UNIT:
        listed = set().union(*(c.edges for c in M.CASES if c.kernel == kernel))
        assert listed >= {"exact_slab", "slab_plus_one", "over_slab", "multi_row", "base_on_head"}, kernel
    assert {c.kernel for c in M.cases("base")} == set(M.STORE_UNIT)
    assert {(c.in_offset, c.out_offset) for c in M.cases("unaligned")} == set(M.OFFSETS)


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_edge_census(walks, case):
    """the kernel the driver picks is the one the case names, and every edge the case is listed for occurs in its input"""
    x, B, base, order = walks[case.input]
    found, ctx, rt = M.census(case, B, base, order)
    assert rt.kernel == case.kernel, rt
    if case.kernel != "walk_store":
        assert ctx.ch.nchains >= 64 * M.num_cu()
    assert case.edges and all(found.values()), (case.id, found)
    # the first cut closes (no chain reaches the walk's step bound): the launch count the GPU test asserts is that of one attempt
    assert ctx.ch.len.max() <= min(4096 << ctx.sbits, x.size)
