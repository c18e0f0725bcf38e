"""GPU: the checks of data the library did not make -- validate / validate_dev / validate_resident_dev (and through them
Block.validate and archon_validate), the E_CORRUPT side of sa_to_bwt, and inverse on corrupted BWTs -- handed WRONG answers.

The expected answer is always plain.  The device validate is 1 if and only if sa is the a7 suffix array of x
(include/archon_hip.h; test_oracle.py::test_device_validate_rule_is_exact), and the resident one also needs the BWT and
the primary index of x: so small cases compare with oracle.sa, and a constructed corruption of a known-correct SA must be
refused.  (oracle.validate is a7's own check, which accepts some wrong permutations: test_oracle.py says which.)  Clean
outputs of blocks too large for the oracle come from the GPU forward, whose outputs test_gpu_golden.py pins.
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

import archon_synth as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _gather(x, P):
    """what sa_to_bwt must return for an in-range P with one n: bwt[i] = x[P[i]] (x[0] on the row of n), that row"""
    P = np.asarray(P, np.int64)
    return x[np.where(P == x.size, 0, P)], int(np.flatnonzero(P == x.size)[0])


def _odd(t):
    """the same bytes at an odd device address"""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t
    return buf[1:]


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _forward_dev(archon, x):
    """clean (x_t, sa_t, bwt_t, base, stats) from the GPU forward"""
    import torch
    n = x.size
    x_t = _cuda(x)
    sa_t = torch.empty(n, dtype=torch.int32, device="cuda")
    bwt_t = torch.empty(n, dtype=torch.uint8, device="cuda")
    base_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    archon.forward_dev(x_t, sa_t, bwt_t, base_t)
    return x_t, sa_t, bwt_t, int(base_t.item()), archon.stats()


# ---------------------------------------------------------------- 1a: exhaustive tiny cases
def test_exhaustive_tiny(archon, oracle):
    """every string of length 1..5 over {0, 1, 255} and every permutation of 1..n (31 287 cases): validate and validate_dev
    return 1 exactly for the suffix array; so does the resident check fed (P, its gather, the row of n).  The cases of
    one length sit in one device buffer each, the calls take slices of it."""
    total = accepted = 0
    for n in range(1, 6):
        xs = np.array(list(itertools.product((0, 1, 255), repeat=n)), np.uint8)
        perms = np.array(list(itertools.permutations(range(1, n + 1))), np.uint32)
        sas = np.stack([oracle.sa(x) for x in xs])
        Pi = perms.astype(np.int64)
        bwts = xs[:, np.where(Pi == n, 0, Pi)]                 # [string][perm][row]
        bases = np.argmax(Pi == n, axis=1)
        x_d, p_d, b_d = _cuda(xs), _cuda(perms), _cuda(bwts.reshape(-1, n))
        m = len(perms)
        for si in range(len(xs)):
            for pi in range(m):
                want = bool((perms[pi] == sas[si]).all())
                got = (archon.validate(xs[si], perms[pi]), archon.validate_dev(x_d[si], p_d[pi]),
                       archon.validate_resident_dev(x_d[si], p_d[pi], b_d[si * m + pi], int(bases[pi])))
                assert got == (want,) * 3, (xs[si].tolist(), perms[pi].tolist(), got)
                total += 1
                accepted += want
    assert total == 31287 and accepted == 3 + 9 + 27 + 81 + 243


# ---------------------------------------------------------------- 1b: foreign outputs
def test_foreign_outputs_small(archon, oracle):
    """every ordered pair x != y of binary strings of equal length 2..8 with equal byte counts (17 066 pairs): the SA, BWT and
    primary index of y are refused for x by the resident check, y's SA by validate_dev; each y's own outputs pass."""
    pairs = 0
    for L in range(2, 9):
        xs = np.array(list(itertools.product((0, 1), repeat=L)), np.uint8)
        fw = [oracle.forward(x) for x in xs]
        x_d = _cuda(xs)
        sa_d = _cuda(np.stack([f[0] for f in fw]))
        bw_d = _cuda(np.stack([f[1] for f in fw]))
        ones = xs.sum(axis=1)
        for yi, (_, _, by) in enumerate(fw):
            assert archon.validate_resident_dev(x_d[yi], sa_d[yi], bw_d[yi], by) and archon.validate_dev(x_d[yi], sa_d[yi])
            for xi in np.flatnonzero(ones == ones[yi]):
                if xi == yi:
                    continue
                assert not archon.validate_resident_dev(x_d[xi], sa_d[yi], bw_d[yi], by), (xs[xi].tolist(), xs[yi].tolist())
                assert not archon.validate_dev(x_d[xi], sa_d[yi]), (xs[xi].tolist(), xs[yi].tolist())
                pairs += 1
    assert pairs == 17066


def _swap_two(x, i):
    """x with the byte at i swapped with the first unequal byte after 2/3 of the block"""
    y = x.copy()
    j = len(x) * 2 // 3 + int(np.flatnonzero(x[len(x) * 2 // 3:] != x[i])[0])
    y[[i, j]] = y[[j, i]]
    return y


@pytest.mark.parametrize("name", ["ab_vs_ba", "motif_phase", "text_4MiB_swap", "random_64MiB_swap"])
def test_foreign_outputs_at_scale(archon, name):
    """the outputs of y for a block x with the same byte counts: ab x k against ba x k (closed form), a 1000-byte motif block
    against the motif rotated by one byte, a 4 MiB text and a 64 MiB random block against themselves with two unequal bytes
    swapped.  The resident check and validate_dev refuse them for x (also at an odd text address) and accept them for y."""
    if name == "ab_vs_ba":
        x, y = S.gen_repeat(1 << 20, b"ab"), S.gen_repeat(1 << 20, b"ba")
    elif name == "motif_phase":
        motif = S.gen_random(1000, S.SEED_BASE + 3)
        x, y = S.gen_repeat(2000 * 1000, motif.tobytes()), S.gen_repeat(2000 * 1000, np.roll(motif, -1).tobytes())
    elif name == "text_4MiB_swap":
        x = S.gen_text(4 << 20)
        y = _swap_two(x, len(x) // 3)
    else:
        x = S.gen_random(64 << 20)
        y = _swap_two(x, 12345)
    assert not (x == y).all() and (np.bincount(x, minlength=256) == np.bincount(y, minlength=256)).all()
    y_t, sa_t, bwt_t, base, st = _forward_dev(archon, y)
    if name == "ab_vs_ba":
        assert st["path"] == 2
    assert archon.validate_resident_dev(y_t, sa_t, bwt_t, base) and archon.validate_dev(y_t, sa_t)
    x_t = _cuda(x)
    for xv in (x_t, _odd(x_t)):
        assert not archon.validate_resident_dev(xv, sa_t, bwt_t, base)
        assert not archon.validate_dev(xv, sa_t)


# ---------------------------------------------------------------- 1c: corruption matrix at kernel edges
MATRIX_SIZES = [1, 2, 3, 255, 256, 257, 8191, 8192, 8193, (1 << 20) + 3, (32 << 20) + 5, 256 << 20]


def _sites(n, base):
    """row 0, row n-1, the primary row and its neighbours, the edges of the 256-row launch blocks and of the 8192-row tiles
    of k_lf_chunk, a chunk edge of lf_build_launch (chunks of ntiles / 2048 tiles)"""
    ntiles = -(-n // 8192)
    tpc = max(1, ntiles // 2048)
    nchunks = -(-ntiles // tpc)
    ce = tpc * 8192 * max(1, nchunks // 2)
    rows = {0, 1, n - 2, n - 1, base - 1, base, base + 1, 255, 256, 8191, 8192, ce - 1, ce}
    return sorted(r for r in rows if 0 <= r < n)


def _corruptions(P, n, base, r):
    """(name, rows, values): every one leaves P no suffix array"""
    v = lambda i: int(P[i])
    out = []
    if r + 1 < n:
        out.append(("swap", [r, r + 1], [v(r + 1), v(r)]))
        out.append(("dup", [r + 1], [v(r)]))                              # one value twice, one missing
    if r + 2 < n:
        out.append(("rot3", [r, r + 1, r + 2], [v(r + 1), v(r + 2), v(r)]))
    for bad in (0, n + 1, 0xFFFFFFFF):
        out.append(("value_%x" % bad, [r], [bad]))
    if r != base:
        out.append(("second_n", [r], [n]))
    else:
        for nb in (base - 1, base + 1):
            if 0 <= nb < n:
                out.append(("swap_n_row", [base, nb], [v(nb), v(base)]))
    return out


def _c_abi_validate(x, tmp_path):
    """archon_validate through include/archon.h on a clean block (read -> compute -> validate)"""
    L = ctypes.CDLL(os.path.join(ROOT, "dark-archon_amd", "libarchon.so"))
    L.archon_create.restype = ctypes.c_void_p
    L.archon_create.argtypes = [ctypes.c_uint32]
    for fn in ("archon_destroy", "archon_validate", "archon_en_compute"):
        getattr(L, fn).argtypes = [ctypes.c_void_p]
    L.archon_en_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    libc = ctypes.CDLL(None)
    libc.fopen.restype = ctypes.c_void_p
    libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    raw = tmp_path / "x.raw"
    x.tofile(raw)
    a = L.archon_create(x.size)
    try:
        fx = libc.fopen(str(raw).encode(), b"rb")
        assert L.archon_en_read(a, fx, x.size) == x.size
        libc.fclose(fx)
        assert L.archon_en_compute(a) == 0
        return L.archon_validate(a)
    finally:
        L.archon_destroy(a)
        os.remove(raw)


@pytest.mark.parametrize("n", MATRIX_SIZES)
def test_corruption_matrix(archon, oracle, n, tmp_path):
    """each corruption of the clean SA at each site, through validate, validate_dev and validate_resident_dev (the device ones
    also with the text at an odd address): 0; clean: 1.  The resident check also refuses the clean SA with two unequal BWT
    bytes swapped and with the primary index off by one either way.  Block.validate and archon_validate accept the clean
    block (they run the same resident kernels on what they computed themselves)."""
    import torch
    x = S.gen_random(n) if n == 256 << 20 else S.gen_text(n)
    if n <= (1 << 20) + 3:
        P, B, base = oracle.forward(x)
        x_t, sa_t, bwt_t = _cuda(x), _cuda(P), _cuda(B)
    else:
        x_t, sa_t, bwt_t, base, _ = _forward_dev(archon, x)
        P = sa_t.cpu().numpy().view(np.uint32)
    x_odd = _odd(x_t)

    def run(want, bwt=bwt_t, b=base):
        got = (archon.validate(x, P), archon.validate_dev(x_t, sa_t), archon.validate_dev(x_odd, sa_t),
               archon.validate_resident_dev(x_t, sa_t, bwt, b), archon.validate_resident_dev(x_odd, sa_t, bwt, b))
        return got == (want,) * 5, got

    ok, got = run(True)
    assert ok, got
    cases = 0
    for r in _sites(n, base):
        for name, rows, vals in _corruptions(P, n, base, r):
            old = P[rows].copy()
            rows_t = torch.tensor(rows, device="cuda")
            P[rows] = vals
            sa_t[rows_t] = _cuda(np.array(vals, np.uint32))
            try:
                ok, got = run(False)
            finally:
                P[rows] = old
                sa_t[rows_t] = _cuda(old)
            assert ok, (n, r, name, got)
            cases += 1
        # resident only: two unequal BWT bytes swapped (row r and the next row with another byte), the primary index off by one
        B_r = bwt_t[r:r + 4096].cpu().numpy()
        other = np.flatnonzero(B_r != B_r[0])
        if other.size:
            j = r + int(other[0])
            bad = bwt_t.clone()
            bad[[r, j]] = bwt_t[[j, r]]
            assert not archon.validate_resident_dev(x_t, sa_t, bad, base) and not archon.validate_resident_dev(x_odd, sa_t, bad, base), (n, r)
            del bad
            cases += 1
    for b in (base - 1, base + 1):
        if b >= 0:
            assert not archon.validate_resident_dev(x_t, sa_t, bwt_t, b) and not archon.validate_resident_dev(x_odd, sa_t, bwt_t, b), (n, b)
    assert cases > 0 or n == 1
    ok, got = run(True)                      # every corruption undone
    assert ok, got
    del x_odd, x_t, sa_t, bwt_t
    blk = archon.Block()
    try:
        sa, b0 = blk.forward(x)
        assert (sa == P).all() and b0 == base and blk.validate()
    finally:
        blk.close()
    assert _c_abi_validate(x, tmp_path) == 1


def test_deep_adjacent_swap(archon, oracle):
    """two adjacent rows whose keys agree for more than 1000 bytes (the duplicated block of test_gpu_forward's
    segmentation cases): swapped, they differ only deep -- and are refused all the same"""
    from test_gpu_forward import _seg_cases
    x = _seg_cases()["duplicated_block"]
    P, B, base = oracle.forward(x)
    x_t, sa_t, bwt_t = _cuda(x), _cuda(P), _cuda(B)
    s, t = P[:-1].astype(np.int64), P[1:].astype(np.int64)
    cand = np.flatnonzero((np.minimum(s, t) > 1500) & (s != x.size) & (t != x.size))
    cand = [int(i) for i in cand if (x[s[i] - 1500:s[i]] == x[t[i] - 1500:t[i]]).all()]
    assert len(cand) > 100
    for i in cand[:: max(1, len(cand) // 8)][:8]:
        Q = P.copy()
        Q[[i, i + 1]] = Q[[i + 1, i]]
        q_t = _cuda(Q)
        assert not archon.validate(x, Q) and not archon.validate_dev(x_t, q_t), i
        assert not archon.validate_resident_dev(x_t, q_t, bwt_t, base), i
    assert archon.validate(x, P) and archon.validate_resident_dev(x_t, sa_t, bwt_t, base)


# ---------------------------------------------------------------- 1d: sa_to_bwt is a gather, not a check
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 4096, 4097, 4098, 4099])
def test_sa_to_bwt_is_a_gather(archon, n):
    """k_sa_to_bwt takes four rows per thread: with n mod 4 = 0..3 the row of n and the bad row sit in the last (partial)
    quad.  In-range wrong permutations come back as the plain gather and the row of n; values outside 1..n, no n or two
    n are E_CORRUPT -- on the host entry and on the device one with aligned and with unaligned buffers."""
    import torch
    rng = np.random.default_rng(1000 + n)
    x = rng.integers(0, 4, n).astype(np.uint8)
    L = archon.lib()

    def dev(P, offset):
        x_t = _cuda(x) if not offset else _odd(_cuda(x))
        sa_t = _cuda(P) if not offset else _odd(_cuda(P))
        bwt_t = torch.zeros(n + offset, dtype=torch.uint8, device="cuda")[offset:]
        base_t = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc = L.archon_hip_sa_to_bwt_dev(_ptr(x_t), n, _ptr(sa_t), _ptr(bwt_t), _ptr(base_t), 0, archon._stream_ptr())
        torch.cuda.synchronize()
        return rc, bwt_t.cpu().numpy(), int(base_t.item())

    last = n - 1
    wrong = []
    for k in range(3):
        P = (rng.permutation(n) + 1).astype(np.uint32)
        j = int(np.flatnonzero(P == n)[0])
        P[[j, last]] = P[[last, j]]                   # n in the last row (the last quad)
        wrong.append(P)
    wrong.append(np.roll(np.arange(1, n + 1, dtype=np.uint32), 1))       # n in row 0
    for P in wrong:
        want_bwt, want_base = _gather(x, P)
        bwt, b = archon.sa_to_bwt(x, P)
        assert (bwt == want_bwt).all() and b == want_base
        for off in (0, 1):
            rc, bwt, b = dev(P, off)
            assert rc == 0 and (bwt == want_bwt).all() and b == want_base, off
    P = wrong[0]
    bad_rows = sorted({last, max(0, last - 1)})
    corrupt = []
    for r in bad_rows:
        for val in (0, n + 1, 0xFFFFFFFF):
            Q = P.copy()
            Q[r] = val
            corrupt.append(Q)
    if n > 1:
        Q = P.copy()
        Q[last] = Q[last - 1]                         # no n
        corrupt.append(Q)
        Q = P.copy()
        Q[last - 1] = n                               # two n
        corrupt.append(Q)
    for Q in corrupt:
        with pytest.raises(archon.ArchonError) as e:
            archon.sa_to_bwt(x, Q)
        assert e.value.code == archon.E_CORRUPT, Q[-4:]
        for off in (0, 1):
            assert dev(Q, off)[0] == archon.E_CORRUPT, (Q[-4:], off)


# ---------------------------------------------------------------- 1e: inverse on corrupted BWTs, against oracle.inverse
def _three_row_swaps(B, P, base, rng):
    """two closing and two breaking swaps of unequal bytes.  Rows i < k < j with bwt[i] == bwt[k] = a, bwt[j] = b != a and
    no other a or b between i and j: swapping i and j composes the LF cycle with the 3-cycle (i j k), which stays one cycle
    when, walking the text from P[i], P[j] comes before P[k] -- and falls into three otherwise."""
    n = B.size
    out = {True: [], False: []}
    for _ in range(20000):
        i = int(rng.integers(0, n - 2))
        nxt = np.flatnonzero(B[i + 1:i + 64] == B[i])
        if nxt.size == 0:
            continue
        k = i + 1 + int(nxt[0])
        j = k + 1
        if j >= n or B[j] == B[i] or (B[i + 1:k] == B[j]).any() or base in (i, j, k):
            continue
        closes = (int(P[j]) - int(P[i])) % n < (int(P[k]) - int(P[i])) % n
        if len(out[closes]) < 2:
            out[closes].append((i, j))
        if len(out[True]) == 2 and len(out[False]) == 2:
            break
    return [(c, ij) for c in (True, False) for ij in out[c]]


INVERSE_ROUTES = [("walk_store", 100003, {}), ("queue_walk", (1 << 20) + 5, {}), ("inv_slab_16", 300001, {"ARCHON_INV_SLAB": "16"}),
                  ("walk_rows", (128 << 20) + 4099, {}),
                  ("sbits6_rows128", (1 << 20) + 5, {"ARCHON_INV_SBITS": "6", "ARCHON_INV_ROWS": "1"}),
                  ("sbits5_rows64_full_slab", (1 << 20) + 5, {"ARCHON_INV_SBITS": "5", "ARCHON_INV_ROWS": "2", "ARCHON_INV_SLAB": "64"}),
                  ("one_chain_per_lane", (1 << 20) + 5, {"ARCHON_INV_WALK_WGS": "0"})]


@pytest.mark.parametrize("route,n,env", INVERSE_ROUTES, ids=[r[0] for r in INVERSE_ROUTES])
def test_inverse_on_corrupted_bwt(archon, oracle, route, n, env, monkeypatch):
    """(bwt, base) with two unequal bytes swapped, or base moved to another row: E_CORRUPT exactly when the oracle's walk does
    not close, else the oracle's output -- on each walk route (k_walk_store below ~131 072 rows, the queue walk, k_walk_rows
    above 128 MiB, tiny slabs).  Both outcomes occur on every route."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x = S.gen_text(n)
    if n <= (1 << 20) + 5:
        P, B, base = oracle.forward(x)
    else:
        _, sa_t, bwt_t, base, _ = _forward_dev(archon, x)
        P, B = sa_t.cpu().numpy().view(np.uint32), bwt_t.cpu().numpy()
        del sa_t, bwt_t
    assert (archon.inverse(B, base) == x).all()
    rng = np.random.default_rng(n)
    cases = [("swap", ij, base, closes) for closes, ij in _three_row_swaps(B, P, base, rng)]
    far = (base + 1 + int(rng.integers(0, n - 1))) % n                          # any other row
    cases += [("base", None, b, None) for b in (base + 1 if base + 1 < n else base - 1, far)]
    outcomes = set()
    for kind, ij, b, closes in cases:
        Bc = B.copy()
        if ij is not None:
            Bc[list(ij)] = Bc[list(ij[::-1])]
        rc, want = oracle.inverse(Bc, b)
        assert rc in (0, -3)
        if closes is not None:
            assert (rc == 0) == closes, (kind, ij)
        outcomes.add(rc)
        if rc == 0:
            got = archon.inverse(Bc, b)
            assert (got == want).all() and not (got == x).all(), (kind, ij, b)
        else:
            with pytest.raises(archon.ArchonError) as e:
                archon.inverse(Bc, b)
            assert e.value.code == archon.E_CORRUPT, (kind, ij, b)
    assert outcomes == {0, -3}
