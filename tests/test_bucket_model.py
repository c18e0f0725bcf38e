"""CPU: the model of the streaming first stage (tests/bucket_model.py) against the definition of the order, and the edge census
of the table of rows that tests/test_gpu_bucket_sort.py runs on the GPU.

The census keeps the GPU rows from passing vacuously: a row listed for "a bin of 63 rows" or "a pair that first differs at key
byte 70" is worth its GPU time only while its input holds one.  A builder that cannot meet an edge is changed; the list is not.
"""
import itertools

import numpy as np
import pytest

import bucket_model as M


# ---------------------------------------------------------------- the model against the definition
def _common_prefix(x, a, b, cap):
    """symbols the items a[i], b[i] share before they part: equal text bytes while neither has run out, at most cap"""
    L = np.zeros(a.size, np.int64)
    alive = np.ones(a.size, bool)
    for d in range(1, cap + 1):
        alive &= (a >= d) & (b >= d)
        alive[alive] = x[a[alive] - d] == x[b[alive] - d]
        if not alive.any():
            break
        L += alive
    return L


def _check_against_sa(x, P, q):
    """the three properties that pin the model to the order the oracle computes"""
    c = M.census(x, q)
    n = x.size
    P = P.astype(np.int64)
    # 1. along the suffix array bucket << 24 | key never decreases: sorting on it and refining the ties IS the order
    code = M.codes(x, q)[P - 1]
    assert (np.diff(code) >= 0).all()
    assert (np.bincount(code >> 24, minlength=65536) == c.sizes).all() and c.max_bucket == c.sizes.max()
    # 2. a group -- rows equal on five key bytes -- is a contiguous run of rows of the suffix array
    pos = np.empty(n + 1, np.int64)
    pos[P] = np.arange(n)
    for g in range(c.g_start.size):
        at = pos[M.group_items(c, g)]
        assert at.max() - at.min() + 1 == c.g_len[g] == at.size
        assert at.min() == c.g_start[g]                     # ... and the model's rows[] is the first stage's order
    # 3. the depth at which a compared group's rows part is their true common key prefix + 1 (0: beyond the compared window)
    first, last = M.KEY_BYTES * q + 1, (M.KEY_BYTES + M.RESOLVE_BYTES) * q
    checked = 0
    for g in np.flatnonzero(c.g_listed & (c.g_len <= M.TIE_GROUP_MAX)):
        s = M.group_items(c, g)
        s = s[np.argsort(pos[s])]
        part = _common_prefix(x, s[:-1], s[1:], last + 1) + 1
        want = max(int(part.max()), first)                  # (packed keys: the pad code can tie what the text's end already parts)
        assert c.g_depth[g] == (want if want <= last else 0), (g, s, part)
        assert c.g_left[g] == (want > last)
        # an item that has run out where the rows part, against one that has not / against another that has
        one = ((s[:-1] < np.maximum(part, first)) ^ (s[1:] < np.maximum(part, first))) & (part <= last)
        both = (s[:-1] < first) & (s[1:] < first)
        assert c.g_one_exhausted[g] == one.any() and c.g_both_exhausted[g] == both.any(), (g, s, part)
        checked += 1
    # the counters are sums over what was just checked
    assert c.tie_groups == int(c.g_listed.sum())
    assert c.tie_items == int((c.sizes[c.sizes > M.LS_CAP] - 1).sum() + (c.bin_size[c.bin_size > M.LS_MAX_BIN] - 1).sum()
                              + (c.g_len[c.g_listed] - 1).sum())
    return checked


def test_model_exhaustive_tiny(oracle):
    """every string of length 1..6 over {0, 1, 255}"""
    cases = 0
    for n in range(1, 7):
        for t in itertools.product((0, 1, 255), repeat=n):
            x = np.array(t, np.uint8)
            _check_against_sa(x, oracle.sa(x, brute=True), 1)
            cases += 1
    assert cases == sum(3 ** n for n in range(1, 7))


@pytest.mark.parametrize("alphabet,q", [((0, 255), 1), ((254, 255), 1), ((3, 9), 8), ((65, 67, 71, 84), 1), ((65, 67, 71, 84), 4),
                                        ((1, 2, 250, 255), 4), (tuple(range(100, 116)), 2), (tuple(range(40, 52)), 1), (tuple(range(256)), 1)])
def test_model_on_random_strings(oracle, alphabet, q):
    """40 random strings of up to 2000 bytes per alphabet, small ones (long ties, exhausted items, packed keys) and the full one"""
    rng = np.random.default_rng(len(alphabet) * 10 + q)
    alpha = np.array(alphabet, np.uint8)
    checked = 0
    for k in range(40):
        n = int(rng.integers(1, 2001)) if k else 2000
        x = alpha[rng.integers(0, alpha.size, size=n)]
        if k % 3 == 0 and n > 300:                          # a repeated passage: pairs that part far behind the fifth key byte
            x[n - 130:] = x[20:150]
        if np.unique(x).size < alpha.size and q > 1:
            continue                                         # (the recode ranks the bytes that occur)
        checked += _check_against_sa(x, oracle.sa(x), q)
    assert checked > 0 or len(alphabet) == 256


def test_census_by_hand():
    """eight equal bytes: item s has s sevens and then the padding.  Items 5..8 agree on five key bytes; item 5 has run out at key
    byte 6, item 6 at 7, item 7 at 8, where it parts from item 8"""
    x = np.full(8, 7, np.uint8)
    c = M.census(x)
    assert c.sizes[(7 << 8) | 0xFF] == 1 and c.sizes[(7 << 8) | 7] == 7 and c.sizes.sum() == 8 and c.max_bucket == 7
    assert list(c.g_len) == [4] and list(M.group_items(c, 0)) == [5, 6, 7, 8] and c.g_listed.all()
    assert list(c.g_depth) == [8] and c.g_one_exhausted[0] and not c.g_both_exhausted[0] and not c.g_left[0]
    assert (c.tie_groups, c.tie_items, c.rows_left, c.min_depth) == (1, 3, 0, 5)
    # bucket (7, 7) holds items 2..8: keys FFFFFF, 07FFFF, 0707FF and four times 070707 -- the last two share bin 7 << 5
    assert sorted(c.bin_size) == [1, 1, 5] and c.item_n == "resolved_group"
    # 0xFF only: every item is padding all the way.  One bucket, one group, five of its items run out together
    c = M.census(np.full(40, 0xFF, np.uint8))
    assert c.max_bucket == 40 and list(c.g_len) == [40] and c.g_left.all() and (c.tie_groups, c.tie_items, c.rows_left) == (1, 39, 40)
    c = M.census(np.full(9, 0xFF, np.uint8))
    assert list(c.g_len) == [9] and c.g_both_exhausted[0] and c.g_one_exhausted[0] and list(c.g_depth) == [9] and c.rows_left == 0


def test_instance_rule_by_hand():
    """Fwd::streaming queues the one-round instance up to 400 rows per bucket on average, the three-round one up to 1350; the
    count's largest bucket decides between it and the general one"""
    assert [M.instance_of(300000, m) for m in (1, 512, 513, 4609)] == [1, 1, 9, 9]
    assert M.instance_of(400 << 16, 512) == 1 and M.instance_of(401 << 16, 512) == 3
    assert [M.instance_of(70 << 20, m) for m in (1536, 1537)] == [3, 9]
    assert M.instance_of(1350 << 16, 1536) == 3 and M.instance_of(1351 << 16, 1536) == 9
    assert M.instance_of(300000, 100, hot=True) == 9


def test_key_text_by_hand():
    """k_build_y at four symbols a byte: codes by rank, the newest symbol in the top bits, all-ones in front of the text"""
    x = np.frombuffer(b"ACGTTA", np.uint8)
    assert list(M.build_y(x, 4)) == [0b00111111, 0b01001111, 0b10010011, 0b11100100, 0b11111001, 0b00111110]
    assert list(M.build_y(np.array([5, 9, 9, 5], np.uint8), 8)) == [0b01111111, 0b10111111, 0b11011111, 0b01101111]
    # item 6 of ACGTTA: key bytes y[5], y[1], then the padding
    assert M.codes(x, 4)[5] == (0b00111110 << 32) | (0b01001111 << 24) | 0xFFFFFF


# ---------------------------------------------------------------- the table and its census
@pytest.fixture(scope="module")
def censuses():
    out = {}

    def get(case):
        if case.id not in out:
            out[case.id] = M.census(M.gen_input(case), case.q, case.hot)
        return out[case.id]
    return get


def test_table_covers_the_issue():
    ids = [c.id for c in M.CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == {"sizes_short", "sizes_short_plus1", "sizes_cap", "pairs_full", "small_bins", "long_bins", "bins_settled",
                        "resolve_depths_one_row_bucket", "resolve_depths_resolved_group", "resolve_depths_oversized_bucket",
                        "resolve_depths_long_bin", "list_overflow", "hot_unpack", "dna_depths"}
    forced = {"ARCHON_FORCE_PATH": "1"}
    want = [forced, dict(forced, ARCHON_NO_ALIGNED="1"), dict(forced, ARCHON_ALIGNED_MIN="65536", ARCHON_REL_MIN_SEG="1"),
            dict(forced, ARCHON_ALIGNED_MIN="65536", ARCHON_NO_REL_RECORDS="1")]
    for c in M.CASES:
        n = M.gen_input(c).size
        assert n <= 400000 or c.id == "list_overflow", (c.id, n)
        routes = list(c.routes.values())
        if c.id == "hot_unpack":                    # the hot form needs the period probe: no FORCE_PATH
            assert routes == [{k: v for k, v in r.items() if k != "ARCHON_FORCE_PATH"} for r in want[1:]] and c.hot
        elif c.q > 1:                               # the driver recodes a four-symbol block by itself; FORCE_PATH would keep byte keys
            assert all("ARCHON_FORCE_PATH" not in r for r in routes) and {} in routes
        else:
            assert routes == want, c.id
    assert 2_300_000 <= M.gen_input(M.case("list_overflow")).size <= 2_500_000
    assert len(M.set_partitions(2)) == 2 and len(M.set_partitions(3)) == 5 and len(M.set_partitions(4)) == 15
    assert M.LS_CAP == 9 * M.LS_BLOCK and M.LIST_CAP == 1 << 20


def test_constants_follow_the_kernels():
    """the limits the model restates, read out of the sources: a change to one of them has to come with its rows"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dark-archon_amd", "csrc")
    bs = open(os.path.join(csrc, "bucket_sort.hiph")).read()
    drv = open(os.path.join(csrc, "forward_driver.hiph")).read()
    num = lambda src, name: int(re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9]+)", src).group(1))
    assert num(bs, "kLsBlock") == M.LS_BLOCK and num(bs, "kLsIPT") * M.LS_BLOCK == M.LS_CAP
    assert num(bs, "kLsMaxBin") == M.LS_MAX_BIN and num(bs, "kTieGroupMax") == M.TIE_GROUP_MAX
    assert num(bs, "kBigRows") == M.BIG_ROWS and num(bs, "kUnpackChunk") == M.UNPACK_CHUNK and num(bs, "kLsBinBits") == 13
    assert "kTieListCap = 1u << 20" in drv and "kTieSample = 1u << 16" in bs
    assert "5u * (uint32_t)q, 64u * (uint32_t)q" in drv          # k_resolve_ties: from key byte 5 (0-based), 64 further ones
    assert "avg_rows <= 400u ? 1u : avg_rows <= 1350u ? 3u : 0u" in drv


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_edge_census(censuses, case):
    """every edge the row is listed for occurs in its input; a row that FORCE_PATH=1 carries would take the streaming stage
    without it as well (at most half its items in buckets beyond the sort's capacity)"""
    x = M.gen_input(case)
    c = censuses(case)
    found = {e: bool(M.EDGES[e](c, x)) for e in case.edges}
    assert all(found.values()), (case.id, found)
    if any("ARCHON_FORCE_PATH" in r for r in case.routes.values()):
        assert c.big_items * 2 <= c.n
    if case.hot:
        assert c.big_items * 2 > c.n and np.unique(x).size > 4        # the first count sends it on; its alphabet is not recoded
    if case.q > 1:
        assert np.unique(x).size == 4 and c.big_items * 2 <= c.n


def test_counters_of_the_rows_that_settle(censuses):
    """rows written for "no rounds at all" leave nothing, the others leave what their edges say"""
    for id, left in (("sizes_short", False), ("sizes_short_plus1", False), ("pairs_full", False), ("small_bins", False), ("bins_settled", False),
                     ("sizes_cap", True), ("long_bins", True), ("list_overflow", True), ("hot_unpack", True)):
        c = censuses(M.case(id))
        assert (c.rows_left > 0) == left, (id, c.rows_left)
    c = censuses(M.case("pairs_full"))
    assert c.tie_groups >= M.LS_CAP // 2 and c.tie_items >= M.LS_CAP // 2
    c = censuses(M.case("hot_unpack"))
    assert c.tie_groups == 0 and c.tie_items == int((c.sizes[c.sizes > M.LS_CAP] - 1).sum())
