"""GPU: the streaming first stage (bucket_sort.hiph: k_local_sort<1|3|9>, k_resolve_ties, k_unpack_big) at its size edges.

Every row of the table in tests/bucket_model.py -- inputs built so that a bucket, a bin, a tie group or a compared depth sits
exactly ON a limit of the kernels and one step past it; tests/test_bucket_model.py proves on the CPU that each does -- runs
under each of its routes.  The order is the oracle's bit for bit, and the counters the stage reports EQUAL the model's census
of the whole text: a variant that is wrong at one limit shows as a wrong order, or as a group listed, compared or left that
should not have been.  Which instance of k_local_sort ran is not reported; it is observable as a wrong order (<1> on a bucket
of 513 rows drops a row).  No tolerances: every assertion is an equality.
"""
import numpy as np
import pytest

import bucket_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.streaming_machinery]


@pytest.fixture(scope="module")
def expected(oracle):
    """row -> (text, the oracle's SA, BWT and primary index, the model's census), computed once and left unchanged"""
    out = {}

    def get(case):
        if case.id not in out:
            x = M.gen_input(case)
            P, B, b0 = oracle.forward(x)
            for a in (P, B):
                a.setflags(write=False)
            out[case.id] = (x, P, B, b0, M.census(x, case.q, case.hot))
        return out[case.id]
    return get


def _check_stats(st, case, c):
    assert st["path"] == 1, st["path"]
    if case.hot:
        assert st["period"] == len(M.HOT_MOTIF)          # the period probe named it: the hot form of the passes ran
    assert st["alphabet_bits"] == (8 // case.q if case.q > 1 else 0)
    assert st["tie_groups"] == c.tie_groups, (st["tie_groups"], c.tie_groups)
    assert st["tie_items"] == c.tie_items, (st["tie_items"], c.tie_items)
    settled = st["text_rounds"] + st["doubling_rounds"] == 0 and st["unresolved_initial"] == 0
    assert settled == (c.rows_left == 0), (st["text_rounds"], st["doubling_rounds"], st["unresolved_initial"], c.rows_left)
    # what the general stage's entry sweep finds tied, head rows included (k_first_groups).  The periodic row's working set is
    # not listed (the run shortcut is about to empty it)
    if c.rows_left and not case.hot:
        assert st["unresolved_initial"] == c.rows_left == c.rows_left_max, (st["unresolved_initial"], c.rows_left)


_ROWS = [(c, r) for c in M.CASES for r in c.routes]


@pytest.mark.parametrize("case,route", _ROWS, ids=["%s-%s" % (c.id, r) for c, r in _ROWS])
def test_bucket_sort_edges(archon, expected, monkeypatch, case, route):
    x, P, B, b0, c = expected(case)
    for k, v in case.routes[route].items():
        monkeypatch.setenv(k, v)
    sa, bwt, base = archon.forward(x)
    st = archon.stats()
    assert (sa == P).all(), int(np.argmax(sa != P))
    assert (bwt == B).all() and base == b0
    _check_stats(st, case, c)


def test_bucket_sort_edges_at_odd_addresses(archon, expected, monkeypatch):
    """the capacity row once more with device buffers at odd addresses (text + 3 bytes, SA + 1 word, BWT + 1 byte): every bucket
    leaves through the one-row stores of the sort's last step, whatever its start mod 4; nothing is written around the buffers"""
    import torch
    case = M.case("sizes_cap")
    x, P, B, b0, c = expected(case)
    n = x.size
    monkeypatch.setenv("ARCHON_FORCE_PATH", "1")
    xb = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    xb[3:3 + n] = torch.from_numpy(np.array(x)).cuda()
    sab = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    bwb = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    base_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    archon.forward_dev(xb[3:3 + n], sab[1:1 + n], bwb[1:1 + n], base_t)
    st = archon.stats()
    assert (sab[1:1 + n].cpu().numpy().view(np.uint32) == P).all()
    assert (bwb[1:1 + n].cpu().numpy() == B).all() and int(base_t.item()) == b0
    assert int(sab[0].item()) == 0 and int(sab[1 + n].item()) == 0 and int(bwb[0].item()) == 0 and int(bwb[1 + n].item()) == 0
    _check_stats(st, case, c)
