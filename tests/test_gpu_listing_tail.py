"""GPU: how the five calls that list records END (analysis.hiph: ana_list_tail) -- repeats, lz_parse, kmers, maws and runs, each
through host buffers, device buffers and the resident block.  One random four-letter block of 6145 bytes: three tiles of the
largest default tile (2048 rows) and one row, so that the scan of the tile words has more than one word to sum in every family.
SA and BWT are the oracle's, the LCP array Kasai's, the expected records the naive models'.

Per call: counting alone launches no emit pass and leaves ms_emit 0; room for exactly the records gives the model's records, a
sentinel record behind them untouched, two launches more (the scan, the emit pass) and ONE wait more, whatever the form; room for
one record fewer is refused with ARCHON_E_ARG, the count still written, the buffer untouched, the text below, and the launches
and waits of counting alone.  The refusal texts are the ones the library printed before the five endings became one."""
import ctypes

import numpy as np
import pytest

import kmers_naive
import lcp_kasai
import lz_naive
import maw_naive
import repeats_naive
import runs_naive

pytestmark = pytest.mark.gpu

N = 3 * 2048 + 1
K = 8                                   # 4^8 possible 8-mers over 6145 rows: nearly every row its own group, so groups in every tile
SENTINEL = 0xA5A5A5A5
FORMS = ("host", "dev", "block")
# the call's name and its record noun, as the refusal words them: "<call>: <total> <noun>, room for <cap>"
TEXT = {"repeats": "repeats: %d repeats, room for %d", "lz_parse": "lz_parse: %d phrases, room for %d", "kmers": "kmers: %d k-mers, room for %d",
        "maws": "maws: %d words, room for %d", "runs": "runs: %d runs, room for %d"}
# waits of the block form's count that are not the LCP step's: the counters' (and, for lz, the LPF pass's before them), as
# test_gpu_block_calls.py and test_gpu_kmers.py pin them; maws and runs build more (a rank table, a second sort) and are only
# held to "one more with the records"
BLOCK_OWN_WAITS = {"repeats": 1, "lz_parse": 2, "kmers": 1}


def _arrays(oracle, kasai, x):
    sa, bwt, base = oracle.forward(x)
    return np.ascontiguousarray(sa, np.uint32), np.ascontiguousarray(bwt, np.uint8), int(base), kasai(x, sa)


def _runs_model(x, sa, lcp, sa_c):
    rank = []
    for a in (sa, sa_c):
        r = np.zeros(x.size + 1, np.int64)
        r[a] = np.arange(x.size)
        rank.append(r.tolist())
    recs, _ = runs_naive.runs_rule(x.tobytes(), lce=runs_naive.SparseLce(sa, lcp).scalar(), rank=rank)
    return np.array(recs, np.uint32).reshape(-1, 4).copy().view(runs_naive.RUN).ravel()


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    """the block and the 256 distinct bytes with their arrays and the models' records: made once, shared, left unchanged"""
    kasai = lcp_kasai.build(tmp_path_factory.mktemp("tail_kasai"))
    rep = repeats_naive.build(tmp_path_factory.mktemp("tail_repeats"))
    lz = lz_naive.build(tmp_path_factory.mktemp("tail_lz"))
    out = {}
    for name, x in (("block", np.random.default_rng(6145).integers(0, 4, N).astype(np.uint8) + 97), ("distinct", np.arange(256, dtype=np.uint8))):
        sa, bwt, base, lcp = _arrays(oracle, kasai, x)
        sa_c = np.ascontiguousarray(oracle.forward(255 - x)[0], np.uint32)
        lpf = lz.lpf(sa, lcp, 0)
        d = {"x": x, "sa": sa, "bwt": bwt, "base": base, "lcp": lcp, "sa_c": sa_c, "lpf": lpf,
             "want": {"repeats": rep(lcp, bwt, base, 1)[0], "lz_parse": lz.parse(lpf), "kmers": kmers_naive.kmers_arrays(sa, lcp, K)[0],
                      "maws": maw_naive.model(sa, lcp, bwt, base)[0], "runs": _runs_model(x, sa, lcp, sa_c)}}
        for a in list(d.values())[:7] + list(d["want"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = d
    return out


class _Call:
    """one listing call of one form over the arrays of d: run(out pointer or None, cap) -> (rc, total); its statistics record"""

    def __init__(self, archon, family, form, d, blk):
        import torch
        L, p = archon.lib(), archon._p
        n = d["x"].size
        self.archon, self.family, self.form = archon, family, form
        self.stats = {"repeats": archon.repeat_stats, "lz_parse": archon.lz_stats, "kmers": archon.kmer_stats, "maws": archon.maw_stats,
                      "runs": archon.run_stats}[family]
        self.dtype = {"repeats": archon.REPEAT, "lz_parse": archon.PHRASE, "kmers": archon.KMER, "maws": archon.MAW, "runs": archon.RUN}[family]
        if form == "dev":
            self.keep = {k: torch.from_numpy(np.ascontiguousarray(d[k]).view(np.uint8).copy()).to("cuda:0") for k in ("sa", "lcp", "bwt", "sa_c", "lpf")}
            a = {k: ctypes.c_void_p(t.data_ptr()) for k, t in self.keep.items()}
            end = (0, archon._stream_ptr())
        else:
            a = {k: p(d[k]) for k in ("sa", "lcp", "bwt", "sa_c", "lpf")}
            end = (0,)
        base = d["base"]
        if form == "block":
            self.fn = {"repeats": lambda o, c, t: L.archon_hip_block_repeats(blk.h, 1, 1, 2, o, c, t),
                       "lz_parse": lambda o, c, t: L.archon_hip_block_lz(blk.h, 0, None, o, c, t),
                       "kmers": lambda o, c, t: L.archon_hip_block_kmers(blk.h, K, 1, 0, o, c, t, None, 0),
                       "maws": lambda o, c, t: L.archon_hip_block_maws(blk.h, 2, 0, o, c, t),
                       "runs": lambda o, c, t: L.archon_hip_block_runs(blk.h, 0, 0, 2, 0, o, c, t)}[family]
        else:
            sfx = "_dev" if form == "dev" else ""
            self.fn = {"repeats": lambda o, c, t: getattr(L, "archon_hip_repeats" + sfx)(a["lcp"], a["bwt"], n, base, 1, 1, 2, o, c, t, *end),
                       "lz_parse": lambda o, c, t: getattr(L, "archon_hip_lz_parse" + sfx)(a["lpf"], n, o, c, t, *end),
                       "kmers": lambda o, c, t: getattr(L, "archon_hip_kmers" + sfx)(a["sa"], a["lcp"], n, K, 1, 0, o, c, t, None, 0, *end),
                       "maws": lambda o, c, t: getattr(L, "archon_hip_maws" + sfx)(a["sa"], a["lcp"], a["bwt"], n, base, 2, 0, o, c, t, *end),
                       "runs": lambda o, c, t: getattr(L, "archon_hip_runs" + sfx)(a["sa"], a["lcp"], a["sa_c"], n, 0, 0, 2, 0, o, c, t, *end)}[family]

    def buffer(self, records):
        """room for `records` records and one more, every word the sentinel: (pointer, read() -> the words as they are now)"""
        import torch
        words = (records + 1) * self.dtype.itemsize // 4
        if self.form == "dev":
            t = torch.full((words,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
            return ctypes.c_void_p(t.data_ptr()), lambda: t.cpu().numpy().view(np.uint32)
        h = np.full(words, SENTINEL, np.uint32)
        return self.archon._p(h), lambda: h

    def run(self, out, cap):
        total = ctypes.c_uint64(77)
        rc = self.fn(out, cap, ctypes.cast(ctypes.byref(total), ctypes.c_void_p))
        st = self.stats()
        print("    %s %s cap %d: rc %d total %d launches %d waits %d ms_emit %.3f" % (self.family, self.form, cap, rc, total.value, st.kernel_launches,
                                                                                       st.host_syncs, st.ms_emit))
        return rc, total.value, st


@pytest.fixture(scope="module")
def resident(archon, data):
    blk = archon.Block()
    assert (blk.forward(data["block"]["x"], want_sa=True)[0] == data["block"]["sa"]).all()
    yield blk
    blk.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", list(TEXT))
def test_count_emit_refuse(archon, data, resident, family, form):
    d = data["block"]
    want = d["want"][family]
    k = want.size
    assert k >= 256, "the model lists too few records for every tile to hold some"
    call = _Call(archon, family, form, d, resident)
    # 1  counting alone (the second such call is the one to compare with: the first builds what a block keeps for later calls, the
    #    rank table of block_maws)
    call.run(None, 0)
    rc, total, st0 = call.run(None, 0)
    assert (rc, total) == (archon.OK, k) and st0.ms_emit == 0
    # 2  room for exactly the records
    ptr, read = call.buffer(k)
    rc, total, st = call.run(ptr, k)
    got = read()
    per = call.dtype.itemsize // 4
    assert (rc, total) == (archon.OK, k)
    assert got[:k * per].view(call.dtype).tolist() == want.tolist()
    assert (got[k * per:] == SENTINEL).all()
    # 4  the emit pass: the scan and the pass, one wait more -- host buffer, device buffer or block
    assert st.kernel_launches == st0.kernel_launches + 2 and st.ms_emit > 0
    assert st.host_syncs == st0.host_syncs + 1
    if form == "block":
        lcp = archon.lcp_stats()
        assert lcp.n == N and st0.host_syncs > lcp.host_syncs
        if family in BLOCK_OWN_WAITS:
            assert st.host_syncs == BLOCK_OWN_WAITS[family] + 1 + lcp.host_syncs
    # 3  room for one record fewer
    ptr, read = call.buffer(k - 1)
    rc, total, st = call.run(ptr, k - 1)
    assert rc == archon.E_ARG and total == k
    assert (read() == SENTINEL).all()
    assert archon.lib().archon_hip_last_error().decode() == TEXT[family] % (k, k - 1)
    assert (st.kernel_launches, st.host_syncs, st.ms_emit) == (st0.kernel_launches, st0.host_syncs, 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", ["repeats", "runs"])
def test_nothing_to_list(archon, data, family, form):
    """256 distinct bytes hold no repeat and no run: a call with a buffer returns 0 records, launches no emit pass, waits as the
    count does and leaves the buffer alone"""
    d = data["distinct"]
    assert d["want"][family].size == 0
    blk = archon.Block()
    try:
        if form == "block":
            blk.forward(d["x"], want_sa=True)
        call = _Call(archon, family, form, d, blk)
        rc, total, st0 = call.run(None, 0)
        assert (rc, total) == (archon.OK, 0)
        ptr, read = call.buffer(4)
        rc, total, st = call.run(ptr, 4)
        assert (rc, total) == (archon.OK, 0) and (read() == SENTINEL).all()
        assert (st.kernel_launches, st.host_syncs, st.ms_emit) == (st0.kernel_launches, st0.host_syncs, 0)
    finally:
        blk.close()
