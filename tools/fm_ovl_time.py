"""Device time of the ends of a block's documents and of the suffix-prefix overlap search.

Per block size and shape: the block and its forward (with its suffix array) on cuda:0 and a handle of its BWT.  The block is cut
into documents of --doc bytes; a query is a piece of the block that begins inside a document's last bytes and runs on into the
next one, so that real overlaps exist.  Medians of --reps runs after one warm-up of
  attach     the block form of attach_ends: the build's device time (HIP events) and the wall time of the call, beside the device
             time of the LCP step of the same block
  count      overlaps(emit=False): the count pass alone, beside fm_count on the same patterns -- the same rank steps with no end
             reads, the floor -- and the ratio of the two
  emit       overlaps(): the count pass with the scan of its counts, the emit pass, the wall time of the whole call
Two cases: 65 536 queries of 100 bytes with min_len 20, and of 250 bytes with min_len 50.  Every device figure comes from
archon_hip_fm_ovl_last_stats and archon_hip_get_fm_stats.

    python tools/fm_ovl_time.py [--mib 16] [--shapes dna,text] [--out profiles/fm/fm_ovl_time16.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))

CASES = ((100, 20), (250, 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="dna,text")
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--doc", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm", "fm_ovl_time16.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    out = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def wall(call):
        t = time.perf_counter()
        r = call()
        return r, (time.perf_counter() - t) * 1e3

    med = statistics.median
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_dna(n) if shape == "dna" else S.gen_shape(shape, n)
            rng = np.random.default_rng(mib * 1000 + len(shape))
            ends = np.arange(args.doc, n + 1, args.doc, dtype=np.uint32)
            blk = pyarchon.Block()
            blk.forward(x)
            blk.lcp()
            ms_lcp = pyarchon.lcp_stats().ms_total
            f = blk.fm_index(32)
            dev, wl = [], []
            for _ in range(args.reps + 1):
                wl.append(wall(lambda: pyarchon._check(L.archon_hip_block_fm_attach_ends(blk.h, f.h, ctypes.c_void_p(ends.ctypes.data), ends.size)))[1])
                a = pyarchon.fm_ovl_stats()
                dev.append(a.ms_attach)
            row = dict(mib=mib, shape=shape, what="attach", docs=int(ends.size), ms_attach=med(dev[1:]), wall_ms=med(wl[1:]), ms_lcp=ms_lcp,
                       end_mib=a.end_bytes / 2.0 ** 20, kernel_launches=a.kernel_launches, host_syncs=a.host_syncs)
            say("%5d MiB %-5s attach %.3f ms on the device (%d documents, %.2f MiB), %.3f ms wall; the LCP step %.3f ms" % (
                mib, shape, row["ms_attach"], ends.size, row["end_mib"], row["wall_ms"], ms_lcp))
            say(json.dumps(row))
            say("%5s %-5s %5s %7s %9s %9s %7s %11s %9s %9s %11s %11s %11s %11s" % ("MiB", "shape", "bytes", "min_len", "count ms", "fm_count", "ratio",
                                                                                  "count+scan", "emit ms", "wall ms", "steps", "tested", "hit", "overlaps"))
            for m, min_len in CASES:
                # a query starts 1 .. m - 1 bytes before a document's end: its first bytes are that document's last
                e = ends[rng.integers(0, ends.size - 2, args.queries)].astype(np.int64)
                q = e - rng.integers(1, m, args.queries)
                pats = [x[s:s + m] for s in q.tolist()]
                co, fl, ce, em, wl = [], [], [], [], []
                for _ in range(args.reps + 1):
                    f.overlaps(pats, min_len, emit=False)
                    co.append(pyarchon.fm_ovl_stats().ms_count)
                    f.count(pats)
                    fl.append(pyarchon.fm_stats().ms_query)
                    wl.append(wall(lambda: f.overlaps(pats, min_len))[1])
                    st = pyarchon.fm_ovl_stats()
                    ce.append(st.ms_count)
                    em.append(st.ms_emit)
                row = dict(mib=mib, shape=shape, what="overlaps", queries=args.queries, bytes=m, min_len=min_len, ms_count=med(co[1:]),
                           ms_fm_count=med(fl[1:]), ratio=med(co[1:]) / med(fl[1:]), ms_count_scan=med(ce[1:]), ms_emit=med(em[1:]), wall_ms=med(wl[1:]),
                           steps=st.steps, fm_count_steps=pyarchon.fm_stats().steps, tested=st.tested, hit=st.hit, overlaps=st.overlaps,
                           longest=st.longest, kernel_launches=st.kernel_launches, host_syncs=st.host_syncs)
                say("%5d %-5s %5d %7d %9.3f %9.3f %7.2f %11.3f %9.3f %9.3f %11d %11d %11d %11d" % (
                    mib, shape, m, min_len, row["ms_count"], row["ms_fm_count"], row["ratio"], row["ms_count_scan"], row["ms_emit"], row["wall_ms"],
                    st.steps, st.tested, st.hit, st.overlaps))
                say(json.dumps(row))
            f.close()
            blk.close()
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
