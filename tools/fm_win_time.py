"""Device time of the wavelet matrix over the suffix array and of its window queries.

Per block size and shape: the block and its forward (with its suffix array) on cuda:0 and a handle of its BWT.  Medians of --reps
runs after one warm-up of
  attach          Block.fm_index(32, wm=True): the build's device time (HIP events) and its rate against the model of 12 n L bytes;
                  beside it the wall time of the block forms of attach_wm and attach_sa (the calls are complete on return) and the
                  device time of the LCP step of the same block
  count, select   2^20 queries over random row ranges with random windows, and over the ranges of 65 536 patterns of 4 and of 32
                  bytes repeated to 2^20 queries; device time of the one kernel
  list1, list16   win_list with most = 1 and most = 16 of the 65 536 patterns of 4 and of 32 bytes: count + emit device time and
                  the wall time of the whole call; beside it what it replaces, Block.fm_locate of the same patterns and a sort of
                  every pattern's starts on the host (wall time; of the first 256 patterns at 4 bytes, whose rows no one locate holds)
Every device figure comes from archon_hip_fm_win_last_stats.

    python tools/fm_win_time.py [--mib 16] [--shapes text,dna] [--out profiles/fm/fm_win_time16.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="text,dna")
    ap.add_argument("--patterns", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm", "fm_win_time16.txt"))
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

    def ok(rc):
        if rc:
            raise pyarchon.ArchonError(rc, L.archon_hip_last_error().decode())

    med = statistics.median
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_dna(n) if shape == "dna" else S.gen_shape(shape, n)
            rng = np.random.default_rng(mib * 1000 + len(shape))
            blk = pyarchon.Block()
            blk.forward(x)
            blk.lcp()
            ms_lcp = pyarchon.lcp_stats().ms_total
            dev, w_wm, w_sa = [], [], []
            f = None
            for _ in range(args.reps + 1):
                if f is not None:
                    f.close()
                f = blk.fm_index(32)
                w_sa.append(wall(lambda: ok(L.archon_hip_block_fm_attach_sa(blk.h, f.h)))[1])
                w_wm.append(wall(lambda: ok(L.archon_hip_block_fm_attach_wm(blk.h, f.h)))[1])
                a = pyarchon.fm_win_stats()
                dev.append(a.ms_attach)
            row = dict(mib=mib, shape=shape, what="attach", levels=a.levels, ms_attach=med(dev[1:]), wall_attach_wm=med(w_wm[1:]),
                       wall_attach_sa=med(w_sa[1:]), ms_lcp=ms_lcp, wm_mib=a.wm_bytes / 2.0 ** 20, kernel_launches=a.kernel_launches,
                       host_syncs=a.host_syncs)
            row["model_gb"] = 12.0 * n * a.levels / 1e9
            row["gbs"] = row["model_gb"] / (row["ms_attach"] * 1e-3)
            say("%5d MiB %-5s attach %.3f ms on the device (%d levels, %.1f MiB; the model's %.2f GB at %.0f GB/s), %.3f ms wall; attach_sa %.3f ms wall, "
                "the LCP step %.3f ms" % (mib, shape, row["ms_attach"], a.levels, row["wm_mib"], row["model_gb"], row["gbs"], row["wall_attach_wm"],
                                          row["wall_attach_sa"], ms_lcp))
            say(json.dumps(row))
            starts = rng.integers(0, n - 32, args.patterns)
            pats = {m: [x[q:q + m] for q in starts] for m in (4, 32)}
            ranges = {m: f.count_ranges(pats[m]) for m in (4, 32)}
            K = args.queries
            lo = rng.integers(0, n, K).astype(np.uint32)
            hi = np.minimum(lo + np.exp(rng.uniform(0, np.log(n), K)).astype(np.int64), n).astype(np.uint32)
            ab = np.sort(rng.integers(0, n + 2, (2, K)), axis=0).astype(np.uint32)
            sets = {"random": (lo, hi)}
            for m in (4, 32):
                sets["pat%d" % m] = tuple(np.resize(v, K) for v in ranges[m])
            say("%5s %-5s %-7s %-8s %9s %9s %9s %12s %12s %12s" % ("MiB", "shape", "what", "ranges", "count ms", "emit ms", "wall ms", "rows", "in window",
                                                                   "walks"))
            for name, (qlo, qhi) in sets.items():
                t = [_dev(torch, v) for v in (qlo, qhi, ab[0], ab[1], np.zeros(K, np.uint32))]
                out_t = torch.zeros(K, dtype=torch.int32, device="cuda:0")
                for what, call in (("count", lambda: f.win_count_dev(t[0], t[1], out_t, t[2], t[3])),
                                   ("select", lambda: f.win_select_dev(t[0], t[1], t[4], out_t, t[2], t[3]))):
                    co, wl = [], []
                    for _ in range(args.reps + 1):
                        wl.append(wall(call)[1])
                        st = pyarchon.fm_win_stats()
                        co.append(st.ms_count)
                    row = dict(mib=mib, shape=shape, what=what, ranges=name, queries=K, ms_count=med(co[1:]), ms_emit=0.0, wall_ms=med(wl[1:]), rows=st.rows,
                               in_window=st.in_window, walks=st.walks, kernel_launches=st.kernel_launches, host_syncs=st.host_syncs)
                    say("%5d %-5s %-7s %-8s %9.3f %9.3f %9.3f %12d %12d %12d" % (mib, shape, what, name, row["ms_count"], 0.0, row["wall_ms"], st.rows,
                                                                                 st.in_window, st.walks))
                    say(json.dumps(row))
            for m in (4, 32):
                qlo, qhi = ranges[m]
                for most in (1, 16):
                    co, em, wl = [], [], []
                    for _ in range(args.reps + 1):
                        wl.append(wall(lambda: f.win_list(qlo, qhi, most=most))[1])
                        st = pyarchon.fm_win_stats()
                        co.append(st.ms_count)
                        em.append(st.ms_emit)
                    row = dict(mib=mib, shape=shape, what="list%d" % most, ranges="pat%d" % m, queries=qlo.size, ms_count=med(co[1:]), ms_emit=med(em[1:]),
                               wall_ms=med(wl[1:]), rows=st.rows, in_window=st.in_window, listed=st.listed, walks=st.walks,
                               kernel_launches=st.kernel_launches, host_syncs=st.host_syncs)
                    say("%5d %-5s %-7s %-8s %9.3f %9.3f %9.3f %12d %12d %12d" % (mib, shape, row["what"], row["ranges"], row["ms_count"], row["ms_emit"],
                                                                                 row["wall_ms"], st.rows, st.in_window, st.walks))
                    say(json.dumps(row))
                # what the list replaces: every row located, then sorted on the host.  The 4-byte patterns have more rows than one
                # locate takes (2^32 - 1), so theirs is timed on the first 256 of them
                some = 256 if m == 4 else qlo.size
                wl = []
                for _ in range(args.reps + 1):
                    wl.append(wall(lambda: [np.sort(p) for p in blk.fm_locate(pats[m][:some])])[1])
                row = dict(mib=mib, shape=shape, what="locate+sort", ranges="pat%d" % m, queries=some, wall_ms=med(wl[1:]),
                           rows=int((qhi[:some].astype(np.int64) - qlo[:some]).sum()))
                say("%5d %-5s %-7s %-8s %9s %9s %9.3f %12d   (Block.fm_locate and a host sort of the starts of the first %d patterns)" % (
                    mib, shape, "locate", row["ranges"], "", "", row["wall_ms"], row["rows"], some))
                say(json.dumps(row))
            f.close()
            blk.close()
            torch.cuda.empty_cache()
    out.close()


def _dev(torch, a):
    return torch.from_numpy(a.view(np.int32)).to("cuda:0")


if __name__ == "__main__":
    main()
