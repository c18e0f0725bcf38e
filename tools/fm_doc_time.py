"""Device time of the document listing, per tile size.

Per block size and shape: the block and its forward (with its suffix array) on cuda:0, a handle of its BWT, and per document count
D in {1, 256, n / 1000} random bounds attached from the resident suffix array (Block.fm_index(32, docs=bounds)).  Per D the median
of --reps attaches after one warm-up, and per tile T (test route DOC_TILE) the medians of --reps calls after one warm-up of
  df8, df32       document frequencies only (no emit pass) of 65 536 patterns of 8 and of 32 bytes cut from the block
  list8, list32   their listing
  range           the listing of the single range [0, n); its count pass also as GB/s of pv read (4 n bytes), beside the 6.29 TB/s
                  a float4 copy reaches from HBM on this chip -- at 16 MiB pv is 64 MiB and lies in the 256 MiB Infinity Cache
Every figure comes from archon_hip_get_fm_doc_stats: HIP events on the call's stream.  The last lines give, per T, the median over
all workloads of the call's device time, and the T with the least.

    python tools/fm_doc_time.py [--mib 16] [--shapes text,dna] [--tiles 1024,4096,16384] [--out profiles/fm/fm_doc_time16.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def bounds_of(n, D, rng):
    cuts = np.sort(rng.choice(np.arange(1, n), D - 1, replace=False)) if D > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [n]]).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="text,dna")
    ap.add_argument("--tiles", default="1024,4096,16384")
    ap.add_argument("--patterns", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm", "fm_doc_time16.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    out = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    tiles = [int(v) for v in args.tiles.split(",")]
    per_tile = {T: [] for T in tiles}
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_dna(n) if shape == "dna" else S.gen_shape(shape, n)
            rng = np.random.default_rng(mib * 1000 + len(shape))
            blk = pyarchon.Block()
            blk.forward(x)
            starts = rng.integers(0, n - 32, args.patterns)
            pats = {m: [x[q:q + m] for q in starts] for m in (8, 32)}
            for D in (1, 256, n // 1000):
                bounds = bounds_of(n, D, rng)
                os.environ.pop("ARCHON_DOC_TILE", None)
                att = []
                f = None
                for _ in range(args.reps + 1):
                    if f is not None:
                        f.close()
                    f = blk.fm_index(32, docs=bounds)
                    a = pyarchon.fm_doc_stats()
                    att.append(a.ms_attach)
                row = dict(mib=mib, shape=shape, docs=D, what="attach", ms_attach=statistics.median(att[1:]), sort_passes=a.sort_passes,
                           doc_mib=a.doc_bytes / 2.0 ** 20, kernel_launches=a.kernel_launches, host_syncs=a.host_syncs)
                say("%5d MiB %-5s D = %-6d attach %.3f ms, %d sort passes, %.1f MiB on the device" % (mib, shape, D, row["ms_attach"], a.sort_passes, row["doc_mib"]))
                say(json.dumps(row))
                say("%5s %-5s %6s %6s %-7s %10s %9s %9s %9s %10s %10s %9s" % ("MiB", "shape", "D", "T", "what", "search ms", "count ms", "emit ms", "total ms",
                                                                             "rows", "listed", "pv GB/s"))
                for T in tiles:
                    os.environ["ARCHON_DOC_TILE"] = str(T)
                    work = [("df8", lambda: f.docs(pats[8], emit=False)), ("list8", lambda: f.docs(pats[8])),
                            ("df32", lambda: f.docs(pats[32], emit=False)), ("list32", lambda: f.docs(pats[32])),
                            ("range", lambda: f.docs_ranges([0], [n]))]
                    for what, call in work:
                        se, co, em = [], [], []
                        for _ in range(args.reps + 1):
                            call()
                            t = pyarchon.fm_doc_stats()
                            se.append(t.ms_search)
                            co.append(t.ms_count)
                            em.append(t.ms_emit)
                        row = dict(mib=mib, shape=shape, docs=D, tile=T, what=what, ms_search=statistics.median(se[1:]), ms_count=statistics.median(co[1:]),
                                   ms_emit=statistics.median(em[1:]), rows=t.rows, tiles=t.tiles, listed=t.listed, probes=t.probes,
                                   longest_tf=t.longest_tf, kernel_launches=t.kernel_launches, host_syncs=t.host_syncs)
                        row["ms_total"] = row["ms_search"] + row["ms_count"] + row["ms_emit"]
                        row["pv_gbs"] = 4.0 * n / (row["ms_count"] * 1e6) if what == "range" and row["ms_count"] else 0.0
                        per_tile[T].append(row["ms_total"])
                        say("%5d %-5s %6d %6d %-7s %10.3f %9.3f %9.3f %9.3f %10d %10d %9.1f" % (mib, shape, D, T, what, row["ms_search"], row["ms_count"],
                                                                                              row["ms_emit"], row["ms_total"], t.rows, t.listed, row["pv_gbs"]))
                        say(json.dumps(row))
                os.environ.pop("ARCHON_DOC_TILE", None)
                f.close()
            blk.close()
            torch.cuda.empty_cache()
    med = {T: statistics.median(v) for T, v in per_tile.items() if v}
    for T in tiles:
        say("T = %6d: median of %d workloads %.3f ms" % (T, len(per_tile[T]), med[T]))
    best = min(med, key=med.get)
    say("the least median: T = %d" % best)
    say(json.dumps(dict(medians={str(T): med[T] for T in med}, chosen=best)))
    out.close()


if __name__ == "__main__":
    main()
