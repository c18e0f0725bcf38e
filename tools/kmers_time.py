"""Device time of the k-mer calls of a block (the k-mer row) at a block size a user runs.

Per block size and shape: the block and its forward on cuda:0 with its suffix array, its LCP array by archon_hip_lcp_dev into a
device buffer (ms_total of archon_hip_get_lcp_stats: the yardstick -- every call here consumes that array and the suffix array),
then per k, on those two arrays:
  count     archon_hip_kmers_dev counting only, with a 256-bin histogram: bounds, scan, starts and the count pass (ms_count)
  emit      the same with room for every k-mer: the scan of the group tiles and the emit pass (ms_emit)
  occ       archon_hip_kmer_occ_dev: bounds, scan, starts (ms_count) and the scatter (ms_scatter)
  sus       archon_hip_sus_dev: the check and the pass (ms_scatter); it does not depend on k and is timed once per block
each also as a multiple of the LCP time.  Each figure is the median of --reps calls after one warm-up, from
archon_hip_get_kmer_stats.  The output is printed and written to --out (default profiles/kmers/kmers_time<MiB>.txt).

    python tools/kmers_time.py [--mib 16] [--shapes dna,text] [--k 8,16,32] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="dna,text")
    ap.add_argument("--k", default="8,16,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon

    out_path = args.out or os.path.join(ROOT, "profiles", "kmers", "kmers_time%s.txt" % args.mib.replace(",", "_"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    out = open(out_path, "w")

    def say(line):
        print(line)
        out.write(line + "\n")
        out.flush()
        sys.stdout.flush()

    def median_of(call, field):
        got = []
        for _ in range(args.reps + 1):
            call()
            st = pyarchon.kmer_stats()
            got.append([getattr(st, f) for f in field])
        return [statistics.median(v[i] for v in got[1:]) for i in range(len(field))], st

    say("%5s %-6s %3s %10s %10s %8s %8s %8s %8s %8s %8s   (x LCP: count, count+emit, occ, sus)" %
        ("MiB", "shape", "k", "distinct", "unique", "lcp ms", "count", "emit", "occ bnd", "occ sct", "sus"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_shape(shape, n)
            x_t = torch.from_numpy(x).to("cuda:0")
            sa_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            bwt_t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            base_t = torch.zeros(1, dtype=torch.int32, device="cuda:0")
            lcp_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            pyarchon.forward_dev(x_t, sa_t, bwt_t, base_t)
            lcp_ms = []
            for _ in range(args.reps + 1):
                pyarchon.lcp_dev(x_t, sa_t, lcp_t)
                lcp_ms.append(pyarchon.lcp_stats().ms_total)
            lcp_ms = statistics.median(lcp_ms[1:])
            del x_t, bwt_t
            words_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            hist_t = torch.empty(256, dtype=torch.int32, device="cuda:0")
            (sus_ms,), _ = median_of(lambda: pyarchon.sus_dev(sa_t, lcp_t, words_t), ["ms_scatter"])
            for k in [int(v) for v in args.k.split(",")]:
                (count_ms,), st = median_of(lambda: pyarchon.kmers_dev(sa_t, lcp_t, k, hist_t=hist_t), ["ms_count"])
                total = st.kmers
                out_t = torch.empty(3 * max(total, 1), dtype=torch.int32, device="cuda:0")
                (count2_ms, emit_ms), st = median_of(lambda: pyarchon.kmers_dev(sa_t, lcp_t, k, out_t=out_t), ["ms_count", "ms_emit"])
                del out_t
                (bounds_ms, scatter_ms), _ = median_of(lambda: pyarchon.kmer_occ_dev(sa_t, lcp_t, k, words_t[:n - k + 1]), ["ms_count", "ms_scatter"])
                row = dict(mib=mib, shape=shape, k=k, groups=st.groups, short_rows=st.short_rows, distinct=st.distinct, unique=st.unique, most=st.most,
                           lcp_ms=lcp_ms, count_only_ms=count_ms, count_ms=count2_ms, emit_ms=emit_ms, occ_bounds_ms=bounds_ms, occ_scatter_ms=scatter_ms,
                           sus_ms=sus_ms, tile=st.tile, x_lcp=dict(count=count_ms / lcp_ms, list=(count2_ms + emit_ms) / lcp_ms,
                                                                  occ=(bounds_ms + scatter_ms) / lcp_ms, sus=sus_ms / lcp_ms))
                say("%5d %-6s %3d %10d %10d %8.3f %8.3f %8.3f %8.3f %8.3f %8.3f   %.2f %.2f %.2f %.2f" %
                    (mib, shape, k, st.distinct, st.unique, lcp_ms, count_ms, emit_ms, bounds_ms, scatter_ms, sus_ms, row["x_lcp"]["count"],
                     row["x_lcp"]["list"], row["x_lcp"]["occ"], row["x_lcp"]["sus"]))
                say(json.dumps(row))
            del sa_t, lcp_t, words_t, hist_t
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    np.seterr(over="ignore")
    main()
