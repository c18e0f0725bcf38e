"""Device time of the minimal-absent-words call of a block (the MAW row) at a block size a user runs.

Per block size and shape: the block and its forward on cuda:0 with its suffix array, its LCP array by archon_hip_lcp_dev into a
device buffer (ms_total of archon_hip_get_lcp_stats: the yardstick), archon_hip_repeats_dev of kind 1 counting on the same
arrays (ms_count of its record: the same hierarchy, flag sums and searches without the walk), then per max_len (0 = no limit):
  build     the rank table over a copy of the BWT that the device form makes per call (ms_build)
  count     archon_hip_maws_dev counting only: the check, the hierarchy, the flag sums and the count pass (ms_count)
  emit      the same with room for every word: the scan of the tile words and the emit pass (ms_emit); left out (-1) when the
            words would take more than --emit-gib of device memory
each also as a multiple of the LCP time.  Each figure is the median of --reps calls after one warm-up, from
archon_hip_maw_last_stats.  The output is printed and written to --out (default profiles/maw/maw_time<MiB>.txt).

    python tools/maw_time.py [--mib 16] [--shapes dna,text] [--max-len 8,12,0] [--reps 3] [--emit-gib 4] [--out FILE]
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
    ap.add_argument("--max-len", default="8,12,0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--emit-gib", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon

    out_path = args.out or os.path.join(ROOT, "profiles", "maw", "maw_time%s.txt" % args.mib.replace(",", "_"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    out = open(out_path, "w")

    def say(line):
        print(line)
        out.write(line + "\n")
        out.flush()
        sys.stdout.flush()

    def median_of(call, stats, field):
        got = []
        for _ in range(args.reps + 1):
            call()
            st = stats()
            got.append([getattr(st, f) for f in field])
        return [statistics.median(v[i] for v in got[1:]) for i in range(len(field))], st

    say("%5s %-6s %7s %12s %10s %10s %8s %8s %8s %8s %8s   (x LCP: count, count+emit)" %
        ("MiB", "shape", "max_len", "words", "nodes", "children", "lcp ms", "rep1 ms", "build", "count", "emit"))
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
            base = int(base_t.item())
            (lcp_ms,), _ = median_of(lambda: pyarchon.lcp_dev(x_t, sa_t, lcp_t), pyarchon.lcp_stats, ["ms_total"])
            del x_t
            (rep_ms,), rst = median_of(lambda: pyarchon.repeats_dev(lcp_t, bwt_t, base, 1), pyarchon.repeat_stats, ["ms_count"])
            for max_len in [int(v) for v in args.max_len.split(",")]:
                call = lambda out_t=None: pyarchon.maws_dev(sa_t, lcp_t, bwt_t, base, 2, max_len, out_t=out_t)      # noqa: E731
                (build_ms, count_ms), st = median_of(call, pyarchon.maw_stats, ["ms_build", "ms_count"])
                total = st.words
                emit_ms = -1.0
                if total * 20 <= args.emit_gib * (1 << 30):
                    out_t = torch.empty(5 * max(total, 1), dtype=torch.int32, device="cuda:0")
                    (emit_ms,), st = median_of(lambda: call(out_t), pyarchon.maw_stats, ["ms_emit"])
                    del out_t
                row = dict(mib=mib, shape=shape, max_len=max_len, words=total, nodes=st.nodes, children=st.children, intervals=st.intervals,
                           maximal_repeats=rst.repeats, sets_direct=st.sets_direct, sets_table=st.sets_table, probes=st.probes, shortest=st.shortest,
                           longest=st.longest, absent_bytes=st.absent_bytes, lcp_ms=lcp_ms, repeats1_count_ms=rep_ms, build_ms=build_ms,
                           count_ms=count_ms, emit_ms=emit_ms, launches=st.kernel_launches,
                           x_lcp=dict(count=count_ms / lcp_ms, list=(count_ms + max(emit_ms, 0)) / lcp_ms))
                say("%5d %-6s %7d %12d %10d %10d %8.3f %8.3f %8.3f %8.3f %8.3f   %.2f %.2f" %
                    (mib, shape, max_len, total, st.nodes, st.children, lcp_ms, rep_ms, build_ms, count_ms, emit_ms, row["x_lcp"]["count"],
                     row["x_lcp"]["list"]))
                say(json.dumps(row))
            del sa_t, lcp_t, bwt_t
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    np.seterr(over="ignore")
    main()
