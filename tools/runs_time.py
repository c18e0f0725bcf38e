"""Device time of the runs call of a block (the runs row) at a block size a user runs.

Per block size and shape: the block and its forward on cuda:0 with its suffix array, the forward of the complemented block (the
second sort: ms_total of archon_hip_get_stats), its LCP array by archon_hip_lcp_dev into a device buffer (ms_total of
archon_hip_get_lcp_stats: the yardstick), then
  count    archon_hip_runs_dev without an output: the inverse arrays and the three hierarchies (ms_build), the count pass (ms_count)
  emit     the same with room for the records: the scan of the tile words and the emit pass, which runs the rule again (ms_emit)
  lce      archon_hip_lce_dev over 2^20 random pairs: the query kernel (ms_count of that call)
  block    Block.runs(count_only=True) on the resident block: its own second sort (ms_forward) and LCP step (ms_lcp)
each stage also as a multiple of the LCP time, with the rule's counters.  Each figure is the median of --reps calls after one
warm-up, from archon_hip_runs_last_stats.  The output is printed and written to --out (default profiles/runs/runs_time<MiB>.txt).

    python tools/runs_time.py [--mib 16] [--shapes dna,text,motif_defects,random] [--reps 3] [--out FILE]
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
    ap.add_argument("--shapes", default="dna,text,motif_defects,random")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon

    out_path = args.out or os.path.join(ROOT, "profiles", "runs", "runs_time%s.txt" % args.mib.replace(",", "_"))
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
            res = call()
            st = stats()
            got.append([getattr(st, f) for f in field])
        return [statistics.median(v[i] for v in got[1:]) for i in range(len(field))], st, res

    say("%5s %-13s %-6s %10s %10s %10s %10s %8s %8s %8s %8s %8s %7s" % ("MiB", "shape", "what", "runs", "candidates", "roots", "lce", "lcp ms", "sort 2",
                                                                       "build", "count", "emit", "x LCP"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_shape(shape, n)
            x_t = torch.from_numpy(x).to("cuda:0")
            sa_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            sa_c_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            bwt_t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            base_t = torch.zeros(1, dtype=torch.int32, device="cuda:0")
            lcp_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            pyarchon.forward_dev(x_t, sa_t, bwt_t, base_t)
            xc_t = 255 - x_t
            (sort2_ms,), _, _ = median_of(lambda: pyarchon.forward_dev(xc_t, sa_c_t, bwt_t, base_t), pyarchon.stats_raw, ["ms_total"])
            (lcp_ms,), _, _ = median_of(lambda: pyarchon.lcp_dev(x_t, sa_t, lcp_t), pyarchon.lcp_stats, ["ms_total"])
            del x_t, xc_t, bwt_t

            def row_of(what, st, total, **ms):
                row = dict(mib=mib, shape=shape, what=what, total=int(total), runs=st.runs, emitted=st.emitted, candidates=st.candidates, roots=st.roots,
                           lce_queries=st.lce_queries, probes=st.probes, longest_period=st.longest_period, lcp_ms=lcp_ms, sort2_ms=sort2_ms,
                           launches=st.kernel_launches, waits=st.host_syncs, **ms)
                row["x_lcp"] = sum(ms.values()) / lcp_ms
                return row

            def line_of(row):
                f = lambda k: "%8.3f" % row[k] if k in row else "%8s" % ""      # noqa: E731
                say("%5d %-13s %-6s %10d %10d %10d %10d %8.3f %8.3f %s %s %s %7.2f" %
                    (mib, shape, row["what"], row["total"], row["candidates"], row["roots"], row["lce_queries"], lcp_ms, sort2_ms, f("build_ms"),
                     f("count_ms"), f("emit_ms"), row["x_lcp"]))
                say(json.dumps(row))

            (build_ms, count_ms), st, total = median_of(lambda: pyarchon.runs_dev(sa_t, lcp_t, sa_c_t), pyarchon.run_stats, ["ms_build", "ms_count"])
            line_of(row_of("count", st, total, build_ms=build_ms, count_ms=count_ms))
            out_t = torch.empty(4 * max(total, 1), dtype=torch.int32, device="cuda:0")
            (build_ms, count_ms, emit_ms), st, total = median_of(lambda: pyarchon.runs_dev(sa_t, lcp_t, sa_c_t, out_t=out_t), pyarchon.run_stats,
                                                                 ["ms_build", "ms_count", "ms_emit"])
            line_of(row_of("emit", st, total, build_ms=build_ms, count_ms=count_ms, emit_ms=emit_ms))
            del out_t
            k = 1 << 20
            rng = np.random.default_rng(n)
            s_t = torch.from_numpy(rng.integers(0, n + 1, k).astype(np.int32)).to("cuda:0")
            t_t = torch.from_numpy(rng.integers(0, n + 1, k).astype(np.int32)).to("cuda:0")
            lce_t = torch.empty(k, dtype=torch.int32, device="cuda:0")
            (build_ms, count_ms), st, _ = median_of(lambda: pyarchon.lce_dev(sa_t, lcp_t, s_t, t_t, lce_t), pyarchon.run_stats, ["ms_build", "ms_count"])
            line_of(row_of("lce", st, k, build_ms=build_ms, count_ms=count_ms))
            del sa_t, sa_c_t, lcp_t, s_t, t_t, lce_t
            torch.cuda.empty_cache()
            blk = pyarchon.Block()
            try:
                blk.forward(x, want_sa=True)
                (fwd_ms, blk_lcp_ms, build_ms, count_ms), st, total = median_of(lambda: blk.runs(count_only=True), pyarchon.run_stats,
                                                                                ["ms_forward", "ms_lcp", "ms_build", "ms_count"])
                row = row_of("block", st, total, build_ms=build_ms, count_ms=count_ms)
                row.update(block_forward_ms=fwd_ms, block_lcp_ms=blk_lcp_ms)
                line_of(row)
            finally:
                blk.close()
    out.close()


if __name__ == "__main__":
    np.seterr(over="ignore")
    main()
