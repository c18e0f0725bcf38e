"""Device time of the entropy and complexity calls of a block (the entropy row) at a block size a user runs.

Per block size and shape: the block and its forward on cuda:0 with its suffix array, its LCP array by archon_hip_lcp_dev into a
device buffer (ms_total of archon_hip_get_lcp_stats: the yardstick), then
  entropy      archon_hip_entropy_dev with ONE order per call, per k: the passes (ms_count) and the rank table the device form
               builds per call (ms_build), with the record and the three kinds of group
  all orders   the same with every k of --orders in one call: one wait for all of them
  complexity   archon_hip_complexity_dev at the default max_len with the BWT (histogram, runs pass and finish: ms_count)
each also as a multiple of the LCP time.  Each figure is the median of --reps calls after one warm-up, from
archon_hip_entropy_last_stats.  The output is printed and written to --out (default profiles/entropy/entropy_time<MiB>.txt).

    python tools/entropy_time.py [--mib 16] [--shapes dna,text] [--orders 0,1,2,4,8,16] [--reps 3] [--out FILE]
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
    ap.add_argument("--orders", default="0,1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon

    out_path = args.out or os.path.join(ROOT, "profiles", "entropy", "entropy_time%s.txt" % args.mib.replace(",", "_"))
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

    orders = [int(v) for v in args.orders.split(",")]
    say("%5s %-6s %-10s %12s %12s %14s %8s %8s %8s %7s" % ("MiB", "shape", "what", "contexts", "pairs", "bits/symbol", "lcp ms", "build", "count", "x LCP"))
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
            (lcp_ms,), _, _ = median_of(lambda: pyarchon.lcp_dev(x_t, sa_t, lcp_t), pyarchon.lcp_stats, ["ms_total"])
            del x_t
            for ks in [[k] for k in orders] + [orders]:
                (build_ms, count_ms), st, recs = median_of(lambda: pyarchon.entropy_dev(sa_t, lcp_t, bwt_t, base, ks), pyarchon.entropy_stats,
                                                           ["ms_build", "ms_count"])
                row = dict(mib=mib, shape=shape, ks=ks, records=[dict(zip(r.dtype.names, r.tolist())) for r in recs], groups_direct=st.groups_direct,
                           groups_table=st.groups_table, groups_in_wave=st.groups_in_wave, tile=st.tile, lcp_ms=lcp_ms, build_ms=build_ms,
                           count_ms=count_ms, launches=st.kernel_launches, waits=st.host_syncs, x_lcp=count_ms / lcp_ms)
                r = recs[-1]
                say("%5d %-6s %-10s %12d %12d %14.6f %8.3f %8.3f %8.3f %7.2f" %
                    (mib, shape, "k=%d" % ks[0] if len(ks) == 1 else "all %d" % len(ks), r["contexts"], r["pairs"], r["bits"] / max(int(r["symbols"]), 1),
                     lcp_ms, build_ms, count_ms, row["x_lcp"]))
                say(json.dumps(row))
            (count_ms,), st, rec = median_of(lambda: pyarchon.complexity_dev(lcp_t, bwt_t), pyarchon.entropy_stats, ["ms_count"])
            row = dict(mib=mib, shape=shape, complexity=rec.asdict(), lcp_ms=lcp_ms, count_ms=count_ms, launches=st.kernel_launches,
                       waits=st.host_syncs, x_lcp=count_ms / lcp_ms)
            say("%5d %-6s %-10s %12s %12s %14s %8.3f %8s %8.3f %7.2f" %
                (mib, shape, "complexity", "runs %d" % rec.runs, "d_%d=%d" % (rec.delta_len, rec.delta_count), "lcp<=%d" % rec.lcp_max, lcp_ms, "", count_ms,
                 row["x_lcp"]))
            say(json.dumps(row))
            del sa_t, lcp_t, bwt_t
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    np.seterr(over="ignore")
    main()
