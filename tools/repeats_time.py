"""Device time of the repeats of a block (the repeats rows) at block sizes a user runs.

Per block size and shape: the block and its forward on cuda:0 with its suffix array, its LCP array by archon_hip_lcp_dev into a
device buffer (ms_total of archon_hip_get_lcp_stats: the yardstick -- both calls consume the same 4n-byte array), then
archon_hip_repeats_dev on that array and the resident BWT, per kind, counting only and with room for every repeat:
  count     ms_count: the hierarchy, the flag sums (kind 1) and the count pass (HIP events on the call's stream)
  emit      ms_emit: the scan of the tile counts and the emit pass, the identical search again storing the records
  probes    entries the searches of the count pass read, per row; the header's bound per row beside it
Each figure is the median of --reps calls after one warm-up, from archon_hip_get_repeat_stats.

    python tools/repeats_time.py [--mib 16,256] [--shapes random,dna,text,prose,a] [--kinds 1,2] [--reps 3]
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
    ap.add_argument("--mib", default="16,256")
    ap.add_argument("--shapes", default="random,dna,text,prose,a")
    ap.add_argument("--kinds", default="1,2")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon

    print("%5s %-7s %4s %10s %10s %9s %9s %9s %9s %10s" % ("MiB", "shape", "kind", "repeats", "intervals", "lcp ms", "count ms", "emit ms",
                                                          "probes/row", "bound/row"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_prose(n, S.SEED_BASE + 6) if shape == "prose" else S.gen_shape(shape, n)
            x_t = torch.from_numpy(x).to("cuda:0")
            sa_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            bwt_t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            base_t = torch.zeros(1, dtype=torch.int32, device="cuda:0")
            lcp_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
            pyarchon.forward_dev(x_t, sa_t, bwt_t, base_t)
            base = int(base_t.item())
            lcp_ms = []
            for _ in range(args.reps + 1):
                pyarchon.lcp_dev(x_t, sa_t, lcp_t)
                lcp_ms.append(pyarchon.lcp_stats().ms_total)
            lcp_ms = statistics.median(lcp_ms[1:])
            del x_t, sa_t
            for kind in [int(v) for v in args.kinds.split(",")]:
                total = pyarchon.repeats_dev(lcp_t, bwt_t, base, kind)
                only = []
                for _ in range(args.reps + 1):
                    pyarchon.repeats_dev(lcp_t, bwt_t, base, kind)
                    only.append(pyarchon.repeat_stats().ms_count)
                out_t = torch.empty(4 * max(total, 1), dtype=torch.int32, device="cuda:0")
                cms, ems = [], []
                for _ in range(args.reps + 1):
                    assert pyarchon.repeats_dev(lcp_t, bwt_t, base, kind, out_t=out_t) == total
                    st = pyarchon.repeat_stats()
                    cms.append(st.ms_count)
                    ems.append(st.ms_emit)
                del out_t
                row = dict(mib=mib, shape=shape, kind=kind, repeats=total, intervals=st.intervals, occurrences=st.occurrences, longest=st.longest,
                           lcp_ms=lcp_ms, count_only_ms=statistics.median(only[1:]), count_ms=statistics.median(cms[1:]),
                           emit_ms=statistics.median(ems[1:]), probes_per_row=st.probes / max(n - 1, 1),
                           bound_per_row=2 * (2 * st.fan - 1) * st.levels, fan=st.fan, levels=st.levels, launches=st.kernel_launches,
                           distinct_substrings=st.distinct_substrings)
                print("%5d %-7s %4d %10d %10d %9.3f %9.3f %9.3f %9.2f %10d" % (mib, shape, kind, total, st.intervals, lcp_ms, row["count_only_ms"],
                                                                               row["emit_ms"], row["probes_per_row"], row["bound_per_row"]))
                print(json.dumps(row))
                sys.stdout.flush()
            del lcp_t, bwt_t
            torch.cuda.empty_cache()


if __name__ == "__main__":
    np.seterr(over="ignore")
    main()
