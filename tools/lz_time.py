"""Device time of the LZ77 factorization of a block (the LZ rows) at block sizes a user runs.

Per block size, shape and direction: the block and its forward on cuda:0 with its suffix array, its LCP array by
archon_hip_lcp_dev into a device buffer (ms_total of archon_hip_get_lcp_stats: the yardstick -- the LPF pass consumes that array
and the suffix array), then archon_hip_lpf_dev and archon_hip_lz_parse_dev on device buffers:
  lpf       ms_lpf: the two hierarchies and the LPF pass (HIP events on the call's stream)
  parse     ms_parse: the F arrays, the descent and the count pass
  emit      ms_emit: the scan of the tile counts and the emit pass
  probes    node pairs the searches read, per row; hops: the dependent steps of the descent, the header's bound beside it
Each figure is the median of --reps calls after one warm-up, from archon_hip_get_lz_stats.

    python tools/lz_time.py [--mib 16,256] [--shapes random,dna,text,prose,a] [--dirs 0,1] [--reps 3]
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
    ap.add_argument("--dirs", default="0,1")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon

    print("%5s %-7s %3s %10s %9s %9s %9s %9s %10s %6s %6s" % ("MiB", "shape", "dir", "phrases", "lcp ms", "lpf ms", "parse ms", "emit ms",
                                                             "probes/row", "hops", "bound"))
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
            lcp_ms = []
            for _ in range(args.reps + 1):
                pyarchon.lcp_dev(x_t, sa_t, lcp_t)
                lcp_ms.append(pyarchon.lcp_stats().ms_total)
            lcp_ms = statistics.median(lcp_ms[1:])
            del x_t, bwt_t
            rec_t = torch.empty(2 * n, dtype=torch.int32, device="cuda:0")
            for d in [int(v) for v in args.dirs.split(",")]:
                lms = []
                for _ in range(args.reps + 1):
                    pyarchon.lpf_dev(sa_t, lcp_t, d, rec_t)
                    lst = pyarchon.lz_stats()
                    lms.append(lst.ms_lpf)
                total = pyarchon.lz_parse_dev(rec_t)
                out_t = torch.empty(3 * total, dtype=torch.int32, device="cuda:0")
                pms, ems = [], []
                for _ in range(args.reps + 1):
                    assert pyarchon.lz_parse_dev(rec_t, out_t=out_t) == total
                    st = pyarchon.lz_stats()
                    pms.append(st.ms_parse)
                    ems.append(st.ms_emit)
                del out_t
                top = st.tile ** (st.parse_levels - 1)
                row = dict(mib=mib, shape=shape, dir=d, phrases=total, literals=st.literals, longest=st.longest, lcp_ms=lcp_ms,
                           lpf_ms=statistics.median(lms[1:]), parse_ms=statistics.median(pms[1:]), emit_ms=statistics.median(ems[1:]),
                           probes_per_row=lst.probes / n, probe_bound_per_row=2 * (2 * lst.fan - 1) * lst.levels, fan=lst.fan, levels=lst.levels,
                           tile=st.tile, parse_levels=st.parse_levels, hops=st.hops, hop_bound=(n + top - 1) // top + (st.parse_levels - 1) * st.tile,
                           lpf_launches=lst.kernel_launches, parse_launches=st.kernel_launches)
                print("%5d %-7s %3d %10d %9.3f %9.3f %9.3f %9.3f %10.2f %6d %6d" % (mib, shape, d, total, lcp_ms, row["lpf_ms"], row["parse_ms"],
                                                                                    row["emit_ms"], row["probes_per_row"], st.hops, row["hop_bound"]))
                print(json.dumps(row))
                sys.stdout.flush()
            del lcp_t, sa_t, rec_t
            torch.cuda.empty_cache()


if __name__ == "__main__":
    np.seterr(over="ignore")
    main()
