"""Device time of archon_hip_lcp_dev next to the forward of the same block (the LCP table).

Per shape: the block and its forward on cuda:0 (torch tensors), then `--reps` timed forward_dev calls and `--reps` timed
lcp_dev calls, each bracketed by HIP events on the current stream after one untimed warm-up; prints the medians, the
call's work counters (archon_hip_lcp_stats), and one JSON line per shape.

    python tools/lcp_time.py [--mib 256] [--reps 7] [--shapes random,text,prose,a,motif_defects,random_copy]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="random,text,prose,a,motif_defects,random_copy")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    n = args.mib << 20

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    print("%-14s %10s %10s %8s %8s %12s %14s %7s" % ("shape", "fwd ms", "lcp ms", "max_lcp", "rounds", "irreducible", "compared/n", "long"))
    for shape in args.shapes.split(","):
        x_t = torch.from_numpy(S.gen_shape(shape, n)).to("cuda:0")
        sa_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
        bwt_t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        base_t = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        lcp_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
        fwd = timed(lambda: pyarchon.forward_dev(x_t, sa_t, bwt_t, base_t))
        lcp = timed(lambda: pyarchon.lcp_dev(x_t, sa_t, lcp_t))
        st = pyarchon.lcp_stats().asdict()
        print("%-14s %10.3f %10.3f %8d %8d %12d %14.3f %7d" % (shape, fwd, lcp, st["max_lcp"], st["long_rounds"], st["irreducible"],
                                                            st["compared_bytes"] / n, st["long_items"]))
        print(json.dumps(dict(shape=shape, forward_ms=fwd, lcp_ms=lcp, reps=args.reps, **st)))
        sys.stdout.flush()
        del x_t, sa_t, bwt_t, base_t, lcp_t


if __name__ == "__main__":
    main()
