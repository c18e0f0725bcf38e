"""Device time of the approximate FM search (the approximate FM rows): the count and the emit pass of
archon_hip_block_fm_approx at block sizes a user runs.

Per block size, shape, pattern length m and distance K: the block and its forward on cuda:0 (its table built by a first
call), then patterns that are substrings of x at seeded offsets with 0 .. K random substitutions.  A probe of --probe
patterns (counting only) gives the nodes (expansions + steps) per pattern; the batch is then as many patterns as keep one
call under --node-budget nodes (at most --patterns).  Per rep, one call with room for every hit:
  count     ms_count: the count pass (HIP events on the call's stream), median of --reps after one warm-up
  emit      ms_emit: the emit pass, the identical search again writing the hits, median
  per node  ns per node of the whole count pass (the batch's waves run side by side), expansions and steps per pattern
Every figure comes from archon_hip_get_fm_approx_stats.

    python tools/fm_approx_time.py [--mib 16,256] [--shapes dna,random,text] [--lengths 32,100] [--ks 1,2]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def patterns(x, rng, count, m, K):
    n = x.size
    out = []
    for q in rng.integers(0, n - m + 1, count):
        p = x[q:q + m].copy()
        for _ in range(int(rng.integers(0, K + 1))):
            p[int(rng.integers(0, m))] = rng.integers(0, 256)
        out.append(p.tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16,256")
    ap.add_argument("--shapes", default="dna,random,text")
    ap.add_argument("--lengths", default="32,100")
    ap.add_argument("--ks", default="1,2")
    ap.add_argument("--patterns", type=int, default=16384)
    ap.add_argument("--probe", type=int, default=64)
    ap.add_argument("--node-budget", type=float, default=2e7)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    vp = ctypes.c_void_p

    print("%5s %-7s %4s %2s %6s %10s %10s %9s %9s %9s %8s" % ("MiB", "shape", "m", "K", "pats", "exp/pat", "steps/pat", "count ms",
                                                           "emit ms", "ns/node", "hits"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_shape(shape, n)
            blk = pyarchon.Block()
            blk.forward(x, want_sa=False)
            blk.fm_count([x[:4].tobytes()])
            for m in [int(v) for v in args.lengths.split(",")]:
                for K in [int(v) for v in args.ks.split(",")]:
                    rng = np.random.default_rng(mib * 1000 + m * 10 + K + len(shape))
                    probe = patterns(x, rng, args.probe, m, K)
                    blk.fm_approx(probe, K, hits=False)
                    st = pyarchon.fm_approx_stats()
                    per = max((st.expansions + st.steps) / args.probe, 1.0)
                    count = int(min(args.patterns, max(args.probe, args.node_budget // per)))
                    pats = patterns(x, rng, count, m, K)
                    packed, off = pyarchon._pack_patterns(pats)
                    nh, no = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
                    tot = ctypes.c_uint64(0)
                    assert L.archon_hip_block_fm_approx(blk.h, pyarchon._p(packed), pyarchon._p(off), count, K, pyarchon._p(nh),
                                                        pyarchon._p(no), None, 0, ctypes.cast(ctypes.byref(tot), vp)) == 0
                    hits = np.zeros(max(tot.value, 1), pyarchon.FM_HIT)
                    cms, ems = [], []
                    for _ in range(args.reps + 1):
                        rc = L.archon_hip_block_fm_approx(blk.h, pyarchon._p(packed), pyarchon._p(off), count, K, pyarchon._p(nh),
                                                          pyarchon._p(no), pyarchon._p(hits), hits.size, ctypes.cast(ctypes.byref(tot), vp))
                        assert rc == 0, pyarchon.lib().archon_hip_last_error()
                        st = pyarchon.fm_approx_stats()
                        cms.append(st.ms_count)
                        ems.append(st.ms_emit)
                    c_ms, e_ms = statistics.median(cms[1:]), statistics.median(ems[1:])
                    nodes = st.expansions + st.steps
                    row = dict(mib=mib, shape=shape, m=m, K=K, patterns=count, expansions_per_pattern=st.expansions / count,
                               steps_per_pattern=st.steps / count, count_ms=c_ms, emit_ms=e_ms, ns_per_node=c_ms * 1e6 / max(nodes, 1),
                               hits=st.hits, occurrences=st.occurrences, nodes=nodes)
                    print("%5d %-7s %4d %2d %6d %10.1f %10.1f %9.3f %9.3f %9.2f %8d" % (
                        mib, shape, m, K, count, row["expansions_per_pattern"], row["steps_per_pattern"], c_ms, e_ms, row["ns_per_node"],
                        st.hits))
                    print(json.dumps(row))
                    sys.stdout.flush()
            blk.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
