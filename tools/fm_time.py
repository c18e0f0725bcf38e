"""Device time of the FM index (the FM rows): table build, count and locate at block sizes a user runs.

Per block size and shape: the block and its forward on cuda:0, then
  build   FmIndex.from_dev over the device BWT (archon_hip_fm_create_dev): ms_build of the call, median of --reps after one
          warm-up build
  count   --patterns patterns of each length in --lengths, half substrings of the block at seeded offsets and half seeded
          random bytes, on the device (archon_hip_fm_count_dev): ms_query (HIP events around the count kernel), median of
          --reps after one warm-up; patterns per second; steps and shared_steps of the call
  locate  a resident block with its SA (archon_hip_block_fm_locate) on a prefix of the same patterns holding at most
          --locate-max occurrences: ms_query of the call (count and gather kernels) and the occurrences located
The bytes model of a count: each rank step reads the 1024-byte sub-chunk of lo and of hi (one when they share it:
2 steps - shared_steps sub-chunks) and a 64-byte line of the superblock and of the sub-chunk table for each of them, so
bytes = (2 steps - shared_steps) x (1024 + 2 x 64); printed over the count's device time.

    python tools/fm_time.py [--mib 16,256] [--shapes random,text,dna,prose] [--patterns 1048576] [--lengths 8,32,128]
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

SUB_BYTES, LINE = 1024, 64


def make_patterns(x, k, m, seed):
    """k patterns of m bytes: the first half substrings of x at seeded offsets, the rest seeded random bytes"""
    rng = np.random.default_rng(seed)
    h = k // 2
    starts = rng.integers(0, x.size - m + 1, h)
    sub = x[starts[:, None] + np.arange(m)[None, :]]
    rnd = rng.integers(0, 256, (k - h, m), dtype=np.uint8)
    packed = np.concatenate([sub, rnd]).reshape(-1)
    off = (np.arange(k + 1, dtype=np.uint64) * m).astype(np.uint32)
    return packed, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16,256")
    ap.add_argument("--shapes", default="random,text,dna,prose")
    ap.add_argument("--patterns", type=int, default=1 << 20)
    ap.add_argument("--lengths", default="8,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--locate-max", type=int, default=1 << 26)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    k = args.patterns

    print("%6s %-8s %4s %9s %9s %10s %9s %12s %12s %9s %9s %11s" % ("MiB", "shape", "m", "build ms", "count ms", "Mpat/s", "GB/s", "steps",
                                                                   "shared", "locate ms", "loc pats", "located"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_shape(shape, n)
            x_t = torch.from_numpy(x).to("cuda:0")
            bwt_t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            base_t = torch.zeros(1, dtype=torch.int32, device="cuda:0")
            pyarchon.forward_dev(x_t, None, bwt_t, base_t)
            torch.cuda.synchronize()
            base = int(base_t.item())
            builds = []
            for _ in range(args.reps + 1):
                f = pyarchon.FmIndex.from_dev(bwt_t, base)
                builds.append(pyarchon.fm_stats().ms_build)
                table_bytes = pyarchon.fm_stats().table_bytes
                f.close()
            build_ms = statistics.median(builds[1:])
            f = pyarchon.FmIndex.from_dev(bwt_t, base)
            del x_t
            blk = pyarchon.Block()
            blk.forward(x)
            for m in [int(v) for v in args.lengths.split(",")]:
                packed, off = make_patterns(x, k, m, seed=mib * 1000 + m)
                p_t = torch.from_numpy(packed).to("cuda:0")
                o_t = torch.from_numpy(off.view(np.int32)).to("cuda:0")
                lo_t = torch.empty(k, dtype=torch.int32, device="cuda:0")
                hi_t = torch.empty(k, dtype=torch.int32, device="cuda:0")
                counts = []
                for _ in range(args.reps + 1):
                    f.count_dev(p_t, o_t, lo_t, hi_t)
                    st = pyarchon.fm_stats()
                    counts.append(st.ms_query)
                count_ms = statistics.median(counts[1:])
                occ = (hi_t.cpu().numpy().view(np.uint32).astype(np.int64) - lo_t.cpu().numpy().view(np.uint32))
                cum = np.cumsum(occ)
                kl = int(np.searchsorted(cum, args.locate_max, side="right"))
                total = int(cum[kl - 1]) if kl else 0
                pos = np.empty(max(total, 1), np.uint32)
                tot = ctypes.c_uint64(0)
                lps = []
                for _ in range(2):
                    rc = L.archon_hip_block_fm_locate(blk.h, pyarchon._p(packed), pyarchon._p(off), kl, pyarchon._p(pos), total,
                                                      ctypes.cast(ctypes.byref(tot), ctypes.c_void_p))
                    assert rc == 0 and tot.value == total, (rc, tot.value, total)
                    lps.append(pyarchon.fm_stats().ms_query)
                model = (2 * st.steps - st.shared_steps) * (SUB_BYTES + 2 * LINE)
                row = dict(mib=mib, shape=shape, m=m, patterns=k, build_ms=build_ms, table_bytes=table_bytes, count_ms=count_ms,
                           patterns_per_s=k / (count_ms * 1e-3), steps=st.steps, shared_steps=st.shared_steps, model_bytes=model,
                           model_gbps=model / (count_ms * 1e-3) / 1e9, occurrences=int(occ.sum()), locate_patterns=kl,
                           located=total, locate_ms=lps[-1])
                print("%6d %-8s %4d %9.3f %9.3f %10.2f %9.1f %12d %12d %9.3f %9d %11d" % (
                    mib, shape, m, build_ms, count_ms, row["patterns_per_s"] / 1e6, row["model_gbps"], st.steps, st.shared_steps,
                    row["locate_ms"], kl, total))
                print(json.dumps(row))
                sys.stdout.flush()
                del p_t, o_t, lo_t, hi_t
            f.close()
            blk.close()
            del bwt_t, base_t
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
