"""Device time of the sampled FM index (the sampled FM rows): sample builds, locate and extract at block
sizes a user runs.

Per block size, shape and rate: the block and its forward with the SA on cuda:0, then
  from SA   Block.fm_index(rate) over the resident SA (archon_hip_block_fm_index, route 1): ms_build of the samples, median of
            --reps after one warm-up
  by walk   the same with the walk route forced (ARCHON_FM_SAMPLE_WALK=1, route 2): ms_build, median
  locate    --patterns substrings of --length bytes at seeded offsets, the first of them holding at most --locate-max
            occurrences (archon_hip_fm_locate): ms_query of the LF walks (the count before them is timed by tools/fm_time.py),
            median; ns per occurrence, LF steps per occurrence, the longest walk
  extract   --requests requests of --extract-len bytes at seeded starts (archon_hip_fm_extract): ms_query of the checks, the
            segment sums and the walks, median; ns per byte and LF steps per byte
Every figure is a HIP-event time of the call's stream (archon_hip_get_fm_walk_stats).

    python tools/fm_walk_time.py [--mib 16,256] [--shapes random,text,dna,prose] [--rates 32] [--patterns 65536] [--length 16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16,256")
    ap.add_argument("--shapes", default="random,text,dna,prose")
    ap.add_argument("--rates", default="32")
    ap.add_argument("--patterns", type=int, default=1 << 16)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--locate-max", type=int, default=1 << 20)
    ap.add_argument("--requests", type=int, default=1 << 16)
    ap.add_argument("--extract-len", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    vp = ctypes.c_void_p

    print("%6s %-8s %6s %9s %9s %9s %9s %9s %9s %7s %9s %9s %9s" % ("MiB", "shape", "rate", "sa ms", "walk ms", "KiB", "located", "loc ms",
                                                                "ns/occ", "steps", "ext ms", "ns/byte", "steps/B"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_shape(shape, n)
            blk = pyarchon.Block()
            blk.forward(x, want_sa=True)
            rng = np.random.default_rng(mib * 1000 + len(shape))
            m = args.length
            q = rng.integers(0, n - m + 1, args.patterns)
            pats = [x[a:a + m].tobytes() for a in q]
            rq = rng.integers(0, n - args.extract_len + 1, args.requests).astype(np.uint32)
            lens = np.full(args.requests, args.extract_len, np.uint32)
            for rate in [int(v) for v in args.rates.split(",")]:
                times = {}
                for route, env in (("sa", None), ("walk", "1")):
                    if env:
                        os.environ["ARCHON_FM_SAMPLE_WALK"] = env
                    ms = []
                    for _ in range(args.reps + 1):
                        f = blk.fm_index(rate)
                        st = pyarchon.fm_walk_stats()
                        assert st.route == (1 if route == "sa" else 2)
                        ms.append(st.ms_build)
                        sample_bytes = st.sample_bytes
                        f.close()
                    os.environ.pop("ARCHON_FM_SAMPLE_WALK", None)
                    times[route] = statistics.median(ms[1:])
                f = blk.fm_index(rate)
                lo, hi = f.count(pats)
                cum = np.cumsum(hi.astype(np.int64) - lo)
                kl = int(np.searchsorted(cum, args.locate_max, side="right"))
                total = int(cum[kl - 1]) if kl else 0
                packed, off = pyarchon._pack_patterns(pats[:kl])
                pos = np.empty(max(total, 1), np.uint32)
                tot = ctypes.c_uint64(0)
                lms = []
                for _ in range(args.reps + 1):
                    rc = L.archon_hip_fm_locate(f.h, pyarchon._p(packed), pyarchon._p(off), kl, pyarchon._p(pos), total,
                                                ctypes.cast(ctypes.byref(tot), vp))
                    assert rc == 0 and tot.value == total, (rc, tot.value, total)
                    lst = pyarchon.fm_walk_stats()
                    lms.append(lst.ms_query)
                loc_ms = statistics.median(lms[1:])
                eoff = np.zeros(args.requests + 1, np.uint32)
                np.cumsum(lens, out=eoff[1:])
                out = np.empty(int(eoff[-1]), np.uint8)
                ems = []
                for _ in range(args.reps + 1):
                    assert L.archon_hip_fm_extract(f.h, pyarchon._p(rq), pyarchon._p(eoff), args.requests, pyarchon._p(out)) == 0
                    est = pyarchon.fm_walk_stats()
                    ems.append(est.ms_query)
                ext_ms = statistics.median(ems[1:])
                assert out[:args.extract_len].tobytes() == x[rq[0]:rq[0] + args.extract_len].tobytes()
                f.close()
                nbytes = int(eoff[-1])
                row = dict(mib=mib, shape=shape, rate=rate, from_sa_ms=times["sa"], by_walk_ms=times["walk"], sample_bytes=sample_bytes,
                           located=total, locate_patterns=kl, locate_ms=loc_ms, ns_per_occ=loc_ms * 1e6 / max(total, 1),
                           steps_per_occ=lst.lf_steps / max(total, 1), max_walk=lst.max_walk, extract_ms=ext_ms, extract_bytes=nbytes,
                           extract_segments=est.walks, ns_per_byte=ext_ms * 1e6 / nbytes, steps_per_byte=est.lf_steps / nbytes)
                print("%6d %-8s %6d %9.3f %9.3f %9.0f %9d %9.3f %9.2f %7.2f %9.3f %9.2f %9.2f" % (
                    mib, shape, rate, times["sa"], times["walk"], sample_bytes / 1024, total, loc_ms, row["ns_per_occ"], row["steps_per_occ"],
                    ext_ms, row["ns_per_byte"], row["steps_per_byte"]))
                print(json.dumps(row))
                sys.stdout.flush()
            blk.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
