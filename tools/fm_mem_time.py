"""Device time of the mirror build and the SMEM search (the SMEM rows) at block sizes a user runs.

Per block size and shape: the block and its forward on cuda:0, a handle of its BWT, and the mirror by both
routes (from the handle's own BWT: inverse + reverse + forward + table; from the resident text: without the inverse), each
the median of --reps builds after one warm-up.  Then, per pattern length m and kind of pattern -- substrings of x at seeded
offsets with 0, 2 or 5 random substitutions, and (at the middle length) chimeras of two substrings -- and per batch size, one
call with room for every SMEM per rep:
  count     ms_count: the count pass (HIP events on the call's stream), median of --reps after one warm-up
  emit      ms_emit: the emit pass, the identical search again writing the SMEMs, median
  per step  ns per rank step of the whole count pass (the batch's waves run side by side); steps (primary + mirror) and
            SMEMs per pattern
Every figure comes from archon_hip_get_fm_mem_stats.

    python tools/fm_mem_time.py [--mib 16,256] [--shapes dna,random,text,prose] [--lengths 32,100,250] [--batches 65536,1048576]
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


def substrings(x, rng, count, m, subs):
    """count substrings of length m at seeded offsets with `subs` random substitutions each: (packed uint8, uint32 offsets)"""
    q = rng.integers(0, x.size - m + 1, count)
    p = x[q[:, None] + np.arange(m)[None, :]]
    for _ in range(subs):
        p[np.arange(count), rng.integers(0, m, count)] = rng.integers(0, 256, count, dtype=np.uint8)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16,256")
    ap.add_argument("--shapes", default="dna,random,text,prose")
    ap.add_argument("--lengths", default="32,100,250")
    ap.add_argument("--subs", default="0,2,5")
    ap.add_argument("--batches", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    vp = ctypes.c_void_p
    lengths = [int(v) for v in args.lengths.split(",")]
    mid = lengths[len(lengths) // 2]

    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_prose(n, S.SEED_BASE + 6) if shape == "prose" else S.gen_shape(shape, n)
            blk = pyarchon.Block()
            _, base = blk.forward(x, want_sa=False)
            f = pyarchon.FmIndex(blk.read_bwt(), base)
            own, text = [], []
            for _ in range(args.reps + 1):
                f.mirror()
                own.append(pyarchon.fm_mem_stats().ms_mirror)
                pyarchon._check(L.archon_hip_block_fm_mirror(blk.h, f.h))
                text.append(pyarchon.fm_mem_stats().ms_mirror)
            st = pyarchon.fm_mem_stats()
            row = dict(mib=mib, shape=shape, mirror_own_bwt_ms=statistics.median(own[1:]), mirror_text_ms=statistics.median(text[1:]),
                       mirror_bytes=st.mirror_bytes, mirror_launches=st.kernel_launches)
            print("%5d MiB %-7s mirror: %.3f ms from the handle's BWT, %.3f ms from the text, %.1f MiB" % (
                mib, shape, row["mirror_own_bwt_ms"], row["mirror_text_ms"], st.mirror_bytes / 2.0 ** 20))
            print(json.dumps(row))
            blk.close()
            print("%5s %-7s %4s %-8s %8s %9s %9s %9s %9s %9s %9s" % ("MiB", "shape", "m", "kind", "pats", "fwd/pat", "bwd/pat", "smems/pat",
                                                                    "count ms", "emit ms", "ns/step"))
            kinds = [(m, "sub%d" % s, s) for m in lengths for s in [int(v) for v in args.subs.split(",")]] + [(mid, "chimera", -1)]
            for m, kind, subs in kinds:
                for count in [int(v) for v in args.batches.split(",")]:
                    rng = np.random.default_rng(mib * 1000 + m * 10 + subs + len(shape))
                    if subs >= 0:
                        p = substrings(x, rng, count, m, subs)
                    else:
                        p = np.concatenate([substrings(x, rng, count, m // 2, 0), substrings(x, rng, count, m - m // 2, 0)], axis=1)
                    packed = np.concatenate([p.ravel(), np.zeros(64, np.uint8)])
                    off = (np.arange(count + 1, dtype=np.uint64) * m).astype(np.uint32)
                    del p
                    nm, no = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
                    tot = ctypes.c_uint64(0)
                    tp = ctypes.cast(ctypes.byref(tot), vp)
                    assert L.archon_hip_fm_smems(f.h, pyarchon._p(packed), pyarchon._p(off), count, 1, pyarchon._p(nm), pyarchon._p(no), None, 0, tp) == 0
                    mems = np.zeros(max(tot.value, 1), pyarchon.FM_MEM)
                    cms, ems = [], []
                    for _ in range(args.reps + 1):
                        rc = L.archon_hip_fm_smems(f.h, pyarchon._p(packed), pyarchon._p(off), count, 1, pyarchon._p(nm), pyarchon._p(no),
                                                   pyarchon._p(mems), mems.size, tp)
                        assert rc == 0, L.archon_hip_last_error()
                        st = pyarchon.fm_mem_stats()
                        cms.append(st.ms_count)
                        ems.append(st.ms_emit)
                    c_ms, e_ms = statistics.median(cms[1:]), statistics.median(ems[1:])
                    steps = st.fwd_steps + st.bwd_steps
                    row = dict(mib=mib, shape=shape, m=m, kind=kind, patterns=count, fwd_steps_per_pattern=st.fwd_steps / count,
                               bwd_steps_per_pattern=st.bwd_steps / count, smems_per_pattern=st.found / count, count_ms=c_ms, emit_ms=e_ms,
                               ns_per_step=c_ms * 1e6 / max(steps, 1), ns_per_step_emit=e_ms * 1e6 / max(steps, 1), occurrences=st.occurrences)
                    print("%5d %-7s %4d %-8s %8d %9.1f %9.1f %9.2f %9.3f %9.3f %9.3f" % (
                        mib, shape, m, kind, count, row["fwd_steps_per_pattern"], row["bwd_steps_per_pattern"], row["smems_per_pattern"], c_ms,
                        e_ms, row["ns_per_step"]))
                    print(json.dumps(row))
                    sys.stdout.flush()
            f.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
