"""Device time of the LCP attach and the matching statistics (the matching-statistics rows), with the
mirror build and the SMEM count pass of the same handle and patterns beside them as the yardstick.

Per block size and shape: the block and its forward (with its suffix array) on cuda:0, a sampled handle of its BWT with its
mirror and with the block's LCP array attached from the device (Block.fm_index(32, mirror=True, lcp=True)), the median of
--reps builds after one warm-up:
  ms_lcp     the LCP array of the resident block
  ms_attach  the guard and the minimum hierarchy over the attached array
  ms_mirror  the mirror from the resident text (reverse + forward + table)
Then, per pattern length m, --patterns substrings of x at seeded offsets, pattern i with i mod 4 random substitutions, one
call per rep:
  ms_query   archon_hip_fm_ms with rows and with lengths only (HIP events on the call's stream), median after one warm-up
  ms_count   the count pass of archon_hip_fm_smems over the same patterns, median
  steps, parents, probes per pattern byte; the SMEM search's steps (primary + mirror) per pattern byte
Every figure comes from archon_hip_get_fm_ms_stats and archon_hip_get_fm_mem_stats.

    python tools/fm_ms_time.py [--mib 16] [--shapes text,dna] [--lengths 100,1000] [--patterns 65536] [--out profiles/fm/fm_ms_time16.txt]
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


def substrings(x, rng, count, m):
    """count substrings of length m at seeded offsets, pattern i with i mod 4 random substitutions"""
    q = rng.integers(0, x.size - m + 1, count)
    p = x[q[:, None] + np.arange(m)[None, :]]
    for s in range(1, 4):
        rows = np.flatnonzero(np.arange(count) % 4 >= s)
        p[rows, rng.integers(0, m, rows.size)] = rng.integers(0, 256, rows.size, dtype=np.uint8)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="text,dna")
    ap.add_argument("--lengths", default="100,1000")
    ap.add_argument("--patterns", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm", "fm_ms_time16.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    vp = ctypes.c_void_p
    out = open(args.out, "w")

    def say(line):
        print(line)
        out.write(line + "\n")
        out.flush()

    count = args.patterns
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_prose(n, S.SEED_BASE + 6) if shape == "prose" else S.gen_shape(shape, n)
            blk = pyarchon.Block()
            blk.forward(x)
            f = blk.fm_index(32, mirror=True, lcp=True)
            lcp_ms, attach_ms, mirror_ms = [], [], []
            for _ in range(args.reps + 1):
                pyarchon._check(L.archon_hip_block_fm_mirror(blk.h, f.h))
                mirror_ms.append(pyarchon.fm_mem_stats().ms_mirror)
                pyarchon._check(L.archon_hip_block_fm_attach_lcp(blk.h, f.h))
                st = pyarchon.fm_ms_stats()
                lcp_ms.append(st.ms_lcp)
                attach_ms.append(st.ms_attach)
            row = dict(mib=mib, shape=shape, ms_lcp=statistics.median(lcp_ms[1:]), ms_attach=statistics.median(attach_ms[1:]),
                       ms_mirror=statistics.median(mirror_ms[1:]), lcp_bytes=st.lcp_bytes, mirror_bytes=pyarchon.fm_mem_stats().mirror_bytes,
                       fan=st.fan, levels=st.levels)
            say("%5d MiB %-7s lcp %.3f ms, attach %.3f ms (%.1f MiB, F = %d, %d levels); mirror %.3f ms (%.1f MiB)" % (
                mib, shape, row["ms_lcp"], row["ms_attach"], st.lcp_bytes / 2.0 ** 20, st.fan, st.levels, row["ms_mirror"],
                row["mirror_bytes"] / 2.0 ** 20))
            say(json.dumps(row))
            blk.close()
            say("%5s %-7s %5s %8s %9s %9s %9s %10s %10s %10s %10s" % ("MiB", "shape", "m", "pats", "steps/B", "parents/B", "probes/B", "query ms",
                                                                     "len-only", "smem count", "smem st/B"))
            for m in [int(v) for v in args.lengths.split(",")]:
                rng = np.random.default_rng(mib * 1000 + m * 10 + len(shape))
                p = substrings(x, rng, count, m)
                packed = np.concatenate([p.ravel(), np.zeros(64, np.uint8)])
                off = (np.arange(count + 1, dtype=np.uint64) * m).astype(np.uint32)
                del p
                total = count * m
                ln, lo, hi = np.zeros(total, np.uint32), np.zeros(total, np.uint32), np.zeros(total, np.uint32)
                nm, no = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
                tot = ctypes.c_uint64(0)
                tp = ctypes.cast(ctypes.byref(tot), vp)
                q_ms, l_ms, c_ms = [], [], []
                for _ in range(args.reps + 1):
                    rc = L.archon_hip_fm_ms(f.h, pyarchon._p(packed), pyarchon._p(off), count, pyarchon._p(ln), pyarchon._p(lo), pyarchon._p(hi))
                    assert rc == 0, L.archon_hip_last_error()
                    st = pyarchon.fm_ms_stats()
                    q_ms.append(st.ms_query)
                    rc = L.archon_hip_fm_ms(f.h, pyarchon._p(packed), pyarchon._p(off), count, pyarchon._p(ln), None, None)
                    assert rc == 0, L.archon_hip_last_error()
                    l_ms.append(pyarchon.fm_ms_stats().ms_query)
                    rc = L.archon_hip_fm_smems(f.h, pyarchon._p(packed), pyarchon._p(off), count, 1, pyarchon._p(nm), pyarchon._p(no), None, 0, tp)
                    assert rc == 0, L.archon_hip_last_error()
                    sm = pyarchon.fm_mem_stats()
                    c_ms.append(sm.ms_count)
                row = dict(mib=mib, shape=shape, m=m, patterns=count, pattern_bytes=st.pattern_bytes, steps_per_byte=st.steps / total,
                           parents_per_byte=st.parents / total, probes_per_byte=st.probes / total, matched_per_byte=st.matched / total,
                           longest=st.longest, ms_query=statistics.median(q_ms[1:]), ms_query_len_only=statistics.median(l_ms[1:]),
                           smems_ms_count=statistics.median(c_ms[1:]), smems_steps_per_byte=(sm.fwd_steps + sm.bwd_steps) / total,
                           smems_found=sm.found)
                say("%5d %-7s %5d %8d %9.3f %9.4f %9.3f %10.3f %10.3f %10.3f %10.3f" % (
                    mib, shape, m, count, row["steps_per_byte"], row["parents_per_byte"], row["probes_per_byte"], row["ms_query"],
                    row["ms_query_len_only"], row["smems_ms_count"], row["smems_steps_per_byte"]))
                say(json.dumps(row))
            f.close()
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
