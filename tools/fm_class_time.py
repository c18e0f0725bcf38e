"""Device time of the class search (the class search row): the width pass, the count and the emit pass of
archon_hip_block_fm_classes at a block size a user runs, beside archon_hip_block_fm_count on the same block and patterns.

Per block size and pattern length m, --patterns patterns that are substrings of x at seeded offsets, under three tables:
  identity   on a text and a DNA block: the call is fm_count; fm_count's ms_query on the same patterns in the same session
  fold       classes_fold_case on the text block: every letter accepts both of its cases
  iupac      classes_iupac on the DNA block, one N per 16 pattern bytes
Per rep, one call with room for every hit:
  width     ms_width: the pass that finds the widths and the empty classes (HIP events on the call's stream)
  count     ms_count: the count pass, median of --reps after one warm-up
  emit      ms_emit: the emit pass, the identical search again writing the hits, median
  per node  ns per node (expansions + steps) of the whole count pass; the largest width of the call (it sizes the LDS stacks)
Every figure comes from archon_hip_get_fm_class_stats and archon_hip_get_fm_stats.  The lines also go to --out.

    python tools/fm_class_time.py [--mib 16] [--lengths 32,100] [--patterns 65536] [--out profiles/fm/fm_class_time16.txt]
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


def patterns(x, rng, count, m, every_n=0):
    out = []
    for q in rng.integers(0, x.size - m + 1, count):
        p = x[q:q + m].copy()
        if every_n:
            p[int(rng.integers(0, every_n))::every_n] = ord("N")
        out.append(p.tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--lengths", default="32,100")
    ap.add_argument("--patterns", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    L = pyarchon.lib()
    vp = ctypes.c_void_p
    out_path = args.out or os.path.join(ROOT, "profiles", "fm", "fm_class_time%s.txt" % args.mib.replace(",", "_"))
    out = open(out_path, "w")

    def say(line):
        print(line)
        out.write(line + "\n")
        out.flush()
        sys.stdout.flush()

    tables = {"identity": pyarchon.classes_identity(), "fold": pyarchon.classes_fold_case(), "iupac": pyarchon.classes_iupac()}
    say("%5s %-5s %-8s %4s %6s %6s %9s %10s %9s %9s %9s %9s %9s %9s" % ("MiB", "shape", "table", "m", "pats", "width", "exp/pat", "steps/pat",
                                                                       "width ms", "count ms", "emit ms", "ns/node", "hits", "fm_count"))
    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape, names in (("text", ("identity", "fold")), ("dna", ("identity", "iupac"))):
            x = S.gen_shape(shape, n)
            blk = pyarchon.Block()
            blk.forward(x, want_sa=False)
            blk.fm_count([x[:4].tobytes()])
            for m in [int(v) for v in args.lengths.split(",")]:
                for name in names:
                    rng = np.random.default_rng(mib * 1000 + m * 10 + len(shape))
                    count = args.patterns
                    pats = patterns(x, rng, count, m, 16 if name == "iupac" else 0)
                    table = tables[name]
                    packed, off = pyarchon._pack_patterns(pats)
                    nh, no = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
                    tot = ctypes.c_uint64(0)
                    tp = ctypes.cast(ctypes.byref(tot), vp)
                    call = lambda hits, cap: L.archon_hip_block_fm_classes(blk.h, pyarchon._p(packed), pyarchon._p(off), count, pyarchon._p(table),   # noqa: E731
                                                                           pyarchon._p(nh), pyarchon._p(no), hits, cap, tp)
                    assert call(None, 0) == 0, L.archon_hip_last_error()
                    hits = np.zeros(max(tot.value, 1), pyarchon.FM_HIT)
                    wms, cms, ems, qms = [], [], [], []
                    for _ in range(args.reps + 1):
                        assert call(pyarchon._p(hits), hits.size) == 0, L.archon_hip_last_error()
                        st = pyarchon.fm_class_stats()
                        wms.append(st.ms_width)
                        cms.append(st.ms_count)
                        ems.append(st.ms_emit)
                        if name == "identity":
                            lo, hi = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
                            assert L.archon_hip_block_fm_count(blk.h, pyarchon._p(packed), pyarchon._p(off), count, pyarchon._p(lo), pyarchon._p(hi)) == 0
                            fst = pyarchon.fm_stats()
                            assert fst.steps == st.steps and st.expansions == 0
                            qms.append(fst.ms_query)
                    w_ms, c_ms, e_ms = (statistics.median(v[1:]) for v in (wms, cms, ems))
                    q_ms = statistics.median(qms[1:]) if qms else None
                    nodes = st.expansions + st.steps
                    row = dict(mib=mib, shape=shape, table=name, m=m, patterns=count, max_width=st.max_width,
                               expansions_per_pattern=st.expansions / count, steps_per_pattern=st.steps / count, width_ms=w_ms, count_ms=c_ms,
                               emit_ms=e_ms, ns_per_node=c_ms * 1e6 / max(nodes, 1), hits=st.hits, occurrences=st.occurrences, nodes=nodes,
                               fm_count_ms=q_ms)
                    say("%5d %-5s %-8s %4d %6d %6d %9.1f %10.1f %9.3f %9.3f %9.3f %9.2f %9d %9s" % (
                        mib, shape, name, m, count, st.max_width, row["expansions_per_pattern"], row["steps_per_pattern"], w_ms, c_ms, e_ms,
                        row["ns_per_node"], st.hits, "%.3f" % q_ms if q_ms is not None else "-"))
                    say(json.dumps(row))
            blk.close()
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
