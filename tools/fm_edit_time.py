"""Device time of the edit-distance search (the edit-distance row), stage by stage, with the
substitution-only search of the same patterns and the bare count + locate of the pieces beside it as context.

Per block size and shape: the block and its forward (with its suffix array) on cuda:0 and a sampled handle of its BWT
(Block.fm_index(32)).  Per pattern length m and K: --patterns cuts of x at seeded offsets, each with K random edits
(substitution, insertion or deletion), one call per rep, the median of --reps calls after one warm-up:
  block    Block.fm_edit: ms_seed (pieces, count, locate from the SA, marks, sweep), ms_count, ms_emit, and the whole call on
           the host's clock around the C call (uploads, waits and the copy of the hits included)
  handle   FmIndex.edit of the first --handle-patterns patterns: ms_seed (locate by the LF walk), ms_extract, ms_count, ms_emit, call
  approx   Block.fm_approx at the same K (substitutions only) on the first --approx-patterns patterns where K <= 2: count + emit
  pieces   Block.fm_locate of the K + 1 pieces of every pattern alone: the seed stage's floor (count + locate kernels)
Every stage figure comes from archon_hip_get_fm_edit_stats, _get_fm_approx_stats and _get_fm_stats (HIP events).

    python tools/fm_edit_time.py [--mib 16] [--shapes text,dna] [--lengths 32,100] [--errors 1,2,4] [--patterns 65536]
                                 [--out profiles/fm/fm_edit_time16.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def edited(x, rng, count, m, K):
    """count patterns of m bytes: cuts of x with K random edits each (a substitution, an insertion or a deletion)"""
    q = rng.integers(0, x.size - m - K, count)
    ops = rng.integers(0, 3, (count, K))
    at = rng.integers(0, m, (count, K))
    val = rng.integers(0, 256, (count, K), dtype=np.uint8)
    out = []
    for i in range(count):
        p = bytearray(x[q[i]:q[i] + m + K].tobytes())
        for op, a, v in zip(ops[i], at[i], val[i]):
            if op == 0:
                p[a] = v
            elif op == 1:
                p.insert(a, v)
            else:
                del p[a]
        out.append(bytes(p[:m]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="text,dna")
    ap.add_argument("--lengths", default="32,100")
    ap.add_argument("--errors", default="1,2,4")
    ap.add_argument("--patterns", type=int, default=65536)
    ap.add_argument("--handle-patterns", type=int, default=4096)
    ap.add_argument("--approx-patterns", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm", "fm_edit_time16.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    out = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def timed(call, stats, fields):
        """medians of the stats' fields and of the call's host time over --reps calls after one warm-up; the last record"""
        rows, wall, st = [], [], None
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = stats()
            rows.append([getattr(st, k) for k in fields])
        med = {k: statistics.median(r[i] for r in rows[1:]) for i, k in enumerate(fields)}
        med["ms_call"] = statistics.median(wall[1:])
        return med, st

    L = pyarchon.lib()

    def edit_call(fn, handle, pats, K):
        """the C call over patterns packed once and a hit array sized by a counting call"""
        packed, off = pyarchon._pack_patterns(pats)
        nh = np.zeros(len(pats), np.uint32)
        tot = ctypes.c_uint64(0)
        tp = ctypes.cast(ctypes.byref(tot), ctypes.c_void_p)
        pyarchon._check(fn(handle, pyarchon._p(packed), pyarchon._p(off), len(pats), K, pyarchon._p(nh), None, 0, tp))
        hits = np.zeros(max(tot.value, 1), pyarchon.FM_EDIT)
        return lambda: pyarchon._check(fn(handle, pyarchon._p(packed), pyarchon._p(off), len(pats), K, pyarchon._p(nh), pyarchon._p(hits), hits.size, tp))

    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = S.gen_prose(n, S.SEED_BASE + 6) if shape == "prose" else S.gen_shape(shape, n)
            blk = pyarchon.Block()
            blk.forward(x)
            f = blk.fm_index(32)
            blk.fm_count([b"a"])
            for m in [int(v) for v in args.lengths.split(",")]:
                for K in [int(v) for v in args.errors.split(",")]:
                    rng = np.random.default_rng(mib * 1000 + m * 10 + K + len(shape))
                    pats = edited(x, rng, args.patterns, m, K)
                    med, st = timed(edit_call(L.archon_hip_block_fm_edit, blk.h, pats, K), pyarchon.fm_edit_stats, ("ms_seed", "ms_count", "ms_emit"))
                    row = dict(mib=mib, shape=shape, m=m, K=K, form="block", patterns=len(pats), tile=st.tile, batches=st.batches,
                               seed_rows=st.seed_rows, tiles=st.tiles, rows=st.rows, hits=st.hits, launches=st.kernel_launches,
                               host_syncs=st.host_syncs, **med)
                    say("%4d MiB %-5s m %3d K %d block   %6d pats %3d batches: seed %9.3f count %8.3f emit %8.3f call %9.3f ms; %d seed rows, %d tiles, %d hits"
                        % (mib, shape, m, K, len(pats), st.batches, med["ms_seed"], med["ms_count"], med["ms_emit"], med["ms_call"], st.seed_rows,
                           st.tiles, st.hits))
                    say(json.dumps(row))
                    # the pieces alone: count + locate from the SA (where their starts fit a host array of 512 MiB)
                    if st.seed_rows <= 1 << 27:
                        o = [i * m // (K + 1) for i in range(K + 2)]
                        pieces = [p[o[i]:o[i + 1]] for p in pats for i in range(K + 1)]
                        med, fst = timed(lambda: blk.fm_locate(pieces), pyarchon.fm_stats, ("ms_query",))
                        say("%4d MiB %-5s m %3d K %d pieces  %6d pieces: count + locate %9.3f ms" % (mib, shape, m, K, len(pieces), med["ms_query"]))
                        say(json.dumps(dict(mib=mib, shape=shape, m=m, K=K, form="pieces", pieces=len(pieces), ms_query=med["ms_query"])))
                        del pieces
                    if K <= 2:
                        sub = pats[:args.handle_patterns]
                        med, st = timed(edit_call(L.archon_hip_fm_edit, f.h, sub, K), pyarchon.fm_edit_stats, ("ms_seed", "ms_extract", "ms_count", "ms_emit"))
                        say("%4d MiB %-5s m %3d K %d handle  %6d pats %3d batches: seed %9.3f extract %9.3f count %8.3f emit %8.3f call %9.3f ms; %d LF steps"
                            % (mib, shape, m, K, len(sub), st.batches, med["ms_seed"], med["ms_extract"], med["ms_count"], med["ms_emit"], med["ms_call"],
                               st.lf_steps))
                        say(json.dumps(dict(mib=mib, shape=shape, m=m, K=K, form="handle", patterns=len(sub), batches=st.batches, seed_rows=st.seed_rows,
                                            tiles=st.tiles, hits=st.hits, lf_steps=st.lf_steps, **med)))
                        sub = pats if (K == 1 or shape == "dna") else pats[:args.approx_patterns]
                        med, ast = timed(lambda: blk.fm_approx(sub, K), pyarchon.fm_approx_stats, ("ms_count", "ms_emit"))
                        say("%4d MiB %-5s m %3d K %d approx  %6d pats: count %9.3f emit %9.3f call %9.3f ms; %d hits (substitutions only)"
                            % (mib, shape, m, K, len(sub), med["ms_count"], med["ms_emit"], med["ms_call"], ast.hits))
                        say(json.dumps(dict(mib=mib, shape=shape, m=m, K=K, form="approx", patterns=len(sub), hits=ast.hits, **med)))
            f.close()
            blk.close()
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
