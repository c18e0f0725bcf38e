"""Device time of the matching statistics of a long text and of its relative LZ parse, per chunk size.

Per block size and shape: the block and its forward (with its suffix array) on cuda:0, a handle of its BWT with the block's LCP
array and suffix array attached from the device (Block.fm_index(32, lcp=True, sa=True)).  Three texts of the block's size:
  unrelated  data of the same kind from another seed
  mutated    a copy of the block with one substitution per ~1000 bytes
  itself     the block: every chunk full, the sweep one chain
Per text and chunk C (test route MS_CHUNK), the median of --reps calls of archon_hip_fm_ms_text after one warm-up:
  walk, sweep, fix   device time of the three steps (HIP events on the call's stream), and their total
  saturated, full chunks, runs, the longest run; probes of sa and lcp per text byte
and one archon_hip_fm_rlz (counting only) at each C for the parse's time and the number of phrases.
Every figure comes from archon_hip_get_fm_text_stats.

--compare MIB times, once each, the new call on a text of MIB MiB (the mutated copy's first MIB) at the default chunk and
archon_hip_fm_ms on the same text as a single pattern -- one wave -- and appends both figures to --out.

    python tools/fm_text_time.py [--mib 16] [--shapes text,dna] [--chunks 256,1024,4096,16384] [--out profiles/fm/fm_text_time16.txt]
    python tools/fm_text_time.py --compare 1 [--mib 16] [--shapes text] --out profiles/fm/fm_text_time16.txt
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))


def shape_of(S, shape, n, other=False):
    if shape == "dna":
        return S.gen_dna(n, S.SEED_BASE + 40) if other else S.gen_dna(n)
    if shape == "text":
        return S.gen_text(n, S.SEED_BASE + 41) if other else S.gen_text(n)
    if other:
        raise SystemExit("no unrelated data for shape %s" % shape)
    return S.gen_shape(shape, n)


def mutated(x, rng):
    """a copy with one substitution per ~1000 bytes"""
    y = x.copy()
    at = np.cumsum(rng.integers(500, 1500, x.size // 900))
    at = at[at < x.size]
    y[at] = rng.integers(0, 256, at.size, dtype=np.uint8)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="16")
    ap.add_argument("--shapes", default="text,dna")
    ap.add_argument("--chunks", default="256,1024,4096,16384")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--compare", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm", "fm_text_time16.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import archon_synth as S
    import pyarchon
    out = open(args.out, "a" if args.compare else "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for mib in [int(v) for v in args.mib.split(",")]:
        n = mib << 20
        for shape in args.shapes.split(","):
            x = shape_of(S, shape, n)
            blk = pyarchon.Block()
            blk.forward(x)
            f = blk.fm_index(32, lcp=True, sa=True)
            st = pyarchon.fm_text_stats()
            blk.close()
            rng = np.random.default_rng(mib * 1000 + len(shape))
            if args.compare:
                m = args.compare << 20
                text = mutated(x, rng)[:m]
                os.environ.pop("ARCHON_MS_CHUNK", None)
                f.ms_text(text, rows=False)
                f.ms_text(text, rows=False)
                t = pyarchon.fm_text_stats()
                new_ms = t.ms_walk + t.ms_sweep + t.ms_fix
                f.ms([text], rows=False)
                one_ms = pyarchon.fm_ms_stats().ms_query
                row = dict(mib=mib, shape=shape, text_mib=args.compare, chunk=t.chunk, ms_text_total=new_ms, ms_single_pattern=one_ms,
                           ratio=one_ms / new_ms if new_ms else 0.0)
                say("%5d MiB %-5s a mutated text of %d MiB: fm_ms_text at C = %d %.3f ms, fm_ms as one pattern on one wave %.3f ms (%.0f x)" % (
                    mib, shape, args.compare, t.chunk, new_ms, one_ms, row["ratio"]))
                say(json.dumps(row))
                f.close()
                continue
            say("%5d MiB %-5s sa + isa %.1f MiB, lcp F = %d, %d levels" % (mib, shape, st.sa_bytes / 2.0 ** 20, st.fan, st.levels))
            say("%5s %-5s %-9s %6s %9s %9s %9s %9s %10s %8s %6s %8s %8s %8s %9s %10s" % (
                "MiB", "shape", "text", "C", "walk ms", "sweep ms", "fix ms", "total ms", "saturated", "full", "runs", "longest", "sa pr/B",
                "lcp pr/B", "parse ms", "phrases"))
            texts = (("unrelated", shape_of(S, shape, n, other=True)), ("mutated", mutated(x, rng)), ("itself", x))
            for name, text in texts:
                for C in [int(v) for v in args.chunks.split(",")]:
                    os.environ["ARCHON_MS_CHUNK"] = str(C)
                    walk, sweep, fix = [], [], []
                    for _ in range(args.reps + 1):
                        f.ms_text(text, rows=False)
                        t = pyarchon.fm_text_stats()
                        walk.append(t.ms_walk)
                        sweep.append(t.ms_sweep)
                        fix.append(t.ms_fix)
                    phrases = f.rlz(text, count_only=True)
                    p = pyarchon.fm_text_stats()
                    row = dict(mib=mib, shape=shape, text=name, m=int(text.size), chunk=C, chunks=t.chunks, ms_walk=statistics.median(walk[1:]),
                               ms_sweep=statistics.median(sweep[1:]), ms_fix=statistics.median(fix[1:]), saturated=t.saturated,
                               full_chunks=t.full_chunks, runs=t.runs, longest_run=t.longest_run, sa_probes_per_byte=t.sa_probes / text.size,
                               lcp_probes_per_byte=t.lcp_probes / text.size, matched_per_byte=t.matched / text.size, longest=t.longest,
                               ms_parse=p.ms_parse, phrases=int(phrases), kernel_launches_rlz=p.kernel_launches)
                    row["ms_total"] = row["ms_walk"] + row["ms_sweep"] + row["ms_fix"]
                    say("%5d %-5s %-9s %6d %9.3f %9.3f %9.3f %9.3f %10d %8d %6d %8d %8.3f %8.3f %9.3f %10d" % (
                        mib, shape, name, C, row["ms_walk"], row["ms_sweep"], row["ms_fix"], row["ms_total"], t.saturated, t.full_chunks, t.runs,
                        t.longest_run, row["sa_probes_per_byte"], row["lcp_probes_per_byte"], row["ms_parse"], phrases))
                    say(json.dumps(row))
            os.environ.pop("ARCHON_MS_CHUNK", None)
            f.close()
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
