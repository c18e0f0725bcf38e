"""Census of the general stage: one forward (with the suffix array) per case of tests/forward_cases.py, CENSUS_CASES, on the
routes the case names; one line per case with the statistics that say which launches, waits and rounds the driver made.
The suffix array is checked on the GPU (validate), not against the CPU oracle: the order is the forward tests' job.

    python tools/general_census.py [--cases a,b,...] [--out FILE]

Small blocks take the streaming machinery (ARCHON_SMALL_BLOCK=0), as they do in the test suite."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forward_cases as F
import pyarchon


def line(case, env, n, st):
    routes = ",".join("%s=%s" % (k[len("ARCHON_"):], v) for k, v in sorted(env.items())) or "-"
    return "%-30s n=%-9d %-60s %s" % (case, n, routes, " ".join("%s=%d" % (f, st[f]) for f in F.CENSUS_FIELDS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    want = set(args.cases.split(",")) if args.cases else None
    os.environ["ARCHON_SMALL_BLOCK"] = "0"
    out = open(args.out, "w") if args.out else None
    primer = F.CENSUS_BLOCKS["random_64ki"]()
    name, x = None, None
    for case, block, env in F.CENSUS_CASES:
        if want is not None and case not in want:
            continue
        if block != name:
            name, x = block, F.CENSUS_BLOCKS[block]()       # (one block at a time: consecutive cases share theirs)
        st, sa = F.census_run(pyarchon, x, env, primer)
        if not pyarchon.validate(x, sa):
            raise SystemExit("%s: the suffix array does not validate" % case)
        text = line(case, env, x.size, st)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()


if __name__ == "__main__":
    main()
