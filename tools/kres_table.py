#!/usr/bin/env python3
"""One row per kernel from a compiler resource report, for comparing two builds of the library.

    hipcc <the Makefile's HIPFLAGS> -Rpass-analysis=kernel-resource-usage -shared -o /dev/null \
        dark-archon_amd/csrc/archon_hip.hip 2> report.log
    tools/kres_table.py report.log [file ...] > table.txt

With file names (repeats lz kmers maw entropy runs fm_ms fm_text analysis ...) only the kernels those headers define are
listed.  --rename OLD=NEW (repeatable) prints a kernel of the report under another name, so that a kernel that moved
between namespaces lines up with itself in a diff of two tables.  Rows are sorted by name: no GPU needed.
"""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds")]


def main():
    args = sys.argv[1:]
    renames = {}
    while "--rename" in args:
        i = args.index("--rename")
        old, new = args[i + 1].split("=")
        renames[old] = new
        del args[i:i + 2]
    log, files = args[0], set(args[1:])
    rows, cur = {}, None
    for line in open(log, errors="replace"):
        m = re.match(r"(?:.*/)?(\w+)\.hiph?:\d+:\d+: remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        src, body = m.groups()
        if body.startswith("Function Name: "):
            cur = None
            if files and src not in files:
                continue
            sym = body[len("Function Name: "):]
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*", "", name).replace("void ", "").replace("archon::", "")
            cur = rows.setdefault(renames.get(name, name), {})
        elif cur is not None:
            for key, short in FIELDS:
                if body.startswith(key + ": "):
                    cur[short] = body[len(key) + 2:]
    for name in sorted(rows):
        print("%-44s %s" % (name, " ".join("%s=%s" % (s, rows[name].get(s, "?")) for _, s in FIELDS)))


if __name__ == "__main__":
    main()
