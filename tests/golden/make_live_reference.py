#!/usr/bin/env python3
"""Generate tests/golden/live_reference.json by running THE REFERENCE ITSELF here.

Records what the reference binaries that oracle/Makefile builds (oracle/_ref/a7lms = a7's own findLMS,
oracle/_ref/a7ref_nt = a7 with sTracking=false) answer on the inputs of test_oracle.py's live-reference
tests (tests/oracle_binding.py: live_lms_inputs, LIVE_SHAPES): number of LMS items + digest of
count[256] || items, and SHA-256 of the little-endian P array and of the BWT with baseId.  The tests
regenerate the inputs; only outputs are stored.

    python tests/golden/make_live_reference.py        # needs oracle/_ref (make -C oracle with the reference tree)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "dark-archon_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import archon_synth as S  # noqa: E402
import oracle_binding as OB  # noqa: E402


def main():
    assert OB.ref_available("a7lms") and OB.ref_available("a7ref_nt"), "run `make -C oracle` first"
    lms = []
    for x in OB.live_lms_inputs():
        count, items = OB.run_ref_lms(x)
        lms.append({"n": int(x.size), "lms_n1": int(items.size), "sha256_lms": OB.lms_digest(count, items)})
    shapes = []
    for shape, n, block in OB.LIVE_SHAPES:
        r = OB.run_ref(S.gen_shape(shape, n, block=block), "a7ref_nt")
        assert r is not None and r["validate"] == 1, (shape, n, block)
        shapes.append({"shape": shape, "n": n, "block": block, "base_id": r["base"],
                       "sha256_P": OB.sha256_bytes(r["P"], "<u4"), "sha256_bwt": OB.sha256_bytes(r["bwt"])})
        print(shape, n, block, r["base"], flush=True)
    out = {"generator": "tests/golden/make_live_reference.py",
           "reference": "kvark/dark-archon bwt/a7 (-O3 -DNDEBUG, 64-bit); a7ref_nt = sTracking=false; a7lms = its findLMS",
           "lms": lms, "shapes": shapes}
    with open(os.path.join(HERE, "live_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", len(lms), "LMS inputs and", len(shapes), "shapes")


if __name__ == "__main__":
    main()
