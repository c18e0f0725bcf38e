"""CPU: archon_hip_test_route (include/archon_hip_test.h) at every edge of every route -- the return code and the exact text
it leaves in archon_hip_last_error.  The call touches no device.  A route's stored value has no getter: what a value does is
the GPU tests' business, what the call answers is pinned here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAGS = ("NO_ALIGNED", "NO_BREAK_ROUND", "NO_CHAINS", "NO_PACK", "NO_PAIR_CHAINS", "NO_PERIOD_HINT", "NO_PERIOD_STREAM", "NO_RANK_WRITER",
         "NO_TEXT_ROUNDS", "NO_MID", "NO_SHALLOW", "NO_CLOSED_FORM", "NO_REL_RECORDS", "FM_SAMPLE_WALK")
# stored as given, or clamped: no value is refused
FREE = ("FORCE_PATH", "SMALL_BLOCK", "ALIGNED_MIN", "REL_MIN_SEG", "KEY_BYTES", "INV_ROWS", "INV_SLAB", "INV_SBITS", "INV_WALK_WGS")
DELETED = ("NO_DEEP_HINT", "NO_PACK_STREAM", "NO_PERIOD_PROBE", "NO_PROBE")      # routes nothing set: gone with their branches
# a power of two in [lo, hi], or 0
POW2 = {"FM_SUB_ROWS": (16, 1024), "FM_SUPER_ROWS": (16, 65536), "REP_FAN": (2, 64), "LZ_FAN": (2, 64), "LZ_TILE": (2, 4096), "KMER_TILE": (4, 2048)}
# a value in [1, hi], or 0: the text behind "NAME=value", and whether a negative value is refused (LCP_CAP and LCP_WINDOW take it as 0)
RANGE = {
    "PASS_RANGES": (1024, " out of range [1, 1024]", True),
    "LCP_CAP": (4096, " out of range [1, 4096]", False),
    "LCP_WINDOW": (1 << 30, " out of range [1, 2^30]", False),
    "MS_CHUNK": (0xFFFFFFFF, ": not a chunk of 1 .. 2^32 - 1 bytes (0: the default)", True),
    "EDIT_TILE": (64, ": not a tile of 1 .. 64 ends (0: the default)", True),
    "EDIT_BATCH": (0x7FFFFFFF, ": not a batch of 1 .. 2^31 - 1 patterns (0: the budget's own)", True),
    "STRIDE_GRID": (2048, ": not a grid of 1 .. 2048 workgroups (0: the default)", True),
}
DOC_TILE = (64, 1 << 20, ": not a tile of 64 .. 2^20 rows, a multiple of 64 (0: the default)")


@pytest.fixture()
def route():
    import pyarchon
    L = pyarchon.lib()

    def call(name, value):
        rc = L.archon_hip_test_route(name.encode() if name is not None else None, value)
        return rc, L.archon_hip_last_error().decode()
    yield call
    assert L.archon_hip_test_route(b"RESET", 0) == 0          # no later test inherits a route


def accepted(route, name, value):
    rc, _ = route(name, value)
    assert rc == 0, (name, value)


def refused(route, name, value, text):
    import pyarchon
    rc, err = route(name, value)
    assert rc == pyarchon.E_ARG and err == text, (name, value, err)


def header_names():
    """the names in the first column of the header's table"""
    names = set()
    for line in open(os.path.join(ROOT, "include", "archon_hip_test.h")):
        m = re.match(r" \*   ([A-Z].*)", line)
        for tok in re.split(r"[ ,]+", m.group(1)) if m else ():
            if not re.fullmatch(r"[A-Z][A-Z0-9_]+", tok):
                break
            names.add(tok)
    return names


def test_every_route_is_covered_and_listed_in_the_header():
    import pyarchon
    here = set(FLAGS) | set(FREE) | set(POW2) | set(RANGE) | {"DOC_TILE"}
    assert set(pyarchon._ROUTE_NAMES) == here and len(pyarchon._ROUTE_NAMES) == len(here)
    assert header_names() == here | {"RESET"}


def test_flags_and_free_values(route):
    for name in FLAGS:
        for v in (1, 0, -1, 7):
            accepted(route, name, v)
    for name in FREE:
        for v in (0, 1, 2, 3, -1, -5, 1 << 20, 1 << 40):
            accepted(route, name, v)


@pytest.mark.parametrize("name", sorted(POW2))
def test_power_of_two_routes(route, name):
    lo, hi = POW2[name]
    text = "%s=%%d: not a power of two in [%d, %d]" % (name, lo, hi)
    for v in (lo, hi, 2 * lo, 0):
        accepted(route, name, v)
    for v in (lo // 2, 2 * hi, -1, -lo, lo + 1, hi - 1, 3 * lo):         # below, above, negative, no power of two inside
        refused(route, name, v, text % v)


@pytest.mark.parametrize("name", sorted(RANGE))
def test_range_routes(route, name):
    hi, tail, negative_refused = RANGE[name]
    for v in (1, hi, hi - 1, 2, 0):
        accepted(route, name, v)
    for v in (hi + 1, 2 * hi, 1 << 40):
        refused(route, name, v, "%s=%d%s" % (name, v, tail))
    for v in (-1, -hi):
        if negative_refused:
            refused(route, name, v, "%s=%d%s" % (name, v, tail))
        else:
            accepted(route, name, v)


def test_doc_tile(route):
    lo, hi, tail = DOC_TILE
    for v in (lo, hi, 2 * lo, hi - 64, 0):
        accepted(route, "DOC_TILE", v)
    for v in (lo - 1, 1, hi + 64, hi + 1, -1, -64, 100, lo + 1, hi - 1):  # below, above, negative, no multiple of 64 inside
        refused(route, "DOC_TILE", v, "DOC_TILE=%d%s" % (v, tail))


def test_reset_unknown_and_null(route):
    accepted(route, "RESET", 0)
    accepted(route, "RESET", 5)
    refused(route, "NO_SUCH_ROUTE", 1, "unknown route 'NO_SUCH_ROUTE'")
    refused(route, "no_chains", 1, "unknown route 'no_chains'")
    refused(route, "", 1, "unknown route ''")
    refused(route, None, 1, "null pointer")
    for name in DELETED:
        refused(route, name, 1, "unknown route '%s'" % name)
