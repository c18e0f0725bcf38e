"""What the STRIDE_GRID tests of the analysis families share (include/archon_hip_test.h): a stride kernel is launched with
min(work, 2048) workgroups, so a workgroup or wave goes round its loop a second time only above 4 Mi rows or 8192 patterns.
The route caps the grid: at 1 one workgroup (four waves) takes every tile and every pattern, each behind another on the same
wave; at 3 the trip counts are uneven, neighbouring tiles lie on different workgroups and the ragged last tile lands on a
workgroup that has done full ones.  The route changes no result and no counter.

N2, N_MAW and K2 are the smallest sizes at which the product's own grid of 2048 gives some workgroups a second trip."""
import numpy as np

GRIDS = (1, 3)
ENV = "ARCHON_STRIDE_GRID"

N2 = 2048 * 2048 + 3 * 2048 + 5         # 2052 tiles of 2048 rows: workgroups 0-3 take a second tile, the last one has 5 rows
N_MAW = 8192 * 256 + 5 * 256 + 7        # 8198 tiles of 256 rows: waves 0-5 take a second tile, the last one has 7 rows
K2 = 8192 + 13                          # patterns: waves 0-12 take a second one


def k2_patterns(x):
    """K2 patterns of 1-24 bytes: a third substrings of x, a third substrings with one byte changed, a third random printable"""
    n = x.size
    rng = np.random.default_rng(K2)
    pats = []
    for j in range(K2):
        m = int(rng.integers(1, 25))
        if j % 3 == 2:
            pats.append(rng.integers(32, 127, m, dtype=np.uint8).tobytes())
        else:
            q = int(rng.integers(0, n - m + 1))
            p = bytearray(x[q:q + m].tobytes())
            if j % 3 == 1:
                p[int(rng.integers(0, m))] ^= 1 + int(rng.integers(0, 255))
            pats.append(bytes(p))
    return pats


def counters(st):
    """every field of a stats record that the input defines: all but the ms_* times"""
    d = st.asdict() if hasattr(st, "asdict") else dict(st)
    return {k: v for k, v in d.items() if not k.startswith("ms_")}


def _bytes(a):
    if a is None:
        return None
    if isinstance(a, (bytes, bytearray)):
        return bytes(a)
    if isinstance(a, (list, tuple)):
        return [_bytes(v) for v in a]
    if isinstance(a, (int, float, str)):
        return a
    if hasattr(a, "asdict"):
        return counters(a)
    a = np.ascontiguousarray(a)
    return (a.dtype.str, a.shape, a.tobytes())


def same_under(monkeypatch, grid, call):
    """call() -> (results, stats records): once with the route unset, once with at most `grid` workgroups.  call() holds its own
    checks against the CPU reference, so both runs pass them; the results are byte-equal and every counter is equal.  Returns
    the routed run's results"""
    monkeypatch.delenv(ENV, raising=False)
    base_out, base_st = call()
    monkeypatch.setenv(ENV, str(grid))
    out, st = call()
    monkeypatch.delenv(ENV, raising=False)
    equal = _bytes(out) == _bytes(base_out)         # (compared outside the assert: pytest would diff megabytes)
    assert equal, "the records differ under %s=%d" % (ENV, grid)
    if not isinstance(st, (list, tuple)):
        st, base_st = [st], [base_st]
    assert len(st) == len(base_st)
    for a, b in zip(st, base_st):
        assert counters(a) == counters(b), "the counters differ under %s=%d" % (ENV, grid)
    return out
