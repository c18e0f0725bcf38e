"""CPU: the oracle (oracle/archon_oracle.c) is pinned against the reference's answers.

  * the ten known answers of SURVEY.md 8(a0)
  * the brute-force statement of the definition (a7 sufCompare) on exhaustive small alphabets
  * tests/golden/golden.json -- outputs of the reference a7 binaries run in the development
    container (generator: tests/golden/make_golden.py)
  * tests/golden/live_reference.json -- the reference's answers on further seeds (make_live_reference.py), and,
    when oracle/_ref is present (development container), the live reference binaries on the same inputs
"""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import archon_synth as S
import oracle_binding as OB

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))
LIVE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "live_reference.json")))


def test_known_answers(oracle):
    for ka in GOLDEN["known_answers_survey_8a0"]:
        x = np.frombuffer(bytes.fromhex(ka["x_hex"]), np.uint8)
        for brute in (True, False):
            P = oracle.sa(x, brute=brute)
            bwt, base = oracle.sa_to_bwt(x, P)
            assert list(P) == ka["P"]
            assert bwt.tobytes().hex() == ka["bwt_hex"] and base == ka["base_id"]
        assert oracle.validate(x, P) and oracle.check_sorted(x, P)


@pytest.mark.parametrize("alpha,maxlen", [((0, 1), 11), ((0, 1, 2), 7), ((254, 255), 9), ((0, 128, 255), 6)])
def test_exhaustive_vs_definition(oracle, alpha, maxlen):
    for n in range(1, maxlen + 1):
        for t in itertools.product(alpha, repeat=n):
            x = np.array(t, np.uint8)
            P = oracle.sa(x)
            assert (P == oracle.sa(x, brute=True)).all(), t
            bwt, base = oracle.sa_to_bwt(x, P)
            rc, back = oracle.inverse(bwt, base)
            assert rc == 0 and (back == x).all(), t


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: "%s-%d" % (c["shape"], c["n"]))
def test_golden_reference_outputs(oracle, case):
    """bit-exact against what the reference a7 produced on the same bytes"""
    x = S.gen_shape(case["shape"], case["n"])
    P, bwt, base = oracle.forward(x)
    assert base == case["base_id"]
    assert hashlib.sha256(np.ascontiguousarray(P, "<u4").tobytes()).hexdigest() == case["sha256_P"]
    assert hashlib.sha256(bwt.tobytes() + int(base).to_bytes(4, "little")).hexdigest() == case["sha256_bwt_base"]
    if "P" in case:
        assert list(P) == case["P"] and bwt.tobytes().hex() == case["bwt_hex"]
    if case["n"] <= (1 << 20):
        assert oracle.validate(x, P)
        rc, back = oracle.inverse(bwt, base)
        assert rc == 0 and (back == x).all()
    # A3: oracle_lms_select against the placement the reference's own findLMS produced (oracle/_ref/a7lms, make_golden.py)
    count, items = oracle.lms_select(x)
    assert items.size == case["lms_n1"] and OB.lms_digest(count, items) == case["sha256_lms"]


def test_live_reference_lms(oracle):
    """the reference's findLMS itself: its recorded answers (tests/golden/live_reference.json, make_live_reference.py) and,
    when oracle/_ref/a7lms is present (development container and GPU box), the live binary on the same inputs"""
    live = OB.ref_available("a7lms")
    inputs = OB.live_lms_inputs()
    assert len(inputs) == len(LIVE["lms"])
    for x, rec in zip(inputs, LIVE["lms"]):
        count, items = oracle.lms_select(x)
        assert x.size == rec["n"] and items.size == rec["lms_n1"] and OB.lms_digest(count, items) == rec["sha256_lms"]
        if live:
            ref = OB.run_ref_lms(x)
            assert ref is not None and (ref[0] == count).all() and ref[1].size == items.size and (ref[1] == items).all()


def test_random_small_vs_definition(oracle):
    rng = np.random.default_rng(1)
    for _ in range(300):
        n = int(rng.integers(1, 200))
        k = int(rng.choice([1, 2, 3, 4, 16, 256]))
        x = rng.integers(0, k, size=n, dtype=np.uint8)
        if rng.random() < 0.3:
            x = 255 - x
        assert (oracle.sa(x) == oracle.sa(x, brute=True)).all()


def test_validate_detects_errors(oracle):
    x = S.gen_text(5000)
    P = oracle.sa(x)
    assert oracle.validate(x, P)
    Q = P.copy()
    Q[[100, 101]] = Q[[101, 100]]
    assert not oracle.validate(x, Q)
    assert not oracle.check_sorted(x, Q)


def test_a7_validate_is_not_a_sortedness_check(oracle):
    """Archon::validate (archon.cpp:862-874, oracle.validate) takes each bucket's first row from sa itself, so it accepts
    some permutations that are not the suffix array: for x = "ab" it accepts {2, 1}, while the a7 suffix array is {1, 2}.
    The device validate is stricter (1 if and only if sa IS the suffix array, test_device_validate_rule_is_exact), so the
    GPU tests of the validators take oracle.sa, not oracle.validate, as their expected answer."""
    x = np.frombuffer(b"ab", np.uint8)
    assert list(oracle.sa(x)) == [1, 2]
    assert oracle.validate(x, np.array([2, 1], np.uint32))
    assert not oracle.check_sorted(x, np.array([2, 1], np.uint32))


def device_validate_rule(x, P):
    """The rule of archon_hip_validate / validate_dev (csrc/inverse.hiph: k_val_bwt, lf_build_launch, k_val_check) in numpy:
    every value in 1..n, exactly one row (the primary row) holds n, bwt[i] = x[P[i]] (x[0] on the primary row), and with T
    the LF table of (bwt, primary row) -- buckets from the byte counts in byte order, the primary row last in its bucket --
    P[T[i]] == P[i] + 1 on every other row."""
    x = np.asarray(x, np.uint8)
    P = np.asarray(P, np.int64)
    n = x.size
    if ((P < 1) | (P > n)).any() or (P == n).sum() != 1:
        return False
    base = int(np.flatnonzero(P == n)[0])
    bwt = x[np.where(P == n, 0, P)].astype(np.int64)
    key = bwt * 2
    key[base] += 1
    T = np.empty(n, np.int64)
    T[np.argsort(key, kind="stable")] = np.arange(n)
    rows = np.arange(n) != base
    return bool((P[T[rows]] == P[rows] + 1).all())


def test_device_validate_rule_is_exact(oracle):
    """the device rule accepts exactly the a7 suffix array: every string of length 1..5 over {0, 1, 255}, every permutation
    of 1..n (31 287 cases), and for n <= 3 every array over 0..n+1 (repeats, values out of range).  Why it holds, by
    induction on key length: the byte counts fix the first column, the stable LF map extends sortedness by one byte per
    step, and the end of the string (the primary row, rolled last) sorts last."""
    cases = accepted_a7 = 0
    for n in range(1, 6):
        perms = [np.array(p, np.uint32) + 1 for p in itertools.permutations(range(n))]
        for t in itertools.product((0, 1, 255), repeat=n):
            x = np.array(t, np.uint8)
            sa = oracle.sa(x)
            for P in perms:
                want = bool((P == sa).all())
                assert device_validate_rule(x, P) == want, (t, list(P))
                accepted_a7 += oracle.validate(x, P) and not want
                cases += 1
            if n <= 3:
                for P in itertools.product(range(n + 2), repeat=n):
                    P = np.array(P, np.uint32)
                    assert device_validate_rule(x, P) == bool((P == sa).all()), (t, list(P))
    assert cases == 31287
    assert accepted_a7 > 0          # the a7 rule accepts wrong permutations on the same set


def test_lf_build_base_last(oracle):
    """row baseId ranks last in its bucket (archon.cpp:931-933)"""
    bwt = np.frombuffer(b"aaaa", np.uint8)
    T = oracle.lf_build(bwt, 1)
    assert list(T) == [0, 3, 1, 2]


def test_hist_and_scatter(oracle):
    x = S.gen_random(1 << 15)
    c, s = oracle.hist256(x)
    assert (c == np.bincount(x, minlength=256)).all()
    assert s[256] == x.size and (np.diff(s.astype(np.int64)) == c).all()
    assert (oracle.radix_scatter(x) == np.sort(x, kind="stable")).all()


def test_live_reference(oracle):
    """the oracle against the reference's recorded answers on fresh seeds (tests/golden/live_reference.json) and, when oracle/_ref
    is present (development container), against the reference binary itself"""
    live = OB.ref_available("a7ref_nt")
    assert len(OB.LIVE_SHAPES) == len(LIVE["shapes"])
    for (shape, n, block), rec in zip(OB.LIVE_SHAPES, LIVE["shapes"]):
        assert (shape, n, block) == (rec["shape"], rec["n"], rec["block"])
        x = S.gen_shape(shape, n, block=block)
        P, bwt, base = oracle.forward(x)
        assert OB.sha256_bytes(P, "<u4") == rec["sha256_P"] and OB.sha256_bytes(bwt) == rec["sha256_bwt"] and base == rec["base_id"]
        if live:
            r = OB.run_ref(x, "a7ref_nt")
            assert r is not None and r["validate"] == 1
            assert (P == r["P"]).all() and (bwt == r["bwt"]).all() and base == r["base"]
