"""GPU: census of the general stage -- the host driver of everything the first stage leaves tied (general_stage.hiph,
Fwd::general_stage: run shortcut, lists, text rounds, rank table, certified break rounds, break and doubling rounds with the pair
chains), in the manner of test_gpu_block_calls.py.  One forward per case of forward_cases.CENSUS_CASES, at the smallest block
that reaches the branch the case is named after; the statistics that say which launches, waits and rounds the driver made are
pinned, and beside them stands a witness: a relation that fails when the block stops reaching its branch.  The suffix array is
checked on the GPU (validate); its order against the oracle is the job of test_gpu_forward.py.

The pinned figures are the ones the library reported at the commit before the one that added this test
(profiles/general/census_parent.txt, the output of tools/general_census.py).  They were recorded twice there, in two processes,
and every field of every case agreed: none is left out.  Every case runs behind a forward of one fixed block, so that what the
context remembers of its last block does not depend on which test ran before.

Where the branches were found, on the parent:
  * _seg_cases()["prose"] runs no text round on either first-stage route (more than a quarter of it is tied: 654 292 and
    287 903 of 700 876 rows): it stays, pinned, as the S and mid lists under doubling rounds; the text rounds over the S list
    alone are archon_synth's text block of 64 Ki.
  * run_inside_random and motif_with_glitches do not reach the recount (k_keep_flags -> k_compact_first -> k_classify) on any
    route of the tests: the shortcut settles every tied row of the first, and takes none of the second (its period's defects
    go to the break rounds).  Both stay, pinned, as what they are; the recount is reached by archon_synth's random block with
    a copy (64 Ki, 7-pass route) and by _dup_cases()["duplicate_behind_runs"].
  * the group of 16 Mi rows reaches the rank writer's B log as it stands (seg_big_items >= n, 268 launches against 174).

The last seven cases pin first-stage routes instead: the product's small-block rule (the row sets SMALL_BLOCK back to the library's
default), the closed form with its nested transform, and a block of four distinct bytes on the streaming machinery, found by the
count that gives up or -- behind a primer of its own -- shown by the presence map first.  Their figures are the library's at the
commit before the one that counts launches where they are made (profiles/launch_count/census_parent.txt and
census_parent_second_process.txt: two processes, every field of every case agreed, none is left out).  A dna block takes the
packed streaming stage at every size that was tried, from 64 bytes (the case) to 1 MiB; from 64 Ki on the period probe adds its
three launches (29 and 17 instead of 26 and 14)."""
import pytest

import forward_cases as F

pytestmark = pytest.mark.gpu

# the fields of F.CENSUS_FIELDS, in its order:
#   path, radix_passes, kernel_launches, host_syncs, text_rounds, doubling_rounds, break_rounds, break_settled,
#   period, chain_items, chain_pairs, mid_items, seg_big_items, unresolved_initial, unresolved_total
PINNED = {
    "nothing_tied":                (1, 2, 15, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    "text_rounds":                 (1, 2, 18, 5, 2, 0, 0, 0, 0, 0, 0, 0, 0, 398, 400),
    "text_rounds-lsb":             (0, 7, 16, 6, 1, 0, 0, 0, 0, 0, 0, 0, 0, 10, 10),
    "prose":                       (1, 2, 31, 9, 0, 4, 0, 0, 0, 0, 0, 182144, 0, 654292, 1629541),
    "prose-lsb":                   (0, 7, 24, 10, 0, 2, 0, 0, 0, 0, 0, 239, 0, 287903, 288135),
    "shortcut_probe":              (1, 2, 40, 8, 0, 0, 0, 0, 2, 299999, 0, 0, 0, 299999, 0),
    "shortcut_gap_sample":         (0, 3, 62, 17, 0, 0, 2, 299958, 1, 0, 0, 130, 299956, 299958, 569927),
    "shortcut_settles_all":        (1, 2, 25, 5, 0, 0, 0, 0, 1000, 249997, 0, 0, 0, 249997, 0),
    "shortcut_reclassify-copy":    (0, 3, 30, 12, 2, 1, 0, 0, 32768, 16320, 0, 0, 0, 16542, 342),
    "shortcut_reclassify-runs":    (1, 2, 77, 24, 0, 16, 0, 0, 205000, 199996, 0, 143570, 0, 513999, 4630844),
    "glitches":                    (1, 2, 49, 16, 0, 9, 1, 197431, 1000, 0, 0, 9621, 0, 200497, 1998892),
    "break_rounds-p7":             (1, 2, 55, 13, 0, 2, 2, 455855, 7, 0, 22046, 10, 499989, 499989, 588253),
    "break_rounds-p7-off":         (1, 2, 134, 44, 0, 17, 0, 0, 7, 0, 0, 6137, 7294543, 499989, 7300680),
    "break_rounds-twin":           (1, 2, 50, 11, 0, 2, 1, 159999, 50, 0, 119994, 399995, 0, 399999, 879991),
    "break_rounds-twin-off":       (1, 2, 133, 36, 0, 17, 0, 0, 50, 0, 0, 6035709, 0, 399999, 6515705),
    "break_rounds-signs":          (0, 7, 52, 12, 0, 2, 1, 199987, 50, 0, 99979, 399973, 0, 399987, 799959),
    "break_rounds-signs-off":      (0, 7, 116, 32, 0, 15, 0, 0, 50, 0, 42656, 5141290, 0, 399987, 5455964),
    "certified-p1000":             (1, 2, 31, 7, 0, 0, 1, 1199985, 1000, 0, 0, 1199985, 0, 1199985, 1199985),
    "certified-p4099":             (1, 2, 53, 18, 0, 11, 1, 1975421, 4099, 0, 0, 237612, 0, 1999985, 23950824),
    "mid_classes":                 (0, 7, 64, 16, 0, 6, 0, 0, 0, 0, 0, 3802935, 766299, 1860616, 7450134),
    "mid_classes-lsb":             (0, 7, 54, 17, 0, 6, 0, 0, 0, 0, 0, 3802935, 766299, 1860616, 7450134),
    "mid_classes-off":             (0, 7, 69, 16, 0, 6, 0, 0, 0, 0, 0, 0, 4622506, 1860616, 7450134),
    "pair_chains":                 (1, 2, 34, 9, 0, 3, 0, 0, 0, 0, 799713, 428, 0, 1599864, 1600294),
    "pair_chains-off":             (1, 2, 56, 22, 0, 18, 0, 0, 0, 0, 0, 428, 0, 1599864, 26176302),
    "writer_log":                  (0, 7, 95, 19, 0, 5, 0, 0, 0, 0, 0, 9120122, 5579314, 5255212, 21626139),
    "writer_log-off":              (0, 7, 84, 19, 0, 5, 0, 0, 0, 0, 0, 9120122, 5579314, 5255212, 21626139),
    "writer_b_log":                (1, 2, 268, 54, 0, 23, 0, 0, 0, 0, 0, 0, 369098777, 16777215, 369098777),
    "writer_b_log-off":            (1, 2, 174, 54, 0, 23, 0, 0, 0, 0, 0, 0, 369098777, 16777215, 369098777),
    "small-random":                (0, 3, 11, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 252, 252),
    "small-text":                  (0, 7, 15, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 10, 10),
    "small-dna":                   (0, 7, 14, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    "small-closed_form":           (2, 0, 33, 6, 0, 0, 0, 0, 2, 300000, 0, 0, 0, 0, 0),
    "closed_form":                 (2, 0, 44, 6, 0, 0, 0, 0, 2, 300000, 0, 0, 0, 0, 0),
    "dna_stream":                  (1, 2, 26, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    "dna_stream-hinted":           (1, 2, 14, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
}
_LAUNCHES = F.CENSUS_FIELDS.index("kernel_launches")

_tied_rounds = lambda st: st["text_rounds"] + st["doubling_rounds"]
_breaks = lambda st, n: st["break_rounds"] >= 1 and st["break_settled"] > 0
_no_breaks = lambda st, n: st["break_rounds"] == 0 and st["period"] > 0
_mid_and_big = lambda st, n: st["mid_items"] > 0 and st["seg_big_items"] > 0
_recount = lambda st, n: 0 < st["chain_items"] < st["unresolved_initial"] and _tied_rounds(st) > 0
_s_text_rounds = lambda st, n: st["text_rounds"] > 0 and st["mid_items"] == 0 and st["seg_big_items"] == 0
_closed = lambda st, n: st["path"] == 2 and st["period"] == 2 and st["chain_items"] == n
_packed_stream = lambda st, n: st["path"] == 1 and st["alphabet_bits"] == 2
WITNESS = {
    "nothing_tied": lambda st, n: st["text_rounds"] == st["doubling_rounds"] == 0,
    "text_rounds": _s_text_rounds,
    "text_rounds-lsb": _s_text_rounds,
    "prose": lambda st, n: st["doubling_rounds"] > 0,
    "prose-lsb": lambda st, n: st["doubling_rounds"] > 0,
    "shortcut_probe": lambda st, n: st["period"] == 2 and st["chain_items"] > 0 and st["doubling_rounds"] == 0,
    "shortcut_gap_sample": lambda st, n: st["period"] == 1 and st["path"] == 0,         # the probe's answer withheld: the gap sample named it
    "shortcut_settles_all": lambda st, n: st["chain_items"] == st["unresolved_initial"] > 0 and _tied_rounds(st) == 0,
    "shortcut_reclassify-copy": _recount,
    "shortcut_reclassify-runs": _recount,
    "glitches": lambda st, n: st["chain_items"] == 0 and st["break_rounds"] >= 1 and st["doubling_rounds"] > 0,
    "break_rounds-p7": _breaks, "break_rounds-p7-off": _no_breaks,
    "break_rounds-twin": _breaks, "break_rounds-twin-off": _no_breaks,
    "break_rounds-signs": _breaks, "break_rounds-signs-off": _no_breaks,
    "certified-p1000": lambda st, n: _breaks(st, n) and st["period"] == 1000,           # (they enter with h = the key depth, below the period)
    "certified-p4099": lambda st, n: _breaks(st, n) and st["period"] == 4099,
    "mid_classes": _mid_and_big,
    "mid_classes-lsb": _mid_and_big,
    "mid_classes-off": lambda st, n: st["mid_items"] == 0 and st["seg_big_items"] > 0,
    "pair_chains": lambda st, n: st["chain_pairs"] > 0,
    "pair_chains-off": lambda st, n: st["chain_pairs"] == 0,
    "writer_log": lambda st, n: n >= 1 << 22,                                           # (with test_rank_writer_routes)
    "writer_log-off": lambda st, n: n >= 1 << 22,
    "writer_b_log": lambda st, n: st["seg_big_items"] >= n,
    "writer_b_log-off": lambda st, n: st["seg_big_items"] >= n,
    # the small-block rule: no streaming stage (path 0 on blocks that take it otherwise); the shallow key depth comes from the
    # byte count's histogram alone; the closed form behind a byte count makes fewer launches than behind the streaming stage
    "small-random": lambda st, n: st["path"] == 0 and 0 < st["radix_passes"] < 7 and st["alphabet_bits"] == 0,
    "small-text": lambda st, n: st["path"] == 0 and st["alphabet_bits"] == 0,
    "small-dna": lambda st, n: st["path"] == 0 and st["alphabet_bits"] == 2,
    "small-closed_form": lambda st, n: _closed(st, n) and st["kernel_launches"] < PINNED["closed_form"][_LAUNCHES],
    "closed_form": lambda st, n: _closed(st, n) and st["kernel_launches"] > PINNED["small-closed_form"][_LAUNCHES],
    # the first attempt (count, streaming stage, round trip) is what the hint saves
    "dna_stream": lambda st, n: _packed_stream(st, n) and st["kernel_launches"] > PINNED["dna_stream-hinted"][_LAUNCHES],
    "dna_stream-hinted": lambda st, n: _packed_stream(st, n) and st["kernel_launches"] < PINNED["dna_stream"][_LAUNCHES],
}


@pytest.fixture(scope="module")
def census(archon):
    """census(case) -> (statistics, n, suffix array): each case runs once, validated; consecutive cases share their block"""
    primer = F.CENSUS_BLOCKS["random_64ki"]()
    cases = {case: (block, env) for case, block, env in F.CENSUS_CASES}
    done, held = {}, {}

    def run(case):
        if case not in done:
            block, env = cases[case]
            if block not in held:
                held.clear()
                held[block] = F.CENSUS_BLOCKS[block]()
            x = held[block]
            st, sa = F.census_run(archon, x, env, primer)
            assert archon.validate(x, sa), case
            done[case] = (st, x.size, sa if case.startswith("writer_") else None)
        return done[case]
    return run


def test_every_case_is_pinned():
    assert [c for c, _, _ in F.CENSUS_CASES] == list(PINNED) and set(PINNED) == set(WITNESS)


@pytest.mark.parametrize("case", [c for c, _, _ in F.CENSUS_CASES])
def test_census(census, case):
    st, n, _ = census(case)
    got = {f: st[f] for f in F.CENSUS_FIELDS}
    print("   ", case, n, got)
    assert WITNESS[case](st, n), (case, got)
    assert got == dict(zip(F.CENSUS_FIELDS, PINNED[case])), case


@pytest.mark.parametrize("case", ["writer_log", "writer_b_log"])
def test_rank_writer_routes(census, case):
    """the rank writer took part in the block's rounds: other launches with it switched off, and the same suffix array"""
    st, _, sa = census(case)
    st_off, _, sa_off = census(case + "-off")
    print("   ", case, st["kernel_launches"], st_off["kernel_launches"])
    assert st["kernel_launches"] != st_off["kernel_launches"]
    assert st["doubling_rounds"] == st_off["doubling_rounds"] and (sa == sa_off).all()
