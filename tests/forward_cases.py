"""Block generators shared by the forward tests (test_gpu_forward.py), the general-stage census (test_gpu_general_stage.py)
and tools/general_census.py: every call builds the same blocks from fixed seeds."""
import numpy as np


def _repeat_cases():
    rng = np.random.default_rng(31)
    motif = rng.integers(0, 256, size=1000, dtype=np.uint8)
    short = np.frombuffer(b"abcabd", np.uint8)
    a = lambda k, c=97: np.full(k, c, np.uint8)
    r = lambda k: rng.integers(0, 256, size=k, dtype=np.uint8)
    lit = lambda s: np.frombuffer(s, np.uint8)
    return {
        "a": a(300000),
        "ab": np.tile(lit(b"ab"), 150000),
        "ba_odd": np.tile(lit(b"ba"), 150000)[:-1],
        "motif1000": np.tile(motif, 300),
        "motif1000_ragged": np.tile(motif, 300)[137:-451],
        "motif6": np.tile(short, 50000),
        "ff": a(200000, 255),
        "feff": np.tile(np.array([254, 255], np.uint8), 100000),
        "three_runs": np.concatenate([a(100000), lit(b"b"), a(100000), lit(b"c"), a(70000), lit(b"\x00"), a(30000)]),
        "run_inside_random": np.concatenate([r(5000), np.tile(motif, 250), r(5000)]),
        "two_periods": np.concatenate([np.tile(lit(b"ab"), 80000), np.tile(lit(b"abc"), 60000)]),
        "run_signs": np.concatenate([lit(b"z"), a(60000), lit(b"A"), a(60000), lit(b"z"), a(60001), lit(b"a"), a(5)]),
        "motif_with_glitches": np.concatenate([np.tile(motif, 100), motif[:500], lit(b"!"), np.tile(motif, 100), motif[:3]]),
        "nested": np.tile(np.concatenate([a(500), lit(b"b")]), 400),
    }


def _defect_cases():
    """a motif repeated with point defects: groups that straddle the defects (never ONE clean run of the period)"""
    rng = np.random.default_rng(4099)
    out = {}
    for p, n, flips in ((1, 300000, 3), (2, 400001, 4), (3, 299999, 2), (7, 500000, 5), (100, 600000, 3), (1000, 1200000, 3),
                        (4099, 2000000, 3), (257, 700000, 12)):
        motif = rng.integers(0, 256, size=p, dtype=np.uint8)
        x = np.tile(motif, n // p + 1)[:n].copy()
        for q in rng.integers(0, n, size=flips):
            x[q] ^= np.uint8(1 + rng.integers(0, 255))
        out["p%d_%dflips" % (p, flips)] = x
    motif = rng.integers(0, 256, size=50, dtype=np.uint8)
    x = np.tile(motif, 8000)
    x[100000] = 0; x[200000] = 255; x[300000] = 0          # same phase, leaving below / above / below the periodic continuation
    out["same_phase_signs"] = x.copy()
    x = np.tile(motif, 8000)
    x[120025] ^= 1; x[240025] ^= 1                          # the same defect twice: items at equal distances behind them stay tied for the rounds
    out["twin_defects"] = x.copy()
    x = np.tile(motif, 8000)
    x[5] ^= 7; x[399990] ^= 9; x[200000:200003] ^= 3        # defects inside the first and the last period, and three in a row
    out["edges_and_burst"] = x.copy()
    x = np.concatenate([np.tile(motif, 4000), np.tile(rng.integers(0, 256, size=50, dtype=np.uint8), 4000)])   # two motifs of one period
    x[77777] ^= 1
    out["two_motifs"] = x
    return out


def _seg_cases():
    rng = np.random.default_rng(77)
    r = lambda k, hi=256: rng.integers(0, hi, size=k, dtype=np.uint8)
    R = r(200000)
    words = [bytes(r(int(k), 26) + 97) for k in rng.integers(2, 9, size=300)]
    prose = np.frombuffer(b" ".join(words[i] for i in rng.integers(0, 300, size=120000)), np.uint8)
    runs = np.concatenate([np.concatenate([np.full(int(k), 32, np.uint8), r(40, 26) + 97]) for k in rng.integers(1, 400, size=2500)])
    return {
        "duplicated_block": np.concatenate([R, r(7), R, r(3), R[:150000]]),                 # pairs and triples, deep repeats
        "prose": prose,                                                                     # skewed groups of every size
        "prose_twice": np.concatenate([prose[:300000], prose[:300000]]),
        "space_runs": runs,                                                                 # long groups next to short ones
        "dups_and_runs": np.concatenate([R[:60000], runs[:200000], R[:60000], np.full(5000, 7, np.uint8), R[:999]]),
    }


def _word_soup(n, vocab, word_len, seed, skew=1.3, alphabet=12):
    """tokens drawn (Zipf-like) from a small vocabulary of fixed-length words over a small alphabet: after the first stage the
    tied groups are the (word, offset) classes -- thousands to tens of thousands of rows each -- and every doubling round
    splits them by the words in front: groups of every size class, each handing groups down to the smaller ones"""
    rng = np.random.default_rng(seed)
    words = rng.integers(97, 97 + alphabet, size=(vocab, word_len)).astype(np.uint8)
    pr = 1.0 / np.arange(1, vocab + 1) ** skew
    pr /= pr.sum()
    toks = rng.choice(vocab, size=n // word_len + 1, p=pr)
    return words[toks].reshape(-1)[:n].copy()


def _dup_cases():
    rng = np.random.default_rng(91)
    r = lambda k, hi=256: rng.integers(0, hi, size=k, dtype=np.uint8)
    R = r(1 << 20)
    words = [bytes(r(int(k), 26) + 97) for k in rng.integers(2, 9, size=400)]
    prose = np.frombuffer(b" ".join(words[i] for i in rng.integers(0, 400, size=200000)), np.uint8)
    return {
        # random block with one long duplicate: every tied group is a pair {s, s + d} of ONE passage
        "one_duplicate": np.concatenate([R, r(11), R[100000:900000], r(5)]),
        # three copies of a passage (groups of three at first, pairs once the copies' left contexts differ), nested copies
        "three_copies": np.concatenate([R[:300000], r(3), R[:300000], r(7), R[:200000], R[50000:250000]]),
        # text with copied passages next to many short repeats: pairs are listed while longer groups keep doubling
        "prose_with_copies": np.concatenate([prose[:400000], prose[100000:350000], prose[400000:600000], prose[120000:300000]]),
        # a duplicate whose predecessors sit in a LONGER group (the run's head cannot be settled at first): 0-runs in front of the copies
        "duplicate_behind_runs": np.concatenate([np.zeros(5000, np.uint8), R[:200000], np.zeros(5000, np.uint8), R[:200000], np.zeros(4000, np.uint8), R[:100000]]),
    }


def _class_limit_block():
    """groups of EXACTLY 512 / 513 / 4096 / 4097 / 16384 / 16385 rows (and their neighbours): distinct 16-byte words that occur
    exactly that often, in random order (test_mid_groups_at_the_class_limits)"""
    rng = np.random.default_rng(16384)
    counts = [16384, 16385, 16383, 4096, 4097, 4095, 1025, 1024, 1023, 513, 512, 511, 8192, 2048, 2, 3, 1, 40000]
    words = rng.integers(0, 256, size=(len(counts), 16)).astype(np.uint8)
    toks = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(toks)
    return words[toks].reshape(-1).copy()


# ---- the census of the general stage (tools/general_census.py, test_gpu_general_stage.py): the smallest blocks that reach each
# branch of the driver, and the routes they run on.  CENSUS_BLOCKS builds a block by name; CENSUS_CASES lists (case, block, routes).
CENSUS_FIELDS = ("path", "radix_passes", "kernel_launches", "host_syncs", "text_rounds", "doubling_rounds", "break_rounds", "break_settled",
                 "period", "chain_items", "chain_pairs", "mid_items", "seg_big_items", "unresolved_initial", "unresolved_total")
_NO_HINT = {"ARCHON_NO_PERIOD_STREAM": "1", "ARCHON_NO_CLOSED_FORM": "1", "ARCHON_NO_PERIOD_HINT": "1"}
_NO_BREAK = {"ARCHON_NO_BREAK_ROUND": "1"}
_NO_WRITER = {"ARCHON_NO_RANK_WRITER": "1"}
_GROUP_16MI = {"ARCHON_NO_CHAINS": "1", "ARCHON_NO_CLOSED_FORM": "1"}
_LSB = {"ARCHON_FORCE_PATH": "0"}
_SMALL = {"ARCHON_SMALL_BLOCK": "-1"}
PRIMER = "ARCHON_PRIMER"       # no route of the library: the block of CENSUS_BLOCKS that census_run sends ahead of the case instead of `primer`


def _shape(shape, n):
    import archon_synth
    return archon_synth.gen_shape(shape, n)


CENSUS_BLOCKS = {
    "random_64ki": lambda: _shape("random", 64 << 10),
    "text_64ki": lambda: _shape("text", 64 << 10),
    "random_copy_64ki": lambda: _shape("random_copy", 64 << 10),
    "prose": lambda: _seg_cases()["prose"],
    "ab": lambda: _repeat_cases()["ab"],
    "three_runs": lambda: _repeat_cases()["three_runs"],
    "run_inside_random": lambda: _repeat_cases()["run_inside_random"],
    "motif_with_glitches": lambda: _repeat_cases()["motif_with_glitches"],
    "duplicate_behind_runs": lambda: _dup_cases()["duplicate_behind_runs"],
    "p7_5flips": lambda: _defect_cases()["p7_5flips"],
    "twin_defects": lambda: _defect_cases()["twin_defects"],
    "same_phase_signs": lambda: _defect_cases()["same_phase_signs"],
    "p1000_3flips": lambda: _defect_cases()["p1000_3flips"],
    "p4099_3flips": lambda: _defect_cases()["p4099_3flips"],
    "class_limits": _class_limit_block,
    "one_duplicate": lambda: _dup_cases()["one_duplicate"],
    "word_soup_5mi": lambda: _word_soup((5 << 20) + 12345, 7, 24, 14),
    "a_16mi": lambda: np.full(16 << 20, 97, np.uint8),
    "dna_64ki": lambda: _shape("dna", 64 << 10),
    "dna_64": lambda: _shape("dna", 64),
}

CENSUS_CASES = [
    ("nothing_tied", "random_64ki", {}),
    ("text_rounds", "text_64ki", {}),
    ("text_rounds-lsb", "text_64ki", _LSB),
    ("prose", "prose", {}),
    ("prose-lsb", "prose", _LSB),
    ("shortcut_probe", "ab", {"ARCHON_NO_CLOSED_FORM": "1"}),
    ("shortcut_gap_sample", "three_runs", _NO_HINT),
    ("shortcut_settles_all", "run_inside_random", {}),
    ("shortcut_reclassify-copy", "random_copy_64ki", _LSB),
    ("shortcut_reclassify-runs", "duplicate_behind_runs", {}),
    ("glitches", "motif_with_glitches", {}),
    ("break_rounds-p7", "p7_5flips", {}),
    ("break_rounds-p7-off", "p7_5flips", _NO_BREAK),
    ("break_rounds-twin", "twin_defects", {}),
    ("break_rounds-twin-off", "twin_defects", _NO_BREAK),
    ("break_rounds-signs", "same_phase_signs", {}),
    ("break_rounds-signs-off", "same_phase_signs", _NO_BREAK),
    ("certified-p1000", "p1000_3flips", {}),
    ("certified-p4099", "p4099_3flips", {}),
    ("mid_classes", "class_limits", {}),
    ("mid_classes-lsb", "class_limits", {"ARCHON_FORCE_PATH": "0", "ARCHON_NO_TEXT_ROUNDS": "1", "ARCHON_NO_RANK_WRITER": "1"}),
    ("mid_classes-off", "class_limits", {"ARCHON_NO_MID": "1"}),
    ("pair_chains", "one_duplicate", {}),
    ("pair_chains-off", "one_duplicate", {"ARCHON_NO_PAIR_CHAINS": "1"}),
    ("writer_log", "word_soup_5mi", {}),
    ("writer_log-off", "word_soup_5mi", _NO_WRITER),
    ("writer_b_log", "a_16mi", _GROUP_16MI),
    ("writer_b_log-off", "a_16mi", dict(_GROUP_16MI, **_NO_WRITER)),
    # first-stage routes: the product's small-block rule (the row sets SMALL_BLOCK back to the library's default itself), the closed
    # form, and a poor alphabet on the streaming machinery -- found by the count that gives up, or shown first behind a dna primer
    ("small-random", "random_64ki", _SMALL),
    ("small-text", "text_64ki", _SMALL),
    ("small-dna", "dna_64ki", _SMALL),
    ("small-closed_form", "ab", _SMALL),
    ("closed_form", "ab", {}),
    ("dna_stream", "dna_64", {}),
    ("dna_stream-hinted", "dna_64", {PRIMER: "dna_64"}),
]


def census_run(archon, x, env, primer):
    """the statistics and the suffix array of one forward of x with the routes of env set for that call alone.  A forward of
    `primer` (CENSUS_BLOCKS["random_64ki"]) goes first: what a context remembers of its last block (a poor alphabet or a period
    sends the next block to its alphabet first) is then the same whichever call came before, and so are the figures.  A case
    that is about that memory names its own primer (env[PRIMER])."""
    import os
    env = dict(env)
    own = env.pop(PRIMER, None)
    archon.forward(CENSUS_BLOCKS[own]() if own else primer, want_sa=False)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sa = archon.forward(x)[0]
        st = archon.stats()
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return st, sa
