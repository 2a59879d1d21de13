"""Inputs and schedules shared by tests/test_gpu_list_passes.py and scripts/make_list_passes_stats.py (which records the row
counters of a build into tests/golden/list_passes_stats.json)."""
import synth

# pass A's schedules: two-sided, one-sided, unshared, many batches (the profiles in ranges), two more block sizes
SCHEDULES = {"two_sided": {"ITSX_SHARE_MIN": 0},
             "one_sided": {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_TWO": 0},
             "unshared": {"ITSX_SHARE": 0},
             "many_batches": {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_GB": 0.0005},
             "block_16": {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_B": 16},
             "block_64": {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_B": 64}}
SWITCHES = ("ITSX_SHARE", "ITSX_SHARE_B", "ITSX_SHARE_GB", "ITSX_SHARE_MIN", "ITSX_SHARE_CHECK", "ITSX_CHUNK_UNIQUES", "ITSX_SHARE_FWD_STREAMS",
            "ITSX_SHARE_TWO", "ITSX_BOUND_FOLD", "ITSX_LAZY_CHECK_BOUND", "ITSX_LAZY_EXACT_BOUND", "ITSX_KEEP_TRACE", "ITSX_ROWS", "ITSX_COMPACT_ROWS")

# the counters' fixed inputs: (reads, seed, 3_ profiles, 4_ profiles)
STATS_INPUTS = {"a": (1500, 41, 12, 12), "b": (2500, 42, 5, 9), "c": (900, 43, 1, 0)}
STATS_SCHEDULES = ("two_sided", "one_sided", "unshared")
STATS_KEYS = ("bound_rows", "bound_rows_full", "bwd_rows")
# The shared schedules' trees are built through hash tables whose insertion order is not fixed: which chain owns a shared prefix, and
# with it the helpers on the list and the rows walked, differ from one run of the SAME build to the next (input "a", one-sided, two runs of
# one build: bound_rows 5635311 / 5636233, bound_rows_full 8602159 / 8603273; two-sided: bwd_rows 266336 / 265120).  Only the unshared
# schedule's counters are a function of the input, so only they are recorded; the shared schedules' are held to the sums pair by pair
# of the same run (ITSX_SHARE_CHECK=1) instead.  What does not vary (representatives, pairs past the filter) is recorded for all three.
STATS_RECORDED = {"unshared": STATS_KEYS + ("n_unique", "n_past_msv"), "one_sided": ("n_unique", "n_past_msv"), "two_sided": ("n_unique", "n_past_msv")}


def its2_subset(hmm_text, n3, n4):
    blocks = [b + "//\n" for b in hmm_text.split("//\n") if "NAME  " in b]
    l3 = [b for b in blocks if b.split("NAME  ")[1].startswith("3_")]
    l4 = [b for b in blocks if b.split("NAME  ")[1].startswith("4_")]
    return "".join(l3[:n3] + l4[:n4])


def bench_reads(t_hmm_text, n, seed):
    """reads of the benchmark's shape (tests/synth.py, config 3), distinct, in generation order"""
    blob, offs = synth.make_reads(t_hmm_text, n, config=3, seed=synth.SEED + seed, fixed_len=0, len_range=(300, 580))
    out, seen = [], set()
    for s in synth.to_strings(blob, offs):
        if s not in seen:
            seen.add(s); out.append(s)
    return out


def stats_input(t_hmm_text, name):
    n, seed, n3, n4 = STATS_INPUTS[name]
    return its2_subset(t_hmm_text, n3, n4), bench_reads(t_hmm_text, n, seed)


def search(engine, hmm, seqs, F=None):
    """derep and search; F: the filters' thresholds (None: the defaults).  Reads of every length are kept"""
    engine.load_profiles(text=hmm)
    engine.set_reads(seqs)
    nu = engine.derep(minseqlength=1)
    if F is None:
        engine.search()
    else:
        engine.search(F1=F, F2=F, F3=F)
    return nu


def lazy_search(engine, hmm, seqs, env, setenv, delenv, F=None):
    """one lazy search under a schedule's switches; setenv / delenv: the caller's (monkeypatch's, or os.environ's)"""
    for k in SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, str(v))
    engine.set_rows_mode("lazy")
    try:
        search(engine, hmm, seqs, F)
    finally:
        engine.set_rows_mode(None)
