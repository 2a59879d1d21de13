"""The passes over the lazy stage's pair list between the MSV filter and round 1 (csrc/k_msv.hip: k_pair_count / k_pair_fill, which
write the list and its padding; k_share.hip: k_share_wavelist / k_share_rows, the wave list and the row counters without a look at the
pairs; k_lazy.hip: the wave's last row inside k_fwd_bound / k_bwd_bound, k_lazy_bound, the marking kernels with several chunks per wave):

* the list as it lies after a lazy one-chunk search (Engine.debug_lazy_pairs) against the full-rows search of the same reads -- its
  pairs, their order, the 64-aligned segments, the padding, the helpers, b10 -- in every schedule of pass A and on the shapes at the
  edges of the kernels' tiles;
* the selection through itsx_debug_select at list lengths around the marking kernels' tiles, against tests/test_gpu_select_passes.py's
  numpy statement of each mode;
* bound_rows / bound_rows_full / bwd_rows against the values recorded from the build before this one
  (tests/golden/list_passes_stats.json, scripts/make_list_passes_stats.py) where that build reports the same values every run --
  the unshared schedule -- and against the same run's sums pair by pair in the shared ones;
* coordinates equal to the full-table search's.
Every comparison is for equality.  `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

import lazy_bound_cases as LB
import list_passes_inputs as LP
from test_gpu_compact import PAIRS, _same
from test_gpu_select_passes import PairLists, _check_list, _flags, _select

pytestmark = pytest.mark.gpu

MARK_WAVE = 4 * 64            # k_lazy.hip: MARK_K chunks of 64 pairs per wave of a marking kernel
MARK_BLOCK = 4 * MARK_WAVE    # ... and four waves per block
FILL_CHUNK = 2048             # k_api.h: CHUNK, the cells one block of k_pair_count / k_pair_fill takes (four waves of 512, 64 at a time)

_FULL = {}                    # per input: the full-rows search's pairs past the filter and its coordinates, made once and left unchanged


def _full(engine, key, hmm, seqs, monkeypatch, F=None):
    if key in _FULL:
        return _FULL[key]
    for k in LP.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
    engine.set_rows_mode("full")
    try:
        nu = LP.search(engine, hmm, seqs, F)
        engine.finalize()
        tr = engine.pairtraces()
        tr = tr[tr["pass_msv"] != 0]
        d = dict(nu=nu, seed=engine.get_uniques()[0].copy(), n_past=engine.stats()["n_past_msv"],
                 triples=sorted(zip(tr["prof"].tolist(), tr["rep"].tolist(), tr["msv_xj"].tolist())),
                 coords=[tuple(a.copy() for a in engine.trim_coords(l, r)) for l, r in PAIRS])
    finally:
        engine.set_rows_mode(None)
        monkeypatch.delenv("ITSX_KEEP_TRACE")
    assert len(d["triples"]) == d["n_past"] > 0
    _FULL[key] = d
    return d


def _common_order(segments):
    """True when one order of the representatives exists in which every segment ascends (no cycle among 'comes right before')"""
    succ, indeg = {}, {}
    for s in segments:
        for a in s:
            indeg.setdefault(a, 0)
        for a, b in zip(s[:-1], s[1:]):
            if b not in succ.setdefault(a, set()):
                succ[a].add(b); indeg[b] += 1
    todo = [a for a, n in indeg.items() if n == 0]
    seen = 0
    while todo:
        a = todo.pop(); seen += 1
        for b in succ.get(a, ()):
            indeg[b] -= 1
            if indeg[b] == 0:
                todo.append(b)
    return seen == len(indeg)


def _check_search(engine, key, hmm, seqs, env, monkeypatch, F=None):
    """a lazy search of (hmm, seqs) under env: its list, then its coordinates, against the full-rows search; returns (stats, records)"""
    full = _full(engine, key, hmm, seqs, monkeypatch, F)
    LP.lazy_search(engine, hmm, seqs, env, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), F)
    st = engine.stats()
    assert st["lazy"] == 1 and st["n_unique"] == full["nu"] and np.array_equal(engine.get_uniques()[0], full["seed"])
    recs, bias = engine.debug_lazy_pairs()
    recs = recs.copy()
    n_prof = engine.n_profiles
    pad = recs["prof"] < 0
    helper = ~pad & (recs["xj"] < 0)
    real = ~pad & ~helper
    # ---- the pairs: exactly the full search's (profile, representative, xJ) past the filter
    assert sorted(zip(recs["prof"][real].tolist(), recs["rep"][real].tolist(), recs["xj"][real].tolist())) == full["triples"]
    assert st["n_past_msv"] == full["n_past"] == int(real.sum())
    # ---- profile order, 64-aligned segments, padding only at a segment's end
    at, segments = 0, []
    for p in range(n_prof):
        idx = np.flatnonzero(recs["prof"] == p)
        if len(idx) == 0:
            continue
        assert idx[0] == at and at % 64 == 0 and idx[-1] - idx[0] + 1 == len(idx), (p, at, idx[0], idx[-1], len(idx))
        at = (int(idx[-1]) + 1 + 63) // 64 * 64
        assert pad[idx[-1] + 1:at].all()
        seg = recs["rep"][idx].tolist()
        assert len(set(seg)) == len(seg)
        segments.append(seg)
        if st["share_B"] == 0:
            assert (np.diff(recs["L"][idx]) >= 0).all()                     # unshared: ascending length
    assert at == len(recs)
    assert _common_order(segments)                                          # ... ascending processing position in every segment
    # ---- padding and helpers
    for f in ("prof", "xj", "L"):
        assert (recs[f][pad] == -1).all(), f                                # (all 0xFF)
    assert (recs["rep"][pad] == -1).all() and (recs["b10"][pad] == 0).all()
    assert (recs["b10"][helper] == 0).all() and (recs["done"][helper] == 1).all()
    assert int(helper.sum()) == st["n_share_helpers"]
    # ---- b10: the float64 restatement on the returned numbers
    R = recs[real]
    assert np.array_equal(R["b10"], LB.b10_model(R["fb"], R["nullsc"], R["lazy_c"], bias))
    assert (R["b10"] >= 1).all()
    # ---- coordinates
    engine.finalize()
    assert engine.stats()["n_lazy_reruns"] == 0
    assert _same(full["coords"], [tuple(a.copy() for a in engine.trim_coords(l, r)) for l, r in PAIRS])
    return st, recs


def _per_prof(recs, n_prof):
    return np.bincount(recs["prof"][recs["prof"] >= 0], minlength=n_prof)


# ------------------------------------------------------------------------------------------------ schedules
@pytest.fixture(scope="module")
def bench_input(t_hmm_text):
    return LP.its2_subset(t_hmm_text, 12, 12), LP.bench_reads(t_hmm_text, 3000, 44)


@pytest.mark.parametrize("sched", list(LP.SCHEDULES))
def test_list_in_every_schedule(engine, bench_input, monkeypatch, sched):
    hmm, seqs = bench_input
    st, recs = _check_search(engine, "bench", hmm, seqs, LP.SCHEDULES[sched], monkeypatch)
    env = LP.SCHEDULES[sched]
    if sched == "unshared":
        assert st["share_B"] == 0 and st["bound_rows"] == st["bound_rows_full"] and st["bwd_rows"] == 0 and st["n_share_helpers"] == 0
    else:
        assert st["share_B"] == env.get("ITSX_SHARE_B", 32) and st["share_chains"] > 0 and 0 < st["bound_rows"] < st["bound_rows_full"]
        assert st["two_sided"] == (0 if sched == "one_sided" else 1) and (st["bwd_rows"] > 0) == (sched != "one_sided")
    if sched == "many_batches":
        assert st["share_batches"] > 1
    print("[%s] pairs %d helpers %d bound_rows %d / %d bwd_rows %d batches %d" % (
        sched, st["n_past_msv"], st["n_share_helpers"], st["bound_rows"], st["bound_rows_full"], st["bwd_rows"], st["share_batches"]))


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("name", ["waves_63", "waves_64", "waves_65", "waves_130", "degenerate_consensus"])
@pytest.mark.parametrize("sched", ["two_sided", "one_sided", "unshared"])
def test_list_at_the_wave_edges(engine, monkeypatch, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads, name, sched):
    """a profile with 63 / 64 / 65 / 130 pairs (a last wave of 63, none, 1 and 2) beside profiles with none; reads that begin and end in N"""
    c = LB.case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1])
    hmm, seqs = c.hmm, c.seqs
    st, recs = _check_search(engine, name, hmm, seqs, LP.SCHEDULES[sched], monkeypatch, F=c.F)      # (the filters at the case's own thresholds)
    per = _per_prof(recs[recs["xj"] >= 0], engine.n_profiles)
    if name.startswith("waves_"):
        assert per.max() == int(name.split("_")[1])
        assert (per == 0).any()                                             # a profile with no pair
    else:
        assert any(s[0] == "N" for s in seqs) and any(s[-1] == "N" for s in seqs)


@pytest.mark.parametrize("sched", ["two_sided", "unshared"])
def test_list_of_one_profile(engine, bench_input, t_hmm_text, monkeypatch, sched):
    """P = 1: one segment, one bit word per chain"""
    hmm = LP.its2_subset(t_hmm_text, 1, 0)
    st, recs = _check_search(engine, "one_profile", hmm, bench_input[1][:700], LP.SCHEDULES[sched], monkeypatch)
    assert engine.n_profiles == 1 and (recs["prof"] <= 0).all()


def test_list_below_the_sharing_threshold(engine, bench_input, monkeypatch):
    """a read set that would share less than ITSX_SHARE_MIN of its rows runs unshared"""
    hmm, seqs = bench_input
    st, recs = _check_search(engine, "bench", hmm, seqs, {"ITSX_SHARE_MIN": 0.99}, monkeypatch)
    assert st["share_B"] == 0 and st["share_chains"] == 0 and st["n_share_helpers"] == 0 and st["bound_rows"] == st["bound_rows_full"]


@pytest.fixture(scope="module")
def representatives(engine, t_hmm_text):
    """reads that dereplication keeps apart: the representatives of a larger set"""
    seqs = LP.bench_reads(t_hmm_text, 2 * FILL_CHUNK, 45)
    engine.load_profiles(text=LP.its2_subset(t_hmm_text, 3, 3))
    engine.set_reads(seqs)
    engine.derep(minseqlength=1)
    reps = [seqs[int(i)] for i in engine.get_uniques()[0]]
    assert len(reps) > FILL_CHUNK
    return reps


@pytest.mark.parametrize("nu", [FILL_CHUNK - 1, FILL_CHUNK, FILL_CHUNK + 1])
@pytest.mark.parametrize("sched", ["two_sided", "unshared"])
def test_list_at_the_fill_tile(engine, representatives, t_hmm_text, monkeypatch, nu, sched):
    """as many representatives as one block of the list builder takes, and one either side (one chunk per profile, and a second of one cell)"""
    hmm = LP.its2_subset(t_hmm_text, 3, 3)
    st, recs = _check_search(engine, ("fill", nu), hmm, representatives[:nu], LP.SCHEDULES[sched], monkeypatch)
    assert st["n_unique"] == nu


def test_list_with_small_blocks_and_many_batches(engine, bench_input, monkeypatch):
    """block size 16 and a small slot budget on the bench-shaped reads: hundreds of (batch, depth, profile) segments"""
    hmm, seqs = bench_input
    st, recs = _check_search(engine, "bench", hmm, seqs, {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_B": 16, "ITSX_SHARE_GB": 0.0005}, monkeypatch)
    assert st["share_B"] == 16 and st["share_batches"] > 1


FAMILY_L = 100                # four blocks of 32 rows: 0..31, 32..63, 64..95, 96..99


def _family(t_hmm_text, nvar):
    """one profile and nvar + 1 reads of FAMILY_L residues that are equal in their first 64 and differ, each from every other, inside the
    third block: whichever of them the prefix tree takes first is its root (depth 0), every other one shares exactly two blocks with
    it and starts at depth 2.  The profile's consensus lies inside the shared part: every read passes the filter alike."""
    import synth
    hmm = LP.its2_subset(t_hmm_text, 1, 0)
    cons = synth.consensus_motifs(hmm, "")[0]
    rng = np.random.default_rng(77)
    rnd = lambda k: "".join(rng.choice(list("ACGT"), k))
    base = rnd(10) + cons + rnd(FAMILY_L - 10 - len(cons))
    assert len(base) == FAMILY_L and 10 + len(cons) <= 64
    seqs = [base]
    for step in (1, 2, 3):
        for pos in range(64, 96):
            v = list(base)
            v[pos] = "ACGT"[("ACGT".index(v[pos]) + step) % 4]
            seqs.append("".join(v))
    seqs = seqs[:nvar + 1]
    assert len(set(seqs)) == nvar + 1 == len(seqs)
    return hmm, seqs


@pytest.mark.parametrize("nvar", [1, 64, 65, 66])
@pytest.mark.parametrize("sched", ["one_sided", "two_sided"])
def test_a_segment_whose_last_wave_holds_one_pair(engine, t_hmm_text, monkeypatch, nvar, sched):
    """the (batch, depth 2, profile) segment of _family holds nvar pairs: 1 (a segment of one wave of one pair), 64 (one full wave), 65 (a
    full wave and a last wave of ONE pair), 66.  That the segments are these is not taken on trust: the one-sided schedule walks
    FAMILY_L rows for the root and FAMILY_L - 64 for each chain of depth 2, no other split of nvar + 1 chains of this length over the
    depths 0..2 with at least one root gives that sum, and bound_rows -- summed per chain by k_share_rows, per pair by k_share_waves under
    ITSX_SHARE_CHECK -- must be that number.  The two-sided schedule's chains start at the same depths (the same prefix tree)."""
    hmm, seqs = _family(t_hmm_text, nvar)
    env = dict(LP.SCHEDULES[sched], ITSX_SHARE_CHECK=1)
    st, recs = _check_search(engine, ("family", nvar), hmm, seqs, env, monkeypatch)
    assert st["n_unique"] == nvar + 1 == st["n_past_msv"] and st["n_share_helpers"] == 0 and st["share_mismatch"] == 0
    assert st["share_B"] == 32 and st["share_batches"] == 1 and st["share_chains"] > 0
    assert st["bound_rows_full"] == (nvar + 1) * FAMILY_L
    if sched == "one_sided":
        assert st["bound_rows"] == FAMILY_L + nvar * (FAMILY_L - 64) and st["bwd_rows"] == 0
        assert st["n_bound_launches"] == 2                                   # depth 0 and depth 2: nothing at depth 1
    else:
        assert st["two_sided"] == 1 and st["bound_rows"] <= FAMILY_L + nvar * (FAMILY_L - 64)


# ------------------------------------------------------------------------------------------------ selection at the marking tiles
class SmallLists(PairLists):
    """two profiles: [0] n pairs, [1] 65"""
    P = 2
    NCLS = 2
    CLS = np.array([0, 1], np.int8)

    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        self.total = np.array([n, 65], np.int64)
        self.seg = np.zeros(self.P + 1, np.int64)
        self.seg[1:] = np.cumsum((self.total + 63) // 64 * 64)
        self.NP = int(self.seg[-1])
        pr = np.full((self.NP, 4), -1, np.int32)
        for p in range(self.P):
            a, k = int(self.seg[p]), int(self.total[p])
            pr[a:a + k, 0] = np.arange(k)
            pr[a:a + k, 1] = p
            pr[a:a + k, 2] = rng.integers(-1, 256, k)                      # (some ran for their row states only)
            pr[a:a + k, 3] = rng.integers(300, 580, k)
        self.pairs = pr
        self.real = pr[:, 1] >= 0
        self.U = int(self.total.max())
        self.done = (rng.random(self.NP) < 0.25).astype(np.uint8)
        self.b10 = np.zeros(self.NP, np.uint32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, MARK_WAVE - 65 - 64, MARK_WAVE - 128 - 1, MARK_WAVE - 128, MARK_WAVE - 128 + 1, MARK_WAVE - 1, MARK_WAVE, MARK_WAVE + 1,
                               MARK_BLOCK - 128 - 1, MARK_BLOCK - 128, MARK_BLOCK - 128 + 1, MARK_BLOCK - 1, MARK_BLOCK, MARK_BLOCK + 1, 2 * MARK_BLOCK - 128, 2 * MARK_BLOCK + 1])
def test_select_at_the_marking_tiles(engine, n):
    """list lengths (with profile 1's 128 records behind) at and one chunk either side of a marking wave's MARK_K chunks and of a block's,
    so that the chunk past the list's end (count 0) is a wave's first, a wave's last and a block's first; every mode"""
    pl = SmallLists(n, 100 + n)
    rng = np.random.default_rng(200 + n)
    b10 = np.zeros(pl.NP, np.uint32)
    b10[pl.real] = rng.integers(990, 1011, int(pl.real.sum()))
    i = np.arange(pl.NP, dtype=np.uint64)
    # round 0: a group's winner is a pair of the list, a pair that is done, or nobody
    gtop = np.zeros(pl.U * pl.NCLS, np.uint64)
    for p in range(pl.P):
        rows = pl.rows(p)
        pick = rows[rng.random(len(rows)) < 0.5]
        gtop[pl.pairs[pick, 0].astype(np.int64) * pl.NCLS + pl.CLS[p]] = (np.uint64(1000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i[pick])
    _check_list(engine, 0, pl, pl.done.copy(), b10, group=gtop)
    # round 1: thresholds around the bounds, groups without a certain row
    su = rng.permutation(pl.U).astype(np.int32)
    thr = rng.integers(990, 1011, pl.U * pl.NCLS).astype(np.uint64)
    bestc = np.where(rng.random(pl.U * pl.NCLS) < 0.2, np.uint64(0), (thr << np.uint64(40)) | np.uint64(0x12345))
    f1 = _check_list(engine, 1, pl, pl.done.copy(), b10, group=bestc, sorted_uniq=su)
    assert n < 8 or 0 < f1.sum() < pl.real.sum()
    # the top-up round: marking and key list
    slot = np.array([0, 1], np.int32) if n % 2 else np.array([1, -1], np.int32)
    cut = np.array([1005, 992, 0, 1000], np.uint32)
    _check_list(engine, 2, pl, pl.done.copy(), b10, slot=slot, cutoff=cut, n_slots=2)
    f3 = _flags(3, pl, pl.done, b10, slot=slot)
    _, _, _, keys, vals, cnt = _select(engine, 3, pl, pl.done, b10, slot=slot, n_slots=2)
    idx = np.flatnonzero(f3)
    assert cnt == len(idx) and np.array_equal(vals, idx.astype(np.int32))
    assert np.array_equal(keys, (slot[pl.pairs[idx, 1]].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - b10[idx].astype(np.uint64)))


# ------------------------------------------------------------------------------------------------ counters
@pytest.fixture(scope="module")
def recorded(gold):
    with open(os.path.join(gold, "list_passes_stats.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("sched", LP.STATS_SCHEDULES)
@pytest.mark.parametrize("name", list(LP.STATS_INPUTS))
def test_row_counters_are_the_recorded_ones(engine, t_hmm_text, recorded, monkeypatch, name, sched):
    """the unshared schedule's counters are the recorded ones.  A shared schedule's differ from run to run of one build
    (list_passes_inputs.STATS_RECORDED: its trees come out of hash tables), so they are held to what does not: the sums pair by pair that
    ITSX_SHARE_CHECK=1 takes over the same run's list (share_mismatch counts a sum by chain that differs), the lengths of the list's own
    records, and the recorded counters of the unshared schedule, which every pair past the filter contributes to in any schedule"""
    hmm, seqs = LP.stats_input(t_hmm_text, name)
    env = dict(LP.SCHEDULES[sched])
    if sched != "unshared":
        env["ITSX_SHARE_CHECK"] = 1
    LP.lazy_search(engine, hmm, seqs, env, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    st = engine.stats()
    want = recorded["%s/%s" % (name, sched)]
    assert set(want) == set(LP.STATS_RECORDED[sched])
    got = {k: int(st[k]) for k in want}
    print("[%s / %s] %s" % (name, sched, {k: int(st[k]) for k in LP.STATS_KEYS + ("n_share_helpers", "share_mismatch")}))
    assert got == want
    if sched == "unshared":
        assert want["bound_rows"] == want["bound_rows_full"] > 0 and want["bwd_rows"] == 0
        return
    assert st["share_B"] == 32 and st["share_chains"] > 0 and st["two_sided"] == (sched == "two_sided")
    assert st["share_mismatch"] == 0
    recs, _ = engine.debug_lazy_pairs()
    on_list, real = recs["prof"] >= 0, (recs["prof"] >= 0) & (recs["xj"] >= 0)
    assert st["bound_rows_full"] == int(recs["L"][on_list].sum(dtype=np.int64))
    assert int(recs["L"][real].sum(dtype=np.int64)) == recorded["%s/unshared" % name]["bound_rows_full"]
    assert 0 < st["bound_rows"] < st["bound_rows_full"] and (st["bwd_rows"] > 0) == (sched == "two_sided")
