"""Sample sharing in the lazy and compact rows modes (itsx_set_sample_sharing_lazy): one holder per score class goes through the MSV
filter, pass A, the lazy rounds and the domain pipeline, every evaluated reported pair counts for every member's sample, and the kept
rows are copied to the members before finalize.  Truth is never the code under test alone; every case runs three searches in one
context:
  (F)  the batch in the full rows mode, unshared: coordinates and the exact [sample][profile] counters;
  (L0) the lazy or compact mode with the setting off;
  (L1) the same mode with the setting on.
Required of every case: rep_coords / trim_coords of three prefix pairs equal in F, L0 and L1; every sample's winners domtbl.txt
(set_kept_rows), uc.txt and rep.fa byte-equal in L0 and L1; L1's lower counters <= F's <= L1's upper counters, and after finalize()
lower == upper == F's for every completed profile in every sample; the device's classes are the plain-text model's
(tests/sample_classes_exact.py).  `pytest -m gpu`."""
import os

import numpy as np
import pytest

import derep_exact
import sample_classes_exact as sce
from test_gpu_compact import PAIRS
from test_gpu_parity import _its2_subset
from test_gpu_share import _bench_reads

pytestmark = pytest.mark.gpu


def _run(engine, hmm, samples, mode, tmp, share_lazy=False, share_full=False, tag="", complete_all=False, narrow=False):
    """one batch through derep / search / finalize / coordinates / the three writers in rows mode `mode`"""
    seqs = [s for x in samples for s in x]
    S = len(samples)
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)]) if S > 1 else None
    out = {}
    engine.share_samples_lazy = share_lazy
    engine.share_samples = share_full
    engine.set_rows_mode(mode)
    try:
        engine.load_profiles(text=hmm)
        engine.set_reads(seqs)
        if S > 1:
            engine.set_samples(smp, S)
        out["n_unique"] = nu = engine.derep()
        if narrow:
            engine.set_active_uniques(np.ones(nu, np.uint8))
        engine.search()
        P = out["P"] = engine.n_profiles
        out["domz"] = engine.get_domz().copy().reshape(-1, S, P)              # [1 or 2 (lower, upper)][S][P]
        out["info"] = engine.sample_sharing_info()
        out["classes"] = engine.debug_sample_classes().copy() if out["info"]["n_classes"] else None
        out["stats"] = engine.stats()
        engine.finalize()
        out["stats_final"] = engine.stats()
        out["info_final"] = engine.sample_sharing_info()
        out["domz_final"] = engine.get_domz().copy().reshape(-1, S, P)
        out["rep_coords"] = [tuple(a.copy() for a in engine.rep_coords(l, r)) for l, r in PAIRS]
        out["trim_coords"] = [tuple(a.copy() for a in engine.trim_coords(l, r)) for l, r in PAIRS]
        if mode != "full":
            engine.set_kept_rows(True)
            out["kept_reps"] = np.unique(engine.domains()["rep"])
        else:
            out["dom"] = engine.domains()
        files = []
        for i in range(S):
            engine.select_sample(i if S > 1 else -1)
            one = {}
            for kind, write in (("uc", engine.write_uc), ("rep", engine.write_rep_fasta), ("domtbl", engine.write_domtbl)):
                p = os.path.join(str(tmp), "%s%s_%d_%d.%s" % (tag, mode, int(share_lazy), i, kind))
                write(p)
                with open(p, "rb") as f:
                    one[kind] = f.read()
                os.remove(p)
            files.append(one)
        engine.select_sample(-1)
        out["files"] = files
        if complete_all and out["stats_final"]["lazy"] == 1:
            # itsx_lazy_complete by hand for EVERY profile: the completion walks the holders again, counts members, expands its segments
            engine.lazy_complete(np.ones(P, np.int32))
            out["domz_all"] = engine.get_domz().copy().reshape(-1, S, P)
            out["info_all"] = engine.sample_sharing_info()
            engine.finalize()
            out["trim_coords_all"] = [tuple(a.copy() for a in engine.trim_coords(l, r)) for l, r in PAIRS]
    finally:
        engine.share_samples_lazy = False
        engine.share_samples = False
        engine.set_kept_rows(False)
        engine.set_rows_mode(None)
    return out


def _same_coords(a, b, what):
    for k in ("rep_coords", "trim_coords"):
        for (l, r), x, y in zip(PAIRS, a[k], b[k]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), (what, k, l, r)


def _model(samples):
    seqs = [s for x in samples for s in x]
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)])
    return sce.batch_classes(seqs, smp)


_FULL = {}


def _full(engine, hmm, samples, tmp, key):
    """(F), once per (samples, chunking): shared by the lazy and the compact case, and left unchanged"""
    if key not in _FULL:
        f = _run(engine, hmm, samples, "full", tmp, tag="F")
        assert f["info"]["n_classes"] == 0
        _FULL[key] = f
    return _FULL[key]


def _three(engine, hmm, samples, mode, tmp, key, complete_all=True):
    """F, L0, L1 and everything required of every case; returns them with the model's classes"""
    F = _full(engine, hmm, samples, tmp, key)
    L0 = _run(engine, hmm, samples, mode, tmp, share_lazy=False)
    L1 = _run(engine, hmm, samples, mode, tmp, share_lazy=True, complete_all=complete_all)
    assert L0["info"]["n_classes"] == 0 and L0["info"]["n_rows_expanded"] == 0
    assert F["n_unique"] == L0["n_unique"] == L1["n_unique"]
    # ---- the classes are the model's
    class_of, holder, off, members, usample = _model(samples)
    assert L1["n_unique"] == len(class_of)
    assert L1["classes"] is not None and np.array_equal(L1["classes"], class_of)
    assert L1["info"]["n_classes"] == len(holder) and L1["info"]["n_uniques_shared"] == len(class_of) - len(holder)
    # ---- coordinates: F == L0 == L1
    _same_coords(F, L0, "F / L0")
    _same_coords(F, L1, "F / L1")
    # ---- files: L0 == L1, byte for byte
    assert len(L0["files"]) == len(L1["files"]) == len(samples)
    for i, (a, b) in enumerate(zip(L0["files"], L1["files"])):
        for kind in ("domtbl", "uc", "rep"):
            assert a[kind] == b[kind], "sample %d: %s differs between L0 and L1" % (i, kind)
    assert sum(len(a["domtbl"]) for a in L0["files"]) > 0
    # ---- counters
    exact = F["domz"][0]
    lazy = mode == "lazy"
    assert L1["stats"]["lazy"] == int(lazy) and L1["domz"].shape[0] == (2 if lazy else 1)
    lower, upper = L1["domz"][0], L1["domz"][-1]
    print("counters %s: exact sum %d, L1 lower sum %d, L1 upper sum %d, L0 lower sum %d" % (mode, exact.sum(), lower.sum(), upper.sum(), L0["domz"][0].sum()))
    assert (lower <= exact).all(), "a lower counter of the sharing search exceeds the exact count"
    assert (exact <= upper).all(), "an upper counter of the sharing search lies below the exact count"
    assert (L0["domz"][0] <= exact).all() and (exact <= L0["domz"][-1]).all()
    lo_f, up_f = L1["domz_final"][0], L1["domz_final"][-1]
    assert (lo_f <= exact).all() and (exact <= up_f).all()
    if lazy:
        # the profiles finalize() completed: their counters moved (a completion replaces both halves by the count)
        done = ((lo_f != lower) | (up_f != upper)).any(axis=0)
        assert done.sum() <= L1["stats_final"]["n_lazy_completed_profiles"]
        assert (lo_f[:, done] == exact[:, done]).all() and (up_f[:, done] == exact[:, done]).all()
        settled = ((lo_f == exact) & (up_f == exact)).all(axis=0)
        assert settled.sum() >= L1["stats_final"]["n_lazy_completed_profiles"]
        if complete_all:
            assert (L1["domz_all"][0] == exact).all() and (L1["domz_all"][1] == exact).all(), "after a completion of every profile the counters are not the exact ones"
            assert L1["info_all"]["n_rows_expanded"] >= L1["info_final"]["n_rows_expanded"]
            for (l, r), x, y in zip(PAIRS, F["trim_coords"], L1["trim_coords_all"]):
                assert all(np.array_equal(p, q) for p, q in zip(x, y)), ("after lazy_complete", l, r)
    else:
        assert np.array_equal(lower, exact) and np.array_equal(L0["domz"][0], exact)          # every pair is evaluated: exact
    # ---- rows were copied wherever a unique that was not scored keeps a row
    not_scored = np.setdiff1d(np.arange(len(class_of)), holder)
    if np.intersect1d(L0["kept_reps"], not_scored).size:
        assert L1["info"]["n_rows_expanded"] > 0
    if len(holder) == len(class_of):
        assert L1["info"]["n_rows_expanded"] == 0
    return F, L0, L1, (class_of, holder, off, members, usample)


@pytest.fixture(scope="module")
def hmm20(t_hmm_text):
    return _its2_subset(t_hmm_text, 20, 20)


@pytest.fixture(scope="module")
def bench300(t_hmm_text):
    return _bench_reads(t_hmm_text, 300, seed=17)


# ------------------------------------------------------------------ 1. three identical samples
@pytest.mark.parametrize("chunk", [None, "37"])
@pytest.mark.parametrize("mode", ["lazy", "compact"])
def test_three_identical_samples_are_scored_once(engine, hmm20, fixture_reads, bench300, tmp_path, monkeypatch, mode, chunk):
    """C = one sample's uniques and the HMM stages walk a third of the pairs; with ITSX_CHUNK_UNIQUES=37 the search leaves several
    row segments per round, each counted before its compaction and each expanded.  Compact: every pair is evaluated, the counters are
    F's exactly.  Lazy, with the prefix-tree schedules off (ITSX_SHARE=0: lane = pair in the unshared kernels, so pass A's arithmetic
    per pair does not depend on which other uniques are searched): the same pairs are evaluated, L1's lower counters are L0's
    (it held on the device: 0 of the counters differ; with the tree schedules on, the general requirement is "valid bounds")."""
    if chunk:
        monkeypatch.setenv("ITSX_CHUNK_UNIQUES", chunk)
    one = list(fixture_reads[1][:150]) + bench300[:100]
    samples = [list(one), list(one), list(one)]
    F, L0, L1, (class_of, holder, _, _, _) = _three(engine, hmm20, samples, mode, tmp_path, ("three", chunk))
    u1 = F["n_unique"] // 3
    assert F["n_unique"] == 3 * u1
    assert L1["info"]["n_classes"] == u1 and L1["info"]["n_uniques_shared"] == 2 * u1
    assert L1["stats"]["n_pairs"] * 3 == L0["stats"]["n_pairs"]                        # the HMM stages walked the holders only
    assert L1["info"]["n_rows_expanded"] > 0 and L1["info"]["n_rows_expanded"] % 2 == 0      # every kept row twice more
    if chunk:
        assert L1["stats"]["n_pairs"] // L1["P"] > 37                                  # (several chunks)
    if mode == "compact":
        assert np.array_equal(L1["domz"], L0["domz"]) and np.array_equal(L1["domz"][0], F["domz"][0])
    else:
        monkeypatch.setenv("ITSX_SHARE", "0")
        P0 = _run(engine, hmm20, samples, mode, tmp_path, share_lazy=False, tag="p")
        P1 = _run(engine, hmm20, samples, mode, tmp_path, share_lazy=True, tag="p")
        monkeypatch.delenv("ITSX_SHARE")
        print("ITSX_SHARE=0 lower counters: L0 sum %d, L1 sum %d, differing %d" % (P0["domz"][0].sum(), P1["domz"][0].sum(), (P0["domz"][0] != P1["domz"][0]).sum()))
        assert P1["info"]["n_classes"] == u1
        assert np.array_equal(P1["domz"][0], P0["domz"][0]), "ITSX_SHARE=0: the sharing search's lower counters are not the unshared search's"
        exact = F["domz"][0]
        assert (P1["domz"][0] <= exact).all() and (exact <= P1["domz"][1]).all()
        _same_coords(F, P0, "F / L0, ITSX_SHARE=0")
        _same_coords(F, P1, "F / L1, ITSX_SHARE=0")
        for a, b in zip(P0["files"], P1["files"]):
            assert a == b


def test_the_environment_switch_turns_the_mode_on(engine, hmm20, fixture_reads, tmp_path, monkeypatch):
    one = list(fixture_reads[1][:60])
    samples = [list(one), one[::-1]]
    off = _run(engine, hmm20, samples, "lazy", tmp_path)
    monkeypatch.setenv("ITSX_SHARE_SAMPLES_LAZY", "1")
    env = _run(engine, hmm20, samples, "lazy", tmp_path)
    full = _run(engine, hmm20, samples, "full", tmp_path)              # the switch is the lazy / compact modes' alone
    monkeypatch.delenv("ITSX_SHARE_SAMPLES_LAZY")
    assert off["info"]["n_classes"] == 0 and env["info"]["n_classes"] == off["n_unique"] // 2 > 0 and full["info"]["n_classes"] == 0
    _same_coords(off, env, "switch")
    _same_coords(full, env, "switch / full")
    assert off["files"] == env["files"]
    assert engine.switches().get("ITSX_SHARE_SAMPLES_LAZY") == "1"


# ------------------------------------------------------------------ 2. reporting differs inside a class
@pytest.mark.parametrize("scale", [None, "500000"])
def test_one_class_is_reported_in_the_small_sample_and_not_in_the_large(engine, hmm20, fixture_reads, bench300, tmp_path, monkeypatch, scale):
    """the samples of tests/test_gpu_sample_sharing.py's case: weak second domains sit in a sample of 20 reads AND in one of 427
    strongly reported reads, so a row is reported under the small sample's domZ and not under the large one's.  The flip must exist
    in F (asserted); L1 must reproduce coordinates and winners files from ONE scored holder.  With ITSX_LAZY_ZUB_SCALE=500000 (upper
    bounds as of a data set that much larger) rows stay undecided and the completion path runs, with sharing too."""
    seqs = list(fixture_reads[1])
    small = seqs[90:110]
    large = seqs + bench300[:200]
    samples = [small, large]
    F = _full(engine, hmm20, samples, tmp_path, "flip")
    class_of, holder, _, members, usample = _model(samples)
    d = F["dom"]
    key = lambda rows: {(int(class_of[r["rep"]]), int(r["prof"]), int(r["dom_idx"])): int(r["dom_reported"]) for r in rows}
    rows_small, rows_large = key(d[usample[d["rep"]] == 0]), key(d[usample[d["rep"]] == 1])
    flips = [k for k, v in rows_small.items() if v == 1 and rows_large.get(k) == 0]
    assert len(flips) >= 1, "no row is reported in the small sample and unreported in the large one: the case tests nothing"
    z = F["domz"][0]
    assert all(z[0, k[1]] < z[1, k[1]] for k in flips)
    if scale:
        monkeypatch.setenv("ITSX_LAZY_ZUB_SCALE", scale)
    F2, L0, L1, _ = _three(engine, hmm20, samples, "lazy", tmp_path, "flip")
    assert L1["info"]["n_uniques_shared"] >= 15 and L1["info"]["n_rows_expanded"] > 0
    if scale:
        print("completed profiles: L0 %d, L1 %d" % (L0["stats_final"]["n_lazy_completed_profiles"], L1["stats_final"]["n_lazy_completed_profiles"]))
        assert L0["stats_final"]["n_lazy_completed_profiles"] > 0
        assert L1["stats_final"]["n_lazy_completed_profiles"] > 0                     # the completion path ran with sharing
        assert L1["stats_final"]["n_lazy_reruns"] == 0
        assert L1["info_final"]["n_rows_expanded"] >= L1["info"]["n_rows_expanded"]


# ------------------------------------------------------------------ 3. degenerate shapes
@pytest.mark.parametrize("mode", ["lazy", "compact"])
def test_degenerate_shapes(engine, hmm20, fixture_reads, tmp_path, mode):
    """an empty sample in the middle, a sample of one read, 65 samples of one shared read each (one class's member list is longer
    than a wave: 65 member counts per counted row), and multidomain targets (s + s[40:], the ensemble stage) shared by two samples"""
    seqs = list(fixture_reads[1])
    multi = [s + s[40:] for s in seqs[:12]]
    samples = [seqs[:60] + multi, [], [seqs[5]], multi[::-1] + seqs[30:80]] + [[seqs[7]] for _ in range(65)]
    F, L0, L1, (class_of, holder, offs, members, usample) = _three(engine, hmm20, samples, mode, tmp_path, "degenerate")
    assert np.diff(offs).max() == 66 and len(samples) == 69                  # seqs[7]: sample 0 and the 65
    assert L0["stats"]["n_mr_clustered"] > 0 and L1["stats"]["n_mr_clustered"] > 0          # the ensemble stage ran, for the holders
    # the 65 one-read samples: each has exactly the counters of the holder's pairs, i.e. all the same row of F
    exact = F["domz"][0]
    assert (exact[4:] == exact[4]).all() and exact[4].sum() > 0
    assert (L1["domz"][0][4:] == L1["domz"][0][4]).all()
    assert L1["info"]["n_rows_expanded"] >= 65


# ------------------------------------------------------------------ 4. a sample and its reverse complement
def test_a_reverse_complemented_sample_shares_nothing(engine, hmm20, fixture_reads, bench300, tmp_path):
    fwd = list(fixture_reads[1][:120]) + bench300[100:160]
    rev = [derep_exact.rc(derep_exact.norm(s)) for s in fwd]
    samples = [fwd, rev]
    F, L0, L1, (class_of, holder, _, _, usample) = _three(engine, hmm20, samples, "lazy", tmp_path, "rc")
    assert len(holder) == len(class_of) and L1["info"]["n_uniques_shared"] == 0 and L1["info"]["n_rows_expanded"] == 0
    assert L1["stats"]["n_pairs"] == L0["stats"]["n_pairs"]                  # C == U: the plain search
    assert np.array_equal(L1["domz"], L0["domz"]) and np.array_equal(L1["domz_final"], L0["domz_final"])
    # with a third sample that repeats part of the first one forward, sharing happens beside it -- and still no class spans 0 and 1
    samples = [fwd, rev, fwd[:50]]
    F, L0, L1, (class_of, holder, _, _, usample) = _three(engine, hmm20, samples, "lazy", tmp_path, "rc3")
    assert L1["info"]["n_uniques_shared"] == (usample == 2).sum() > 0
    assert not set(class_of[usample == 0].tolist()) & set(class_of[usample == 1].tolist())
    assert L1["info"]["n_rows_expanded"] > 0


# ------------------------------------------------------------------ 5. the safety net
def test_the_compact_re_search_after_a_sharing_search(engine, hmm20, fixture_reads, bench300, tmp_path, monkeypatch):
    """ITSX_LAZY_FORCE_PENDING=3: finalize() finds rows pending after the completion and searches again in the compact mode -- a sharing
    search itself -- and the coordinates are F's"""
    one = list(fixture_reads[1][:110]) + bench300[:70]
    samples = [list(one), one[::-1] + bench300[200:230], list(one[:40])]
    F = _full(engine, hmm20, samples, tmp_path, "net")
    monkeypatch.setenv("ITSX_LAZY_FORCE_PENDING", "3")
    L0 = _run(engine, hmm20, samples, "lazy", tmp_path)
    L1 = _run(engine, hmm20, samples, "lazy", tmp_path, share_lazy=True)
    monkeypatch.delenv("ITSX_LAZY_FORCE_PENDING")
    for L in (L0, L1):
        assert L["stats_final"]["n_lazy_reruns"] == 1 and L["stats_final"]["n_lazy_pending"] >= 3 and L["stats_final"]["lazy"] == 0
    class_of, holder, _, _, _ = _model(samples)
    assert L1["info"]["n_classes"] == len(holder) < len(class_of) and np.array_equal(L1["classes"], class_of)
    assert L1["info_final"]["n_classes"] == len(holder) and L1["info_final"]["n_rows_expanded"] > 0        # the re-search shared too
    assert L1["stats_final"]["n_pairs"] == len(holder) * L1["P"]
    _same_coords(F, L0, "F / L0")
    _same_coords(F, L1, "F / L1")
    assert L0["files"] == L1["files"]
    assert np.array_equal(L1["domz_final"][0], F["domz"][0])                 # the compact search counts exactly


def test_pair_traces_of_a_compact_sharing_search_follow_the_classes(hmm20, fixture_reads, bench300):
    """a compact search keeps pair traces, and after a sharing one every member gets its holder's, as in the full mode: the table of
    the unshared compact search, on fresh contexts (the sharing search first: no buffer of a larger search to read from)"""
    from itsxpress_amd import Engine
    one = list(fixture_reads[1][:90]) + bench300[:60]
    samples = [list(one), one[::-1] + bench300[200:230], [], list(one[:40])] + [[one[3]] for _ in range(30)]
    seqs = [s for x in samples for s in x]
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)])
    got = {}
    for share in (True, False):
        eng = Engine(0)
        try:
            eng.share_samples_lazy = share
            eng.set_rows_mode("compact")
            eng.load_profiles(text=hmm20)
            eng.set_reads(seqs)
            eng.set_samples(smp, len(samples))
            nu = eng.derep()
            eng.search()
            tr = eng.pairtraces()
            got[share] = (tr[np.lexsort((tr["rep"], tr["prof"]))], eng.sample_sharing_info(), nu)
        finally:
            eng.close()
    (on, info, nu), (off, info0, nu0) = got[True], got[False]
    assert info0["n_classes"] == 0 and 0 < info["n_classes"] < nu == nu0
    assert len(off) > 2000 and len(on) == len(off)
    for f in off.dtype.names:
        assert on[f].tobytes() == off[f].tobytes(), "pair traces: field %s differs" % f


# ------------------------------------------------------------------ 6. where the setting has no effect
def test_no_effect(engine, hmm20, fixture_reads, bench300, tmp_path):
    one = list(fixture_reads[1][:100]) + bench300[:60]
    zero = dict(n_classes=0, n_uniques_shared=0, n_rows_expanded=0, ms_classes=0.0, ms_expand=0.0)
    # S == 1
    off = _run(engine, hmm20, [one + one], "lazy", tmp_path)
    on = _run(engine, hmm20, [one + one], "lazy", tmp_path, share_lazy=True)
    assert on["info"] == zero and on["stats"]["n_pairs"] == off["stats"]["n_pairs"]
    _same_coords(off, on, "S == 1")
    assert np.array_equal(on["domz_final"], off["domz_final"]) and on["files"] == off["files"]
    samples = [list(one), list(one)]
    # a caller's own choice of active uniques is left alone
    off = _run(engine, hmm20, samples, "lazy", tmp_path)
    on = _run(engine, hmm20, samples, "lazy", tmp_path, share_lazy=True, narrow=True)
    assert on["info"] == zero and on["stats"]["n_pairs"] == off["stats"]["n_pairs"]
    _same_coords(off, on, "narrowed")
    # the full rows mode is share_samples' alone
    full_off = _run(engine, hmm20, samples, "full", tmp_path)
    full_on = _run(engine, hmm20, samples, "full", tmp_path, share_lazy=True)
    assert full_on["info"] == zero and full_on["stats"]["n_pairs"] == full_off["stats"]["n_pairs"]
    assert np.array_equal(full_on["domz"], full_off["domz"]) and full_on["files"] == full_off["files"]
    # ... and the lazy mode is not share_samples': the existing pin, against the new property's default
    assert engine.share_samples_lazy is False
    on = _run(engine, hmm20, samples, "lazy", tmp_path, share_full=True)
    assert on["info"] == zero and on["stats"]["n_pairs"] == off["stats"]["n_pairs"]
    assert np.array_equal(on["domz"], off["domz"]) and on["files"] == off["files"]
    _same_coords(off, on, "share_samples in the lazy mode")
    # with the setting on, the same two samples do share
    on = _run(engine, hmm20, samples, "lazy", tmp_path, share_lazy=True)
    assert on["info"]["n_classes"] == on["n_unique"] // 2 and on["stats"]["n_pairs"] * 2 == off["stats"]["n_pairs"]


# ------------------------------------------------------------------ 7. through SampleBatch
@pytest.mark.parametrize("ali", [False, True])
def test_sample_batch_with_share_samples_lazy(engine, fixture_reads, bench300, t_hmm_text, mini_hmm_text, tmp_path, monkeypatch, ali):
    """ITSXPRESS_DOMTBL=winners searches lazily; with ITSXPRESS_DOMTBL_ALI=1 the aligned columns of a member's row come from the
    member's own copy of the text"""
    from itsxpress_amd import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    names, seqs = fixture_reads
    parts = [(names[:120], seqs[:120]), (names[60:], seqs[60:]),
             (["b%04d" % i for i in range(80)] + names[:40][::-1], bench300[:80] + [derep_exact.rc(s) for s in seqs[:40]][::-1]),
             (names[100:140] + ["c%04d" % i for i in range(40)], seqs[100:140] + bench300[40:80])]
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(mini_hmm_text + _its2_subset(t_hmm_text, 12, 12))
    fqs = []
    for k, (nm, sq) in enumerate(parts):
        fq = tmp_path / ("sample%d.fq" % k)
        fq.write_text("".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in zip(nm, sq)))
        fqs.append(str(fq))
    monkeypatch.setenv("ITSXPRESS_DOMTBL", "winners")
    if ali:
        monkeypatch.setenv("ITSXPRESS_DOMTBL_ALI", "1")
    got = {}
    try:
        for share in (False, True):
            d = tmp_path / ("share%d" % share)
            os.makedirs(d)
            objs = [SeqSampleNotPaired(fq, str(d)) for fq in fqs]
            b = SampleBatch(objs, engine=engine)
            b.share_samples_lazy = share
            assert b.share_samples_lazy is share and engine.share_samples_lazy is share and b.share_samples is False
            b.deduplicate(threads=1)
            b._search(hmmfile=str(hmm), threads=1)
            info = engine.sample_sharing_info()
            assert engine.stats()["lazy"] == 1
            coords = [[x.copy() for x in per] for per in b.trim_coordinates("ITS2")]
            outs = [str(d / ("trimmed%d.fq" % k)) for k in range(len(objs))]
            written = b.write_trimmed(outs, "ITS2")
            files = [{f: open(getattr(s, f), "rb").read() for f in ("uc_file", "rep_file", "dom_file")} for s in objs]
            got[share] = (coords, [tuple(w) for w in written], files, [open(o, "rb").read() for o in outs], info)
    finally:
        engine.share_samples_lazy = False
    assert got[False][4]["n_classes"] == 0 and got[True][4]["n_uniques_shared"] > 100 and got[True][4]["n_rows_expanded"] > 0
    for k in range(len(parts)):
        for x, y in zip(got[False][0][k], got[True][0][k]):
            assert np.array_equal(x, y)
        for f in ("uc_file", "rep_file", "dom_file"):
            assert got[False][2][k][f] == got[True][2][k][f], (k, f)
        assert got[False][3][k] == got[True][3][k]
        assert len(got[True][2][k]["dom_file"]) > 1000
    assert got[False][1] == got[True][1] and sum(len(t) for t in got[True][3]) > 10000
