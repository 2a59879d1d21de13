"""Sample sharing (itsx_set_sample_sharing): a batch scores each distinct representative once for all the samples it occurs in (the
reference runs one hmmsearch per manifest row, q2_itsxpress.py:273-333) and every sample still gets exactly the results of a batch
without the mode.  Truth in every case is the SAME batch in the same context with the mode off; compared exactly: every field of the
row table, the [sample][profile] counters, the coordinates per unique and per read for three prefix pairs, and every sample's
domtbl.txt / uc.txt / rep.fa byte for byte.  The classes the device built are held to the plain-text model
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


def _run(engine, hmm, samples, share, tmp, rows_mode=None, tag=""):
    """one batch through derep / search / finalize / coordinates / the three writers; everything the mode must leave alone"""
    seqs = [s for x in samples for s in x]
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)]) if len(samples) > 1 else None
    S = len(samples)
    out = {}
    engine.share_samples = share
    if rows_mode:
        engine.set_rows_mode(rows_mode)
    try:
        engine.load_profiles(text=hmm)
        engine.set_reads(seqs)
        if S > 1:
            engine.set_samples(smp, S)
        out["n_unique"] = engine.derep()
        engine.search()
        out["domz"] = engine.get_domz().copy()
        out["info"] = engine.sample_sharing_info()
        out["classes"] = engine.debug_sample_classes().copy() if out["info"]["n_classes"] else None
        out["stats"] = engine.stats()
        engine.finalize()
        if rows_mode in (None, "full"):
            dom = engine.domains()
            out["dom"] = dom[np.lexsort((dom["dom_idx"], dom["prof"], dom["rep"]))]
        out["rep_coords"] = [tuple(a.copy() for a in engine.rep_coords(l, r)) for l, r in PAIRS]
        out["trim_coords"] = [tuple(a.copy() for a in engine.trim_coords(l, r)) for l, r in PAIRS]
        files = []
        for i in range(S):
            engine.select_sample(i if S > 1 else -1)
            one = {}
            for kind, write in (("uc", engine.write_uc), ("rep", engine.write_rep_fasta)) + ((("domtbl", engine.write_domtbl),) if "dom" in out else ()):
                p = os.path.join(str(tmp), "%s%s_%d.%s" % (tag, "on" if share else "off", i, kind))
                write(p)
                with open(p, "rb") as f:
                    one[kind] = f.read()
                os.remove(p)
            files.append(one)
        engine.select_sample(-1)
        out["files"] = files
    finally:
        engine.share_samples = False
        if rows_mode:
            engine.set_rows_mode(None)
    return out


def _assert_equal(off, on):
    assert on["n_unique"] == off["n_unique"]
    assert np.array_equal(on["domz"], off["domz"]), "domZ counters differ"
    if "dom" in off:
        assert len(on["dom"]) == len(off["dom"]), (len(on["dom"]), len(off["dom"]))
        for f in off["dom"].dtype.names:
            assert on["dom"][f].tobytes() == off["dom"][f].tobytes(), "row table: field %s differs" % f
    for k in ("rep_coords", "trim_coords"):
        for (l, r), a, b in zip(PAIRS, off[k], on[k]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, l, r)
    assert len(on["files"]) == len(off["files"])
    for i, (a, b) in enumerate(zip(off["files"], on["files"])):
        for kind in a:
            assert a[kind] == b[kind], "sample %d: %s differs" % (i, kind)


def _model(samples):
    seqs = [s for x in samples for s in x]
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)])
    return sce.batch_classes(seqs, smp)


def _assert_classes(on, samples):
    """the device's classes are the model's: same numbering (holders in rising unique index), none merged, none split"""
    class_of, holder, off, members, usample = _model(samples)
    assert on["n_unique"] == len(class_of)
    assert on["classes"] is not None and np.array_equal(on["classes"], class_of)
    assert on["info"]["n_classes"] == len(holder) and on["info"]["n_uniques_shared"] == len(class_of) - len(holder)
    return class_of, holder, off, members, usample


def _both(engine, hmm, samples, tmp, tag=""):
    off = _run(engine, hmm, samples, False, tmp, tag=tag)
    assert off["info"] == dict(n_classes=0, n_uniques_shared=0, n_rows_expanded=0, ms_classes=0.0, ms_expand=0.0)
    on = _run(engine, hmm, samples, True, tmp, tag=tag)
    _assert_equal(off, on)
    return off, on


@pytest.fixture(scope="module")
def hmm20(t_hmm_text):
    return _its2_subset(t_hmm_text, 20, 20)


@pytest.fixture(scope="module")
def bench300(t_hmm_text):
    return _bench_reads(t_hmm_text, 300, seed=17)


# ------------------------------------------------------------------ 1. three identical samples
@pytest.mark.parametrize("chunk", [None, "37"])
def test_three_identical_samples_are_scored_once(engine, hmm20, fixture_reads, bench300, tmp_path, monkeypatch, chunk):
    """C = one sample's uniques, twice that many uniques are not scored; with ITSX_CHUNK_UNIQUES=37 the search leaves several row
    segments and every one of them is expanded"""
    if chunk:
        monkeypatch.setenv("ITSX_CHUNK_UNIQUES", chunk)
    one = list(fixture_reads[1][:150]) + bench300[:100]
    samples = [list(one), list(one), list(one)]
    off, on = _both(engine, hmm20, samples, tmp_path)
    _assert_classes(on, samples)
    u1 = off["n_unique"] // 3
    assert off["n_unique"] == 3 * u1
    assert on["info"]["n_classes"] == u1 and on["info"]["n_uniques_shared"] == 2 * u1
    assert on["info"]["n_rows_expanded"] == 2 * len(off["dom"]) // 3 > 1000
    assert on["stats"]["n_pairs"] * 3 == off["stats"]["n_pairs"]                       # the HMM stages walked the holders only
    # the model's consequence holds in the unshared run itself: a member's rows are its holder's
    class_of, holder, _, _, usample = _model(samples)
    assert sce.expected_from_unshared(off["dom"], off["domz"], class_of, holder, usample, off["domz"].size // 3) == []


def test_the_environment_switch_turns_the_mode_on(engine, hmm20, fixture_reads, tmp_path, monkeypatch):
    one = list(fixture_reads[1][:60])
    samples = [list(one), one[::-1]]
    off = _run(engine, hmm20, samples, False, tmp_path)
    monkeypatch.setenv("ITSX_SHARE_SAMPLES", "1")
    env = _run(engine, hmm20, samples, False, tmp_path)
    monkeypatch.delenv("ITSX_SHARE_SAMPLES")
    assert off["info"]["n_classes"] == 0 and env["info"]["n_classes"] == off["n_unique"] // 2 > 0
    _assert_equal(off, env)
    assert engine.switches().get("ITSX_SHARE_SAMPLES") == "1"


# ------------------------------------------------------------------ 2. a sample and its reverse complement
def test_a_reverse_complemented_sample_shares_nothing(engine, hmm20, fixture_reads, bench300, tmp_path):
    fwd = list(fixture_reads[1][:120]) + bench300[100:160]
    rev = [derep_exact.rc(derep_exact.norm(s)) for s in fwd]
    samples = [fwd, rev]
    off, on = _both(engine, hmm20, samples, tmp_path)
    class_of, holder, _, _, usample = _assert_classes(on, samples)
    assert len(holder) == len(class_of) and on["info"]["n_uniques_shared"] == 0 and on["info"]["n_rows_expanded"] == 0
    # with a third sample that repeats part of the first one forward, sharing happens beside it -- and still no class spans 0 and 1
    samples = [fwd, rev, fwd[:50]]
    off, on = _both(engine, hmm20, samples, tmp_path, tag="b")
    class_of, holder, _, _, usample = _assert_classes(on, samples)
    assert on["info"]["n_uniques_shared"] == (usample == 2).sum() > 0
    assert not set(class_of[usample == 0].tolist()) & set(class_of[usample == 1].tolist())


# ------------------------------------------------------------------ 3. reporting differs inside a class
def test_one_class_is_reported_in_the_small_sample_and_not_in_the_large(engine, hmm20, fixture_reads, bench300, tmp_path):
    """dom_reported = seq_reported and exp(lnP) * domZ[sample][prof] <= domE.  The weak second domains of the fixture reads (the CPU
    oracle gives e.g. read 96 a domain with lnP = -2.93 against a profile that reports every read: exp(lnP) = 0.054, reported while
    that profile's domZ is at most 186) sit in a sample of 20 reads AND in one of 427 strongly reported reads.  The flip must exist in
    the mode-off run -- asserted, so the case cannot pass vacuously -- and the shared run must reproduce it from ONE scored holder."""
    seqs = list(fixture_reads[1])
    small = seqs[90:110]
    large = seqs + bench300[:200]
    samples = [small, large]
    off, on = _both(engine, hmm20, samples, tmp_path)
    class_of, holder, _, members, usample = _assert_classes(on, samples)
    d = off["dom"]
    key = lambda rows: {(int(class_of[r["rep"]]), int(r["prof"]), int(r["dom_idx"])): int(r["dom_reported"]) for r in rows}
    rows_small, rows_large = key(d[usample[d["rep"]] == 0]), key(d[usample[d["rep"]] == 1])
    flips = [k for k, v in rows_small.items() if v == 1 and rows_large.get(k) == 0]
    assert len(flips) >= 1, "no row is reported in the small sample and unreported in the large one: the case tests nothing"
    P = off["domz"].size // 2
    z = off["domz"].reshape(2, P)
    assert all(z[0, k[1]] < z[1, k[1]] for k in flips)
    # (the equality of the two runs, flips included, is _both's)
    dn = on["dom"]
    assert key(dn[usample[dn["rep"]] == 0]) == rows_small and key(dn[usample[dn["rep"]] == 1]) == rows_large


# ------------------------------------------------------------------ 4. packing edges
def _other(b):
    return "C" if b != "C" else "G"


def test_classes_at_the_packing_edges(engine, hmm20, fixture_reads, tmp_path):
    """representatives of 31 / 32 / 33 and 63 / 64 / 65 bases (the 16-base word and the 64-bit key word end there), pairs equal but
    for the last base, pairs equal but for N against A at one position (first base, word boundary, last base), one sample's copy
    in lower case: the classes are the model's, none merged and none split"""
    rng = np.random.default_rng(5)
    variants = []
    for L in (31, 32, 33, 63, 64, 65):
        t = "".join(rng.choice(list("CGT"), L))                  # no A: "A at p" is always another text
        variants += [t, t[:-1] + _other(t[-1])]
        for p in sorted({0, 15, 16, 31 if L > 32 else L - 1, L - 1}):
            variants += [t[:p] + "N" + t[p + 1:], t[:p] + "A" + t[p + 1:], t[:p] + "R" + t[p + 1:]]
    assert len(set(variants)) == len(variants)
    assert not {derep_exact.rc(v) for v in variants} & set(variants)      # (no variant is another's reverse complement: a sample keeps them all)
    real = list(fixture_reads[1][:40])
    samples = [variants + real,
               [v.lower() for v in variants[::-1]] + real,               # lower case, other order
               [derep_exact.rc(v) for v in variants[::2]] + variants[1::2],      # every other one only as its reverse complement
               variants[:7]]
    off, on = _both(engine, hmm20, samples, tmp_path)
    class_of, holder, offs, members, usample = _assert_classes(on, samples)
    nv = len(variants)
    # what the model says here, spelled out: every variant forward in samples 0 and 1 (and 3, the first seven), the odd ones in 2
    sizes = np.diff(offs)
    assert (sizes == 1).sum() == (nv + 1) // 2 and sizes.max() == 4
    assert on["info"]["n_classes"] == nv + (nv + 1) // 2 + derep_exact.derep(real)[0]


# ------------------------------------------------------------------ 5. degenerate shapes
def test_degenerate_shapes(engine, hmm20, fixture_reads, tmp_path):
    """an empty sample in the middle, a sample of one read, 65 samples of one shared read each (one class's member list is longer
    than a wave), and multidomain targets (s + s[40:], the ensemble stage) shared by two samples"""
    seqs = list(fixture_reads[1])
    multi = [s + s[40:] for s in seqs[:12]]
    samples = [seqs[:60] + multi, [], [seqs[5]], multi[::-1] + seqs[30:80]] + [[seqs[7]] for _ in range(65)]
    off, on = _both(engine, hmm20, samples, tmp_path)
    class_of, holder, offs, members, usample = _assert_classes(on, samples)
    assert np.diff(offs).max() == 66 and len(samples) == 69                  # seqs[7]: sample 0 and the 65
    assert off["stats"]["n_mr_clustered"] > 0 and on["stats"]["n_mr_clustered"] > 0          # the ensemble stage ran, for the holders
    d = on["dom"]
    assert ((d["flags"] & 1) == 1).any()
    shared_multi = d[(usample[d["rep"]] == 3) & ((d["flags"] & 1) == 1)]
    assert len(shared_multi) > 0                                             # ... and its envelopes reached the sample that did not run it


# ------------------------------------------------------------------ the pair traces follow the classes too
@pytest.mark.parametrize("prefix_share", [None, "0"])
@pytest.mark.parametrize("keep_trace", [False, True])
def test_pair_traces_equal_the_unshared_search(hmm20, fixture_reads, bench300, monkeypatch, prefix_share, keep_trace):
    """itsx_get_pairtraces after a sharing search, on a FRESH context (no buffer of an earlier, larger search to read from): a
    one-chunk search fetches its traces after the search has returned, when the context walks all its uniques again, so the traces
    must be mapped through the list the search walked (the holders) -- with prefix sharing's processing order (the default) and with
    the plain length order (ITSX_SHARE=0) -- and every member gets its holder's traces.  With ITSX_KEEP_TRACE=1 and several chunks
    the traces are appended chunk by chunk during the search."""
    from itsxpress_amd import Engine
    if prefix_share is not None:
        monkeypatch.setenv("ITSX_SHARE", prefix_share)
    if keep_trace:
        monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
        monkeypatch.setenv("ITSX_CHUNK_UNIQUES", "41")
    one = list(fixture_reads[1][:90]) + bench300[:60]
    samples = [list(one), one[::-1] + bench300[200:230], [], list(one[:40])] + [[one[3]] for _ in range(30)]
    seqs = [s for x in samples for s in x]
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)])
    got = {}
    for share in (True, False):                        # the sharing search first: nothing larger has run on its context
        eng = Engine(0)
        try:
            eng.share_samples = share
            eng.load_profiles(text=hmm20)
            eng.set_reads(seqs)
            eng.set_samples(smp, len(samples))
            nu = eng.derep()
            eng.search()
            info = eng.sample_sharing_info()
            tr = eng.pairtraces()
            got[share] = (tr[np.lexsort((tr["rep"], tr["prof"]))], info, nu, eng.stats())
        finally:
            eng.close()
    (on, info, nu, st_on), (off, info0, nu0, st_off) = got[True], got[False]
    assert info0["n_classes"] == 0 and 0 < info["n_classes"] < nu == nu0
    assert len(off) > 2000 and len(on) == len(off)
    for f in off.dtype.names:
        assert on[f].tobytes() == off[f].tobytes(), "pair traces: field %s differs" % f
    # itsx_stats describes the work done: the holders' residues, not the first n_classes uniques'
    assert 0 < st_on["msv_rows_full"] < st_off["msv_rows_full"]
    class_of, holder, _, _, _ = _model(samples)
    lens = np.array([len(t) for t in sce.representatives(seqs, smp)[0]])
    assert st_on["msv_rows_full"] == int(lens[holder].sum()) * (st_on["n_pairs"] // info["n_classes"])
    assert st_off["msv_rows_full"] == int(lens.sum()) * (st_off["n_pairs"] // nu)


# ------------------------------------------------------------------ 6. where the mode has no effect
def test_no_effect_on_one_sample_and_in_the_lazy_mode(engine, hmm20, fixture_reads, bench300, tmp_path):
    one = list(fixture_reads[1][:100]) + bench300[:60]
    off, on = _both(engine, hmm20, [one + one], tmp_path)                    # S == 1
    assert on["info"]["n_classes"] == 0 and on["info"]["n_rows_expanded"] == 0
    samples = [list(one), list(one)]
    off = _run(engine, hmm20, samples, False, tmp_path, rows_mode="lazy")
    on = _run(engine, hmm20, samples, True, tmp_path, rows_mode="lazy")
    _assert_equal(off, on)
    assert on["info"]["n_classes"] == 0 and on["info"]["n_uniques_shared"] == 0
    assert on["stats"]["n_pairs"] == off["stats"]["n_pairs"]
    # a caller's own choice of active uniques is left alone
    engine.share_samples = True
    try:
        engine.load_profiles(text=hmm20)
        engine.set_reads(one + one)
        engine.set_samples(np.repeat(np.arange(2, dtype=np.int32), len(one)), 2)
        nu = engine.derep()
        engine.set_active_uniques(np.ones(nu, np.uint8))
        engine.search()
        assert engine.sample_sharing_info()["n_classes"] == 0
        engine.derep()                                                       # a new dereplication gives the choice back to the engine
        engine.search()
        assert engine.sample_sharing_info()["n_classes"] == nu // 2
    finally:
        engine.share_samples = False


# ------------------------------------------------------------------ 7. through SampleBatch
def test_sample_batch_with_share_samples(engine, fixture_reads, bench300, t_hmm_text, mini_hmm_text, tmp_path):
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
    got = {}
    try:
        for share in (False, True):
            d = tmp_path / ("share%d" % share)
            os.makedirs(d)
            objs = [SeqSampleNotPaired(fq, str(d)) for fq in fqs]
            b = SampleBatch(objs, engine=engine)
            b.share_samples = share
            assert b.share_samples is share and engine.share_samples is share
            b.deduplicate(threads=1)
            b._search(hmmfile=str(hmm), threads=1)
            info = engine.sample_sharing_info()
            coords = [[x.copy() for x in per] for per in b.trim_coordinates("ITS2")]
            outs = [str(d / ("trimmed%d.fq" % k)) for k in range(len(objs))]
            written = b.write_trimmed(outs, "ITS2")
            files = [{f: open(getattr(s, f), "rb").read() for f in ("uc_file", "rep_file", "dom_file")} for s in objs]
            got[share] = (coords, [tuple(w) for w in written], files, [open(o, "rb").read() for o in outs], info)
    finally:
        engine.share_samples = False
    assert got[False][4]["n_classes"] == 0 and got[True][4]["n_uniques_shared"] > 100 and got[True][4]["n_rows_expanded"] > 1000
    for k in range(len(parts)):
        for x, y in zip(got[False][0][k], got[True][0][k]):
            assert np.array_equal(x, y)
        assert got[False][2][k] == got[True][2][k] and got[False][3][k] == got[True][3][k]
    assert got[False][1] == got[True][1] and sum(len(t) for t in got[True][3]) > 10000
