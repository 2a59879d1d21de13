"""GPU tests of orientation by the profiles (itsx_orient_profiles / itsx_orient_profiles_apply): the strands and counts equal the
plain-Python rule of tests/orient_profiles_exact.py, fed from the oracle's pair traces and from the engine's own; they do not depend on
the schedule; applying them leaves the read set a forward-strand input leaves; the mirror's batch equals its solo runs.  Every
comparison is exact."""
import gzip
import os

import numpy as np
import pytest

import orc
import orient_profiles_exact as ope

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ inputs, the model's side computed once
@pytest.fixture(scope="module")
def mini(mini_hmm_text):
    return orc.HmmSet(text=mini_hmm_text)


@pytest.fixture(scope="module")
def cat(mini, mini_hmm_text):
    reads, samples, kinds = ope.catalogue(mini_hmm_text)
    rep_of, rs = ope.derep(reads, samples)
    nf, nr = ope.oracle_counts(mini, reads)
    return dict(reads=reads, samples=samples, kinds=kinds, rep_of=rep_of, rs=rs, nf=nf, nr=nr, model=ope.model(nf, nr, rep_of, rs))


@pytest.fixture(scope="module")
def flipped_fixture(fixture_reads):
    _, seqs = fixture_reads
    return [ope.revcomp(s) if i % 3 == 2 else s for i, s in enumerate(seqs)]


def _engine_counts(engine, texts, F1=1e-6):
    """(n_fwd, n_rev) from the engine's own pair traces of a plain search over explicit texts (ITSX_KEEP_TRACE is set by the caller)"""
    def search(distinct):
        engine.set_reads(distinct)
        assert engine.derep(strand_both=False, minseqlength=1) == len(distinct)      # unique u is text u
        engine.search(F1=F1)
        return ope.trace_counts(engine.pairtraces(), len(distinct))
    return ope.counts_by(texts, search)


def _load(engine, c):
    engine.set_reads(c["reads"])
    engine.set_samples(c["samples"], int(c["samples"].max()) + 1)


def _same(got, m):
    strand, cf, cr = got
    bad = [r for r in range(len(strand)) if (int(strand[r]), int(cf[r]), int(cr[r])) != (int(m["strand"][r]), int(m["count_fwd"][r]), int(m["count_rev"][r]))]
    assert not bad, [(r, int(strand[r]), int(cf[r]), int(cr[r]), int(m["strand"][r]), int(m["count_fwd"][r]), int(m["count_rev"][r])) for r in bad[:8]]
    assert strand.dtype == np.int8 and cf.dtype == np.int32 and cr.dtype == np.int32


# ------------------------------------------------------------------ test 1: verdicts
def test_catalogue_precondition(cat):
    """on the MODEL's output: every amplicon of the catalogue is decided, and exactly the ties, the random and short reads and the
    empty read are not"""
    s, kinds = cat["model"]["strand"], cat["kinds"]
    assert all(s[r] != 0 for r, k in enumerate(kinds) if k == "decided")
    assert [r for r in range(len(s)) if s[r] == 0] == [r for r, k in enumerate(kinds) if k == "zero"]
    assert (s == -1).sum() > 200 and (s == 1).sum() > 1500
    rep_of, rs = cat["rep_of"], cat["rs"]
    n = len(s)
    # the pairs: the reverse complement second, then first; and again in the second sample, with seeds of their own
    assert rs[n - 14] == -1 and rs[n - 12] == -1 and rep_of[n - 4] == n - 4 and rs[n - 3] == -1 and rs[n - 1] == -1


def test_verdicts_equal_the_model_fed_from_the_oracle(engine, mini_hmm_text, cat):
    engine.load_profiles(text=mini_hmm_text)
    assert engine.n_profiles == 10
    _load(engine, cat)
    got = engine.orient_profiles()
    _same(got, cat["model"])
    assert engine.last_orient_ms > 0 and engine.n_reads == len(cat["reads"])


def test_verdicts_equal_the_model_fed_from_the_engines_traces(engine, mini_hmm_text, cat, monkeypatch):
    monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
    engine.load_profiles(text=mini_hmm_text)
    nf, nr = _engine_counts(engine, cat["reads"])
    m = ope.model(nf, nr, cat["rep_of"], cat["rs"])
    monkeypatch.delenv("ITSX_KEEP_TRACE")
    for k in ("strand", "count_fwd", "count_rev"):
        assert np.array_equal(m[k], cat["model"][k]), k              # the engine's filter is the oracle's
    _load(engine, cat)
    _same(engine.orient_profiles(), m)


def test_verdicts_with_224_profiles(engine, t_hmm_text, flipped_fixture, monkeypatch):
    """Ppad = 256 > P = 224: the padding columns never count"""
    hs = orc.HmmSet(text=t_hmm_text)
    reads = flipped_fixture
    rep_of, rs = ope.derep(reads)
    nf, nr = ope.oracle_counts(hs, reads)
    m = ope.model(nf, nr, rep_of, rs)
    assert all(int(m["strand"][r]) == (-1 if r % 3 == 2 else 1) for r in range(len(reads))) and len(reads) == 227
    engine.load_profiles(text=t_hmm_text)
    assert engine.n_profiles == 224
    engine.set_reads(reads)
    _same(engine.orient_profiles(), m)
    monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
    nf2, nr2 = _engine_counts(engine, reads)
    assert np.array_equal(nf2, nf) and np.array_equal(nr2, nr)


# ------------------------------------------------------------------ test 2: schedule independence
@pytest.mark.parametrize("name,value", [("ITSX_CHUNK_UNIQUES", "64"), ("ITSX_MSV_PB", "1"), ("ITSX_MSV_PB", "32")])
def test_schedule_does_not_change_the_arrays(engine, mini_hmm_text, cat, monkeypatch, name, value):
    engine.load_profiles(text=mini_hmm_text)
    monkeypatch.setenv(name, value)
    _load(engine, cat)
    _same(engine.orient_profiles(), cat["model"])
    _same(engine.orient_profiles(), cat["model"])                    # and a second call in the same context


def test_another_threshold_changes_the_counts_as_the_model_says(engine, mini, mini_hmm_text, cat, monkeypatch):
    engine.load_profiles(text=mini_hmm_text)
    monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
    nf, nr = _engine_counts(engine, cat["reads"], F1=0.02)
    monkeypatch.delenv("ITSX_KEEP_TRACE")
    m = ope.model(nf, nr, cat["rep_of"], cat["rs"])
    assert not np.array_equal(m["count_fwd"], cat["model"]["count_fwd"])
    of, orv = ope.oracle_counts(mini, cat["reads"], F1=0.02)
    assert np.array_equal(of, nf) and np.array_equal(orv, nr)
    _load(engine, cat)
    _same(engine.orient_profiles(F1=0.02), m)
    _same(engine.orient_profiles(), cat["model"])                    # back at the default: the threshold rows follow F1


# ------------------------------------------------------------------ test 3: apply
def _records(gold):
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]


def _write(path, recs):
    with open(path, "w") as f:
        for h, s, q in recs:
            f.write("%s\n%s\n+\n%s\n" % (h, s, q))
    return str(path)


def _packed(eng):
    return [tuple(x.copy() for x in eng.debug_packed_read(i)) for i in range(eng.n_reads)]


def _downstream(engine, tmp_path, tag, mode):
    """derep, search, finalize and everything that hangs on the read set"""
    engine.set_rows_mode(mode)
    try:
        nu = engine.derep()
        engine.search()
        engine.finalize()
        out = dict(nu=nu, coords=[x.copy() for x in engine.trim_coords("3_", "4_")], derep=[x.copy() for x in engine.get_derep()])
        if mode == "full":
            out["rows"] = engine.domains()
        uc, rep, tr = (str(tmp_path / ("%s_%s_%s" % (tag, mode, x))) for x in ("uc.txt", "rep.fa", "trimmed.fq"))
        engine.write_uc(uc); engine.write_rep_fasta(rep)
        engine.write_trimmed_samples([tr], region_prefixes=("3_", "4_"))
        out["files"] = [open(p, "rb").read() for p in (uc, rep, tr)]
    finally:
        engine.set_rows_mode(None)
    return out


@pytest.mark.parametrize("mode", ["full", "lazy"])
def test_apply_equals_the_unflipped_input(engine, gold, t_hmm_text, tmp_path, mode):
    recs = _records(gold)
    flipped = [(h, ope.revcomp(s), q[::-1]) if i % 3 == 2 else (h, s, q) for i, (h, s, q) in enumerate(recs)]
    plain, flip = _write(tmp_path / "plain.fq", recs), _write(tmp_path / "flip.fq", flipped)
    engine.load_profiles(text=t_hmm_text)
    engine.keep_records(True)
    try:
        engine.load_reads_files([plain])
        e_packed = _packed(engine)
        exp = _downstream(engine, tmp_path, "e", mode)
        n = int(engine.load_reads_files([flip])[0])
        before = engine.read_set
        strand, cf, cr = engine.orient_profiles_apply()
        assert engine.read_set > before and engine.n_reads == n == len(recs) and engine.n_samples == 1
        assert [int(x) for x in strand] == [-1 if i % 3 == 2 else 1 for i in range(n)]
        assert (cf[strand < 0] == 0).all() and (cr[strand < 0] >= 7).all() and (cf[strand > 0] >= 7).all()
        got_packed = _packed(engine)
        for j, (g, e) in enumerate(zip(got_packed, e_packed)):
            assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), j
        got = _downstream(engine, tmp_path, "g", mode)
    finally:
        engine.keep_records(False)
    assert got["nu"] == exp["nu"]
    for g, e in zip(got["coords"] + got["derep"], exp["coords"] + exp["derep"]):
        assert np.array_equal(g, e)
    if mode == "full":
        assert len(got["rows"]) == len(exp["rows"]) > 1000 and got["rows"].tobytes() == exp["rows"].tobytes()
    assert got["files"] == exp["files"] and all(len(f) > 1000 for f in exp["files"])      # uc.txt, rep.fa (the host text), the trimmed records
    assert (exp["coords"][0] >= 0).sum() > 150


def test_apply_keeps_what_it_cannot_judge(engine, mini_hmm_text, cat):
    """strand 0 comes back as it was, in place; strand -1 as the model's text -- IUPAC symbols, lower case and U included"""
    engine.load_profiles(text=mini_hmm_text)
    idx = [r for r, k in enumerate(cat["kinds"]) if k != "free" and cat["samples"][r] == 0]
    reads = [cat["reads"][r] for r in idx]
    sub = ope.model(cat["nf"][idx], cat["nr"][idx], *ope.derep(reads), texts=reads)
    want = sub["texts"]
    from itsxpress_amd import Engine
    exp = Engine(0)
    try:
        exp.set_reads(want)
        e_packed = _packed(exp)
    finally:
        exp.close()
    engine.set_reads(reads)
    _same(engine.orient_profiles_apply(), sub)
    assert engine.n_reads == len(reads)
    got = _packed(engine)
    for j, (g, e) in enumerate(zip(got, e_packed)):
        assert np.array_equal(g[0], e[0]), ("words", j, len(reads[j]))
        assert np.array_equal(g[1], e[1]), ("exceptions", j, len(reads[j]))
    assert sum(len(e[1]) for e in e_packed) > 100 and (sub["strand"] == 0).sum() == 76 and (sub["strand"] == -1).sum() > 100


def test_apply_host_text_keeps_its_case(engine, mini_hmm_text, cat, tmp_path):
    engine.load_profiles(text=mini_hmm_text)
    idx = [r for r, k in enumerate(cat["kinds"]) if k != "free" and cat["samples"][r] == 0 and cat["reads"][r]]
    reads = [cat["reads"][r] for r in idx]
    want = ope.model(cat["nf"][idx], cat["nr"][idx], *ope.derep(reads), texts=reads)["texts"]
    engine.set_reads(reads, names=["r%d" % i for i in range(len(reads))])
    engine.orient_profiles_apply()
    engine.derep(strand_both=False)
    p = str(tmp_path / "rep.fa")
    engine.write_rep_fasta(p)
    text = {}
    name = None
    for line in open(p):
        if line[0] == ">":
            name = line[1:].split(";")[0].strip()
            text[name] = ""
        else:
            text[name] += line.strip()
    seeds, _ = engine.get_uniques()
    assert len(text) == len(seeds) > 100
    for s in seeds:
        assert text["r%d" % int(s)] == want[int(s)], int(s)
    assert any(c.islower() for t in text.values() for c in t) and any("u" in t for t in text.values())


# ------------------------------------------------------------------ test 4: the mirror's batch
def test_batch_equals_solo_and_the_model(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd.SeqSample import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    monkeypatch.delenv("ITSXPRESS_ORIENT", raising=False)
    recs = _records(gold)
    rng = np.random.default_rng(21)
    flip = rng.random(len(recs)) < 0.4
    flipped = [(h, ope.revcomp(s), q[::-1]) if f else (h, s, q) for (h, s, q), f in zip(recs, flip)]
    cuts = [(0, 60), (60, 61), (61, len(recs))]
    files = [_write(tmp_path / ("in_%d.fq" % k), flipped[lo:hi]) for k, (lo, hi) in enumerate(cuts)]
    hmm = tmp_path / "T.hmm"
    hmm.write_text(t_hmm_text)
    solo = []
    for k, f in enumerate(files):
        d = str(tmp_path / "solo" / str(k))
        os.makedirs(d)
        s = SeqSampleNotPaired(fastq=f, tempdir=d)
        s._engine = engine
        s.orient_reads_by_profiles(str(hmm), threads=1)
        assert s.fastq == s.seq_file == s.r1 == os.path.join(d, "oriented.fq")
        solo.append((s.orient_strand.copy(), open(s.seq_file, "rb").read()))
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    objs = [SeqSampleNotPaired(fastq=f, tempdir=bd) for f in files]
    b = SampleBatch(objs, engine=engine)
    b.orient_reads_by_profiles(str(hmm), threads=1)
    for k, (s, (lo, hi)) in enumerate(zip(objs, cuts)):
        assert s.fastq == s.seq_file == s.r1 == os.path.join(bd, b.subdirs[k], "oriented.fq")
        assert np.array_equal(s.orient_strand, solo[k][0]), k
        assert [int(x) for x in s.orient_strand] == [-1 if f else 1 for f in flip[lo:hi]], k      # the model: every fixture read is a forward one
        text = open(s.seq_file, "rb").read()
        assert text == solo[k][1], k
        assert text == "".join("%s\n%s\n+\n%s\n" % r for r in recs[lo:hi]).encode(), k      # the model's text: the unflipped records
    assert list(b.counts) == [hi - lo for lo, hi in cuts] and 0.25 < flip.mean() < 0.55
    # with the environment setting and the sample's attribute instead of the argument
    monkeypatch.setenv("ITSXPRESS_ORIENT", "profiles")
    d = str(tmp_path / "env")
    os.makedirs(d)
    s = SeqSampleNotPaired(fastq=files[0], tempdir=d)
    s._engine = engine
    s.orient_hmmfile = str(hmm)
    s.orient_reads(threads=1)
    assert open(s.seq_file, "rb").read() == solo[0][1] and np.array_equal(s.orient_strand, solo[0][0])
    bd2 = str(tmp_path / "batch_env")
    os.makedirs(bd2)
    objs = [SeqSampleNotPaired(fastq=f, tempdir=bd2) for f in files]
    for o in objs:
        o.orient_hmmfile = str(hmm)
    SampleBatch(objs, engine=engine).orient_reads(threads=1)
    for k, o in enumerate(objs):
        assert open(o.seq_file, "rb").read() == solo[k][1] and np.array_equal(o.orient_strand, solo[k][0]), k
    objs[1].orient_hmmfile = str(hmm) + ".other"
    with pytest.raises(ValueError, match="one profile file"):
        SampleBatch(objs, engine=engine).orient_reads(threads=1)


# ------------------------------------------------------------------ test 5: state and errors
def test_call_order_and_state(mini_hmm_text, cat):
    from itsxpress_amd import Engine, EngineError
    reads = cat["reads"][:40]
    e = Engine(0)
    try:
        for fn in (e.orient_profiles, e.orient_profiles_apply):      # neither profiles nor reads
            with pytest.raises(EngineError) as x:
                fn()
            assert x.value.code == -1
        e.load_profiles(text=mini_hmm_text)
        for fn in (e.orient_profiles, e.orient_profiles_apply):      # profiles, no reads
            with pytest.raises(EngineError) as x:
                fn()
            assert x.value.code == -1 and "read set" in str(x.value)
    finally:
        e.close()
    e = Engine(0)
    try:
        e.set_reads(reads)
        before = _packed(e)
        assert e.derep() > 0
        for fn in (e.orient_profiles, e.orient_profiles_apply):      # reads, no profiles: the call fails and the read set is intact
            with pytest.raises(EngineError) as x:
                fn()
            assert x.value.code == -1 and "profiles" in str(x.value)
        after = _packed(e)
        assert len(after) == len(before) == 40 and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(after, before))
        e.get_derep()                                                # (a refused call leaves the dereplication too)
        e.load_profiles(text=mini_hmm_text)
        for fn in (e.orient_profiles, e.orient_profiles_apply):
            e.derep()
            fn()
            with pytest.raises(EngineError):
                e.get_derep()                                        # the dereplication was the call's own
            with pytest.raises(EngineError):
                e.search()
        assert e.n_reads == 40 and e.derep() > 0
    finally:
        e.close()


def test_streamed_and_sharded_engines_refuse():
    from itsxpress_amd import EngineError
    from itsxpress_amd.multi import MultiEngine
    from itsxpress_amd.stream import StreamEngine
    for cls in (StreamEngine, MultiEngine):
        for fn in ("orient_profiles", "orient_profiles_apply"):
            with pytest.raises(EngineError) as x:
                getattr(cls, fn)(object.__new__(cls))
            assert x.value.code == -5 and fn in str(x.value)


def test_without_a_profile_file_orient_reads_is_the_kmer_path(engine, gold, tmp_path, monkeypatch):
    import importlib
    import itsxpress_amd.definitions as D
    from itsxpress_amd.SeqSample import SeqSampleNotPaired
    from itsxpress_amd.trim import write_oriented_fastq
    monkeypatch.setenv("ITSXPRESS_DB_DIR", gold)
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    monkeypatch.delenv("ITSXPRESS_ORIENT", raising=False)
    importlib.reload(D)
    recs = _records(gold)[:90]
    fq = _write(tmp_path / "in.fq", [(h, ope.revcomp(s), q[::-1]) if i % 3 == 2 else (h, s, q) for i, (h, s, q) in enumerate(recs)])
    s = SeqSampleNotPaired(fastq=fq, tempdir=str(tmp_path / "solo"))
    s._engine = engine
    s.orient_hmmfile = "/nonexistent.hmm"                            # (ignored without ITSXPRESS_ORIENT=profiles)
    s.orient_reads(threads=1)
    assert s.orient_strand is None
    engine.load_reads_files([fq])
    engine.orient_load_db(os.path.join(gold, "universal_orient_ref_clean.fasta.gz"))
    strand, _, _, kept = engine.orient_apply()
    out = str(tmp_path / "direct.fq")
    assert write_oriented_fastq(fq, out, strand) == int(kept[0])
    assert open(s.seq_file, "rb").read() == open(out, "rb").read() and (strand == -1).sum() > 10
