"""The feature table of the trimmed regions made on the device (itsx_trimmed_table, Engine.trimmed_table, SampleBatch.feature_table):
distinct trimmed sequences by samples.  Every case is compared exactly with the text model (tests/feature_table_model.py); the
coordinates come from the caller except in the last test, which searches.  `pytest -m gpu`."""
import gzip
import hashlib
import os

import numpy as np
import pytest

from feature_table_model import feature_table

pytestmark = pytest.mark.gpu
_ACGT = np.array(list("ACGT"))


def _rand(rng, n):
    return "".join(_ACGT[rng.integers(0, 4, n)])


def _check(engine, seqs, start, stop, samples=None, n_samples=1, min_len=1):
    """the device's table of these reads == the model's, field by field; returns (table, model)"""
    engine.set_reads(list(seqs))
    engine.set_samples(None if samples is None else np.asarray(samples, np.int32), n_samples)
    t = engine.trimmed_table(start=np.asarray(start, np.int32), stop=np.asarray(stop, np.int32), min_len=min_len)
    m = feature_table(seqs, start, stop, samples, n_samples, min_len)
    assert t.n_features == len(m["sequences"]) and t.n_samples == n_samples
    assert t.sequences == m["sequences"]
    assert t.totals.tolist() == m["totals"] and t.first_read.tolist() == m["first_read"]
    assert t.lengths.tolist() == [len(s) for s in m["sequences"]]
    assert t.dense().tolist() == m["counts"]
    assert t.feature_of_read.tolist() == m["feature_of_read"]
    assert t.n_counted == sum(m["totals"]) and t.ms_kernels > 0
    assert int(t.row_off[0]) == 0 and int(t.row_off[-1]) == len(t.entry_sample) == sum(1 for r in m["counts"] for c in r if c)
    for f in range(t.n_features):                               # CSR rows: samples ascend, no empty cells
        row = t.entry_sample[int(t.row_off[f]):int(t.row_off[f + 1])]
        assert (np.diff(row) > 0).all() and (t.entry_count[int(t.row_off[f]):int(t.row_off[f + 1])] > 0).all()
    return t, m


def test_alignment_of_the_slice_in_its_read(engine):
    """the same text at two offsets is one feature; a copy that differs in its last base is another"""
    rng = np.random.default_rng(11)
    seqs, start, stop, trip = [], [], [], []
    for off in range(16):
        for L in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257):
            text = _rand(rng, L)
            other = text[:-1] + "ACGT"[("ACGT".index(text[-1]) + 1 + int(rng.integers(0, 3))) % 4]
            off2, off3 = (off + 5) % 16 + 16 * int(rng.integers(0, 3)), int(rng.integers(0, 40))
            trip.append(len(seqs))
            for o, s in ((off, text), (off2, text), (off3, other)):
                seqs.append(_rand(rng, o) + s + _rand(rng, int(rng.integers(0, 20))))      # the bases behind the slice must not leak in
                start.append(o)
                stop.append(o + L)
    t, _ = _check(engine, seqs, start, stop)
    f = t.feature_of_read
    for i in trip:
        assert f[i] == f[i + 1] >= 0 and f[i + 2] >= 0 and f[i + 2] != f[i]


def test_exceptions_are_part_of_the_key(engine):
    body = "ACGTTGCAACGTAGCTAGGATC"
    big = "N" * 4096
    seqs = ["ACGTNACGT", "ACGTAACGT", "ACGTRACGT",              # 0-2: N, A and R at one position: three features
            "TN" + "N" + body + "N" + "NT",                     # 3: exceptions at start - 1, start, stop - 1, stop (start 2, stop 2 + 24)
            "CA" + "N" + body + "N" + "AC",                     # 4: only the inner two count: the same feature as 3
            "CA" + "A" + body + "N" + "AC",                     # 5: A at start: another
            "acgtuacgu", "ACGTTACGT",                           # 6, 7: lower case and U: equal
            "ACGTACGTACGTACGTAC", "ACGTACGTACGTACGTACG",         # 8, 9: a prefix of another differs (whole reads)
            "ACGTACGTACGTACGTACGG",                             # 10: ... and so does a prefix taken by the coordinates
            big, "A" + big + "C", big[:-1],                     # 11-13: 4 096 N, the same inside flanks, 4 095 N
            "NNNNACGTNNNN", "ACGT"]                             # 14, 15: exceptions on both sides of the slice only
    start = [0, 0, 0, 2, 2, 2, 0, 0, 0, 0, 0, 0, 1, 0, 4, 0]
    stop = [9, 9, 9, 26, 26, 26, 9, 9, 18, 19, 18, 4096, 4097, 4095, 8, 4]
    t, _ = _check(engine, seqs, start, stop)
    f = t.feature_of_read.tolist()
    assert len({f[0], f[1], f[2]}) == 3
    assert f[3] == f[4] != f[5]
    assert f[6] == f[7]
    assert f[8] != f[9] and f[10] == f[8]
    assert f[11] == f[12] != f[13]
    assert f[14] == f[15]
    assert t.sequences[f[11]] == big and t.sequences[f[3]] == "N" + body + "N"


def test_the_counting_rule(engine):
    rng = np.random.default_rng(12)
    core = _rand(rng, 30)
    #        clamped         whole          start == stop  start > stop   -1 left        -1 right       start past end   19 bases        20 bases
    seqs = ["GG" + core, "GG" + core, "GG" + core, "GG" + core, "GG" + core, "GG" + core, "GG" + core, "GG" + core, "GG" + core]
    start = [2, 2, 5, 9, -1, 2, 40, 2, 2]
    stop = [99, 32, 5, 4, 20, -1, 50, 21, 22]
    t1, m1 = _check(engine, seqs, start, stop, min_len=1)
    assert m1["feature_of_read"][:2] == [0, 0] and m1["feature_of_read"][2:7] == [-1] * 5 and t1.n_counted == 4
    t20, m20 = _check(engine, seqs, start, stop, min_len=20)
    assert m20["feature_of_read"][7:] == [-1, 1] and t20.n_counted == 3
    # a read shorter than its coordinates say: the clamped slice decides
    _check(engine, ["ACGTACGTAC", "ACGTACGTACGTACGTACGTACGT"], [0, 0], [24, 24], min_len=11)


def test_samples_ties_and_one_long_read(engine):
    rng = np.random.default_rng(13)
    sizes = [255, 256, 257, 0]
    n = sum(sizes)
    pool = [_rand(rng, int(rng.integers(20, 90))) for _ in range(40)]
    samples = np.repeat(np.arange(4, dtype=np.int32), sizes)
    seqs, start, stop = [], [], []
    for i in range(n):
        o = int(rng.integers(0, 33))
        s = pool[int(rng.integers(0, len(pool)))]
        seqs.append(_rand(rng, o) + s + _rand(rng, int(rng.integers(0, 9))))
        start.append(o)
        stop.append(o + len(s))
    shared, solo_a, solo_b = "TTGACCA" * 5, "CCATGGA" * 5, "GGATCCA" * 5
    for i in (3, 300, 301, 700):                                # one sequence in three of the samples: one feature, three entries
        seqs[i], start[i], stop[i] = "AC" + shared, 2, 2 + len(shared)
    for i, s in ((10, solo_a), (11, solo_b), (600, solo_b), (601, solo_a)):      # a tie of two totals: the first read decides
        seqs[i], start[i], stop[i] = s, 0, len(s)
    long_read = _rand(rng, 65535)
    seqs[520], start[520], stop[520] = long_read, 3, 65530
    t, m = _check(engine, seqs, start, stop, samples, 4)
    f = int(t.feature_of_read[3])
    assert t.sequences[f] == shared and t.dense()[f].tolist() == [1, 2, 1, 0]
    assert int(t.row_off[f + 1] - t.row_off[f]) == 3
    fa, fb = int(t.feature_of_read[10]), int(t.feature_of_read[11])
    assert t.totals[fa] == t.totals[fb] == 2 and fb == fa + 1
    assert t.sequences[int(t.feature_of_read[520])] == long_read[3:65530]
    assert len(set(m["totals"])) < len(m["totals"])             # and ties among the drawn ones
    one, _ = _check(engine, seqs, start, stop)                  # itsx_set_samples(NULL): one column
    assert one.dense().shape[1] == 1 and one.sequences == t.sequences


def test_a_full_table(engine):
    """20 000 reads of 3 000 distinct slices at random offsets: every total, entry, read and sequence"""
    rng = np.random.default_rng(14)
    alpha = np.array(list("ACGT" * 12 + "NRYacgtu"))
    slices = ["".join(alpha[rng.integers(0, len(alpha), int(rng.integers(8, 140)))]) for _ in range(3000)]
    pick = np.minimum(rng.integers(0, 3000, 20000), rng.integers(0, 3000, 20000))      # skewed: totals from 1 to dozens
    samples = rng.integers(0, 5, 20000).astype(np.int32)
    seqs, start, stop = [], [], []
    for k in pick:
        o = int(rng.integers(0, 48))
        seqs.append(_rand(rng, o) + slices[int(k)] + _rand(rng, int(rng.integers(0, 16))))
        start.append(o)
        stop.append(o + len(slices[int(k)]))
    t, _ = _check(engine, seqs, start, stop, samples, 5)
    assert 2000 < t.n_features <= 3000 and t.totals[0] > 10


def test_errors(engine):
    from itsxpress_amd import Engine, EngineError
    from itsxpress_amd.multi import MultiEngine
    from itsxpress_amd.stream import StreamEngine
    eng = Engine(0)                                             # its own context: nothing loaded, no search
    try:
        a = np.zeros(2, np.int32)
        with pytest.raises(EngineError, match="read set") as ei:       # no reads loaded
            eng.trimmed_table(start=a[:0], stop=a[:0])
        assert ei.value.code == -1
        eng.set_reads(["ACGTACGT", "ACGTACGA"])
        for bad in (dict(region_prefixes=("3_", "4_"), start=a, stop=a + 4), dict(), dict(start=a)):
            with pytest.raises(EngineError, match="either") as ei:
                eng.trimmed_table(**bad)
            assert ei.value.code == -1
        with pytest.raises(EngineError, match="itsx_search_finalize") as ei:
            eng.trimmed_table(region_prefixes=("3_", "4_"))
        assert ei.value.code == -1
        with pytest.raises(EngineError, match="min_len") as ei:
            eng.trimmed_table(start=a, stop=a + 4, min_len=0)
        assert ei.value.code == -1
        assert eng.trimmed_table(start=a, stop=a + 8).sequences == ["ACGTACGT", "ACGTACGA"]
    finally:
        eng.close()
    with pytest.raises(EngineError, match="trimmed_table") as ei:
        MultiEngine.trimmed_table(MultiEngine.__new__(MultiEngine), start=a, stop=a)      # (the call needs no worker)
    assert ei.value.code == -5
    st = StreamEngine(0)
    try:
        with pytest.raises(EngineError, match="trimmed_table") as ei:
            st.trimmed_table(start=a, stop=a)
        assert ei.value.code == -5
    finally:
        st.close()


def _fixture_records(gold):
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]


def test_end_to_end_against_the_trimmed_files(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from bench import its2_profiles
    from itsxpress_amd.SeqSample import SeqSampleNotPaired, _REGION_PREFIX
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    recs = _fixture_records(gold)
    cut = len(recs) // 2
    files = []
    for k, part in enumerate((recs[:cut], recs[cut:])):
        p = str(tmp_path / ("in_%d.fq" % k))
        with open(p, "w") as f:
            f.write("".join("%s\n%s\n+\n%s\n" % r for r in part))
        files.append(p)
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    objs = [SeqSampleNotPaired(fastq=f, tempdir=str(tmp_path)) for f in files]
    b = SampleBatch(objs, engine=engine, keep_records=True)
    b.deduplicate(threads=1)
    b._search(hmmfile=str(hmm), threads=1)

    def state(tag):
        out = [x.tobytes() for x in engine.trim_coords(*_REGION_PREFIX["ITS2"])]
        for i in range(2):
            engine.select_sample(i)
            for w, name in ((engine.write_uc, "uc"), (engine.write_rep_fasta, "rep")):
                p = str(tmp_path / ("%s_%s_%d" % (tag, name, i)))
                w(p)
                out.append(open(p, "rb").read())
        engine.select_sample(-1)
        return out
    before = state("before")
    t = b.feature_table("ITS2")
    assert state("after") == before and [open(o.uc_file, "rb").read() for o in objs] == [before[4], before[6]]
    # the model over the base lines of the files write_trimmed writes for the same batch
    outs = [str(tmp_path / ("trimmed_%d.fq" % k)) for k in range(2)]
    b.write_trimmed(outs, "ITS2")
    seqs, samples = [], []
    for k, p in enumerate(outs):
        lines = open(p).read().split("\n")
        for s in lines[1::4]:
            if s:
                seqs.append(s.upper())
                samples.append(k)
    assert len(seqs) > 100 and len(set(samples)) == 2
    m = feature_table(seqs, [0] * len(seqs), [len(s) for s in seqs], samples, 2)
    assert t.sequences == m["sequences"] and t.totals.tolist() == m["totals"] and t.dense().tolist() == m["counts"]
    assert t.n_counted == len(seqs) and (t.feature_of_read >= 0).sum() == len(seqs)
    assert t.feature_of_read[t.feature_of_read >= 0].tolist() == m["feature_of_read"]
    assert t.labels == [hashlib.sha1(s.encode()).hexdigest() for s in t.sequences]
    names = engine.read_names()
    assert b.feature_table("ITS2", ids="first").labels == [names[r].split()[0] for r in t.first_read]
    # the two files parse back to the table
    fa, tsv = str(tmp_path / "features.fa"), str(tmp_path / "features.tsv")
    t2 = b.write_feature_table(fa, tsv, "ITS2")
    assert t2.sequences == t.sequences
    fl = open(fa).read().split("\n")
    assert fl[-1] == "" and fl[0:-1:2] == [">%s;size=%d" % (l, c) for l, c in zip(t.labels, t.totals)] and fl[1::2] == t.sequences
    tl = open(tsv).read().split("\n")
    assert tl[0].split("\t") == ["#feature", "in_0.fq", "in_1.fq"] and tl[-1] == ""
    assert [x.split("\t") for x in tl[1:-1]] == [[l] + [str(c) for c in row] for l, row in zip(t.labels, m["counts"])]
