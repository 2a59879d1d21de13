"""The feature table denoised into ZOTUs on the device (itsx_denoise_table, Engine.denoise_table, SampleBatch.denoise_features).  Every
array of itsx_denoise_table_get / _features is compared exactly with the model (tests/denoise_model.py) run on the feature table the
device made; read sets are built with caller start / stop arrays, so only the last test searches.  `pytest -m gpu`."""
import gzip
import os

import numpy as np
import pytest

from denoise_model import denoise, levenshtein

pytestmark = pytest.mark.gpu
_ACGT = np.array(list("ACGT"))
HALF = [0.5] * 31                                               # a hand-made skew table: abundances 1 against 2 reach every d


def _rand(rng, n):
    return "".join(_ACGT[rng.integers(0, 4, n)])


def _sub(s, p):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]


def _table(engine, feats, n_samples=1, flanks=("GG", "T")):
    """the feature table of a read set that holds feature (seq, counts) counts[s] times in sample s (an int: all in sample 0)"""
    reads, samples = [], []
    for seq, cnt in feats:
        for s, c in enumerate([cnt] if isinstance(cnt, int) else cnt):
            reads += [flanks[0] + seq + flanks[1]] * c           # (flanks: the slice, not the read, is the feature)
            samples += [s] * c
    engine.set_reads(reads)
    engine.set_samples(np.asarray(samples, np.int32) if n_samples > 1 else None, n_samples)
    ft = engine.trimmed_table(start=np.full(len(reads), len(flanks[0]), np.int32),
                              stop=np.array([len(r) - len(flanks[1]) for r in reads], np.int32))
    assert sorted(ft.sequences) == sorted({f[0] for f in feats})
    return ft


def _same(t, m, ft):
    assert t.zotu_feature.tolist() == m["zotu_feature"]
    assert t.zotu_of_feature.tolist() == m["zotu_of_feature"]
    assert t.dist_of_feature.tolist() == m["dist_of_feature"]
    assert t.totals.tolist() == m["zotu_total"]
    assert t.dense().tolist() == m["counts"]
    assert t.n_dropped_reads == m["n_dropped_reads"]
    assert int(t.row_off[0]) == 0 and int(t.row_off[-1]) == len(t.entry_sample) == len(t.entry_count) == sum(1 for r in m["counts"] for c in r if c)
    for z in range(t.n_zotus):                                   # CSR rows: samples ascend, no empty cells
        row = slice(int(t.row_off[z]), int(t.row_off[z + 1]))
        assert (np.diff(t.entry_sample[row]) > 0).all() and (t.entry_count[row] > 0).all()
    # the collapse against the feature table itself: a ZOTU's row is the column sum of its members' rows
    dense = ft.dense()
    for z in range(t.n_zotus):
        assert t.dense()[z].tolist() == dense[t.zotu_of_feature == z].sum(axis=0).tolist()
    assert int(t.totals.sum()) + t.n_dropped_reads == ft.n_counted
    assert t.ms_kernels > 0 and t.n_pairs >= 0


def _check(engine, ft, max_skew=None, alpha=2.0, minsize=8, max_diffs=None):
    """the device's denoised table of the engine's current feature table == the model's, array by array; returns (table, model)"""
    t = engine.denoise_table(alpha=alpha, minsize=minsize, max_diffs=max_diffs, max_skew=max_skew)
    m = denoise(ft.sequences, ft.totals.tolist(), ft.dense().tolist(), t.max_skew.tolist(), minsize)
    _same(t, m, ft)
    return t, m


def test_lengths_and_the_corners_of_the_band(engine):
    """lengths 1 .. 129 against each other; edits at the first and the last symbol and on both sides of a word boundary; runs of k
    insertions and deletions at the very start and the very end for k = 1, 2, D"""
    rng = np.random.default_rng(31)
    D = 5
    feats, seen = [], set()

    def add(s, c):
        if s and s not in seen:
            seen.add(s)
            feats.append((s, c))
    for L in (1, 2, 63, 64, 65, 127, 128, 129):
        base = _rand(rng, L)
        add(base, 4)
        for p in (0, L - 1, 62, 63, 64, 65, 126, 127, 128):
            if 0 <= p < L:
                add(_sub(base, p), 2)
        for k in (1, 2, D):
            ins = _rand(rng, k)
            add(ins + base, 2)
            add(base + ins, 1)
            add(base[k:], 1)
            add(base[:-k], 2)
            add(base[:63] + ins + base[63:], 1)
    ft = _table(engine, feats)
    t, m = _check(engine, ft, max_skew=HALF[:D], minsize=1)
    assert set(m["dist_of_feature"]) >= {0, 1, 2, D} and t.n_pairs > 0 and t.n_levels == 3
    _check(engine, ft, max_skew=HALF[:2], minsize=1)
    _check(engine, ft, max_skew=[0.5, 0.25, 0.25], minsize=2)


def test_cut_off_edges(engine):
    """d exactly dmax and dmax + 1; a length difference of exactly dmax and of dmax + 1 (alpha = 2: 4 reads against 256 have dmax = 2 of
    D = 3); a feature at exactly max_skew[0] times the level's first total and one read above it"""
    rng = np.random.default_rng(32)
    base = _rand(rng, 90)
    two, three = _sub(_sub(base, 10), 50), _sub(_sub(_sub(base, 5), 45), 88)
    feats = [(base, 256), (two, 4), (three, 4), (base + "AC", 4), (base + "ACG", 4), (base[2:], 4), (base[3:], 4), (_sub(base, 70), 32), (_sub(base, 71), 33)]
    assert levenshtein(base, two) == 2 and levenshtein(base, three) == 3
    ft = _table(engine, feats)
    t, m = _check(engine, ft, alpha=2.0, minsize=1)
    assert t.max_skew.tolist() == [2.0 ** -3, 2.0 ** -5, 2.0 ** -7]
    by = dict(zip(ft.sequences, m["dist_of_feature"]))
    assert by[two] == 2 and by[three] == 0 and by[base + "AC"] == 2 and by[base + "ACG"] == 0 and by[base[2:]] == 2 and by[base[3:]] == 0
    # the level's edge: 32 reads are exactly max_skew[0] * 256 (the next level, taken), 33 are one read above it (the first level)
    assert by[_sub(base, 70)] == 1 and by[_sub(base, 71)] == 0 and t.n_levels == 3
    assert t.n_skipped_length > 0


def test_31_differences_and_none(engine):
    rng = np.random.default_rng(33)
    base = _rand(rng, 200)
    v31, v32 = base, base
    for k in range(32):
        if k < 31:
            v31 = _sub(v31, 3 + 6 * k)
        v32 = _sub(v32, 4 + 6 * k)
    assert levenshtein(base, v31) == 31 and levenshtein(base, v32) == 32
    ends = _rand(rng, 31) + base                                # 31 insertions at the very start
    ft = _table(engine, [(base, 2), (v31, 1), (v32, 1), (ends, 1)])
    t, m = _check(engine, ft, max_skew=HALF, minsize=1)
    by = dict(zip(ft.sequences, m["dist_of_feature"]))
    assert by[v31] == 31 and by[v32] == 0 and by[ends] == 31
    t0, m0 = _check(engine, ft, max_diffs=0, minsize=1)          # D = 0: nothing is taken
    assert t0.max_skew.size == 0 and t0.n_zotus == 4 and t0.n_pairs == 0 and m0["dist_of_feature"] == [0] * 4
    t1, _ = _check(engine, ft, max_skew=[], minsize=2)
    assert t1.n_zotus == 1 and t1.n_dropped_reads == 3


def test_iupac_symbols_are_compared_literally(engine):
    base = "ACGTTGCAACGTAGCTAGGATCCATG"
    feats = [(base, 64), (base[:8] + "N" + base[9:], 2), (base[:8] + "R" + base[9:], 2), ("N" + base[1:], 2), (base[:-1] + "K", 1),
             (base[:8] + "N" + base[9:20] + "Y" + base[21:], 1)]
    assert base[8] == "A" and base[-1] == "G"
    ft = _table(engine, feats)
    t, m = _check(engine, ft, minsize=8)
    assert m["dist_of_feature"][:5] == [0, 1, 1, 1, 1] and sorted(m["dist_of_feature"])[-1] == 2 and t.n_zotus == 1


@pytest.mark.parametrize("C", [63, 64, 65])
def test_many_centroids_for_one_query(engine, C):
    """C centroids of equal total (so none takes another, and they stand in the order given); queries one edit from the centroid at
    index 0, 63 and 64; with 65, a query at d = 1 from centroid 2 and from centroid 64: a tie across two 64-lane chunks"""
    rng = np.random.default_rng(34)
    T = _rand(rng, 40)
    cents = [_rand(rng, 40) for _ in range(C)]
    if C == 65:
        cents[2], cents[64] = _sub(T, 3), _sub(T, 30)
    feats = [(c, 8) for c in cents]
    for w in (0, 63, 64):
        if w < C:
            feats.append((_sub(cents[w], 17), 4))
    if C == 65:
        feats.append((T, 4))
    ft = _table(engine, feats)
    assert ft.sequences[:C] == cents
    t, m = _check(engine, ft, max_skew=[0.5, 0.5], minsize=8)
    want = [w for w in (0, 63, 64) if w < C] + ([2] if C == 65 else [])
    assert m["zotu_of_feature"][C:] == want and t.n_zotus == C and t.n_pairs == C * len(want)


def test_three_levels(engine):
    """a level-2 centroid takes a level-3 feature that a level-1 centroid also takes, at a larger d"""
    rng = np.random.default_rng(35)
    X = _rand(rng, 100)
    Y = _sub(_sub(_sub(X, 20), 50), 80)
    q = _sub(_sub(X, 20), 50)
    ft = _table(engine, [(X, 512), (Y, 64), (q, 4)])
    t, m = _check(engine, ft, alpha=2.0, minsize=8)
    assert m["zotu_of_feature"] == [0, 1, 1] and m["dist_of_feature"] == [0, 0, 1] and t.n_levels == 3 and t.n_pairs == 3


def test_one_feature_and_errors(engine):
    from itsxpress_amd import Engine, EngineError
    from itsxpress_amd.multi import MultiEngine
    from itsxpress_amd.stream import StreamEngine
    ft = _table(engine, [("ACGTTGCA", 3)])
    t, _ = _check(engine, ft, minsize=3)
    assert t.n_zotus == 1 and t.totals.tolist() == [3] and t.n_levels == 1
    t, _ = _check(engine, ft, minsize=4)
    assert t.n_zotus == 0 and t.n_dropped_reads == 3 and t.row_off.tolist() == [0] and t.entry_sample.size == 0
    eng = Engine(0)                                             # its own context
    try:
        with pytest.raises(EngineError, match="no table") as ei:       # nothing loaded
            eng.denoise_table()
        assert ei.value.code == -1
        eng.set_reads(["ACGTACGT", "ACGTACGA", "ACGTACGT"])
        with pytest.raises(EngineError, match="no table") as ei:       # reads, but no table
            eng.denoise_table()
        assert ei.value.code == -1
        a = np.zeros(3, np.int32)
        eng.trimmed_table(start=a, stop=a + 8)
        for bad, what in ((dict(max_skew=[0.5] * 32), "n_diffs"), (dict(max_skew=[0.5, 1.0]), "inside"), (dict(max_skew=[0.0]), "inside"),
                          (dict(max_skew=[0.25, 0.5]), "above"), (dict(max_skew=[float("nan")]), "inside"), (dict(minsize=0), "minsize")):
            with pytest.raises(EngineError, match=what) as ei:
                eng.denoise_table(**bad)
            assert ei.value.code == -1
        assert eng.L.itsx_denoise_table_get(eng.h, None, None, None, None, None) == -1      # a refused call left no result
        assert eng.denoise_table(minsize=1).n_zotus == 2
        assert eng.L.itsx_denoise_table_get(eng.h, None, None, None, None, None) == 0
        eng.trimmed_table(start=a, stop=a + 8)                  # a new table drops the result ...
        assert eng.L.itsx_denoise_table_features(eng.h, None, None) == -1
        assert eng.denoise_table(minsize=1).n_zotus == 2
        eng.set_reads(["ACGT"])                                 # ... and so does a new read set
        assert eng.L.itsx_denoise_table_get(eng.h, None, None, None, None, None) == -1
        with pytest.raises(EngineError) as ei:
            eng.denoise_table()
        assert ei.value.code == -1
    finally:
        eng.close()
    with pytest.raises(EngineError, match="denoise_table") as ei:
        MultiEngine.denoise_table(MultiEngine.__new__(MultiEngine))      # (the call needs no worker)
    assert ei.value.code == -5
    st = StreamEngine(0)
    try:
        with pytest.raises(EngineError, match="denoise_table") as ei:
            st.denoise_table()
        assert ei.value.code == -5
    finally:
        st.close()


def test_array_sizes_come_from_the_context(engine):
    """a table made on the handle by the C call itself, after a smaller one through Engine.trimmed_table: denoise_table sizes its
    arrays by the table the context holds"""
    import ctypes as C
    rng = np.random.default_rng(38)
    seqs = [_rand(rng, 30) for _ in range(6)]
    engine.set_reads([seqs[0]] * 3 + seqs[1:])
    engine.set_samples(None, 1)
    n = 8
    small = engine.trimmed_table(start=np.zeros(n, np.int32), stop=np.array([30, 30, 30, 0, 0, 0, 0, 0], np.int32))
    assert small.n_features == 1
    start, stop = np.zeros(n, np.int32), np.full(n, 30, np.int32)
    nf = C.c_int64(0)
    assert engine.L.itsx_trimmed_table(engine.h, None, None, start.ctypes.data, stop.ctypes.data, 1, C.byref(nf), None, None, None) == 0
    assert nf.value == 6
    t = engine.denoise_table(max_skew=[0.5], minsize=1)
    assert t.zotu_of_feature.tolist() == list(range(6)) and t.dist_of_feature.tolist() == [0] * 6 and t.totals.tolist() == [3, 1, 1, 1, 1, 1]


def test_a_query_longer_than_the_match_table(engine):
    """One feature of 65 535 bases with a one-edit and a two-edit variant: the windowed path.  The model's full matrix of 4.3 G cells
    would take minutes, so this case is held to what its construction proves: sequences of one length that differ in exactly one
    (two) places are at distance exactly one (two) -- a single insertion or deletion changes the length."""
    rng = np.random.default_rng(36)
    big = _rand(rng, 65535)
    one, two = _sub(big, 40000), _sub(_sub(big, 7), 65534)
    short = big[:-2]                                            # two deletions at the very end
    ft = _table(engine, [(big, 40), (one, 4), (two, 3), (short, 2)], flanks=("", ""))      # (65 535 bases is the longest read there is)
    assert ft.sequences == [big, one, two, short]
    t = engine.denoise_table(max_skew=[0.125, 0.125], minsize=100)
    assert t.zotu_of_feature.tolist() == [-1] * 4 and t.n_pairs == 0
    t = engine.denoise_table(max_skew=[0.125, 0.125], minsize=8)
    assert t.zotu_of_feature.tolist() == [0, 0, 0, 0] and t.dist_of_feature.tolist() == [0, 1, 2, 2] and t.totals.tolist() == [49]
    assert t.n_pairs == 3 and t.n_dropped_reads == 0
    t = engine.denoise_table(max_skew=[0.125], minsize=3)        # D = 1: the two-edit variants are out
    assert t.zotu_of_feature.tolist() == [0, 0, 1, -1] and t.dist_of_feature.tolist() == [0, 1, 0, -1] and t.n_dropped_reads == 2


def _random_features():
    """600 features of 60 - 140 bases: 0 - 4 random substitutions, insertions or deletions of 12 templates; geometric abundances"""
    rng = np.random.default_rng(37)
    templates = [_rand(rng, int(rng.integers(60, 141))) for _ in range(12)]
    seqs = list(templates)
    seen = set(seqs)
    while len(seqs) < 600:
        s = list(templates[int(rng.integers(0, 12))])
        for _ in range(int(rng.integers(0, 5))):
            op, p = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
            if op == 0:
                s[p] = "ACGTN"[int(rng.integers(0, 5))]
            elif op == 1:
                s.insert(p, "ACGT"[int(rng.integers(0, 4))])
            else:
                del s[p]
        s = "".join(s)
        if s not in seen and 60 <= len(s) <= 140:
            seen.add(s)
            seqs.append(s)
    feats = []
    for i, s in enumerate(seqs):
        a = max(1, int(1500 * 0.96 ** i))
        feats.append((s, np.bincount(rng.integers(0, 5, a) if i % 7 else rng.integers(0, 2, a), minlength=5).tolist()))
    return feats


@pytest.fixture(scope="module")
def random_case():
    """the random features and, per minsize, the model's table over five samples (made once: the one-sample table has the same features
    in the same order, and its cells are the rows' sums)"""
    return {"feats": _random_features(), "models": {}}


@pytest.mark.parametrize("n_samples", [5, 1])
def test_random_table(engine, random_case, n_samples):
    """sample counts 5 and 1: the collapse's sample bits are 3 and 0; minsize 8 and above every total, with one sample also 1 (the
    model's table for minsize 8 is made once for both)"""
    feats = random_case["feats"] if n_samples == 5 else [(s, sum(c)) for s, c in random_case["feats"]]
    ft = _table(engine, feats, n_samples)
    assert ft.n_features == 600 and ft.n_samples == n_samples
    top = int(ft.totals[0])
    for minsize in (8, top + 1) if n_samples == 5 else (8, 1, top + 1):
        t = engine.denoise_table(alpha=2.0, minsize=minsize)
        key = (minsize, tuple(ft.sequences))
        if key not in random_case["models"]:
            random_case["models"][key] = denoise(ft.sequences, ft.totals.tolist(), ft.dense().tolist(), t.max_skew.tolist(), minsize)
        m = random_case["models"][key]
        if len(m["counts"]) and len(m["counts"][0]) != n_samples:
            m = dict(m, counts=[[sum(r)] for r in m["counts"]])
        _same(t, m, ft)
        if minsize == top + 1:
            assert t.n_zotus == 0 and t.entry_count.size == 0 and t.n_dropped_reads == ft.n_counted
        else:
            assert 12 <= t.n_zotus < 600 and t.n_pairs > 1000 and max(m["dist_of_feature"]) >= 2


def _fixture_records(gold):
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]


def test_a_searched_batch(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    """SampleBatch.denoise_features("ITS2") == the model run on feature_table("ITS2"); the two files parse back to the table"""
    from bench import its2_profiles
    from itsxpress_amd.SeqSample import SeqSampleNotPaired
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
    ft = b.feature_table("ITS2")
    assert ft.n_features > 10
    for minsize in (8, 1):
        t = b.denoise_features("ITS2", alpha=2.0, minsize=minsize)
        m = denoise(ft.sequences, ft.totals.tolist(), ft.dense().tolist(), t.max_skew.tolist(), minsize)
        assert t.features.sequences == ft.sequences
        _same(t, m, ft)
        assert t.sequences == [ft.sequences[f] for f in m["zotu_feature"]] and t.labels == [ft.labels[f] for f in m["zotu_feature"]]
    assert t.n_zotus > 0
    fa, tsv = str(tmp_path / "zotus.fa"), str(tmp_path / "zotus.tsv")
    t2 = b.write_denoised_table(fa, tsv, "ITS2", minsize=1)
    assert t2.sequences == t.sequences
    fl = open(fa).read().split("\n")
    assert fl[-1] == "" and fl[0:-1:2] == [">%s;size=%d" % (l, c) for l, c in zip(t.labels, t.totals)] and fl[1::2] == t.sequences
    tl = open(tsv).read().split("\n")
    assert tl[0].split("\t") == ["#feature", "in_0.fq", "in_1.fq"] and tl[-1] == ""
    assert [x.split("\t") for x in tl[1:-1]] == [[l] + [str(c) for c in row] for l, row in zip(t.labels, m["counts"])]
