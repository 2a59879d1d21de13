"""GPU tests of read orientation for long reads and for a batch of samples: `itsx_orient` on reads of up to
65 535 bases equals the oracle; `itsx_orient_apply` leaves the context as loading the samples' oriented.fq files does;
`SampleBatch.orient_reads` writes, per sample, the files of the sample's own run.  Every comparison is exact."""
import gzip
import os
import re

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RC = str.maketrans("ACGTURYMKSWHBVDNacgturymkswhbvdn", "TGCAAYRKMSWDVBHNtgcaayrkmswdvbhn")
_IUPAC = "RYKMSWBVDHNU"


def _rc(s):
    return s[::-1].translate(_RC)


@pytest.fixture(scope="module")
def db(gold):
    seqs, cur = [], []
    with gzip.open(os.path.join(gold, "universal_orient_ref_clean.fasta.gz"), "rt") as f:
        for line in f:
            if line.startswith(">"):
                if cur:
                    seqs.append("".join(cur))
                cur = []
            else:
                cur.append(line.strip().upper())
    if cur:
        seqs.append("".join(cur))
    assert len(seqs) == 599
    return seqs


@pytest.fixture(scope="module")
def oriented_engine(engine, gold):
    assert engine.orient_load_db(os.path.join(gold, "universal_orient_ref_clean.fasta.gz")) == 599
    return engine


def _concat(db, rng, L):
    out, n = [], 0
    while n < L:
        s = db[int(rng.integers(0, len(db)))]
        out.append(s); n += len(s)
    return "".join(out)[:L]


def _short_reads(db, rng, count):
    reads = []
    for i in range(count):
        src = db[int(rng.integers(0, len(db)))]
        a = int(rng.integers(0, max(1, len(src) - 300)))
        s = src[a:a + int(rng.integers(40, 900))]
        kind = i % 4
        if kind == 1:
            s = _rc(s)
        elif kind == 2:
            s = "".join(rng.choice(list("ACGT"), len(s)))
        elif kind == 3:
            s = s[:len(s) // 2] + _rc(s[len(s) // 2:])
        reads.append(s)
    return reads


# ------------------------------------------------------------------ test 1: long reads equal the oracle
_LONG = (12011, 12012, 12013, 16395, 16396, 30000, 65535)


def test_long_reads_equal_the_oracle(oriented_engine, db):
    engine = oriented_engine
    rng = np.random.default_rng(11)
    reads, flavours = [], {}
    for L in _LONG:
        c = _concat(db, rng, L)
        four = [c, _rc(c), c[:L // 2] + _rc(c[L // 2:]), "".join(rng.choice(list("ACGT"), L))]
        assert all(len(x) == L for x in four)
        flavours[L] = list(range(len(reads), len(reads) + 4))
        reads += four
    unit = _concat(db, rng, 6000)
    rep = (unit * 11)[:65535]                                  # few distinct words in a long read
    i_rep = len(reads)
    reads += [rep, _rc(rep)]
    reads += _short_reads(db, rng, 50)                          # both kernels run on one read set
    es, ef, er = orc.orient(db, reads)
    # the precondition, on the ORACLE's output: every long length shows a forward, a reverse and an undetermined read
    for L in _LONG:
        if L >= 12012:
            got = sorted(int(es[i]) for i in flavours[L])
            assert got[0] == -1 and got[-1] == 1 and 0 in got, (L, got)
    assert es[i_rep] == 1 and es[i_rep + 1] == -1 and ef[i_rep] < 6000 and ef[i_rep] > 4 * er[i_rep]
    engine.set_reads(reads)
    strand, cf, cr = engine.orient()
    for i in range(len(reads)):
        assert (int(strand[i]), int(cf[i]), int(cr[i])) == (int(es[i]), int(ef[i]), int(er[i])), (i, len(reads[i]))
    # once more in the same context: the long reads' word sets were left empty
    strand2, cf2, cr2 = engine.orient()
    assert np.array_equal(strand2, es) and np.array_equal(cf2, ef) and np.array_equal(cr2, er)


def test_dust_mask_up_to_the_longest_read(oriented_engine, db):
    """k_dust against the oracle's DUST on reads past clustering's 50 000 bases, with low-complexity stretches up to the last base"""
    engine = oriented_engine
    rng = np.random.default_rng(12)
    low = lambda n: ("AT" * n)[:n]
    a = _concat(db, rng, 65535)
    b = list(_concat(db, rng, 65535))
    for p, n in ((50010, 300), (60000, 31), (65535 - 70, 70), (32760, 40)):
        b[p:p + n] = low(n)
    b = "".join(b)
    c = _concat(db, rng, 50001)[:50001 - 40] + "A" * 40
    reads = [a, b, c, low(65535)]
    engine.set_reads(reads)
    got = engine.debug_dust([len(r) for r in reads])
    for r, g in zip(reads, got):
        e = orc.dust(r)
        assert np.array_equal(g, e), (len(r), int(g.sum()), int(e.sum()))
    assert got[1][65535 - 30:].all() and got[3].all() and got[1].sum() > 400


# ------------------------------------------------------------------ test 2: orient_apply equals loading the oriented files
def _tile():
    src = open(os.path.join(ROOT, "itsxpress_amd", "csrc", "k_orient.hip")).read()
    return int(re.search(r"OA_BLOCK = (\d+);", src).group(1)) * int(re.search(r"OA_ITEMS = (\d+);", src).group(1))


def _spice(s, i, rng):
    """non-ACGT symbols and lower case where the packed form can go wrong"""
    s = list(s)
    L = len(s)
    sym = lambda k: _IUPAC[(i + k) % len(_IUPAC)]
    pat = i % 8
    if pat == 1:
        s[0] = sym(0)
    elif pat == 2:
        s[L - 1] = sym(0)
    elif pat == 3 and L > 20:
        p = int(rng.integers(1, L - 2)); s[p] = sym(0); s[p + 1] = sym(1)
    elif pat == 4 and L > 17:
        s[15] = sym(0); s[16] = sym(1)                          # one on each side of a word boundary
    elif pat == 5:
        for k in range(int(rng.integers(1, 6))):
            s[int(rng.integers(0, L))] = sym(k)
    elif pat == 6:
        a = int(rng.integers(0, L)); b = min(L, a + int(rng.integers(1, 60)))
        s[a:b] = [c.lower() for c in s[a:b]]
        s[int(rng.integers(0, L))] = sym(0).lower()
    elif pat == 7 and L > 40:
        s[0] = sym(0); s[L - 1] = sym(1); s[L - 17] = sym(2); s[L - 16] = sym(3)
    return "".join(s)


def _read(db, rng, i, kind=None, L=None):
    src = db[int(rng.integers(0, len(db)))]
    if L is None:
        L = (12, 13, 15, 16, 17, 31, 32, 33)[(i // 16) % 8] if i % 16 == 0 else 40 + int(rng.integers(0, 640))
    L = min(L, len(src))
    a = int(rng.integers(0, len(src) - L + 1))
    s = src[a:a + L]
    kind = i % 5 if kind is None else kind
    if kind == 1:
        s = _rc(s)
    elif kind == 2:
        s = "".join(rng.choice(list("ACGT"), len(s)))
    elif kind == 3:
        s = s[:len(s) // 2] + _rc(s[len(s) // 2:])
    return _spice(s, i, rng)


def _write_fastq(path, recs):
    with open(path, "w") as f:
        for name, s in recs:
            f.write("@%s extra words\n%s\n+\n%s\n" % (name, s, "".join(chr(33 + (k * 7 + len(s)) % 40) for k in range(len(s)))))
    return path


def _packed(eng):
    return [tuple(x.copy() for x in eng.debug_packed_read(i)) for i in range(eng.n_reads)]


def test_orient_apply_equals_loading_the_oriented_files(oriented_engine, db, gold, tmp_path):
    from itsxpress_amd import Engine
    from itsxpress_amd.trim import write_oriented_fastq
    engine = oriented_engine
    T = _tile()
    rng = np.random.default_rng(13)
    sizes = [0, 1, 63, 64, 65, T - 193, 0, T + 300, 200, 0, 40, 150, 1300, 0]
    i_none, i_rev, i_through = 10, 11, 7
    S = len(sizes)
    samples, i = [], 0
    for s, n in enumerate(sizes):
        recs = []
        for k in range(n):
            if s == i_none:
                r = ["ACGTACGTACG", "N" * 60, "acgtn", db[k][:11], "NNNNNNNNNNNNACGTACGTNNNNNNNNNNN"][k % 5]
            elif s == i_rev:
                r = _read(db, rng, i, kind=1)
            else:
                r = _read(db, rng, i)
            recs.append(("s%d_r%d" % (s, k), r))
            i += 1
        samples.append(recs)
    c1, c2 = _concat(db, rng, 12012), _concat(db, rng, 20000)
    samples[i_through][T // 2] = ("long12012", _spice(_rc(c1), 7, rng))      # two long reads inside ordinary samples
    samples[12][17] = ("long20000", _spice(c2, 4, rng))
    lens = [len(r) for recs in samples for _, r in recs]
    assert {L % 16 for L in lens} == set(range(16)) and {12, 13, 15, 16, 17, 31, 32, 33} <= set(lens)
    text = "".join(r for recs in samples for _, r in recs)
    assert all(c in text for c in _IUPAC) and any(c.islower() for c in text)
    first = np.concatenate([[0], np.cumsum(sizes)])
    # one sample ends exactly on the first tile boundary, an empty one sits there, the next runs through the second tile into the third,
    # the rest lie inside the third: about 3 T reads in all
    assert first[6] == first[7] == T and first[7] < 2 * T < first[8] < first[9] and 2.9 * T < first[-1] < 3 * T
    ins = [_write_fastq(str(tmp_path / ("in_%02d.fq" % s)), recs) for s, recs in enumerate(samples)]
    # ---- the expectation: each sample alone through the existing calls, then the S oriented files loaded as a batch
    exp = Engine(0)
    try:
        exp.orient_load_db(os.path.join(gold, "universal_orient_ref_clean.fasta.gz"))
        outs, e_strand, e_cf, e_cr = [], [], [], []
        for s in range(S):
            exp.load_reads_file(ins[s])
            st, cf, cr = exp.orient()
            outs.append(str(tmp_path / ("oriented_%02d.fq" % s)))
            assert write_oriented_fastq(ins[s], outs[s], st) == int((st != 0).sum())
            e_strand.append(st.copy()); e_cf.append(cf.copy()); e_cr.append(cr.copy())
        e_strand, e_cf, e_cr = (np.concatenate(x) for x in (e_strand, e_cf, e_cr))
        e_kept = np.asarray(exp.load_reads_files(outs))
        assert exp.n_samples == S
        e_names, e_packed, e_ids = exp.read_names(), _packed(exp), exp.debug_read_samples()
        e_nu = exp.derep()
        e_derep = [x.copy() for x in exp.get_derep()]
        e_files = []
        for s in range(S):
            exp.select_sample(s)
            exp.write_uc(str(tmp_path / "e_uc.txt")); exp.write_rep_fasta(str(tmp_path / "e_rep.fa"))
            e_files.append((open(tmp_path / "e_uc.txt", "rb").read(), open(tmp_path / "e_rep.fa", "rb").read()))
    finally:
        exp.close()
    # neither path is idle, on the expectation: reverse reads, dropped reads, a sample that keeps nothing, one that is all reverse
    n_in, n_kept = int(first[-1]), int(e_kept.sum())
    assert (e_strand == -1).sum() > n_kept / 5 and n_in - n_kept > n_in / 10
    assert e_kept[i_none] == 0 and sizes[i_none] == 40
    assert (e_strand[first[i_rev]:first[i_rev + 1]] <= 0).all() and e_kept[i_rev] > 100
    assert [int(e_kept[s]) for s in (0, 6, 9, 13)] == [0, 0, 0, 0] and e_kept[1] + e_kept[2] + e_kept[3] > 60
    o_strand, o_cf, o_cr = orc.orient(db, [r for recs in samples for _, r in recs])
    assert np.array_equal(e_strand, o_strand) and np.array_equal(e_cf, o_cf) and np.array_equal(e_cr, o_cr)
    i_l1, i_l2 = int(first[i_through]) + T // 2, int(first[12]) + 17
    assert o_strand[i_l1] == -1 and o_strand[i_l2] == 1                       # the long reads are kept, one of them reversed
    # ---- the batch: one load, one orient_apply
    n_before = np.asarray(engine.load_reads_files(ins))
    assert list(n_before) == sizes
    before = engine.read_set
    strand, cf, cr, kept = engine.orient_apply()
    assert engine.read_set > before and engine.n_reads == n_kept and engine.n_samples == S and engine.L.itsx_num_samples(engine.h) == S
    assert np.array_equal(strand, o_strand) and np.array_equal(cf, o_cf) and np.array_equal(cr, o_cr)
    assert np.array_equal(kept, e_kept)
    assert engine.read_names() == e_names
    got = _packed(engine)
    for j, (g, e) in enumerate(zip(got, e_packed)):
        assert np.array_equal(g[0], e[0]), ("words", j, e_names[j])
        assert np.array_equal(g[1], e[1]), ("exceptions", j, e_names[j])
    assert sum(len(e[1]) for e in e_packed) > 500
    ids = engine.debug_read_samples()
    assert np.array_equal(ids[0], e_ids[0]) and np.array_equal(ids[1], e_ids[1])
    assert np.array_equal(ids[0], np.repeat(np.arange(S, dtype=np.int32), e_kept))
    # ---- what hangs on it: dereplication, and the host text (rep.fa keeps the case of the oriented file)
    assert engine.derep() == e_nu
    for g, e in zip(engine.get_derep(), e_derep):
        assert np.array_equal(g, e)
    for s in range(S):
        engine.select_sample(s)
        engine.write_uc(str(tmp_path / "g_uc.txt")); engine.write_rep_fasta(str(tmp_path / "g_rep.fa"))
        assert open(tmp_path / "g_uc.txt", "rb").read() == e_files[s][0], s
        assert open(tmp_path / "g_rep.fa", "rb").read() == e_files[s][1], s
    engine.select_sample(-1)
    assert any(any(c.islower() for c in f[1].decode()) for f in e_files)


# ------------------------------------------------------------------ test 3: the mirror
def _fixture_records(gold):
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]


def _mirror_inputs(gold, d):
    """five single-end samples from the fixture reads, cut unevenly, about 40 % of the records reverse-complemented (qualities
    reversed); the third is empty and the fifth repeats the second"""
    os.makedirs(d, exist_ok=True)
    recs = _fixture_records(gold)
    rng = np.random.default_rng(14)
    flip = rng.random(len(recs)) < 0.4
    recs = [(h, _rc(s), q[::-1]) if f else (h, s, q) for (h, s, q), f in zip(recs, flip)]
    cuts = [(0, 37), (37, 120), (120, 120), (120, len(recs)), (37, 120)]
    files = []
    for k, (lo, hi) in enumerate(cuts):
        p = os.path.join(d, "ccs_%d.fq" % k)
        with open(p, "w") as f:
            for h, s, q in recs[lo:hi]:
                f.write("%s\n%s\n+\n%s\n" % (h, s, q))
        files.append(p)
    assert 0.25 < flip.mean() < 0.55
    return files


def _its2_hmm(tmp_path, t_hmm_text):
    from bench import its2_profiles
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    return str(hmm)


def _db_dir(monkeypatch, gold):
    monkeypatch.setenv("ITSXPRESS_DB_DIR", gold)
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    import importlib
    import itsxpress_amd.definitions as D
    importlib.reload(D)


def _solo_trimmed(s, d):
    from itsxpress_amd.SeqSample import Dedup, ItsPosition
    pos = ItsPosition(domtable=s.dom_file, region="ITS2")
    dd = Dedup(uc_file=s.uc_file, rep_file=s.rep_file, seq_file=s.seq_file, fastq=s.r1, fastq2=None)
    out = os.path.join(d, "trimmed.fq")
    dd.create_trimmed_seqs(out, gzipped=False, zstd_file=False, itspos=pos, wri_file=True, tempdir=d, trim_ccs=True)
    return open(out, "rb").read()


def test_batch_orient_reads_writes_each_samples_files(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd.SeqSample import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    _db_dir(monkeypatch, gold)
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    files = _mirror_inputs(gold, str(tmp_path / "in"))
    hmm = _its2_hmm(tmp_path, t_hmm_text)
    kinds = ("seq_file", "uc_file", "rep_file", "dom_file")
    solo, solo_cl = [], []
    for k, f in enumerate(files):
        d = str(tmp_path / "solo" / str(k))
        os.makedirs(d)
        s = SeqSampleNotPaired(fastq=f, tempdir=d)
        s._engine = engine
        s.orient_reads(threads=1)
        assert s.seq_file == os.path.join(d, "oriented.fq")
        s.deduplicate(threads=1)
        s._search(hmmfile=hmm, threads=1)
        solo.append([open(getattr(s, x), "rb").read() for x in kinds] + [_solo_trimmed(s, d)])
        s.cluster(threads=1, cluster_id=0.995)
        solo_cl.append([open(s.uc_file, "rb").read(), open(s.rep_file, "rb").read()])
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    objs = [SeqSampleNotPaired(fastq=f, tempdir=bd) for f in files]
    b = SampleBatch(objs, engine=engine)
    b.orient_reads(threads=1)
    loads = []
    monkeypatch.setattr(engine, "load_reads_files", lambda paths: loads.append(paths))
    b.deduplicate(threads=1)
    b._search(hmmfile=hmm, threads=1)
    outs = [os.path.join(bd, "trimmed_%d.fq" % k) for k in range(len(objs))]
    b.write_trimmed(outs, "ITS2", trim_ccs=True)
    assert loads == []                                          # the oriented reads were resident: no oriented.fq was parsed
    for k, s in enumerate(objs):
        assert s.fastq == s.seq_file == s.r1 == os.path.join(bd, b.subdirs[k], "oriented.fq")
        got = [open(getattr(s, x), "rb").read() for x in kinds] + [open(outs[k], "rb").read()]
        for name, g, e in zip(kinds + ("trimmed",), got, solo[k]):
            assert g == e, (k, name)
    assert solo[2][:3] == [b""] * 3 and solo[2][4] == b"" and solo[1] == solo[4] and all(len(solo[k][4]) > 1000 and len(solo[k][3]) > 1000 for k in (0, 1, 3))
    assert list(b.counts) == [x[0].count(b"\n") // 4 for x in solo] and 200 <= int(b.counts[[0, 1, 3]].sum()) <= 227
    # greedy clustering of every sample, still from the resident oriented reads
    b.cluster_per_sample(threads=1, cluster_id=0.995)
    assert loads == []
    for k, s in enumerate(objs):
        assert [open(s.uc_file, "rb").read(), open(s.rep_file, "rb").read()] == solo_cl[k], k


def test_batch_orient_reads_arrays_mode(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd import EngineError
    from itsxpress_amd.SeqSample import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    _db_dir(monkeypatch, gold)
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "1")
    files = _mirror_inputs(gold, str(tmp_path / "in"))
    hmm = _its2_hmm(tmp_path, t_hmm_text)
    solo = []
    for k, f in enumerate(files):
        d = str(tmp_path / "solo" / str(k))
        os.makedirs(d)
        s = SeqSampleNotPaired(fastq=f, tempdir=d)
        s._engine = engine
        s.orient_reads(threads=1)
        s.deduplicate(threads=1)
        s._search(hmmfile=hmm, threads=1)
        solo.append([np.asarray(c).copy() for c in s.trim_coordinates("ITS2")])
    engine.set_rows_mode(None)                                  # (an arrays-mode SeqSample._search leaves the shared engine in the lazy rows mode)
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    objs = [SeqSampleNotPaired(fastq=f, tempdir=bd) for f in files]
    b = SampleBatch(objs, engine=engine)
    b.orient_reads(threads=1, write_seq_files=False)
    assert not any(os.path.exists(o.seq_file) for o in objs)
    held = engine.read_set
    b.deduplicate(threads=1)
    assert engine.read_set == held                              # no reload between orient_reads and deduplicate
    b._search(hmmfile=hmm, threads=1)
    per = b.trim_coordinates("ITS2")
    for k in range(len(objs)):
        assert len(per[k]) == len(solo[k]) == 4
        for g, e in zip(per[k], solo[k]):
            assert np.array_equal(g, e), k
    assert sum(int((x[0] >= 0).sum()) for x in solo) > 150
    with pytest.raises(EngineError, match="write_seq_files"):
        b.write_trimmed([os.path.join(bd, "t%d.fq" % k) for k in range(len(objs))], "ITS2", trim_ccs=True)
    # the default writes the files in this mode too
    objs2 = [SeqSampleNotPaired(fastq=f, tempdir=bd) for f in files]
    b2 = SampleBatch(objs2, engine=engine, subdirs=["w%d" % k for k in range(len(objs2))])
    b2.orient_reads(threads=1)
    assert all(os.path.exists(o.seq_file) for o in objs2)
    with pytest.raises(EngineError, match="orient_reads\\(\\) again"):
        b.deduplicate(threads=1)                                # the first batch's reads are gone and were never written


# ------------------------------------------------------------------ test 4: errors and edges
def test_orient_apply_errors_and_edges(db, gold, tmp_path):
    from itsxpress_amd import Engine, EngineError
    from itsxpress_amd.trim import write_oriented_fastq
    rng = np.random.default_rng(15)
    reads = _short_reads(db, rng, 60)
    reads = [_spice(r, i, rng) for i, r in enumerate(reads)]
    eng = Engine(0)
    try:
        # before the database: refused, and the context keeps its reads and works
        eng.set_reads(reads, ["q%d" % i for i in range(len(reads))])
        with pytest.raises(EngineError) as ei:
            eng.orient_apply()
        assert ei.value.code == -1 and "itsx_orient_load_db" in str(ei.value)
        assert eng.n_reads == len(reads) and eng.read_names()[-1] == "q59"
        eng.orient_load_db(os.path.join(gold, "universal_orient_ref_clean.fasta.gz"))
        es, ef, er = orc.orient(db, reads)
        strand, cf, cr = eng.orient()
        assert np.array_equal(strand, es) and np.array_equal(cf, ef) and np.array_equal(cr, er)
        codes, offs = orc.digitize(reads)
        nc, orep, ostrand = orc.derep(codes, offs)
        assert eng.derep() == nc
        rep_of, dstrand, _ = eng.get_derep()
        assert np.array_equal(rep_of, orep) and np.array_equal(dstrand, ostrand)
        # S = 1: the single-sample path's oriented file, loaded
        fq = _write_fastq(str(tmp_path / "one.fq"), [("q%d" % i, r) for i, r in enumerate(reads)])
        eng.load_reads_file(fq)
        strand, cf, cr, kept = eng.orient_apply()
        assert np.array_equal(strand, es) and list(kept) == [int((es != 0).sum())] and eng.n_samples == 1 and 20 < kept[0] < 60
        got_names, got_packed = eng.read_names(), _packed(eng)
        nu = eng.derep()
        eng.write_rep_fasta(str(tmp_path / "g_rep.fa")); eng.write_uc(str(tmp_path / "g_uc.txt"))
        out = str(tmp_path / "one_oriented.fq")
        write_oriented_fastq(fq, out, es)
        assert eng.load_reads_file(out) == kept[0] and eng.read_names() == got_names
        for g, e in zip(got_packed, _packed(eng)):
            assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1])
        assert eng.derep() == nu
        eng.write_rep_fasta(str(tmp_path / "e_rep.fa")); eng.write_uc(str(tmp_path / "e_uc.txt"))
        assert open(tmp_path / "g_rep.fa", "rb").read() == open(tmp_path / "e_rep.fa", "rb").read()
        assert open(tmp_path / "g_uc.txt", "rb").read() == open(tmp_path / "e_uc.txt", "rb").read()
        # an empty read set
        eng.set_reads([])
        strand, cf, cr, kept = eng.orient_apply()
        assert len(strand) == 0 and list(kept) == [0] and eng.n_reads == 0 and eng.derep() == 0
        # every read undetermined: N = 0, S samples, empty per-sample files
        junk = [_write_fastq(str(tmp_path / ("junk_%d.fq" % s)), [("j%d_%d" % (s, k), r) for k, r in enumerate(rs)])
                for s, rs in enumerate((["ACGTACGTAC", "N" * 40], [], ["acgt", "NNNNNNNNNNNNNNNN", "ACGTACGTACG"]))]
        assert list(eng.load_reads_files(junk)) == [2, 0, 3]
        strand, cf, cr, kept = eng.orient_apply()
        assert not strand.any() and list(kept) == [0, 0, 0] and eng.n_reads == 0 and eng.n_samples == 3 and eng.L.itsx_num_samples(eng.h) == 3
        assert eng.derep() == 0
        for s in range(3):
            eng.select_sample(s)
            eng.write_uc(str(tmp_path / "j_uc.txt")); eng.write_rep_fasta(str(tmp_path / "j_rep.fa"))
            assert open(tmp_path / "j_uc.txt", "rb").read() == b"" and open(tmp_path / "j_rep.fa", "rb").read() == b""
    finally:
        eng.close()
