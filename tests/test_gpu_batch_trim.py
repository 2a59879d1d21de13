"""The trimmed FASTQ of every sample of a batch cut on the device from the records the context keeps (itsx_keep_records,
itsx_write_trimmed_samples, SampleBatch(keep_records=True)).  The reference in every case is the host writer
itsx_write_trimmed_fastq on the sample's own file with the same coordinates.  `pytest -m gpu`."""
import gzip
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGTN", "TGCAN")
_ACGT = np.array(list("ACGT"))
_LENS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]          # trimmed lengths; with start 0..7: every source / destination misalignment
_LONG = 65535


def _rc(s):
    return s[::-1].translate(_COMP)


def _scan_tile():
    """reads per block of the plan's scan, from the kernel source (k_trim.hip: TR_BLOCK threads x TR_ITEMS reads)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "itsxpress_amd", "csrc", "k_trim.hip")) as f:
        src = f.read()
    return int(re.search(r"TR_BLOCK = (\d+);", src).group(1)) * int(re.search(r"TR_ITEMS = (\d+);", src).group(1))


def _have_zstd(engine):
    return bool(engine.L.itsx_io_codecs() & 2)


def _sample(rng, n, tag, long_at=None):
    """n records and their coordinates.  Blocks of 88 reads walk every (trimmed length, start) combination; even blocks are all written
    as they are, odd blocks interleave: stop past the end (clamped), start == stop, start > stop, -1 on either side (not written) and
    a start past the end (written, empty).  Titles are 2..80 bytes, every other one with a comment; bases mix case and IUPAC symbols."""
    alpha = np.array(list("ACGTACGTACGTacgtNRYKMSWBDHVnrykmswbdhv"))
    recs, start, stop = [], [], []
    for i in range(n):
        tl, st = _LENS[i % 11], (i // 11) % 8
        kind = i % 7 if (i // 88) % 2 else 0
        L = st + tl + (i % 3 if kind == 0 else 0)
        a, b = st, st + tl
        if kind == 1:
            b = st + tl + 5
        elif kind == 2:
            b = a
        elif kind == 3:
            a, b = st + tl, st
        elif kind == 4:
            a = -1
        elif kind == 5:
            b = -1
        elif kind == 6:
            a, b = L + 2, L + 9
        if i == long_at:
            L, a, b = _LONG, 3, _LONG - 5
        want = 2 + (i * 7) % 79                              # bytes of the title line, '@' included
        ident = ("%s%d" % (tag, i))[:want - 1]
        if i % 2 and want - 1 - len(ident) >= 2:
            title = ident + " " + "c" * (want - 2 - len(ident))
        else:
            title = ident + "x" * (want - 1 - len(ident))
        assert 2 <= len(title) + 1 <= 80
        seq = "".join(alpha[rng.integers(0, len(alpha), L)])
        qual = "".join(chr(c) for c in rng.integers(35, 64, L))
        recs.append((title, seq, qual))
        start.append(a)
        stop.append(b)
    return recs, np.array(start, np.int32), np.array(stop, np.int32)


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """four samples whose sizes straddle the scan's tile (tile - 1, tile, tile + 1, 0 reads), their files (the second with CRLF line
    ends, the third holding one 65 535-base read) and, per trim_ccs, the host writer's output for every sample"""
    from itsxpress_amd.trim import write_trimmed_fastq
    d = str(tmp_path_factory.mktemp("trim_in"))
    tile = _scan_tile()
    rng = np.random.default_rng(77)
    sizes = [tile - 1, tile, tile + 1, 0]
    files, starts, stops = [], [], []
    for k, n in enumerate(sizes):
        recs, a, b = _sample(rng, n, "s%d_" % k, long_at=500 if k == 2 else None)
        eol = "\r\n" if k == 1 else "\n"
        p = os.path.join(d, "in_%d.fq" % k)
        with open(p, "w", newline="") as f:
            f.write("".join("@%s%s%s%s+%s%s%s" % (t, eol, s, eol, eol, q, eol) for t, s, q in recs))
        files.append(p)
        starts.append(a)
        stops.append(b)
    ref = {}
    for ccs in (0, 1):
        outs, ret = [], []
        for k, p in enumerate(files):
            o = os.path.join(d, "ref_%d_%d.fq" % (ccs, k))
            ret.append(write_trimmed_fastq(p, o, starts[k], stops[k], trim_ccs=bool(ccs)))
            outs.append(open(o, "rb").read())
        ref[ccs] = (outs, ret)
    assert b"\r" not in ref[0][0][1] and ref[0][0][3] == b"" and ref[0][1][2][0] > 500 and len(ref[0][0][2]) > 2 * _LONG
    return dict(dir=d, files=files, start=np.concatenate(starts), stop=np.concatenate(stops), sizes=sizes, ref=ref, tile=tile)


def _decoded(path, kind):
    from itsxpress_amd.trim import read_text
    raw = open(path, "rb").read()
    if kind == "plain":
        return raw
    if kind == "gzip":
        text = gzip.decompress(raw) if raw else b""          # Python's own reader must accept it
        assert text == (read_text(path) if raw else b"")
        return text
    return read_text(path)


@pytest.mark.parametrize("ccs,kind", [(0, "plain"), (1, "plain"), (0, "gzip"), (1, "zstd")])
def test_explicit_coordinates_on_loaded_files(engine, loaded, tmp_path, ccs, kind):
    if kind == "zstd" and not _have_zstd(engine):
        kind = "gzip"
    engine.keep_records(True)
    try:
        counts = engine.load_reads_files(loaded["files"])
    finally:
        engine.keep_records(False)
    assert list(counts) == loaded["sizes"] and loaded["tile"] == 1024
    outs = [str(tmp_path / ("o%d.%s" % (k, kind))) for k in range(4)]
    ret = engine.write_trimmed_samples(outs, start=loaded["start"], stop=loaded["stop"], gzipped=kind == "gzip", zstd_file=kind == "zstd",
                                       trim_ccs=bool(ccs))
    exp, exp_ret = loaded["ref"][ccs]
    for k in range(4):
        assert os.path.exists(outs[k])
        got = _decoded(outs[k], kind)
        assert got == exp[k], (k, len(got), len(exp[k]))
        assert tuple(ret[k]) == tuple(exp_ret[k]), k
    if kind != "plain" or ccs:
        return
    # a sample where nothing is written still gets its empty file, and a None entry is skipped; the others are what they were
    a, b = loaded["start"].copy(), loaded["stop"].copy()
    lo = loaded["sizes"][0]
    a[lo:lo + loaded["sizes"][1]] = -1
    outs2 = [str(tmp_path / ("p%d.fq" % k)) for k in range(4)]
    ret2 = engine.write_trimmed_samples([outs2[0], outs2[1], None, outs2[3]], start=a, stop=b)
    assert open(outs2[0], "rb").read() == exp[0] and open(outs2[1], "rb").read() == b"" and not os.path.exists(outs2[2])
    assert open(outs2[3], "rb").read() == b"" and ret2[1] == (0, 0) and tuple(ret2[0]) == tuple(exp_ret[0]) and tuple(ret2[2]) == tuple(exp_ret[2])


# ------------------------------------------------------------------ the mirror: merged and oriented batches
def _fixture_records(gold):
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]


def _overlapping_pairs(rng, frags, name):
    """one pair per fragment, cut as test_gpu_batch_merge.py's helper cuts them (the fragments given instead of drawn at random, so
    that the stand-in profiles find their ITS2): a few substitutions, qualities 20..40"""
    r1, r2 = [], []
    for i, frag in enumerate(frags):
        L = len(frag)
        fl, rl = int(rng.integers(L // 2 + 8, L)), int(rng.integers(L // 2 + 8, L))
        f, r = list(frag[:fl]), list(_rc(frag[L - rl:]))
        for s in (f, r):
            if rng.random() < 0.3:
                s[int(rng.integers(0, len(s)))] = str(_ACGT[rng.integers(0, 4)])
        q1 = "".join(chr(33 + int(x)) for x in rng.integers(20, 41, fl))
        q2 = "".join(chr(33 + int(x)) for x in rng.integers(20, 41, rl))
        label = "%s%05d" % (name, i)
        r1.append((label + " 1:N:0", "".join(f), q1))
        r2.append((label + " 2:N:0", "".join(r), q2))
    return r1, r2


def _write_fastq(path, recs):
    with open(path, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % r for r in recs))
    return path


def _its2_hmm(tmp_path, t_hmm_text):
    from bench import its2_profiles
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    return str(hmm)


def test_merged_batch_writes_from_the_records(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    rng = np.random.default_rng(5)
    seqs = [s.upper() for _, s, _ in _fixture_records(gold) if set(s.upper()) <= set("ACGT")]
    assert len(seqs) > 150
    d = str(tmp_path / "in")
    os.makedirs(d)
    u1 = [("un%02d" % i, "".join(_ACGT[rng.integers(0, 4, 120)]), "I" * 120) for i in range(40)]          # unrelated mates: nothing merges
    u2 = [("un%02d" % i, "".join(_ACGT[rng.integers(0, 4, 110)]), "I" * 110) for i in range(40)]
    pairs = [_overlapping_pairs(rng, seqs[:70], "a"), (u1, u2), _overlapping_pairs(rng, seqs[70:150], "c")]
    files = [(_write_fastq(os.path.join(d, "m%d_R1.fq" % k), p1), _write_fastq(os.path.join(d, "m%d_R2.fq" % k), p2)) for k, (p1, p2) in enumerate(pairs)]
    hmm = _its2_hmm(tmp_path, t_hmm_text)
    bd = str(tmp_path / "batch")
    os.makedirs(bd)

    def run(keep, subdirs, tag, **kw):
        objs = [SeqSamplePairedNotInterleaved(fastq=r1, tempdir=bd, fastq2=r2) for r1, r2 in files]
        b = SampleBatch(objs, engine=engine, subdirs=subdirs, keep_records=keep)
        b.merge_reads(threads=1, **kw)
        seq_there = [os.path.exists(o.seq_file) for o in objs]
        b.deduplicate(threads=1)                                # writes every rep.fa: the host fetches the merged text here
        rep = [open(o.rep_file, "rb").read() for o in objs]
        b._search(hmmfile=hmm, threads=1)
        outs = [os.path.join(bd, "%s_%d.fq" % (tag, k)) for k in range(len(objs))]
        ret = b.write_trimmed(outs, "ITS2")
        return seq_there, rep, [open(p, "rb").read() for p in outs], [tuple(x) for x in ret], list(b.counts)

    seq_there, rep, got, ret, counts = run(True, ["k%d" % k for k in range(3)], "kept")
    assert seq_there == [False, False, False]                   # no seq.fq: the output came from the records
    seq_there2, rep2, exp, ret2, counts2 = run(False, ["w%d" % k for k in range(3)], "files", write_seq_files=True)
    assert seq_there2 == [True, True, True] and counts == counts2 and counts[1] == 0 and counts[0] > 50 and counts[2] > 50
    assert rep == rep2 and got == exp and ret == ret2
    assert got[1] == b"" and len(got[0]) > 1000 and len(got[2]) > 1000 and ret[0][0] > 20


def _db_dir(monkeypatch, gold):
    monkeypatch.setenv("ITSXPRESS_DB_DIR", gold)
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    import importlib
    import itsxpress_amd.definitions as D
    importlib.reload(D)


def _ccs_inputs(gold, d):
    """three CCS-shaped samples from the fixture reads: about 40 % reverse-complemented (qualities reversed), every third in lower
    case, and a few random reads that orient neither way"""
    os.makedirs(d, exist_ok=True)
    recs = _fixture_records(gold)
    rng = np.random.default_rng(23)
    out = []
    for i, (h, s, q) in enumerate(recs):
        if rng.random() < 0.4:
            s, q = _rc(s), q[::-1]
        if i % 3 == 0:
            s = s.lower()
        out.append((h[1:], s, q))
        if i % 25 == 0:
            out.append(("undet%d extra" % i, "".join(_ACGT[rng.integers(0, 4, 300)]), "I" * 300))
    cuts = [(0, 60), (60, 150), (150, len(out))]
    return [_write_fastq(os.path.join(d, "ccs_%d.fq" % k), out[lo:hi]) for k, (lo, hi) in enumerate(cuts)]


def test_oriented_batch_writes_from_the_records(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd.SeqSample import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    _db_dir(monkeypatch, gold)
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    files = _ccs_inputs(gold, str(tmp_path / "in"))
    hmm = _its2_hmm(tmp_path, t_hmm_text)
    bd = str(tmp_path / "batch")
    os.makedirs(bd)

    def run(keep, subdirs, tag):
        objs = [SeqSampleNotPaired(fastq=f, tempdir=bd) for f in files]
        b = SampleBatch(objs, engine=engine, subdirs=subdirs, keep_records=keep)
        b.orient_reads(threads=1)
        seq_there = [os.path.exists(o.seq_file) for o in objs]
        before = [sum(1 for _ in open(f)) // 4 for f in files]
        b.deduplicate(threads=1)
        b._search(hmmfile=hmm, threads=1)
        outs = [os.path.join(bd, "%s_%d.fq" % (tag, k)) for k in range(len(objs))]
        ret = b.write_trimmed(outs, "ITS2", trim_ccs=True)
        return seq_there, [open(p, "rb").read() for p in outs], [tuple(x) for x in ret], list(b.counts), before

    seq_there, got, ret, counts, before = run(True, ["k%d" % k for k in range(3)], "kept")
    assert seq_there == [False, False, False]                   # no oriented.fq
    seq_there2, exp, ret2, counts2, _ = run(False, ["w%d" % k for k in range(3)], "files")
    assert seq_there2 == [True, True, True] and counts == counts2 and all(c < n for c, n in zip(counts, before))     # undetermined reads were dropped
    assert got == exp and ret == ret2 and all(len(g) > 1000 for g in got)
    assert any(any(c.islower() for c in g.decode().split("\n")[1][17:-17]) for g in got)          # the input's case came through


# ------------------------------------------------------------------ errors
def test_errors_and_what_survives_them(loaded, gold, tmp_path, monkeypatch):
    from itsxpress_amd import Engine, EngineError
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    eng = Engine(0)                                             # its own context: no orientation database, no profiles
    files, a, b = loaded["files"], loaded["start"], loaded["stop"]
    outs = [str(tmp_path / ("e%d.fq" % k)) for k in range(4)]
    eng.load_reads_files(files)
    with pytest.raises(EngineError, match="itsx_keep_records") as ei:
        eng.write_trimmed_samples(outs, start=a, stop=b)
    assert ei.value.code == -1
    eng.keep_records(True)
    eng.load_reads_files(files)
    for bad in (dict(paths=outs[:3], start=a, stop=b), dict(paths=outs + [outs[0]], start=a, stop=b), dict(paths=outs),
                dict(paths=outs, region_prefixes=("3_", "4_"), start=a, stop=b), dict(paths=outs, start=a)):
        with pytest.raises(EngineError) as ei:
            eng.write_trimmed_samples(bad.pop("paths"), **bad)
        assert ei.value.code == -1
    with pytest.raises(EngineError, match="itsx_search_finalize") as ei:
        eng.write_trimmed_samples(outs, region_prefixes=("3_", "4_"))
    assert ei.value.code == -1
    assert not any(os.path.exists(p) for p in outs)
    # a FAILED orient_apply (no database loaded) keeps the read set and its records
    with pytest.raises(EngineError) as ei:
        eng.orient_apply()
    assert ei.value.code == -1
    ret = eng.write_trimmed_samples(outs, start=a, stop=b)
    exp, exp_ret = loaded["ref"][0]
    assert [open(p, "rb").read() for p in outs] == exp and [tuple(x) for x in ret] == [tuple(x) for x in exp_ret]
    # a FASTA file cannot keep records
    fa = str(tmp_path / "x.fa")
    with open(fa, "w") as f:
        f.write(">r1\nACGT\n")
    with pytest.raises(EngineError, match="x.fa") as ei:
        eng.load_reads_files([files[0], fa])
    assert ei.value.code == -3
    # a new read set loaded with records off has none
    eng.keep_records(False)
    eng.load_reads_files(files)
    with pytest.raises(EngineError, match="itsx_keep_records"):
        eng.write_trimmed_samples(outs, start=a, stop=b)
    # and a batch without keep_records still asks for the files
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "1")
    r1 = os.path.join(gold, "4774-1-MSITS3_R1.fastq.gz")
    r2 = os.path.join(gold, "4774-1-MSITS3_R2.fastq.gz")
    bt = SampleBatch([SeqSamplePairedNotInterleaved(fastq=r1, tempdir=str(tmp_path), fastq2=r2)], engine=eng)
    bt.merge_reads(threads=1)
    with pytest.raises(EngineError, match="write_seq_files"):
        bt.write_trimmed([str(tmp_path / "t.fq")], "ITS2")
    eng.close()
