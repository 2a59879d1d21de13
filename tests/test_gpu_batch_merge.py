"""The read pairs of every sample of a batch merged in one GPU pass (itsx_merge_pairs_load_files, SampleBatch.merge_reads):
every sample must get exactly what a merge of that sample alone gives -- counts, pair index, labels, packed reads, sample ids,
and, through the batch mirror, the files and the trimmed reads of its own run.  `pytest -m gpu`."""
import gzip
import os
import re

import numpy as np
import pytest

import orc
from test_gpu_merge import _read_fastq

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGTN", "TGCAN")
_ACGT = np.array(list("ACGT"))


def _rc(s):
    return s[::-1].translate(_COMP)


def _have_zstd(engine):
    return bool(engine.L.itsx_io_codecs() & 2)


def _write_pair(d, name, recs1, recs2, kind):
    """two FASTQ files of one sample: kind "" plain, ".gz" gzip, ".zst" zstd (through the project's own block writer)"""
    from itsxpress_amd.trim import write_trimmed_fastq
    out = []
    for tag, recs in (("R1", recs1), ("R2", recs2)):
        text = "".join("@%s\n%s\n+\n%s\n" % r for r in recs)
        plain = os.path.join(d, "%s_%s.fq" % (name, tag))
        path = plain + kind
        if kind == ".gz":
            with open(path, "wb") as f:
                f.write(gzip.compress(text.encode()))
        else:
            with open(plain, "w") as f:
                f.write(text)
            if kind == ".zst":
                n = len(recs)
                write_trimmed_fastq(plain, path, np.zeros(n, np.int32), np.full(n, 1 << 20, np.int32), zstd_file=True)
        out.append(path)
    return out


def _overlapping_pairs(rng, n, lo, hi, name):
    """n pairs cut from random fragments of lo..hi bases, a few substitutions, qualities 20..40"""
    r1, r2 = [], []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        frag = "".join(_ACGT[rng.integers(0, 4, L)])
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


@pytest.fixture(scope="module")
def fixture_pairs(gold):
    return (_read_fastq(os.path.join(gold, "4774-1-MSITS3_R1.fastq.gz")), _read_fastq(os.path.join(gold, "4774-1-MSITS3_R2.fastq.gz")))


def _compaction_tile():
    """pairs per block of the compaction kernels, from their source (k_merge.hip: MC_BLOCK threads x MC_ITEMS pairs)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "itsxpress_amd", "csrc", "k_merge.hip")) as f:
        src = f.read()
    return int(re.search(r"MC_BLOCK = (\d+);", src).group(1)) * int(re.search(r"MC_ITEMS = (\d+);", src).group(1))


def _solo(engine, r1, r2, **kw):
    """one sample alone through merge_pairs_load: counts, pair index, labels, packed reads"""
    n, m = engine.merge_pairs_load(r1, r2, **kw)
    idx = np.zeros(max(1, n), np.int32)
    engine._chk(engine.L.itsx_merge_pair_index(engine.h, idx.ctypes.data, n))
    assert engine.L.itsx_num_samples(engine.h) == 1
    assert not engine.debug_read_samples()[0].any()
    return n, m, idx[:n].copy(), engine.read_names(), [engine.debug_packed_read(i) for i in range(m)]


def test_batch_merge_equals_each_sample_alone(engine, fixture_pairs, tmp_path):
    a, b = fixture_pairs
    d = str(tmp_path)
    zst = ".zst" if _have_zstd(engine) else ".gz"
    rng = np.random.default_rng(41)
    files, kinds = [], ["", ".gz", zst, "", ".gz", zst]
    cut = np.concatenate([[0], np.cumsum([0, 1, 63, 64, 65, 57])])
    assert cut[-1] == len(a) == 250
    for k in range(6):
        files.append(_write_pair(d, "fx%d" % k, a[cut[k]:cut[k + 1]], b[cut[k]:cut[k + 1]], kinds[k]))
    n_fixture = 6
    # 1 100 short pairs, not a multiple of 64 (with the samples before them they end at pair 1 350: still inside the compaction's first
    # block of 2 048 pairs -- the samples appended below carry the batch over three blocks)
    files.append(_write_pair(d, "short", *_overlapping_pairs(rng, 1100, 60, 110, "sh"), ".gz"))
    # the fifth sample once more: its reads are duplicates ACROSS samples, which only the per-read sample id keeps apart
    i_dup = len(files)
    files.append(_write_pair(d, "dup", a[cut[4]:cut[5]], b[cut[4]:cut[5]], ""))
    i_empty = len(files)
    files.append(_write_pair(d, "e0", [], [], ""))
    files.append(_write_pair(d, "e1", [], [], ".gz"))          # two consecutive empty samples in the middle
    # 40 pairs of unrelated mates: nothing merges, with or without staggered alignments (checked on the CPU)
    u1 = [("un%02d" % i, "".join(_ACGT[rng.integers(0, 4, 120)]), "I" * 120) for i in range(40)]
    u2 = [("un%02d" % i, "".join(_ACGT[rng.integers(0, 4, 110)]), "I" * 110) for i in range(40)]
    for (_, f, fq), (_, r, rq) in zip(u1, u2):
        for st in (False, True):
            assert orc.merge_pair(f, fq, r, rq, allow_stagger=st)[0] != "ok"
    i_unrelated = len(files)
    files.append(_write_pair(d, "unrel", u1, u2, ""))
    # 21 pairs, one of them 2 600 + 2 400 bases: over 4 096 in total, so the batch (and this sample alone) runs the kernel variant
    # without the 5-mer index while the other samples alone run the indexed one.  Quality 40 throughout: about 0.4 expected errors over
    # the 4 200 merged bases, below the default maxee of 2 -- the long pair merges (checked on the CPU)
    l1, l2 = _overlapping_pairs(rng, 20, 150, 400, "lg")
    frag = "".join(_ACGT[rng.integers(0, 4, 4200)])
    lf, lr = frag[:2600], _rc(frag[1800:])
    assert len(lr) == 2400 and orc.merge_pair(lf, "I" * 2600, lr, "I" * 2400)[0] == "ok"
    l1.insert(7, ("longpair", lf, "I" * 2600))
    l2.insert(7, ("longpair", lr, "I" * 2400))
    i_long = len(files)
    files.append(_write_pair(d, "long", l1, l2, zst))
    # The compaction works in blocks of `tile` pairs, scans the blocks' sums in a second level and adds them back.  The batch so far
    # fits one block, so it goes on: a sample that ends exactly ON the first block boundary, an empty sample right there, a sample that
    # starts on that boundary and runs through the whole second block into the third (the second boundary falls inside it), and one
    # more that starts and ends inside the third block
    tile = _compaction_tile()
    so_far = 250 + 1100 + 65 + 40 + 21
    assert tile == 2048 and so_far < tile
    i_fill = len(files)
    files.append(_write_pair(d, "fill", *_overlapping_pairs(rng, tile - so_far, 60, 110, "fi"), ""))
    files.append(_write_pair(d, "e_on_tile", [], [], ""))
    files.append(_write_pair(d, "span", *_overlapping_pairs(rng, tile + 52, 60, 110, "sp"), ".gz"))
    files.append(_write_pair(d, "tail", *_overlapping_pairs(rng, 100, 60, 110, "ta"), ""))
    files.append(_write_pair(d, "e2", [], [], ""))             # and an empty sample at the end
    S = len(files)
    r1s, r2s = [f[0] for f in files], [f[1] for f in files]
    for kw in ({}, {"allow_stagger": True}):
        solo = [_solo(engine, r1, r2, **kw) for r1, r2 in files]
        n, m = engine.merge_pairs_load_files(r1s, r2s, **kw)
        assert engine.n_samples == S == engine.L.itsx_num_samples(engine.h) and engine.n_reads == int(m.sum())
        idx = engine.merge_pair_index()
        names = engine.read_names()
        assert len(idx) == int(n.sum()) and len(names) == int(m.sum())
        pfirst = np.concatenate([[0], np.cumsum(n)])
        rfirst = np.concatenate([[0], np.cumsum(m)])
        for s in range(S):
            sn, sm, sidx, snames, spacked = solo[s]
            assert (int(n[s]), int(m[s])) == (sn, sm), s
            mine = idx[pfirst[s]:pfirst[s + 1]].copy()
            mine[mine >= 0] -= rfirst[s]
            assert np.array_equal(mine, sidx), s
            assert names[rfirst[s]:rfirst[s + 1]] == snames, s
            for j in range(sm):
                w, e = engine.debug_packed_read(int(rfirst[s]) + j)
                assert np.array_equal(w, spacked[j][0]) and np.array_equal(e, spacked[j][1]), (s, j)
        # the blocks of the compaction: the sample boundaries sit where the comments above say, and the third block is reached
        assert pfirst[i_fill + 1] == pfirst[i_fill + 2] == tile and pfirst[i_fill + 2] < 2 * tile < pfirst[i_fill + 3] < pfirst[-1] < 3 * tile
        assert int(n.sum()) > 2 * tile and m[i_fill] > 400 and m[i_fill + 2] > 1800 and m[i_fill + 3] > 70
        # the per-read sample id, as the kernels see it (written by the compaction) and as the writers see it: sample s's reads carry s
        # -- in a run of the sample alone every read carries 0, the only sample there is
        dev_ids, host_ids = engine.debug_read_samples()
        expect = np.repeat(np.arange(S, dtype=np.int32), m)
        assert np.array_equal(dev_ids, expect) and np.array_equal(host_ids, expect)
        # and what hangs on it: dereplication never leaves the sample, and the writers pick the sample's reads
        engine.derep()
        rep_of, _, _ = engine.get_derep()
        for s in range(S):
            mine = rep_of[rfirst[s]:rfirst[s + 1]]
            assert np.all((mine >= rfirst[s]) & (mine < rfirst[s + 1])), s
        assert np.array_equal(rep_of[rfirst[i_dup]:rfirst[i_dup + 1]] - rfirst[i_dup], rep_of[rfirst[4]:rfirst[5]] - rfirst[4]) and m[i_dup] == m[4] > 50
        for s in (0, 3, 6, i_long, i_fill + 2, i_fill + 3):
            engine.select_sample(s)
            uc = str(tmp_path / ("uc_%d.txt" % s))
            engine.write_uc(uc)
            rows = [ln.split("\t") for ln in open(uc).read().splitlines()]
            assert sorted(r[8] for r in rows if r[0] in "SH") == sorted(names[rfirst[s]:rfirst[s + 1]]), s
        engine.select_sample(-1)
        assert list(n[:6]) == [0, 1, 63, 64, 65, 57] and int(n[6]) == 1100 and int(m[6]) > 1000
        assert int(m[:n_fixture].sum()) == 236 if not kw else int(m[:n_fixture].sum()) >= 236
        assert int(m[i_unrelated]) == 0 and int(n[i_unrelated]) == 40
        assert [int(n[s]) for s in (i_empty, i_empty + 1, S - 1)] == [0, 0, 0]
        assert idx[pfirst[i_long] + 7] >= 0 and names[idx[pfirst[i_long] + 7]] == "longpair"      # the long pair merged, in the batch too


def _samples_for_mirror(d, a, b):
    """the fixture pairs as three paired samples (plain, gzip, plain) and an empty one; the second is given with reversed primers"""
    os.makedirs(d, exist_ok=True)
    parts = [(0, 90, ""), (90, 200, ".gz"), (200, 200, ""), (200, 250, "")]
    return [_write_pair(d, "m%d" % k, a[lo:hi], b[lo:hi], kind) for k, (lo, hi, kind) in enumerate(parts)]


def _make_sample(k, files, tempdir):
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    r1, r2 = files
    if k == 1:      # reversed primers: the caller's fastq is R2 and fastq2 is R1; the sample swaps them back (SeqSample.py:244-264)
        return SeqSamplePairedNotInterleaved(fastq=r2, tempdir=tempdir, fastq2=r1, reversed_primers=True)
    return SeqSamplePairedNotInterleaved(fastq=r1, tempdir=tempdir, fastq2=r2)


def _trimmed(s, d, tag):
    """the mirror's Dedup / ItsPosition on a sample's files -> the bytes of its paired and of its merged trimmed output"""
    from itsxpress_amd.SeqSample import Dedup, ItsPosition
    pos = ItsPosition(domtable=s.dom_file, region="ITS2")
    dd = Dedup(uc_file=s.uc_file, rep_file=s.rep_file, seq_file=s.seq_file, fastq=s.r1, fastq2=s.fastq2)
    o1, o2, om = (os.path.join(d, "%s_%s.fq" % (tag, x)) for x in ("o1", "o2", "om"))
    dd.create_paired_trimmed_seqs(o1, o2, gzipped=False, zstd_file=False, itspos=pos, wri_file=True)
    dd.create_trimmed_seqs(om, gzipped=False, zstd_file=False, itspos=pos, wri_file=True, tempdir=d)
    return [open(p, "rb").read() for p in (o1, o2, om)]


def _its2_hmm(tmp_path, t_hmm_text):
    from bench import its2_profiles
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    return str(hmm)


def test_batch_of_paired_samples_writes_each_samples_files(engine, fixture_pairs, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    files = _samples_for_mirror(str(tmp_path / "in"), *fixture_pairs)
    hmm = _its2_hmm(tmp_path, t_hmm_text)
    kinds = ("seq_file", "uc_file", "rep_file", "dom_file")
    solo = []
    for k, f in enumerate(files):
        d = str(tmp_path / "solo" / str(k))
        os.makedirs(d)
        s = _make_sample(k, f, d)
        s._engine = engine
        s._merge_reads(threads=1, stagger=False)
        s.deduplicate(threads=1)
        s._search(hmmfile=hmm, threads=1)
        solo.append([open(getattr(s, x), "rb").read() for x in kinds] + _trimmed(s, d, "solo"))
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    objs = [_make_sample(k, f, bd) for k, f in enumerate(files)]
    assert all(o.seq_file is None for o in objs)
    b = SampleBatch(objs, engine=engine)
    b.merge_reads(threads=1, stagger=False)
    assert list(b.n_pairs) == [90, 110, 0, 50] and int(b.counts.sum()) == 236 and list(b.first) == list(np.cumsum([0] + list(b.counts[:-1])))
    loads = []
    monkeypatch.setattr(engine, "load_reads_files", lambda paths: loads.append(paths))
    b.deduplicate(threads=1)
    b._search(hmmfile=hmm, threads=1)
    assert loads == []                                          # the merged reads were resident: no seq.fq was parsed again
    for k, s in enumerate(objs):
        assert s.seq_file == os.path.join(bd, b.subdirs[k], "seq.fq") and os.path.dirname(s.uc_file) == os.path.dirname(s.seq_file)
        got = [open(getattr(s, x), "rb").read() for x in kinds] + _trimmed(s, os.path.dirname(s.seq_file), "batch")
        for name, g, e in zip(kinds + ("out1", "out2", "merged_out"), got, solo[k]):
            assert g == e, (k, name)
    assert solo[2][0] == solo[2][1] == solo[2][2] == b"" and solo[2][4:] == [b"", b"", b""] and len(solo[0][3]) > 1000 and len(solo[1][4]) > 1000 and len(solo[3][6]) > 1000


def test_batch_arrays_mode_keeps_merged_reads_resident(engine, fixture_pairs, t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd import EngineError
    from itsxpress_amd.SeqSample import Dedup, ItsPosition
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "1")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    files = _samples_for_mirror(str(tmp_path / "in"), *fixture_pairs)
    hmm = _its2_hmm(tmp_path, t_hmm_text)
    solo = []
    for k, f in enumerate(files):
        d = str(tmp_path / "solo" / str(k))
        os.makedirs(d)
        s = _make_sample(k, f, d)
        s._engine = engine
        s._merge_reads(threads=1, stagger=False)
        assert not os.path.exists(os.path.join(d, "seq.fq"))
        s.deduplicate(threads=1)
        s._search(hmmfile=hmm, threads=1)
        coords = [np.asarray(c).copy() for c in s.trim_coordinates("ITS2")]
        pos = ItsPosition(domtable=s.dom_file, region="ITS2")
        dd = Dedup(uc_file=s.uc_file, rep_file=s.rep_file, seq_file=s.seq_file, fastq=s.r1, fastq2=s.fastq2)
        o1, o2, om = (os.path.join(d, x) for x in ("o1.fq", "o2.fq", "om.fq"))
        dd.create_paired_trimmed_seqs(o1, o2, gzipped=False, zstd_file=False, itspos=pos, wri_file=True)
        dd.create_trimmed_seqs(om, gzipped=False, zstd_file=False, itspos=pos, wri_file=True, tempdir=d)     # (writes the solo seq.fq)
        if engine.n_reads:
            s.cluster(threads=1, cluster_id=0.97)
            rep_of, strand, _ = engine.get_derep()
        else:                                                   # the empty sample: no reads, no clusters
            rep_of, strand = np.zeros(0, np.int64), np.zeros(0, np.int8)
        solo.append(dict(coords=coords, out=[open(p, "rb").read() for p in (o1, o2, om)], seq=open(os.path.join(d, "seq.fq"), "rb").read(),
                         rep_of=rep_of.copy(), strand=strand.copy()))
    # an arrays-mode SeqSample._search leaves the engine it ran on in the "lazy" rows mode, which keeps no row table; the batch writes
    # every sample's domtbl.txt, so the shared engine goes back to its default before the batch uses it
    engine.set_rows_mode(None)
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    objs = [_make_sample(k, f, bd) for k, f in enumerate(files)]
    b = SampleBatch(objs, engine=engine)
    with pytest.raises(EngineError, match="never merged"):
        b.deduplicate(threads=1)
    b.merge_reads(threads=1)
    assert not any(os.path.exists(o.seq_file) for o in objs)    # arrays mode: nothing written
    loads = []
    monkeypatch.setattr(engine, "load_reads_files", lambda paths: loads.append(paths))
    b.deduplicate(threads=1)
    b._search(hmmfile=hmm, threads=1)
    per = b.trim_coordinates("ITS2")
    o1s = [os.path.join(bd, "o1_%d.fq" % k) for k in range(len(objs))]
    o2s = [os.path.join(bd, "o2_%d.fq" % k) for k in range(len(objs))]
    oms = [os.path.join(bd, "om_%d.fq" % k) for k in range(len(objs))]
    written = b.write_paired_trimmed(o1s, o2s, "ITS2")
    for k in range(len(objs)):
        for g, e in zip(per[k], solo[k]["coords"]):
            assert np.array_equal(g, e), k
        assert open(o1s[k], "rb").read() == solo[k]["out"][0] and open(o2s[k], "rb").read() == solo[k]["out"][1], k
        assert written[k] == solo[k]["out"][0].count(b"\n") // 4
    with pytest.raises(EngineError, match="write_seq_files"):
        b.write_trimmed(oms, "ITS2")
    # greedy clustering of every sample, still from the resident merged reads
    b.cluster_per_sample(threads=1, cluster_id=0.97)
    assert loads == []
    rep_of, strand, _ = engine.get_derep()
    for k in range(len(objs)):
        lo, hi = int(b.first[k]), int(b.first[k] + b.counts[k])
        mine = rep_of[lo:hi].copy()
        mine[mine >= 0] -= lo
        assert np.array_equal(mine, solo[k]["rep_of"]) and np.array_equal(strand[lo:hi], solo[k]["strand"]), k
    assert sum(int((x["rep_of"] != np.arange(len(x["rep_of"]))).sum()) for x in solo) > 0        # reads did join clusters
    # the merged reads on disk after all: write_trimmed works from them
    objs2 = [_make_sample(k, f, bd) for k, f in enumerate(files)]
    b2 = SampleBatch(objs2, engine=engine, subdirs=["w%d" % k for k in range(len(objs2))])
    b2.merge_reads(threads=1, write_seq_files=True)
    b2.deduplicate(threads=1)
    b2._search(hmmfile=hmm, threads=1)
    assert loads == []
    b2.write_trimmed(oms, "ITS2")
    for k, o in enumerate(objs2):
        assert open(o.seq_file, "rb").read() == solo[k]["seq"], k
        assert open(oms[k], "rb").read() == solo[k]["out"][2], k
    assert len(solo[0]["out"][2]) > 1000 and solo[2]["seq"] == b""
    # the first batch wrote no seq.fq and the shared engine now holds the second batch's reads: it says so instead of running on them
    with pytest.raises(EngineError, match="merge_reads\\(\\) again"):
        b.deduplicate(threads=1)


def test_batch_merge_errors_leave_the_context_usable(engine, fixture_pairs, tmp_path):
    from itsxpress_amd import EngineError
    a, b = fixture_pairs
    d = str(tmp_path)
    good = [_write_pair(d, "g0", a[:40], b[:40], ""), _write_pair(d, "g1", a[40:41], b[40:41], ".gz"), _write_pair(d, "g2", a[41:100], b[41:100], "")]
    r1s, r2s = [f[0] for f in good], [f[1] for f in good]
    n0, m0 = engine.merge_pairs_load_files(r1s, r2s)
    names0, idx0 = engine.read_names(), engine.merge_pair_index().copy()
    assert list(n0) == [40, 1, 59] and int(m0.sum()) > 80

    def still_works():
        assert engine.n_reads == 0 and engine.n_samples == 1 and engine.L.itsx_num_samples(engine.h) == 1
        assert engine.derep() == 0                               # empty, and usable as it is
        n, m = engine.merge_pairs_load_files(r1s, r2s)
        assert np.array_equal(n, n0) and np.array_equal(m, m0) and engine.read_names() == names0
        assert np.array_equal(engine.merge_pair_index(), idx0) and engine.n_samples == 3

    # R2 of the second sample one record short
    short = _write_pair(d, "short", a[40:43], b[40:42], "")
    with pytest.raises(EngineError) as ei:
        engine.merge_pairs_load_files([r1s[0], short[0], r1s[2]], [r2s[0], short[1], r2s[2]])
    assert ei.value.code == -3 and short[0] in str(ei.value) and short[1] in str(ei.value)
    still_works()
    # a file that is not there
    with pytest.raises(FileNotFoundError):
        engine.merge_pairs_load_files(r1s, [r2s[0], str(tmp_path / "nope.fq"), r2s[2]])
    n, m = engine.merge_pairs_load_files(r1s, r2s)
    assert np.array_equal(m, m0)
    # a quality byte outside 33..126 in the third sample
    bad2 = list(b[41:100])
    h, s, q = bad2[30]
    bad2[30] = (h, s, q[:17] + "\x7f" + q[18:])
    bad = _write_pair(d, "bad", a[41:100], bad2, "")
    with pytest.raises(EngineError) as ei:
        engine.merge_pairs_load_files([r1s[0], r1s[1], bad[0]], [r2s[0], r2s[1], bad[1]])
    assert ei.value.code == -3 and "quality" in str(ei.value)
    still_works()
