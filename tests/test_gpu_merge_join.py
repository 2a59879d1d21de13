"""Joining the read pairs that do not overlap (Engine.merge_join, itsx_set_merge_join; csrc/k_merge.hip: JOIN) on the device.
The verdict of every pair is the CPU oracle's (orc.merge_pair), the text of every joined read is the plain-Python model's
(tests/join_exact.py), and every comparison is `==`: the rule has no tolerance.  Parity with vsearch --fastq_join is unpinned (no
vsearch build was at hand), as for the merge itself.  `pytest -m gpu`."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import join_cases as JC
import join_exact as J
import orc

pytestmark = pytest.mark.gpu
TILE = 2048                                                   # pairs per block of the compaction (k_merge.hip: MC_TILE)


@pytest.fixture(scope="module")
def its2_hmm(t_hmm_text, tmp_path_factory):
    from bench import its2_profiles
    p = tmp_path_factory.mktemp("join_hmm") / "its2.hmm"
    p.write_text(its2_profiles(t_hmm_text))
    return str(p)


def _engine(join=False, parse="host"):
    from itsxpress_amd import Engine
    e = Engine(0)
    if parse != "host":
        e.parse = parse
    if join:
        e.merge_join = True
    return e


def _split(cases):
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]


def _oracle(cases):
    """per pair (reason code, merged bases, merged quals, score, shift) of the oracle, on the bases in upper case as every merge entry
    point reads them"""
    out = []
    for f, fq, r, rq in cases:
        o = orc.merge_pair(J.upper(f), fq, J.upper(r), rq)
        out.append((orc.MERGE_REASONS.index(o[0]),) + tuple(o[1:]))
    return out


# ------------------------------------------------------------------ 1. off is the engine as it was
def test_off_and_switched_off_again_are_a_fresh_context(gold, tmp_path):
    cases = JC.synthetic_pairs() + JC.unrelated_pairs() + JC.verdict_pairs() + JC.edge_pairs()
    fresh, toggled = _engine(), _engine()
    try:
        assert fresh.merge_join is False
        toggled.merge_join = True
        assert toggled.merge_join is True
        toggled.merge_join = False
        with pytest.raises(ValueError):
            toggled.merge_join = 1
        res = []
        for e in (fresh, toggled):
            reason, merged, score, shift = e.merge_pairs(*_split(cases))
            out = str(tmp_path / ("seq_%d.fq" % len(res)))
            counts = e.merge_pairs_files(JC.R1, JC.R2, out)
            joined, nj = e.merge_join_info()
            assert nj == 0 and joined.shape == (250,) and not joined.any()
            n, m = e.merge_pairs_load(JC.R1, JC.R2)
            assert e.n_reads == m and e.merge_join_info()[1] == 0
            res.append((reason.tobytes(), merged, score.tobytes(), shift.tobytes(), counts, open(out, "rb").read(), (n, m), e.merge_pair_index().tobytes(),
                        e.read_names()))
        assert res[0] == res[1]
        assert res[0][4] == (250, 236) and res[0][5].count(b"\n") == 4 * 236 and b"NNNNNNNN" not in res[0][5]
        exp = _oracle(cases)
        assert [int(x) for x in np.frombuffer(res[0][0], np.int32)] == [o[0] for o in exp]
        assert all((m is None) == (o[0] != 0) for m, o in zip(res[0][1], exp))
    finally:
        fresh.close()
        toggled.close()


# ------------------------------------------------------------------ 2. on: every pair against the oracle's verdict and the model's text
def _check_buffers(eng_on, eng_off, cases, seen):
    fwd, fq, rev, rq = _split(cases)
    reason, reads, score, shift, joined = eng_on.merge_pairs(fwd, fq, rev, rq, join=True)
    reason0, reads0, score0, shift0 = eng_off.merge_pairs(fwd, fq, rev, rq)
    assert reason.tobytes() == reason0.tobytes() and score.tobytes() == score0.tobytes() and shift.tobytes() == shift0.tobytes()
    exp = _oracle(cases)
    for i, (c, o) in enumerate(zip(cases, exp)):
        k = int(reason[i])
        seen[k] += 1
        assert k == o[0], (i, k, o[0])
        assert np.float64(score[i]).view(np.uint64) == np.float64(o[3]).view(np.uint64) and int(shift[i]) == o[4], i
        assert int(joined[i]) == (1 if k in (1, 3, 5) else 0), (i, k)
        if k == 0:
            assert reads[i] == reads0[i] == (o[1], o[2]), i                # merged pairs: bit for bit the off run's
        elif k in (1, 3, 5):
            assert reads0[i] is None
            assert reads[i] == J.join_pair(*c), (i, k)
            assert len(reads[i][0]) == len(c[0]) + 8 + len(c[2])
        else:
            assert reads[i] is None and reads0[i] is None, (i, k)          # nothing is written for the other reasons


def test_on_buffers_against_the_oracle_and_the_model():
    """itsx_merge_buffers_join.  Two calls: one whose longest pair has 4096 bases (the kernel with the 5-mer index) and one that holds a
    pair of 4097 and one of 12 000 (the plain kernel); both see the whole verdict mix.  The first also holds 70 000 pairs of 1-3 bases:
    more pairs than the launch has blocks."""
    from collections import Counter
    mix = JC.synthetic_pairs() + JC.unrelated_pairs() + JC.verdict_pairs() + JC.edge_pairs()
    on, off = _engine(), _engine()
    try:
        seen = Counter()
        indexed = mix + [JC.long_pair(4096, 1)] + JC.tiny_pairs(70000)
        assert max(len(c[0]) + len(c[2]) for c in indexed) == 4096
        _check_buffers(on, off, indexed, seen)
        assert all(seen[k] >= 1 for k in range(9)), dict(seen)              # guard: every reason 0..8 occurs
        seen2 = Counter()
        plain = mix + [JC.long_pair(4097, 2), JC.long_pair(12000, 3)]
        _check_buffers(on, off, plain, seen2)
        assert all(seen2[k] >= 1 for k in range(9)), dict(seen2)
        # the setting is not consulted by the buffers calls: itsx_merge_buffers stays the merge alone with it on
        on.merge_join = True
        r_on = on.merge_pairs(*_split(mix))
        r_off = off.merge_pairs(*_split(mix))
        assert r_on[0].tobytes() == r_off[0].tobytes() and r_on[1] == r_off[1]
        reason, reads, _, _, joined = on.merge_pairs([], [], [], [], join=True)
        assert len(reason) == 0 and reads == [] and len(joined) == 0
    finally:
        on.close()
        off.close()


def _as_records(cases, tag):
    return [("@%s%d 1:N:0" % (tag, i), c[0], c[1], "@%s%d 2:N:0" % (tag, i), c[2], c[3]) for i, c in enumerate(cases)]


def _model_reads(pairs):
    """the read set the rule leaves: ([(label, bases, quals)] in pair order, per pair its read or -1, per pair joined 0 / 1, merged count)"""
    recs, index, joined, merged = [], [], [], 0
    for t1, s1, q1, t2, s2, q2 in pairs:
        o = orc.merge_pair(J.upper(s1), q1, J.upper(s2), q2)
        rec = J.read_of_pair(o[0], (o[1], o[2]), s1, q1, s2, q2)
        index.append(len(recs) if rec is not None else -1)
        joined.append(1 if rec is not None and o[0] != "ok" else 0)
        merged += o[0] == "ok"
        if rec is not None:
            recs.append((JC.label(t1), rec[0], rec[1]))
    return recs, np.array(index, np.int32), np.array(joined, np.int8), merged


def _load_text(eng, text):
    buf = ctypes.create_string_buffer(text, len(text))
    eng._text_keep = buf                                     # (the context may read the text where it lies)
    eng.load_reads_text(ctypes.addressof(buf), len(text))


def _packed(eng, i):
    w, e = eng.debug_packed_read(i)
    return w.tobytes(), e.tobytes()


def test_on_read_set_across_the_compaction_tiles(tmp_path):
    """merge-and-load with the setting on, pairs of every verdict laid around the compaction's tile edges (pair 2047 / 2048 / 2049 and
    the next tile's), 70 000 pairs in all: the read set is the model's seq.fq, read for read"""
    syn = JC.synthetic_pairs()
    verdicts = [o[0] for o in _oracle(syn)]
    by = {k: [c for c, v in zip(syn, verdicts) if v == k] for k in set(verdicts)}
    assert all(len(by.get(k, [])) >= 4 for k in (0, 1, 2, 3, 6, 7)), {k: len(v) for k, v in by.items()}
    vp = JC.verdict_pairs()[:3]                               # reasons 4, 5, 7 (an empty mate cannot stand in a FASTQ file)
    tiny = JC.tiny_pairs(70000 - 600 - 64 - 6 - 3 - 2 * 12 - 1)

    def edge(j):                                             # twelve pairs: not kept | merged | joined | not kept | joined | merged ...
        return [by[2][j], by[7][j], by[0][j], by[1][j], by[6][j], by[3][j], by[0][j + 2], vp[0], vp[1], by[2][j + 2], by[1][j + 2], by[7][j + 2]]
    cases = tiny[:TILE - 6] + edge(0) + tiny[TILE - 6:2 * TILE - 12 - 6] + edge(1) + tiny[2 * TILE - 12 - 6:] + syn + JC.unrelated_pairs() + JC.edge_pairs() + vp \
        + [JC.long_pair(4096, 1)]
    assert len(cases) == 70000
    pairs = _as_records(cases, "p")
    recs, index, joined, merged = _model_reads(pairs)
    for t in (TILE, 2 * TILE):                                # the verdicts change on both sides of a tile's edge
        assert len({int(index[p]) < 0 for p in range(t - 3, t + 3)}) == 2 and len({int(joined[p]) for p in range(t - 3, t + 3)}) == 2
    r1, r2 = JC.write_pair_files(pairs, str(tmp_path / "t_R1.fq"), str(tmp_path / "t_R2.fq"))
    text = J.fastq_text(recs).encode()
    eng, ref = _engine(join=True), _engine()
    try:
        n, m = eng.merge_pairs_load(r1, r2)
        assert (n, m) == (70000, merged) and eng.n_reads == len(recs)
        got_joined, nj = eng.merge_join_info()
        assert nj == int(joined.sum()) and got_joined.tobytes() == joined.tobytes()
        assert eng.merge_pair_index().tobytes() == index.tobytes()
        assert eng.read_names() == [r[0] for r in recs]
        _load_text(ref, text)
        assert ref.n_reads == len(recs)
        look = set()
        for t in (TILE, 2 * TILE):
            look |= {int(index[p]) for p in range(t - 8, t + 8) if index[p] >= 0}
        look |= {int(index[p]) for p in range(len(tiny) + 24, 70000) if index[p] >= 0}         # every read that is not a tiny one
        assert len(look) > 400
        for i in sorted(look):
            assert _packed(eng, i) == _packed(ref, i), i
        eng.derep()
        ref.derep()
        assert eng.n_unique == ref.n_unique
        assert all(a.tobytes() == b.tobytes() for a, b in zip(eng.get_derep(), ref.get_derep()))
        for e, tag in ((eng, "a"), (ref, "b")):
            e.write_uc(str(tmp_path / ("uc_" + tag)))
            e.write_rep_fasta(str(tmp_path / ("rep_" + tag)))
        assert open(tmp_path / "uc_a", "rb").read() == open(tmp_path / "uc_b", "rb").read()
        assert open(tmp_path / "rep_a", "rb").read() == open(tmp_path / "rep_b", "rb").read()
        # seq.fq: the same records through itsx_merge_pairs_files
        out = str(tmp_path / "seq.fq")
        assert eng.merge_pairs_files(r1, r2, out) == (70000, merged) and eng.n_joined == int(joined.sum())
        assert open(out, "rb").read() == text
    finally:
        eng.close()
        ref.close()


# ------------------------------------------------------------------ 3. the read set on the fixture, host and device parse
@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """the fixture with its odd pairs cut to 150 bases a mate, as files (gzip, like the fixture), and the model's read set"""
    d = tmp_path_factory.mktemp("join_mixed")
    pairs = JC.odd_cut()
    r1, r2 = JC.write_pair_files(pairs, str(d / "mixed_R1.fastq.gz"), str(d / "mixed_R2.fastq.gz"), gz=True)
    recs, index, joined, merged = _model_reads(pairs)
    assert merged == 121 and int(joined.sum()) == 126 and len(recs) == 247       # guards: the oracle's counts (tests/test_merge_join_cpu.py)
    return dict(dir=str(d), pairs=pairs, r1=r1, r2=r2, recs=recs, index=index, joined=joined, text=J.fastq_text(recs).encode())


def _search(eng, hmm, rows):
    eng.set_rows_mode(rows)
    eng.load_profiles(path=hmm)
    eng.derep()
    eng.search()
    eng.finalize()
    return eng.trim_coords("3_", "4_")


@pytest.mark.parametrize("parse", ["host", "device"])
def test_on_read_set_of_the_fixture(mixed, its2_hmm, tmp_path, parse):
    recs, pairs = mixed["recs"], mixed["pairs"]
    eng, ref = _engine(join=True, parse=parse), _engine()
    try:
        n, m = eng.merge_pairs_load(mixed["r1"], mixed["r2"])
        if parse == "device":
            assert eng.stats()["n_parse_device"] >= 2                       # both files were parsed on the device
        assert (n, m) == (250, 121) and eng.n_reads == 247 and eng.n_joined == 126
        got_joined, nj = eng.merge_join_info()
        assert nj == 126 and got_joined.tobytes() == mixed["joined"].tobytes()
        assert eng.merge_pair_index().tobytes() == mixed["index"].tobytes()
        assert eng.read_names() == [r[0] for r in recs]
        _load_text(ref, mixed["text"])
        assert ref.n_reads == 247
        for i in range(247):
            assert _packed(eng, i) == _packed(ref, i), i
        n_span = {}
        for rows in ("full", "lazy"):
            a, b = _search(eng, its2_hmm, rows), _search(ref, its2_hmm, rows)
            assert eng.n_unique == ref.n_unique
            assert all(x.tobytes() == y.tobytes() for x, y in zip(eng.get_derep(), ref.get_derep()))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), rows
            start, stop, tlen, _ = a
            L1 = np.array([len(pairs[p][1]) for p in range(250) if mixed["index"][p] >= 0])
            jr = mixed["joined"][mixed["index"] >= 0] == 1
            assert [int(t) for t in tlen[(start >= 0) & (stop >= 0)]] == [len(recs[i][1]) for i in np.flatnonzero((start >= 0) & (stop >= 0))]
            n_span[rows] = int((jr & (start >= 0) & (stop >= 0) & (start < L1) & (stop > L1 + 8)).sum())
            for e, tag in ((eng, "a"), (ref, "b")):
                e.write_uc(str(tmp_path / ("uc_%s_%s" % (rows, tag))))
                e.write_rep_fasta(str(tmp_path / ("rep_%s_%s" % (rows, tag))))
            assert open(tmp_path / ("uc_%s_a" % rows), "rb").read() == open(tmp_path / ("uc_%s_b" % rows), "rb").read()
            assert open(tmp_path / ("rep_%s_a" % rows), "rb").read() == open(tmp_path / ("rep_%s_b" % rows), "rb").read()
        assert n_span["full"] == n_span["lazy"] >= 100, n_span               # guard: the joined reads are trimmed across their pad
        out = str(tmp_path / "seq.fq")
        assert eng.merge_pairs_files(mixed["r1"], mixed["r2"], out) == (250, 121) and eng.n_joined == 126
        assert open(out, "rb").read() == mixed["text"]
        out2 = str(tmp_path / "again.fq")
        assert eng.write_merged_fastq(out2) == 247 and open(out2, "rb").read() == mixed["text"]
    finally:
        eng.close()
        ref.close()


# ------------------------------------------------------------------ 4. the paired output
def _model_trimmed(pairs, names, start, stop, tlen):
    """Dedup.create_paired_trimmed_seqs in Python's own slices of the INPUT records: a pair is cut with the coordinates of the read its
    R1 identifier names (the first of equal labels)"""
    first = {}
    for k, nm in enumerate(names):
        first.setdefault(nm, k)
    coords = []
    for p in pairs:
        k = first.get(JC.label(p[0]))
        coords.append(None if k is None else (int(start[k]), int(stop[k]), int(tlen[k])))
    o1, o2 = J.trimmed_pair_files(pairs, coords)
    return o1.encode(), o2.encode()


@pytest.fixture(scope="module")
def plain_run(mixed, its2_hmm):
    """the plain engine's run on the mixed fixture with the pair records kept: its coordinates and the model's two trimmed files"""
    eng = _engine(join=True)
    eng.keep_pair_records(True)
    eng.merge_pairs_load(mixed["r1"], mixed["r2"])
    eng.keep_pair_records(False)
    start, stop, tlen, _ = _search(eng, its2_hmm, "full")
    names = eng.read_names()
    o1, o2 = _model_trimmed(mixed["pairs"], names, start, stop, tlen)
    written = o1.count(b"\n") // 4
    spanning = sum(1 for p, i in enumerate(mixed["index"]) if i >= 0 and mixed["joined"][p] and 0 <= start[i] < len(mixed["pairs"][p][1])
                   and stop[i] > len(mixed["pairs"][p][1]) + 8)
    assert written > 200 and spanning >= 100
    yield dict(eng=eng, names=names, start=start, stop=stop, tlen=tlen, o1=o1, o2=o2, written=written)
    eng.close()


@pytest.mark.parametrize("gz", [False, True])
def test_paired_output_from_pair_records_and_from_the_host_writer(mixed, plain_run, tmp_path, gz):
    from itsxpress_amd.trim import write_trimmed_paired
    eng = plain_run["eng"]
    sfx = ".gz" if gz else ""
    rd = (lambda p: gzip.decompress(open(p, "rb").read())) if gz else (lambda p: open(p, "rb").read())
    d1, d2 = str(tmp_path / ("dev_R1.fq" + sfx)), str(tmp_path / ("dev_R2.fq" + sfx))
    assert eng.write_trimmed_paired_samples([d1], [d2], region_prefixes=("3_", "4_"), gzipped=gz) == [plain_run["written"]]
    assert (rd(d1), rd(d2)) == (plain_run["o1"], plain_run["o2"])
    h1, h2 = str(tmp_path / ("host_R1.fq" + sfx)), str(tmp_path / ("host_R2.fq" + sfx))
    n = write_trimmed_paired(mixed["r1"], mixed["r2"], h1, h2, plain_run["names"], plain_run["start"], plain_run["stop"], plain_run["tlen"], gzipped=gz)
    assert n == plain_run["written"] and (rd(h1), rd(h2)) == (plain_run["o1"], plain_run["o2"])
    # a joined pair's mates are cut at their own anchors: R1 from `start` to its end, R2 from its start to the 3' anchor
    rec1 = {r.split(b"\n")[0]: r.split(b"\n")[1] for r in plain_run["o1"].split(b"\n@")}
    p = next(p for p, i in enumerate(mixed["index"]) if i >= 0 and mixed["joined"][p] and 0 <= plain_run["start"][i] < plain_run["stop"][i])
    t1, s1 = mixed["pairs"][p][0], mixed["pairs"][p][1]
    assert rec1[t1.encode().lstrip(b"@")] == s1[int(plain_run["start"][mixed["index"][p]]):].encode()


# ------------------------------------------------------------------ 5. a batch of samples, and the mirror
def test_batch_samples_equal_their_solo_runs(mixed, its2_hmm, tmp_path):
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    pairs = mixed["pairs"]
    slices = [pairs[:90], pairs[90:91], [], pairs[91:]]       # three slices of the fixture (one of a single pair) and an empty sample
    files = [JC.write_pair_files(s, str(tmp_path / ("s%d_R1.fq" % k)), str(tmp_path / ("s%d_R2.fq" % k))) for k, s in enumerate(slices)]
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    eng = _engine()
    try:
        objs = [SeqSamplePairedNotInterleaved(fastq=a, tempdir=bd, fastq2=b) for a, b in files]
        batch = SampleBatch(objs, engine=eng, subdirs=["s%d" % k for k in range(4)], keep_records="pairs")
        assert batch.merge_join is False
        batch.merge_join = True
        assert eng.merge_join is True
        batch.merge_reads(threads=1)
        batch.deduplicate(threads=1)
        batch._search(hmmfile=its2_hmm, threads=1)
        o1s = [os.path.join(bd, "b%d_R1.fq" % k) for k in range(4)]
        o2s = [os.path.join(bd, "b%d_R2.fq" % k) for k in range(4)]
        ret = [int(x) for x in batch.write_paired_trimmed(o1s, o2s, "ITS2")]
        counts, n_joined = [int(x) for x in batch.counts], [int(x) for x in batch.n_joined]
    finally:
        eng.close()
    total_j = 0
    for k, s in enumerate(slices):
        recs, index, joined, merged = _model_reads(s)
        assert counts[k] == len(recs) and n_joined[k] == int(joined.sum()), k
        total_j += int(joined.sum())
        solo = _engine(join=True)
        try:
            if s:
                solo.merge_pairs_load(*files[k])
                start, stop, tlen, _ = _search(solo, its2_hmm, "full")
                e1, e2 = _model_trimmed(s, solo.read_names(), start, stop, tlen)
            else:
                e1 = e2 = b""
        finally:
            solo.close()
        assert (open(o1s[k], "rb").read(), open(o2s[k], "rb").read()) == (e1, e2), k
        assert ret[k] == e1.count(b"\n") // 4
    assert total_j == 126 and sum(ret) > 200


@pytest.mark.parametrize("arrays", ["0", "1"])
def test_mirror_under_the_environment_switch(mixed, plain_run, its2_hmm, tmp_path, monkeypatch, arrays):
    """SeqSamplePairedNotInterleaved._merge_reads with ITSXPRESS_JOIN_UNMERGED=1, in file mode and in arrays mode: the trimmed pairs
    are the plain engine's; without the switch the joined pairs are gone from them"""
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved, Dedup, ItsPosition
    monkeypatch.setenv("ITSXPRESS_ARRAYS", arrays)
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    got = {}
    for join in ("1", "0"):
        monkeypatch.setenv("ITSXPRESS_JOIN_UNMERGED", join)
        d = tmp_path / ("join" + join)
        s = SeqSamplePairedNotInterleaved(fastq=mixed["r1"], tempdir=str(d), fastq2=mixed["r2"])
        s._merge_reads(threads=1, stagger=False)
        assert os.path.exists(d / "seq.fq") == (arrays == "0")
        if arrays == "0" and join == "1":
            assert open(d / "seq.fq", "rb").read() == mixed["text"]
        s.deduplicate(threads=1)
        s._search(hmmfile=its2_hmm, threads=1)
        pos = ItsPosition(domtable=s.dom_file, region="ITS2")
        dd = Dedup(uc_file=s.uc_file, rep_file=s.rep_file, seq_file=s.seq_file, fastq=s.r1, fastq2=s.fastq2)
        o1, o2 = str(d / "o1.fq"), str(d / "o2.fq")
        dd.create_paired_trimmed_seqs(o1, o2, gzipped=False, zstd_file=False, itspos=pos, wri_file=True)
        got[join] = (open(o1, "rb").read(), open(o2, "rb").read(), s.engine.n_reads)
        s._engine.close()
    assert got["1"][:2] == (plain_run["o1"], plain_run["o2"]) and got["1"][2] == 247
    assert got["0"][2] == 121 and got["0"][0].count(b"\n") // 4 <= 121 < got["1"][0].count(b"\n") // 4


def test_mirror_under_the_sample_attribute(mixed, tmp_path, monkeypatch):
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    monkeypatch.delenv("ITSXPRESS_JOIN_UNMERGED", raising=False)
    s = SeqSamplePairedNotInterleaved(fastq=mixed["r1"], tempdir=str(tmp_path), fastq2=mixed["r2"])
    s.join_unmerged = True
    s._merge_reads(threads=1)
    assert open(s.seq_file, "rb").read() == mixed["text"]
    s._engine.close()
