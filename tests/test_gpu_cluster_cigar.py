"""GPU tests for itsx_align_clusters (csrc/k_cigar.hip): column 8 of the H rows of a clustering's uc.txt.

Every member of every case of the catalogue (tests/cluster_edges.py) is held to the two exact models: its text parses
(tests/cigar_exact.py), consumes both reads, rescores to exactly tests/align_exact.py's (score, matches, counted columns) -- so the
path is optimal and tie-broken on the triple -- and 100.0 * matches / columns is get_cluster()'s pct_id, the same double.  On the
small groups the text itself equals cigar_exact.traceback, which pins the rule that picks one path among the optimal ones.  Then
the plumbing: '=', the byte budget, a batch of samples, the file, the mirror's setting, the call order.  No tolerance, no member
excused.  `pytest -m gpu`."""
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import align_exact
import cigar_exact as X
import cluster_edges as CE

pytestmark = pytest.mark.gpu

EXACT = ("threshold", "ties", "rows5")


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as p:
        yield p


def _contained():
    return [c for c in CE.PAIRS["contained"]() if c.name.startswith(("L2041_", "L20000_"))]


def _cases(group):
    if group == "walks":
        return [CE.WALKS[w]() for w in CE.WALKS]
    return _contained() if group == "contained" else CE.PAIRS[group]()


def _cluster(engine, cases, align=True):
    """the cases as the samples of one cluster_samples call per identity threshold: [(reads, names, rep_of, strand, pct, cigars)]"""
    out = []
    for cid in sorted({c.cid for c in cases}):
        cs = [c for c in cases if c.cid == cid]
        reads = [r for c in cs for r in c.reads]
        names = [n for c in cs for n in c.names]
        engine.set_reads(reads, names)
        engine.set_samples(np.repeat(np.arange(len(cs), dtype=np.int32), [len(c.reads) for c in cs]), len(cs))
        engine.cluster_samples(cid)
        info = engine.align_clusters() if align else None
        rep_of, strand, _ = engine.get_derep()
        pct, _ = engine.get_cluster()
        cig = engine.get_cluster_cigars() if align else None
        if align:
            assert info["n_aligned"] == int(((rep_of >= 0) & (rep_of != np.arange(len(reads)))).sum())
        out.append((reads, names, np.asarray(rep_of), np.asarray(strand), np.asarray(pct), cig))
    return out


def _pairs_of(reads, rep_of, strand):
    """(read, query on its strand, centroid) of every member"""
    return [(r, CE.rc(reads[r]) if strand[r] < 0 else reads[r], reads[rep_of[r]]) for r in range(len(reads)) if rep_of[r] >= 0 and rep_of[r] != r]


def _align(pair):
    return align_exact.align(*pair)


def _traceback(pair):
    return X.traceback(*pair)


def _hold(results, pool, exact):
    members = 0
    for reads, names, rep_of, strand, pct, cig in results:
        pairs = _pairs_of(reads, rep_of, strand)
        members += len(pairs)
        for r in range(len(reads)):
            if rep_of[r] < 0 or rep_of[r] == r:
                assert cig[r] == "", (r, cig[r])
        want = list(pool.map(_align, [(q, t) for _, q, t in pairs], chunksize=2))
        for (r, q, t), w in zip(pairs, want):
            X.parse(cig[r])
            got = X.rescore(q, t, cig[r])                    # (fails unless the path consumes both reads)
            assert got == tuple(w), (r, cig[r][:60], got, w, len(q), len(t))
            ident = 100.0 * got[1] / got[2]
            assert np.float64(ident).view(np.uint64) == pct[r].view(np.uint64), (r, ident, pct[r])
        if exact:
            texts = list(pool.map(_traceback, [(q, t) for _, q, t in pairs], chunksize=2))
            for (r, q, t), w in zip(pairs, texts):
                assert cig[r] == w, (r, cig[r], w)
    return members


@pytest.mark.parametrize("group", ["rows5", "rows8", "rows10", "multipass", "threshold", "ties", "unlike_targets", "contained", "limits", "walks"])
def test_every_member_s_path_is_the_optimum(engine, group, pool):
    """rows5 / rows8 / rows10: the three template variants; multipass and contained: queries of more than 640 rows; limits: a 50 000-base
    centroid; the text itself on the small groups"""
    results = _cluster(engine, _cases(group))
    members = _hold(results, pool, exact=group in EXACT or group == "walks")
    assert members >= {"limits": 2, "unlike_targets": 3, "walks": 8}.get(group, 5)


@pytest.mark.parametrize("rows", ["5", "8", "10"])
def test_rows_per_lane_change_no_text(engine, rows, pool, monkeypatch):
    """the word layout of the direction bits follows the rows per lane (32 bits for 5 and 8, 64 for 10): the same strings"""
    cases = CE.PAIRS["ties"]() + CE.PAIRS["rows10"]()
    base = [r[5] for r in _cluster(engine, cases)]
    monkeypatch.setenv("ITSX_CL_ROWS", rows)
    assert [r[5] for r in _cluster(engine, cases)] == base


def test_equal_reads_are_not_aligned(engine):
    rng = np.random.default_rng(77)
    t = "".join(rng.choice(list("ACGT"), 200))
    t2 = "".join(rng.choice(list("ACGT"), 200))
    amb = t2[:50] + "R" + t2[51:120] + "N" + t2[121:160] + "Y" + t2[161:]
    other = amb[:120] + "K" + amb[121:]                      # the same places, another code at one of them
    reads = [t, t, CE.rc(t), t.lower().replace("t", "u"), amb, CE.rc(amb), amb.lower(), other, CE.rc(other)]
    names = ["a", "b", "c", "d", "e", "f", "g", "h", "i"]
    engine.set_reads(reads, names)
    engine.cluster(0.9)
    engine.align_clusters()
    rep_of, strand, _ = engine.get_derep()
    cig = engine.get_cluster_cigars()
    assert list(rep_of[:4]) == [0, 0, 0, 0] and list(strand[:4]) == [1, 1, -1, 1]
    assert cig[:4] == ["", "=", "=", "="]
    # IUPAC codes: equal when the codes are, on either strand; another code at one place is an alignment of 200 columns
    assert rep_of[5] == rep_of[4] and strand[5] == -1 and cig[5] == "=" and cig[6] == "="
    for r in (7, 8):
        assert rep_of[r] == rep_of[4] and cig[r] == "200M", (r, rep_of[r], cig[r])
    assert rep_of[4] == 4 and cig[4] == "" and all(X.parse(c) for c in cig if c)
    pct, _ = engine.get_cluster()
    assert pct[7] == 100.0 and pct[8] == 100.0                 # N against K is a match: identity 100, and still not '='


def test_the_budget_changes_no_text(engine, monkeypatch):
    """ITSX_CIGAR_MB so low that rows5 (about 200 KB of direction bits a pair beside a 2 041-base read) splits into several batches and every pair on the
    2 041-base read (1 MB and more) exceeds it alone: the same strings as with the default"""
    cases = CE.PAIRS["rows5"]() + [c for c in _contained() if c.name.startswith("L2041_")]
    base = [r[5] for r in _cluster(engine, cases)]
    assert sum(1 for cig in base for c in cig if c not in ("", "=")) >= 10
    monkeypatch.setenv("ITSX_CIGAR_MB", "0.25")
    assert [r[5] for r in _cluster(engine, cases)] == base


def test_a_batch_is_its_samples(engine):
    """cluster_samples on four samples -- no read, one read, and two that share sequences across strands: each sample's texts are
    those of that sample clustered alone"""
    rng = np.random.default_rng(78)
    t = "".join(rng.choice(list("ACGT"), 300))
    u = CE._sub(t, [40, 170])
    v = CE._cut(t, [100], 3)
    samples = [[], [t], [t, u, CE.rc(v), t], [CE.rc(u), v, CE.rc(t), CE.rc(u)]]
    reads = [r for s in samples for r in s]
    names = ["r%d" % k for s in samples for k in range(len(s))]
    engine.set_reads(reads, names)
    engine.set_samples(np.repeat(np.arange(4, dtype=np.int32), [len(s) for s in samples]), 4)
    engine.cluster_samples(0.97)
    engine.align_clusters()
    got = engine.get_cluster_cigars()
    assert sum(1 for c in got if c) == 6 and "=" in got
    first = 0
    for s in samples:
        if s:
            engine.set_reads(s, ["r%d" % k for k in range(len(s))])
            engine.cluster(0.97)
            engine.align_clusters()
            assert engine.get_cluster_cigars() == got[first:first + len(s)]
        first += len(s)


def test_the_file_carries_the_texts(engine, tmp_path):
    from itsxpress_amd import EngineError
    cases = CE.PAIRS["ties"]()
    reads = [r for c in cases for r in c.reads]
    names = ["s%d_%s" % (k, n) for k, c in enumerate(cases) for n in c.names]
    smp = np.repeat(np.arange(len(cases), dtype=np.int32), [len(c.reads) for c in cases])
    engine.set_reads(reads, names)
    engine.set_samples(smp, len(cases))
    engine.cluster_samples(0.9)
    plain, full = str(tmp_path / "plain.uc"), str(tmp_path / "full.uc")
    engine.write_uc(plain)
    engine.align_clusters()
    cig = dict(zip(names, engine.get_cluster_cigars()))
    engine.write_uc(full)
    a, b = open(plain).read().split("\n"), open(full).read().split("\n")
    assert len(a) == len(b)
    hrows = 0
    for x, y in zip(a, b):
        fx, fy = x.split("\t"), y.split("\t")
        if fx[0] == "H":
            assert fx[7] == "*" and fy[7] == cig[fy[8]] != "" and fx[:7] + fx[8:] == fy[:7] + fy[8:], (x, y)
            hrows += 1
        else:
            assert x == y
    assert hrows == sum(1 for c in cig.values() if c) > 20
    # one sample of the batch: its rows, with its texts
    engine.select_sample(3)
    one = str(tmp_path / "one.uc")
    engine.write_uc(one)
    engine.select_sample(-1)
    rows = [ln.split("\t") for ln in open(one).read().split("\n") if ln]
    assert rows and all(f[8].startswith("s3_") for f in rows) and all(f[7] == cig[f[8]] for f in rows if f[0] == "H")
    # a fresh clustering, or a dereplication, drops them
    engine.cluster_samples(0.9)
    with pytest.raises(EngineError) as e:
        engine.get_cluster_cigars()
    assert e.value.code == -1
    again = str(tmp_path / "again.uc")
    engine.write_uc(again)
    assert open(again).read() == open(plain).read()
    engine.align_clusters()
    engine.derep()
    with pytest.raises(EngineError):
        engine.get_cluster_cigars()
    engine.write_uc(again)
    assert all(ln.split("\t")[7] == "*" for ln in open(again).read().split("\n") if ln.startswith("H"))


def test_call_order(engine):
    from itsxpress_amd import EngineError
    case = CE.PAIRS["ties"]()[0]
    engine.set_reads(case.reads, case.names)
    for step in (lambda: None, engine.derep, lambda: engine.cluster(1.0)):
        step()
        for call in (engine.align_clusters, engine.get_cluster_cigars):
            with pytest.raises(EngineError) as e:
                call()
            assert e.value.code == -1                           # ITSX_E_ARG
    engine.cluster(case.cid)
    with pytest.raises(EngineError):
        engine.get_cluster_cigars()
    engine.align_clusters()
    assert len(engine.get_cluster_cigars()) == len(case.reads)
    engine.set_reads(case.reads, case.names)                   # a new read set
    with pytest.raises(EngineError):
        engine.align_clusters()


def _fastq(path, cases):
    with open(path, "w") as f:
        for k, c in enumerate(cases):
            for n, r in zip(c.names, c.reads):
                f.write("@s%03d_%s\n%s\n+\n%s\n" % (k, n, r, "I" * len(r)))


def test_mirror_setting(tmp_path, monkeypatch):
    """SeqSample.cluster with ITSXPRESS_UC_CIGAR 0 / 1 (and the `uc_cigar` attribute): Dedup.parse reads the same matchdict from both
    files; with the setting off the file is byte for byte the one of a run that never heard of it"""
    from itsxpress_amd import Dedup, SeqSampleNotPaired
    cases = [c for c in CE.PAIRS["ties"]() if not set("".join(c.reads)) - set("ACGT")]
    fq = tmp_path / "seq.fq"
    _fastq(fq, cases)
    files = {}
    for tag, env, attr in (("none", None, None), ("off", "0", None), ("on", "1", None), ("attr", "0", True), ("attr_off", "1", False)):
        d = tmp_path / tag
        d.mkdir()
        if env is None:
            monkeypatch.delenv("ITSXPRESS_UC_CIGAR", raising=False)
        else:
            monkeypatch.setenv("ITSXPRESS_UC_CIGAR", env)
        s = SeqSampleNotPaired(str(fq), str(d))
        if attr is not None:
            s.uc_cigar = attr
        try:
            s.cluster(threads=1, cluster_id=0.9)
            files[tag] = (open(s.uc_file).read(), Dedup(s.uc_file, s.rep_file, s.seq_file).matchdict)
        finally:
            s.engine.close()
    assert files["off"][0] == files["none"][0] == files["attr_off"][0]
    assert files["on"][0] == files["attr"][0] != files["none"][0]
    assert files["on"][1] == files["none"][1] and len(files["on"][1]) > 10
    texts = [ln.split("\t")[7] for ln in files["on"][0].split("\n") if ln.startswith("H")]
    assert texts and all(X.parse(c) for c in texts)
    assert all(ln.split("\t")[7] == "*" for ln in files["none"][0].split("\n") if ln.startswith("H"))


def test_batch_mirror_setting(tmp_path, monkeypatch):
    """SampleBatch.cluster_per_sample with the setting: every sample's uc.txt is the one SeqSample.cluster writes for it"""
    from itsxpress_amd import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    groups = [CE.PAIRS["ties"]()[:6], CE.PAIRS["ties"]()[6:12]]
    fqs = []
    for k, g in enumerate(groups):
        fqs.append(str(tmp_path / ("s%d.fq" % k)))
        _fastq(fqs[-1], g)
    monkeypatch.setenv("ITSXPRESS_UC_CIGAR", "1")
    solo = []
    for k, fq in enumerate(fqs):
        d = tmp_path / ("solo%d" % k)
        d.mkdir()
        s = SeqSampleNotPaired(fq, str(d))
        try:
            s.cluster(threads=1, cluster_id=0.9)
            solo.append(open(s.uc_file).read())
        finally:
            s.engine.close()
    d = tmp_path / "batch"
    d.mkdir()
    b = SampleBatch([SeqSampleNotPaired(fq, str(d)) for fq in fqs])
    try:
        b.cluster_per_sample(threads=1, cluster_id=0.9)
        assert [open(s.uc_file).read() for s in b.samples] == solo
    finally:
        b.engine.close()
    assert any(ln.split("\t")[7] not in ("*", "=") for ln in solo[0].split("\n") if ln.startswith("H"))
