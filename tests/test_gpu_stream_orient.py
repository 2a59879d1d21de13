"""StreamEngine.plan_orient: a streamed run (ITSXPRESS_STREAM=1 ITSXPRESS_ARRAYS=1) orients its reads by the profiles chunk by chunk
and its writers slice the reverse reads from their reverse complements.  The reference throughout is the staged mirror
(ITSXPRESS_STREAM=0): orient_reads -> oriented.fq -> deduplicate -> _search -> trimmed file.  Every streamed arm must give the staged
arm's trimmed text, its four coordinate arrays and its strands, all `==`, without writing an oriented.fq.  `pytest -m gpu`."""
import gzip
import importlib
import os

import numpy as np
import pytest

import synth
from orient_profiles_exact import revcomp

pytestmark = pytest.mark.gpu
S = importlib.import_module("itsxpress_amd.SeqSample")

_OPEN = []


def _close_all():
    while _OPEN:
        s = _OPEN.pop()
        if getattr(s, "_engine", None) is not None:
            s._engine.close()


@pytest.fixture(autouse=True)
def _close_engines():
    yield
    _close_all()


def _env(mp, stream, fast):
    mp.setenv("ITSXPRESS_GPUS", "1")
    mp.setenv("ITSXPRESS_STREAM", "1" if stream else "0")
    mp.setenv("ITSXPRESS_ARRAYS", "1" if fast else "0")
    mp.setenv("ITSXPRESS_ORIENT", "profiles")
    mp.setenv("ITSX_STREAM_CHUNK_MB", "1.5")
    mp.setenv("ITSX_PINFLATE_CHUNK_KB", "32")
    mp.setenv("ITSX_WRITE_UNIT_KB", "256")
    mp.delenv("ITSX_DEVICE_DEFLATE", raising=False)
    from itsxpress_amd import trim
    trim.cache_clear()


def _input(path, t_hmm_text):
    """6 000 amplicon reads (a fifth already reverse-complemented copies of earlier ones), every third record flipped; ties, random
    300-mers and flipped reads with N / IUPAC symbols / lower case at their ends in between"""
    blob, offs = synth.make_reads(t_hmm_text, 6000, config=3, seed=902, fixed_len=0, len_range=(300, 520), rc_rate=0.2)
    seqs = synth.to_strings(blob, offs)
    rng = np.random.default_rng(902)
    recs = []
    for i, s in enumerate(seqs):
        if i % 3 == 0:
            s = revcomp(s)
        recs.append(s)
        if i % 600 == 7:
            recs.append(s + revcomp(s))                                                  # a tie: as many profiles on either strand
        if i % 600 == 11:
            recs.append("".join(rng.choice(list("ACGT"), 300)))                          # nothing passes on either strand
        if i % 300 == 13:
            recs.append(revcomp("nNr" + seqs[i][3:-4] + "RYkn"))                         # flipped, symbols and case at both ends
    with gzip.open(path, "wb", compresslevel=6) as f:
        for i, s in enumerate(recs):
            q = (rng.integers(2, 41, len(s)) + 33).astype(np.uint8)
            if i % 5 == 0:
                q[0] = ord("@")
            f.write(b"@read%06d extra words\n" % i + s.encode() + b"\n+\n" + q.tobytes() + b"\n")
    return len(recs)


def _run(fq, d, hmm, mp, stream, fast, orient=True, plan=None, deflate=None, outputs=(("trimmed.fq.gz", True),)):
    """the mirror's call sequence (itsxpress/main.py:534-554, 626-638 with orient_reads in front).  plan: the planned output's name."""
    os.makedirs(d, exist_ok=True)
    _env(mp, stream, fast)
    sobj = S.SeqSampleNotPaired(fastq=fq, tempdir=d)
    _OPEN.append(sobj)
    if deflate is not None:
        sobj.engine.deflate = deflate
    if orient:
        sobj.orient_hmmfile = hmm
        sobj.orient_reads(threads=1)
    if plan is not None:
        sobj.plan_output(os.path.join(d, plan), "ITS2", gzipped=plan.endswith(".gz"))
    sobj.deduplicate(threads=1)
    sobj._search(hmmfile=hmm, threads=1)
    res = {"sobj": sobj, "files": {}}
    if fast:
        its_pos = S.ItsPosition(domtable=sobj.dom_file, region="ITS2")
        dd = S.Dedup(uc_file=sobj.uc_file, rep_file=sobj.rep_file, seq_file=sobj.seq_file, fastq=sobj.r1, fastq2=sobj.fastq2)
        for name, gz in outputs:
            out = os.path.join(d, name)
            dd.create_trimmed_seqs(out, gzipped=gz, zstd_file=False, itspos=its_pos, wri_file=True, tempdir=d)
            res["files"][name] = open(out, "rb").read()
        res["coords"] = [np.asarray(c).copy() for c in sobj.trim_coordinates("ITS2")]
    res["strand"] = None if sobj.orient_strand is None else np.asarray(sobj.orient_strand).copy()
    return res


@pytest.fixture(scope="module")
def staged(tmp_path_factory, t_hmm_text):
    """the input, the profile file and the staged arm (arrays mode), once for the module"""
    from bench import its2_profiles
    tmp = str(tmp_path_factory.mktemp("stream_orient"))
    hmm = os.path.join(tmp, "its2.hmm")
    with open(hmm, "w") as f:
        f.write(its2_profiles(t_hmm_text))
    fq = os.path.join(tmp, "in.fq.gz")
    n = _input(fq, t_hmm_text)
    with pytest.MonkeyPatch.context() as mp:
        r = _run(fq, os.path.join(tmp, "staged"), hmm, mp, False, True, outputs=(("trimmed.fq.gz", True), ("trimmed.fq", False)))
        sobj = r["sobj"]
        assert sobj.seq_file == os.path.join(tmp, "staged", "oriented.fq") and os.path.exists(sobj.seq_file)
        _close_all()
    text = gzip.decompress(r["files"]["trimmed.fq.gz"])
    assert text == r["files"]["trimmed.fq"]
    start, stop = r["coords"][0], r["coords"][1]
    written = (start >= 0) & (stop >= 0) & (start < stop)
    # the preconditions: the test cannot pass on a run that flips nothing, or on reads whose strand does not matter
    assert r["strand"].shape[0] == n == start.shape[0]
    assert int((r["strand"] == -1).sum()) >= 1500 and int((r["strand"] == 0).sum()) >= 1
    assert int((written & (r["strand"] == -1)).sum()) >= 1000
    assert text.count(b"\n") == 4 * int(written.sum())
    return dict(tmp=tmp, hmm=hmm, fq=fq, n=n, text=text, coords=r["coords"], strand=r["strand"], written=int(written.sum()))


def _check(r, staged, d):
    from itsxpress_amd.stream import StreamEngine
    eng = r["sobj"]._engine
    assert isinstance(eng, StreamEngine) and eng.world >= 4, eng.world
    assert not os.path.exists(os.path.join(d, "oriented.fq"))
    assert r["sobj"].seq_file == r["sobj"].fastq == staged["fq"]
    assert np.array_equal(r["strand"], staged["strand"])
    assert all(np.array_equal(x, y) for x, y in zip(r["coords"], staged["coords"]))
    sd, cf, cr = eng.orient_strands()
    assert np.array_equal(sd, staged["strand"]) and cf.shape == cr.shape == sd.shape
    assert np.array_equal(np.sign(cf.astype(np.int64) - cr), sd)


def test_streamed_with_a_planned_output(staged, monkeypatch):
    d = os.path.join(staged["tmp"], "planned")
    r = _run(staged["fq"], d, staged["hmm"], monkeypatch, True, True, plan="trimmed.fq.gz")
    assert r["sobj"]._engine._out is not None and r["sobj"]._engine._out.result is not None
    assert r["sobj"]._engine._out.result[0] == staged["written"]
    _check(r, staged, d)
    assert gzip.decompress(r["files"]["trimmed.fq.gz"]) == staged["text"]
    # the same run without the orientation writes fewer records: the flipped reads matter to this output
    _close_all()
    d0 = os.path.join(staged["tmp"], "unoriented")
    r0 = _run(staged["fq"], d0, staged["hmm"], monkeypatch, True, True, orient=False, plan="trimmed.fq.gz")
    assert r0["strand"] is None
    assert gzip.decompress(r0["files"]["trimmed.fq.gz"]).count(b"\n") < 4 * staged["written"]


def test_streamed_with_a_planned_plain_output(staged, monkeypatch):
    d = os.path.join(staged["tmp"], "planned_plain")
    r = _run(staged["fq"], d, staged["hmm"], monkeypatch, True, True, plan="trimmed.fq", outputs=(("trimmed.fq", False),))
    assert r["sobj"]._engine._out is not None and r["sobj"]._engine._out.result is not None
    _check(r, staged, d)
    assert r["files"]["trimmed.fq"] == staged["text"]


def test_streamed_without_a_planned_output(staged, monkeypatch):
    """Dedup.create_trimmed_seqs hands the strands to write_trimmed_fastq: it never slices the unoriented file as it is"""
    d = os.path.join(staged["tmp"], "unplanned")
    r = _run(staged["fq"], d, staged["hmm"], monkeypatch, True, True, outputs=(("trimmed.fq.gz", True), ("trimmed.fq", False)))
    assert r["sobj"]._engine._out is None
    _check(r, staged, d)
    assert gzip.decompress(r["files"]["trimmed.fq.gz"]) == staged["text"]
    assert r["files"]["trimmed.fq"] == staged["text"]


def test_streamed_with_the_device_writer(staged, monkeypatch):
    d = os.path.join(staged["tmp"], "device")
    r = _run(staged["fq"], d, staged["hmm"], monkeypatch, True, True, plan="trimmed.fq.gz", deflate="device")
    o = r["sobj"]._engine._out
    assert o is not None and o.plan["deflate"] == "device" and o.result is not None and o.dev_eng is None
    assert o.units_device >= 4 and o.units_host == 0 and o.ms_deflate > 0
    _check(r, staged, d)
    assert gzip.decompress(r["files"]["trimmed.fq.gz"]) == staged["text"]


def test_file_mode_under_the_stream_switch(staged, monkeypatch):
    """ITSXPRESS_STREAM=1 without arrays mode: the whole file is oriented on the stream engine's plain context and oriented.fq is
    written as the staged run writes it; uc.txt, rep.fa and domtbl.txt follow"""
    from itsxpress_amd.stream import StreamEngine
    one = os.path.join(staged["tmp"], "file_one")
    two = os.path.join(staged["tmp"], "file_stream")
    r1 = _run(staged["fq"], one, staged["hmm"], monkeypatch, False, False)
    _close_all()
    r2 = _run(staged["fq"], two, staged["hmm"], monkeypatch, True, False)
    assert isinstance(r2["sobj"]._engine, StreamEngine) and r2["sobj"]._engine._orient_plan is None
    assert r2["sobj"].seq_file == os.path.join(two, "oriented.fq")
    assert np.array_equal(r1["strand"], staged["strand"]) and np.array_equal(r2["strand"], staged["strand"])
    for name in ("oriented.fq", "uc.txt", "rep.fa", "domtbl.txt"):
        a, b = open(os.path.join(one, name), "rb").read(), open(os.path.join(two, name), "rb").read()
        assert len(a) > 100 and a == b, name
    assert open(os.path.join(one, "oriented.fq"), "rb").read() == open(os.path.join(staged["tmp"], "staged", "oriented.fq"), "rb").read()


def test_refusals(staged, monkeypatch):
    from itsxpress_amd import EngineError
    from itsxpress_amd.stream import StreamEngine
    d = os.path.join(staged["tmp"], "refusals")
    os.makedirs(d, exist_ok=True)
    _env(monkeypatch, True, True)
    # a search with another profile file than the one the orientation was planned with
    sobj = S.SeqSampleNotPaired(fastq=staged["fq"], tempdir=d)
    _OPEN.append(sobj)
    sobj.orient_hmmfile = staged["hmm"]
    sobj.orient_reads(threads=1)
    sobj.deduplicate(threads=1)
    other = os.path.join(d, "other.hmm")
    with open(other, "w") as f:
        f.write(open(staged["hmm"]).read())
    with pytest.raises(EngineError) as x:
        sobj._search(hmmfile=other, threads=1)
    assert x.value.code == -5 and other in str(x.value) and staged["hmm"] in str(x.value)
    # a paired load after plan_orient, and plan_orient after a paired load
    eng = StreamEngine(0)
    try:
        eng.plan_orient()
        with pytest.raises(EngineError) as x:
            eng.merge_pairs_load(staged["fq"], staged["fq"])
        assert x.value.code == -5 and "plan_orient" in str(x.value)
        with pytest.raises(EngineError) as x:
            eng.orient_strands()
        assert x.value.code == -1
        # the plan without profiles at pipeline time
        eng.load_reads_file(staged["fq"])
        with pytest.raises(EngineError) as x:
            eng.n_reads
        assert x.value.code == -1 and "no profiles" in str(x.value)
    finally:
        eng.close()
    eng = StreamEngine(0)
    try:
        eng.merge_pairs_load(staged["fq"], staged["fq"])
        with pytest.raises(EngineError) as x:
            eng.plan_orient()
        assert x.value.code == -5
    finally:
        eng.close()
