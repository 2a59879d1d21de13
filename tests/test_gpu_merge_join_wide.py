"""Joining the read pairs that do not overlap, beyond one context: a streamed paired sample (ITSXPRESS_STREAM=1 ITSXPRESS_ARRAYS=1,
the two outputs planned and written by the pipeline) and a sample over two workers on one GPU (ITSXPRESS_GPUS=2).  The setting must
reach every context these engines create; their coordinates and both trimmed files must be the plain engine's, which
tests/test_gpu_merge_join.py holds to the model.  `pytest -m gpu`."""
import importlib
import os

import numpy as np
import pytest

import join_cases as JC
import join_exact as J

pytestmark = pytest.mark.gpu
S = importlib.import_module("itsxpress_amd.SeqSample")
_OPEN = []


@pytest.fixture(autouse=True)
def _close_engines():
    yield
    while _OPEN:
        s = _OPEN.pop()
        if getattr(s, "_engine", None) is not None:
            s._engine.close()


@pytest.fixture(scope="module")
def inputs(t_hmm_text, tmp_path_factory):
    """the fixture with its odd pairs cut to 150 bases a mate (plain files), and the ITS2 profiles"""
    from bench import its2_profiles
    d = tmp_path_factory.mktemp("join_wide")
    hmm = d / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    pairs = JC.odd_cut()
    r1, r2 = JC.write_pair_files(pairs, str(d / "mixed_R1.fastq"), str(d / "mixed_R2.fastq"))
    return dict(dir=str(d), hmm=str(hmm), pairs=pairs, r1=r1, r2=r2)


def _run(inputs, name, mp, stream=False, gpus=1, arrays="1", planned=False):
    d = os.path.join(inputs["dir"], name)
    os.makedirs(d, exist_ok=True)
    mp.setenv("ITSXPRESS_JOIN_UNMERGED", "1")
    mp.setenv("ITSXPRESS_GPUS", str(gpus))
    mp.setenv("ITSXPRESS_GPU_IDS", ",".join(["0"] * gpus))
    mp.setenv("ITSXPRESS_STREAM", "1" if stream else "0")
    mp.setenv("ITSXPRESS_ARRAYS", arrays)
    mp.setenv("ITSX_STREAM_CHUNK_MB", "0.02")                  # the inputs are ~100 KB a side: a handful of chunks
    sobj = S.SeqSamplePairedNotInterleaved(fastq=inputs["r1"], tempdir=d, fastq2=inputs["r2"])
    _OPEN.append(sobj)
    o1, o2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    if planned:
        sobj.plan_output_paired(o1, o2, "ITS2")
    sobj._merge_reads(threads=1)
    sobj.deduplicate(threads=1)
    sobj._search(hmmfile=inputs["hmm"], threads=1)
    pos = S.ItsPosition(domtable=sobj.dom_file, region="ITS2")
    dd = S.Dedup(uc_file=sobj.uc_file, rep_file=sobj.rep_file, seq_file=sobj.seq_file, fastq=sobj.r1, fastq2=sobj.fastq2)
    dd.create_paired_trimmed_seqs(o1, o2, gzipped=False, zstd_file=False, itspos=pos, wri_file=True)
    coords = [np.asarray(c).copy() for c in sobj.trim_coordinates("ITS2")]
    return sobj, open(o1, "rb").read(), open(o2, "rb").read(), coords


@pytest.fixture(scope="module")
def plain(inputs):
    """the plain engine's run (one context, arrays mode), held to the model here once more: both files are Python's own slices of the
    input records with the engine's coordinates"""
    mp = pytest.MonkeyPatch()
    try:
        sobj, o1, o2, coords = _run(inputs, "plain", mp)
        eng = sobj._engine
        assert eng.n_reads == 247 and eng.n_joined == 126
        names = eng.read_names()
        first = {}
        for k, nm in enumerate(names):
            first.setdefault(nm, k)
        cs = []
        for p in inputs["pairs"]:
            k = first.get(JC.label(p[0]))
            cs.append(None if k is None else (int(coords[0][k]), int(coords[1][k]), int(coords[2][k])))
        e1, e2 = J.trimmed_pair_files(inputs["pairs"], cs)
        assert (o1, o2) == (e1.encode(), e2.encode()) and o1.count(b"\n") // 4 > 200
        eng.close()
        sobj._engine = None
        _OPEN.remove(sobj)
        return dict(o1=o1, o2=o2, coords=coords)
    finally:
        mp.undo()


@pytest.mark.parametrize("planned", [True, False])
def test_streamed_paired_sample(inputs, plain, monkeypatch, planned):
    from itsxpress_amd.stream import StreamEngine
    sobj, o1, o2, coords = _run(inputs, "stream%d" % planned, monkeypatch, stream=True, planned=planned)
    eng = sobj._engine
    assert isinstance(eng, StreamEngine) and eng.merge_join is True and eng.world >= 3, eng.world
    assert eng.n_pairs == 250 and eng.n_reads == 247 and eng.n_joined == 126
    assert (o1, o2) == (plain["o1"], plain["o2"])
    assert all(np.array_equal(x, y) for x, y in zip(coords, plain["coords"]))


@pytest.mark.parametrize("arrays", ["1", "0"])
def test_two_workers_on_one_gpu(inputs, plain, monkeypatch, arrays):
    from itsxpress_amd.multi import MultiEngine
    sobj, o1, o2, coords = _run(inputs, "multi" + arrays, monkeypatch, gpus=2, arrays=arrays)
    eng = sobj._engine
    assert isinstance(eng, MultiEngine) and eng.merge_join is True and eng.world == 2
    assert eng.n_reads == 247 and eng.n_joined == 126
    assert (o1, o2) == (plain["o1"], plain["o2"])
    assert all(np.array_equal(x, y) for x, y in zip(coords, plain["coords"]))
