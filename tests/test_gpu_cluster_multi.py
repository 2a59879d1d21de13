"""GPU tests for itsx_cluster_multi / Engine.cluster(helpers=...): greedy clustering (cluster_id < 1) of one sample with the centroid
stream spread over the leader and helper contexts -- all on device 0 here.  Bar: order, cluster map, strands, n_unique and the bit
patterns of the identities equal itsx_cluster's on the same reads (and the CPU oracle's at oracle size), for every helper count,
window size and tuning switch; the files and the search after it are those of one context.
"""
import os

import numpy as np
import pytest

import orc
import synth
from test_gpu_cluster import _low_complexity_reads, _noisy_library
from itsxpress_amd import Engine, EngineError

pytestmark = pytest.mark.gpu

CID = 0.995


@pytest.fixture(scope="module")
def helpers():
    hs = [Engine(0) for _ in range(4)]
    yield hs
    for h in hs:
        h.close()


def _cfg4(hmm_text, n, seed):
    blob, offs = synth.make_reads(hmm_text, n, config=5, left="1_", right="4_", fixed_len=0, len_range=(300, 480), seed=seed)
    reads = synth.to_strings(blob, offs)
    return reads, ["r%09d" % i for i in range(len(reads))]


def _run(engine, reads, names, cid, hs=None, strand_both=True):
    engine.set_reads(reads, names)
    nu = engine.cluster(cid, strand_both=strand_both, helpers=hs)
    rep_of, strand, _ = engine.get_derep()
    pct, order = engine.get_cluster()
    assert engine.stats()["n_unique"] == nu
    return nu, rep_of.copy(), strand.copy(), pct.copy(), order.copy()


def _same(got, exp, what=""):
    assert got[0] == exp[0], ("n_unique", what)
    assert np.array_equal(got[4], exp[4]), ("order", what)
    assert np.array_equal(got[1], exp[1]), ("rep_of", what)
    assert np.array_equal(got[2], exp[2]), ("strand", what)
    assert np.array_equal(got[3].view(np.uint64), exp[3].view(np.uint64)), ("pct_id", what)


def _check(engine, hs, reads, names, cid, counts=(1, 2, 3, 4), strand_both=True, oracle=False):
    exp = _run(engine, reads, names, cid, None, strand_both)
    if oracle and reads:
        codes, off = orc.digitize(reads)
        o = orc.cluster(codes, off, names, cid, strand_both=strand_both)
        _same(exp, (o["n_centroids"], o["rep_of"], o["strand"], o["pct_id"], o["order"]), "oracle")
    for k in counts:
        _same(_run(engine, reads, names, cid, hs[:k], strand_both), exp, "%d helpers" % k)
    return exp


def test_cfg4_shape_every_helper_count(engine, helpers, t_hmm_text):
    reads, names = _cfg4(t_hmm_text, 2500, 505)
    exp = _check(engine, helpers, reads, names, CID, oracle=True)
    assert 0 < exp[0] < len(reads) and (exp[2] < 0).sum() > 20


@pytest.mark.parametrize("cid,strand_both", [(0.97, True), (0.99, True), (0.99, False)])
def test_noisy_library(engine, helpers, cid, strand_both):
    reads, names = _noisy_library(11, 2000, 50, (280, 310))
    exp = _check(engine, helpers, reads, names, cid, counts=(1, 3), strand_both=strand_both)
    assert 50 <= exp[0] < 2000


def test_dust_masked_low_complexity(engine, helpers):
    reads, names = _low_complexity_reads(7, 600)
    _check(engine, helpers, reads, names, 0.97, counts=(2,), oracle=True)


@pytest.mark.parametrize("env", [("ITSX_CL_WINDOW", "64"), ("ITSX_CL_CCAP", "32"), ("ITSX_CL_HEAVY", "0"), ("ITSX_CL_NOSCORE", "1")])
def test_switches(engine, helpers, env, monkeypatch):
    monkeypatch.setenv(*env)
    reads, names = _noisy_library(41, 1200, 30, (200, 260), n_rate=0.01)
    _check(engine, helpers, reads, names, 0.985, counts=(1, 3))


def test_edge_cases(engine, helpers):
    base = "ACGTTGCAAGCTTAGGCTAACGGTCAGTCCATGGATCAGGCTTAAGCCGGTATCGATTACGGCAT" * 3
    # more shards than centroids: two centroids, five shards
    reads = [base] * 6 + [base[::-1]] * 3
    _check(engine, helpers, reads, ["a%d" % i for i in range(len(reads))], 0.99, oracle=True)
    # no read of 32 bases or more
    assert _check(engine, helpers, [base[:20], "ACGT", base[:31]], ["x", "y", "z"], 0.99, counts=(2,))[0] == 0
    # no reads at all
    assert _check(engine, helpers, [], [], 0.99, counts=(2,))[0] == 0
    # every read the same
    assert _check(engine, helpers, [base] * 300, ["s%03d" % i for i in range(300)], 0.99, counts=(4,))[0] == 1


def test_many_windows_at_200k_reads(engine, helpers, t_hmm_text, monkeypatch):
    monkeypatch.setenv("ITSX_CL_WINDOW", "128")               # (thousands of windows, each with its stream, merge and adoption)
    reads, names = _cfg4(t_hmm_text, 200_000, 909)
    exp = _check(engine, helpers, reads, names, CID, counts=(2,))
    assert engine.stats()["cl_windows"] > 1000 and exp[0] > 1000


def test_files_are_byte_identical(engine, helpers, t_hmm_text, tmp_path):
    reads, names = _cfg4(t_hmm_text, 3000, 77)
    out = {}
    for k in (0, 3):
        engine.set_reads(reads, names)
        engine.cluster(CID, helpers=helpers[:k])
        engine.write_uc(str(tmp_path / ("uc%d.txt" % k)))
        engine.write_rep_fasta(str(tmp_path / ("rep%d.fa" % k)))
        out[k] = [open(tmp_path / ("uc%d.txt" % k), "rb").read(), open(tmp_path / ("rep%d.fa" % k), "rb").read()]
    assert out[0] == out[3] and out[0][0].count(b"\nH\t") > 100


def test_helpers_are_reused(engine, helpers, t_hmm_text):
    a = _cfg4(t_hmm_text, 1500, 11)
    b = _noisy_library(12, 1500, 40, (250, 300))
    first = _run(engine, *a, CID, helpers[:2])
    _same(_run(engine, *b, 0.98, helpers[:2]), _run(engine, *b, 0.98), "other reads")
    _same(_run(engine, *a, CID, helpers[:2]), first, "again")
    _same(first, _run(engine, *a, CID), "one context")


def test_search_after_multi_cluster(engine, helpers, mini_hmm_text):
    blob, offs = synth.make_reads(mini_hmm_text, 1500, seed=5, sub_rate=0.004)
    reads = synth.to_strings(blob, offs)
    names = ["q%05d" % ((i * 7919) % 100000) for i in range(len(reads))]
    engine.load_profiles(text=mini_hmm_text)
    got = []
    for hs in (None, helpers[:3]):
        engine.set_reads(reads, names)
        engine.cluster(0.99, helpers=hs)
        engine.search()
        engine.finalize()
        got.append([x.copy() for x in engine.trim_coords("3_", "4_")])
    for g, e in zip(got[1], got[0]):
        assert np.array_equal(g, e)
    assert (got[0][0] >= 0).sum() > 1000


def test_refusals(engine, helpers):
    reads, names = _noisy_library(3, 200, 10, (200, 240))
    engine.set_reads(reads, names)
    for bad in ([engine], [helpers[0], helpers[0]], [helpers[0], engine]):
        with pytest.raises(EngineError) as e:
            engine.cluster(0.99, helpers=bad)
        assert e.value.code == -1
    engine.set_reads(reads, names)
    engine.set_samples(np.repeat(np.arange(2, dtype=np.int32), [100, 100]), 2)
    with pytest.raises(EngineError) as e:
        engine.cluster(0.99, helpers=helpers[:1])
    assert e.value.code == -5
    engine.set_reads(reads, names)                           # (the context is usable again)
    _same(_run(engine, reads, names, 0.99, helpers[:1]), _run(engine, reads, names, 0.99))


def test_seqsample_two_gpus_writes_the_one_gpu_files(t_hmm_text, tmp_path, monkeypatch):
    from itsxpress_amd import SeqSampleNotPaired
    reads, _ = _cfg4(t_hmm_text, 1500, 31)
    fq = tmp_path / "s.fq"
    with open(fq, "w") as f:
        for i, s in enumerate(reads):
            f.write("@q%05d\n%s\n+\n%s\n" % ((i * 7919) % 100000, s, "I" * len(s)))
    files = {}
    for gpus in ("1", "2"):
        monkeypatch.setenv("ITSXPRESS_GPUS", gpus)
        monkeypatch.setenv("ITSXPRESS_GPU_IDS", ",".join(["0"] * int(gpus)))
        d = tmp_path / gpus
        os.makedirs(d)
        s = SeqSampleNotPaired(str(fq), str(d))
        s.cluster(threads=1, cluster_id=CID)
        files[gpus] = [open(s.uc_file, "rb").read(), open(s.rep_file, "rb").read()]
        assert getattr(s.engine, "world", 1) == 1 and s.engine.device == 0
        s.engine.close()
    assert files["1"] == files["2"] and files["1"][0].count(b"\nH\t") > 50
