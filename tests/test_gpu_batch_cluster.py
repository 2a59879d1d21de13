"""GPU tests for itsx_cluster_samples / SampleBatch.cluster_per_sample: greedy clustering (cluster_id < 1) of every sample of a
batch in one engine call.  Bar: every sample's order, cluster map, strands and identities (exact doubles) equal those of the
sample clustered alone -- by the CPU oracle (orc.cluster, run per sample) and by the engine's own single-sample path -- for
every window size and tuning switch; files written per sample are byte-identical to the single-sample files.
"""
import os

import numpy as np
import pytest

import orc
import synth
from test_gpu_batch import _rc
from test_gpu_cluster import _low_complexity_reads, _noisy_library
from test_gpu_parity import _its2_subset

pytestmark = pytest.mark.gpu


def _solo(engine, reads, names, cid, strand_both=True):
    engine.set_reads(reads, names)
    nu = engine.cluster(cid, strand_both=strand_both)
    rep_of, strand, _ = engine.get_derep()
    pct, order = engine.get_cluster()
    return nu, rep_of.copy(), strand.copy(), pct.copy(), order.copy()


def _batch(engine, samples, cid, strand_both=True):
    reads = [r for s in samples for r in s[0]]
    names = [n for s in samples for n in s[1]]
    engine.set_reads(reads, names)
    engine.set_samples(np.repeat(np.arange(len(samples), dtype=np.int32), [len(s[0]) for s in samples]), len(samples))
    nu = engine.cluster_samples(cid, strand_both=strand_both)
    rep_of, strand, _ = engine.get_derep()
    pct, order = engine.get_cluster()
    return nu, rep_of.copy(), strand.copy(), pct.copy(), order.copy()


def _expected(engine, samples, cid, strand_both=True, oracle=True):
    """each sample alone (engine; and the oracle), in batch coordinates: (n_unique, rep_of, strand, pct, order)"""
    nus, reps, strs, pcts, ords = 0, [], [], [], []
    first = 0
    for reads, names in samples:
        nu, rep_of, strand, pct, order = _solo(engine, reads, names, cid, strand_both)
        if oracle and reads:
            codes, off = orc.digitize(reads)
            o = orc.cluster(codes, off, names, cid, strand_both=strand_both)
            assert np.array_equal(order, o["order"]) and np.array_equal(rep_of, o["rep_of"]) and np.array_equal(strand, o["strand"])
            assert np.array_equal(pct.view(np.uint64), o["pct_id"].view(np.uint64)) and nu == o["n_centroids"]
        nus += nu
        reps.append(np.where(rep_of >= 0, rep_of + first, -1))
        strs.append(strand)
        pcts.append(pct)
        ords.append(order + first)
        first += len(reads)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return nus, cat(reps, np.int64), cat(strs, np.int8), cat(pcts, np.float64), cat(ords, np.int64)


def _check(engine, samples, cid, strand_both=True, oracle=True):
    exp = _expected(engine, samples, cid, strand_both, oracle)
    got = _batch(engine, samples, cid, strand_both)
    assert got[0] == exp[0]
    assert engine.stats()["n_unique"] == exp[0]
    assert np.array_equal(got[4], exp[4]), "order"
    assert np.array_equal(got[1], exp[1]), "rep_of"
    assert np.array_equal(got[2], exp[2]), "strand"
    assert np.array_equal(got[3].view(np.uint64), exp[3].view(np.uint64)), "pct_id"
    return got


def _families(n_samples, n_reads, seed):
    return [_noisy_library(seed + k, n_reads, 12, (270, 320)) for k in range(n_samples)]


@pytest.mark.parametrize("cid", [0.97, 0.99, 0.995])
def test_batch_equals_each_sample_alone(engine, cid):
    samples = [_noisy_library(100 + k, n, 10, (260, 320)) for k, n in enumerate([400, 250, 600, 50, 300, 150, 500, 350])]
    _check(engine, samples, cid)


def test_no_leakage_between_samples(engine):
    """sample B holds members of sample A's templates in both orientations, under A's read names; a third sample holds a
    byte-identical copy of A (same window, identical reads: the shared-search hash must keep them apart)"""
    a_reads, a_names = _noisy_library(7, 300, 8, (280, 300), rc_rate=0.0)
    rng = np.random.default_rng(8)
    b_reads = [a_reads[i] if rng.random() < 0.5 else _rc(a_reads[i]) for i in rng.permutation(len(a_reads))[:200]]
    b_reads = [r[: len(r) - int(rng.integers(0, 4))] for r in b_reads]
    b_names = list(a_names[:200])
    samples = [(a_reads, a_names), (b_reads, b_names), (list(a_reads), list(a_names))]
    got = _check(engine, samples, 0.99)
    # the control: the concatenation clustered as ONE sample is a different answer (B's reads would join A's centroids)
    one = _solo(engine, [r for s in samples for r in s[0]], [n for s in samples for n in s[1]], 0.99)
    assert one[0] < got[0] and not np.array_equal(one[1], got[1])
    # the copy of A is clustered as A itself, on its own centroids
    n_a = len(a_reads)
    off = n_a + len(b_reads)
    assert np.array_equal(got[1][off:] - off, got[1][:n_a])


def test_edge_samples(engine):
    base = "ACGTTGCAAGCTTAGGCTAACGGTCAGTCCATGGATCAGGCTTAAGCCGGTATCGATTACGGCAT" * 3
    fam_r, fam_n = _noisy_library(21, 200, 6, (280, 300))
    rng = np.random.default_rng(3)
    long_reads = ["".join(rng.choice(list("ACGT"), 1400))]
    long_reads += [long_reads[0][:700] + "T" + long_reads[0][701:], _rc(long_reads[0]), long_reads[0][5:]]
    samples = [
        ([], []),                                                        # empty
        ([base], ["one"]),                                               # one read
        (["ACGT" * 7, "ACGTA" * 6], ["s1", "s2"]),                        # all shorter than 32: nothing kept
        (fam_r, fam_n),
        ([base, "N" * 40, base[::-1].translate(str.maketrans("ACGT", "TGCA")), "N" * 40], ["b%d" % i for i in range(4)]),   # all-N reads
        (long_reads, ["l%d" % i for i in range(4)]),                      # multipass alignment (1 400 bases)
    ]
    _check(engine, samples, 0.99)
    _check(engine, samples, 0.97, strand_both=False)
    # a batch in which no read is kept
    _check(engine, [(["ACGT" * 5], ["x"]), ([], []), (["ACG" * 10], ["y"])], 0.99)


@pytest.mark.parametrize("window", ["1", "7", "64", "4096"])
def test_windows_and_segments(engine, window, monkeypatch):
    monkeypatch.setenv("ITSX_CL_WINDOW", window)
    big = _noisy_library(31, 600 if window != "1" else 150, 10, (270, 320))
    tiny = [_noisy_library(40 + k, int(n), 4, (270, 300)) for k, n in enumerate([1, 3, 5, 2, 9, 4, 1, 7])]
    _check(engine, tiny[:3] + [big] + tiny[3:], 0.99, oracle=window in ("7", "4096"))


def test_many_tiny_samples_queue_for_room(engine, monkeypatch):
    monkeypatch.setenv("ITSX_CL_WINDOW", "64")
    rng = np.random.default_rng(5)
    samples = [_noisy_library(1000 + k, int(rng.integers(1, 21)), 3, (260, 300)) for k in range(600)]
    _check(engine, samples, 0.99, oracle=False)


@pytest.mark.parametrize("env", [{"ITSX_CL_CCAP": "40"}, {"ITSX_CL_HEAVY": "0"}, {"ITSX_CL_NOPRECHECK": "1"}, {"ITSX_CL_NOSCORE": "1"}])
def test_tuning_switches(engine, env, monkeypatch):
    samples = _families(5, 300, 300)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(engine, samples, 0.99, oracle=False)


def test_dust_masked_low_complexity(engine):
    samples = [_low_complexity_reads(60 + k, n) for k, n in enumerate([300, 200, 250])]
    _check(engine, samples, 0.97)


@pytest.mark.parametrize("winners", [False, True])
def test_files_through_the_mirror(engine, t_hmm_text, mini_hmm_text, tmp_path, winners, monkeypatch):
    """SampleBatch.cluster_per_sample + _search: uc.txt, rep.fa, domtbl.txt per sample byte-identical to SeqSample.cluster +
    _search of that sample alone; trim_coordinates("ITS2") equal to the solo coordinates"""
    from itsxpress_amd import SeqSampleNotPaired
    from itsxpress_amd.batch import SampleBatch
    if winners:
        monkeypatch.setenv("ITSXPRESS_DOMTBL", "winners")
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(mini_hmm_text + _its2_subset(t_hmm_text, 12, 12))
    fqs = []
    for k, n in enumerate([400, 150, 300, 1]):
        blob, offs = synth.make_reads(t_hmm_text, n, seed=70 + k, sub_rate=0.004)
        seqs = synth.to_strings(blob, offs)
        fq = tmp_path / ("sample%d.fq" % k)
        with open(fq, "w") as f:
            for i, s in enumerate(seqs):
                f.write("@q%05d\n%s\n+\n%s\n" % ((i * 7919) % 100000, s, "I" * len(s)))
        fqs.append(str(fq))
    solo, solo_coords = [], []
    for k, fq in enumerate(fqs):
        d = tmp_path / "solo" / str(k)
        os.makedirs(d)
        s = SeqSampleNotPaired(fq, str(d))
        s._engine = engine
        s.cluster(threads=1, cluster_id=0.995)
        s._search(hmmfile=str(hmm), threads=1)
        solo.append({f: open(getattr(s, f), "rb").read() for f in ("uc_file", "rep_file", "dom_file")})
        solo_coords.append([x.copy() for x in s.trim_coordinates("ITS2")])
    os.makedirs(tmp_path / "batch")
    objs = [SeqSampleNotPaired(fq, str(tmp_path / "batch")) for fq in fqs]
    b = SampleBatch(objs, engine=engine)
    b.cluster_per_sample(threads=1, cluster_id=0.995)
    b._search(hmmfile=str(hmm), threads=1)
    per = b.trim_coordinates("ITS2")
    for k, s in enumerate(objs):
        for f in ("uc_file", "rep_file", "dom_file"):
            assert open(getattr(s, f), "rb").read() == solo[k][f], (k, f)
        for g, e in zip(per[k], solo_coords[k]):
            assert np.array_equal(g, e)
    assert sum(x["uc_file"].count(b"\nH\t") for x in solo) > 50 and sum(len(x["dom_file"]) for x in solo) > 5000
    # every sample at once (select_sample(-1)): the samples' rows one after another, clusters numbered on
    engine.select_sample(-1)
    engine.write_uc(str(tmp_path / "all_uc.txt"))
    rows = [r.split("\t") for r in open(tmp_path / "all_uc.txt").read().splitlines()]
    sh = [r[8] for r in rows if r[0] in "SH"]
    assert sh == [r[8] for x in solo for r in (ln.split("\t") for ln in x["uc_file"].decode().splitlines()) if r[0] in "SH"]
    assert [r[1] for r in rows if r[0] == "C"] == [str(c) for c in range(engine.n_unique)]


def test_size_96_samples_of_3000_reads(engine, t_hmm_text):
    from scripts.batch_cluster_bench import cfg4_samples
    samples = cfg4_samples(96, 3000, t_hmm_text)
    _check(engine, samples, 0.995, oracle=False)
