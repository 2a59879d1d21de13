"""itsx_align_domains (csrc/k_float.hip: k_env_align) against the float64 model of tests/oa_exact.py, and the plumbing around it:
alignments() parallel to domains(), the same alignments in every mode of the search, the domtbl.txt columns, invalidation, the
mirror's ITSXPRESS_DOMTBL_ALI.

Per aligned row, with eps = 18 (Ld + M) 2^-24 max(1, oasc) (oa_exact.eps):
  (a) |oasc_gpu - oasc_model| <= eps
  (b) constrained(gpu's coordinates) >= oasc_model - eps: the engine's alignment is an optimal-accuracy alignment
  (c) the coordinates equal the model's wherever the model's margin > 2 eps; at most 10 % of a case's rows may be skipped for (c)."""
import os

import numpy as np
import pytest

import oa_cases as OC

pytestmark = pytest.mark.gpu
REGIONS = ("ITS2", "ITS1")
FIELDS = ("hmm_from", "hmm_to", "ali_from", "ali_to", "oasc", "aligned")


def _search(engine, hmm, seqs, kw, domE, mode="full", samples=None, share=False):
    engine.share_samples = share
    engine.set_rows_mode(mode)
    engine.load_profiles(text=hmm)
    engine.set_reads(seqs)
    if samples is not None:
        engine.set_samples(samples, int(samples.max()) + 1)
    engine.derep()
    engine.search(**kw)
    engine.finalize(domE=domE)
    engine.set_kept_rows(mode != "full")


def _reset(engine):
    engine.share_samples = False
    engine.set_kept_rows(False)
    engine.set_rows_mode(None)


def _table(engine):
    """{(prof, rep, dom_idx): alignment tuple} of the aligned rows; checks that alignments() is parallel to domains()"""
    dom, ali = engine.domains(), engine.alignments()
    assert len(dom) == len(ali)
    assert np.array_equal(ali["aligned"] == 1, dom["dom_reported"] == 1)
    z = ali[ali["aligned"] != 1]
    assert all((z[f] == 0).all() for f in FIELDS)
    return dom, ali, {(int(d["prof"]), int(d["rep"]), int(d["dom_idx"])): tuple(a[f].item() for f in FIELDS) for d, a in zip(dom, ali) if a["aligned"] == 1}


@pytest.mark.parametrize("name", OC.NAMES)
def test_alignments_against_the_float64_model(name, engine, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads):
    hmm, seqs, kw = OC.inputs(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1])
    try:
        _search(engine, hmm, seqs, kw, 1e9)
        r = engine.align_domains()
        dom, ali, tab = _table(engine)
        seed, _ = engine.get_uniques()
    finally:
        _reset(engine)
    n = int((ali["aligned"] == 1).sum())
    assert n > 0 and r["n_aligned"] == n and r["ms_kernels"] > 0.0
    if name.startswith("lanes"):
        assert n == int(name[5:])
    if name == "multidomain":
        assert ((dom["flags"] & 1 != 0) & (ali["aligned"] == 1)).any()          # ensemble envelopes are aligned too
    rows = [(int(d["prof"]), int(seed[d["rep"]]), int(d["ienv"]), int(d["jenv"]), {f: a[f].item() for f in FIELDS})
            for d, a in zip(dom, ali) if a["aligned"] == 1]
    for d, a in zip(dom, ali):
        if a["aligned"] == 1:
            assert d["ienv"] <= a["ali_from"] <= a["ali_to"] <= d["jenv"] and 1 <= a["hmm_from"] <= a["hmm_to"]
            assert 0.0 < a["oasc"] <= (d["jenv"] - d["ienv"] + 1) * (1.0 + 1e-5)
    res = OC.checks(hmm, seqs, rows)
    worst = max(x["dev"] / x["eps"] for x in res)
    skipped = sum(x["skipped"] for x in res)
    print("[%s] aligned=%d largest |oasc - model| = %.3g (%.2f eps) skipped for (c) = %d (%.1f %%) ms_kernels=%.2f" %
          (name, n, max(x["dev"] for x in res), worst, skipped, 100.0 * skipped / n, r["ms_kernels"]))
    fails = [f for x in res for f in x["fails"]]
    assert not fails, "\n".join(fails[:20])
    assert skipped <= OC.SKIP_CAP * n, (skipped, n)


@pytest.fixture(scope="module")
def its_inputs(fixture_reads, mini_hmm_text):
    return mini_hmm_text, list(fixture_reads[1])


@pytest.fixture(scope="module")
def baseline(engine, its_inputs):
    """the full table's alignments of the fixture reads under the reference's settings, and its two domtbl.txt files"""
    hmm, seqs = its_inputs
    try:
        _search(engine, hmm, seqs, {}, 10.0)
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "domtbl.txt")
            engine.write_domtbl(p)
            before = open(p, "rb").read()
            r = engine.align_domains()
            dom, ali, tab = _table(engine)
            engine.write_domtbl(p)
            after = open(p, "rb").read()
    finally:
        _reset(engine)
    assert r["n_aligned"] == len(tab) > 100
    return dict(tab=tab, before=before, after=after, dom=dom, ali=ali)


def test_domtbl_changes_in_five_columns_only(engine, its_inputs, baseline, tmp_path):
    hmm, seqs = its_inputs
    # a run that never heard of the feature: byte for byte the file written before align_domains()
    try:
        _search(engine, hmm, seqs, {}, 10.0)
        p = tmp_path / "plain.txt"
        engine.write_domtbl(str(p))
        assert p.read_bytes() == baseline["before"]
    finally:
        _reset(engine)
    b, a = baseline["before"].decode().split("\n"), baseline["after"].decode().split("\n")
    assert len(a) == len(b) and a[:2] == b[:2]
    dom, ali = baseline["dom"], baseline["ali"]
    rep = [i for i in range(len(dom)) if dom[i]["dom_reported"] == 1]
    data = [(x, y) for x, y in zip(b[2:], a[2:]) if x]
    assert len(data) == len(rep)
    changed = 0
    for (x, y), i in zip(data, rep):
        fx, fy = x.split(), y.split()
        assert len(fx) == len(fy) == 23 and len(x) == len(y)
        keep = [c for c in range(23) if c not in (15, 16, 17, 18, 21)]
        assert [fx[c] for c in keep] == [fy[c] for c in keep]
        d, q = dom[i], ali[i]
        acc = float(q["oasc"]) / (1.0 + abs(int(d["jenv"]) - int(d["ienv"])))
        assert fy[15:19] == [str(q["hmm_from"]), str(q["hmm_to"]), str(q["ali_from"]), str(q["ali_to"])] and fy[21] == "%4.2f" % acc
        assert (fy[19], fy[20]) == (str(d["ienv"]), str(d["jenv"]))
        changed += x != y
    assert changed > 100


def _same_as_baseline(tab, base, subset):
    assert tab
    if not subset:
        assert set(tab) == set(base)
    for k, v in tab.items():
        assert base[k] == v, (k, v, base[k])


def test_same_alignments_with_kept_rows_of_a_lazy_search(engine, its_inputs, baseline):
    hmm, seqs = its_inputs
    try:
        _search(engine, hmm, seqs, {}, 10.0, mode="lazy")
        engine.align_domains()
        _, _, tab = _table(engine)
    finally:
        _reset(engine)
    _same_as_baseline(tab, baseline["tab"], subset=True)
    assert len(tab) > 50


@pytest.mark.parametrize("switch", ["ITSX_CHUNK_UNIQUES=37", "ITSX_ALIGN_SLAB_MB=2"])
def test_same_alignments_over_segments_and_batches(engine, its_inputs, baseline, monkeypatch, switch):
    """several row segments (chunks of 37 uniques); several batches of waves (a slab of 2 MB holds 78 rows: one or two waves)"""
    hmm, seqs = its_inputs
    k, v = switch.split("=")
    monkeypatch.setenv(k, v)
    try:
        _search(engine, hmm, seqs, {}, 10.0)
        engine.align_domains()
        _, _, tab = _table(engine)
    finally:
        _reset(engine)
    _same_as_baseline(tab, baseline["tab"], subset=False)


def test_members_of_shared_samples_get_their_holders_alignment(engine, its_inputs):
    hmm, seqs = its_inputs
    q = len(seqs) // 3
    two = seqs[:2 * q] + seqs[q:3 * q]                          # sample 1 repeats half of sample 0's reads
    smp = np.concatenate([np.zeros(2 * q, np.int32), np.ones(2 * q, np.int32)])
    tabs = {}
    for share in (False, True):
        try:
            _search(engine, hmm, two, {}, 10.0, samples=smp, share=share)
            if share:
                assert engine.sample_sharing_info()["n_uniques_shared"] > 0
            engine.align_domains()
            _, _, tabs[share] = _table(engine)
        finally:
            _reset(engine)
            engine.set_samples(None, 1)
    assert tabs[True] == tabs[False] and len(tabs[True]) > 100


def test_call_order_and_invalidation(engine, its_inputs):
    from itsxpress_amd import EngineError
    hmm, seqs = its_inputs
    try:
        engine.set_rows_mode("full")
        engine.load_profiles(text=hmm)
        engine.set_reads(seqs[:60])
        engine.derep()
        engine.search()
        with pytest.raises(EngineError) as e:
            engine.align_domains()
        assert e.value.code == -1
        engine.finalize()
        with pytest.raises(EngineError) as e:
            engine.alignments()
        assert e.value.code == -1
        engine.align_domains()
        n = int((engine.alignments()["aligned"] == 1).sum())
        assert n > 0
        engine.finalize(domE=1e-3)                 # fewer rows are reported: the old alignments are gone, new ones follow the new rows
        with pytest.raises(EngineError):
            engine.alignments()
        engine.align_domains()
        dom, ali, _ = _table(engine)
        assert 0 < int((ali["aligned"] == 1).sum()) <= n
        engine.set_domz(engine.get_domz())
        with pytest.raises(EngineError):
            engine.alignments()
    finally:
        _reset(engine)


@pytest.mark.parametrize("mode", ["full", "winners"])
def test_mirror_setting(fixture_reads, mini_hmm_text, tmp_path, monkeypatch, mode):
    """SeqSample._search with ITSXPRESS_DOMTBL_ALI=1: the parser's dictionary is the one without the setting, the hmm / ali columns
    are real coordinates"""
    from itsxpress_amd import ItsPosition, SeqSampleNotPaired
    names, seqs = fixture_reads
    fq = tmp_path / "seq.fq"
    with open(fq, "w") as f:
        for n, s in zip(names, seqs):
            f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    hmm = tmp_path / "mini.hmm"
    hmm.write_text(mini_hmm_text)
    if mode == "winners":
        monkeypatch.setenv("ITSXPRESS_DOMTBL", "winners")
    res = {}
    for on in (False, True):
        d = tmp_path / ("ali%d" % on)
        d.mkdir()
        monkeypatch.setenv("ITSXPRESS_DOMTBL_ALI", "1" if on else "0")
        s = SeqSampleNotPaired(str(fq), str(d))
        try:
            s.deduplicate(threads=1)
            s._search(hmmfile=str(hmm), threads=1)
            res[on] = ({r: ItsPosition(s.dom_file, r).ddict for r in REGIONS}, [ln.split() for ln in open(s.dom_file) if not ln.startswith("#")])
        finally:
            s.engine.close()
    assert res[True][0] == res[False][0] and len(res[True][0]["ITS2"]) > 50
    assert len(res[True][1]) == len(res[False][1]) > 50
    real = 0
    for off, on in zip(res[False][1], res[True][1]):
        assert (off[15], off[16], off[17], off[18], off[21]) == ("1", off[5], off[19], off[20], "0.00")
        assert 1 <= int(on[15]) <= int(on[16]) <= int(on[5])
        assert int(on[19]) <= int(on[17]) <= int(on[18]) <= int(on[20])
        assert 0.0 < float(on[21]) <= 1.0
        real += (on[15], on[16], on[17], on[18]) != (off[15], off[16], off[17], off[18])
    assert real > 0
