"""Orientation by the profiles, without a GPU: the plain-Python rule (tests/orient_profiles_exact.py) fed from the oracle's pair traces
reproduces the strand separation the feature rests on, and the ABI names the two entry points.  Every comparison is exact."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import orc
import orient_profiles_exact as ope
from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("itsx_orient_profiles", "itsx_orient_profiles_apply")


@pytest.fixture(scope="module")
def mini(mini_hmm_text):
    return orc.HmmSet(text=mini_hmm_text)


@pytest.fixture(scope="module")
def synthetic(mini, mini_hmm_text):
    reads = ope.synthetic_reads(mini_hmm_text)
    distinct = list(dict.fromkeys(reads))
    nf, nr = ope.oracle_counts(mini, distinct)
    return reads, distinct, nf, nr


def _strands(nf, nr):
    return [ope.verdict(int(a), int(b)) for a, b in zip(nf, nr)]


def test_fixture_reads_are_forward_for_every_profile_set(fixture_reads, t_hmm_text):
    hs = orc.HmmSet(text=t_hmm_text)
    assert hs.n == 224
    _, seqs = fixture_reads
    assert len(seqs) == 227
    nf, nr = ope.oracle_counts(hs, seqs)
    assert (nf >= 7).all() and (nr == 0).all()
    assert _strands(nf, nr) == [1] * 227


def test_synthetic_reads_separate_without_a_tie(mini, synthetic):
    assert mini.n == 10
    reads, distinct, nf, nr = synthetic
    assert len(reads) == 2000 and len(distinct) == 1340
    pairs = list(zip(nf.tolist(), nr.tolist()))
    assert pairs.count((6, 0)) == 1259 and pairs.count((0, 6)) == 81 and set(pairs) == {(6, 0), (0, 6)}
    assert 0 not in _strands(nf, nr)


def test_random_reads_and_palindromes_are_undecided(mini, synthetic):
    nf, nr = ope.oracle_counts(mini, ope.random_reads())
    assert len(nf) == 50 and not nf.any() and not nr.any()
    _, distinct, _, _ = synthetic
    ties = ope.tie_reads([s for s in distinct if set(s) <= set("ACGT")])
    nf, nr = ope.oracle_counts(mini, ties)
    assert len(ties) == 20 and list(zip(nf.tolist(), nr.tolist())) == [(6, 6)] * 20
    assert _strands(nf, nr) == [0] * 20


def test_model_composes_reads_from_their_seeds():
    texts = ["AACG", "CGTT", "", "aacg", "GGGA", "AACG"]
    samples = [0, 0, 0, 0, 0, 1]
    rep_of, rs = ope.derep(texts, samples)
    assert rep_of.tolist() == [0, 0, -1, 0, 4, 5] and rs.tolist() == [1, -1, 0, 1, 1, 1]
    nf, nr = np.array([1, 9, 9, 9, 2, 0]), np.array([3, 9, 9, 9, 2, 0])
    m = ope.model(nf, nr, rep_of, rs, texts=texts, quals=["abcd", "efgh", "", "ijkl", "mnop", "qrst"])
    assert m["strand"].tolist() == [-1, 1, 0, -1, 0, 0]
    assert m["count_fwd"].tolist() == [1, 3, 0, 1, 2, 0] and m["count_rev"].tolist() == [3, 1, 0, 3, 2, 0]
    assert m["texts"] == ["CGTT", "CGTT", "", "cgtt", "GGGA", "AACG"] and m["quals"] == ["dcba", "efgh", "", "lkji", "mnop", "qrst"]
    assert ope.revcomp("ACGTURYMKSWHBVDNacgtn") == "nacgtNHBVDWSMKRYAACGT"


def test_catalogue_holds_what_the_gpu_test_needs(mini_hmm_text):
    reads, samples, kinds = ope.catalogue(mini_hmm_text)
    assert len(reads) == len(samples) == len(kinds)
    lens = {len(r) for r in reads}
    assert set(range(300, 316)) <= lens and {0, 1, 15, 16, 17, 33, 20000} <= lens
    text = "".join(reads)
    assert all(c in text for c in ope.IUPAC) and "U" in text and "u" in text and any(c.islower() for c in text)
    assert samples.max() == 1 and kinds.count("zero") == 20 + 50 + 1 + 5


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler builds the oracle: it must be there"
    src = tmp_path / "t.c"
    src.write_text('#include "itsx_hip.h"\nint (*f)(itsx_ctx *, double, int8_t *, int32_t *, int32_t *, float *) = itsx_orient_profiles;\n'
                   'int (*g)(itsx_ctx *, double, int8_t *, int32_t *, int32_t *, float *) = itsx_orient_profiles_apply;\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_abi_names_the_new_symbols_and_keeps_its_version():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 6
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6 and L.itsx_abi_version() == 6
    for name in NEW:
        assert re.search(r"int %s\(itsx_ctx \*ctx, double F1, int8_t \*strand, int32_t \*count_fwd, int32_t \*count_rev, float \*ms_kernels\);" % name, header)


def test_the_mirror_keeps_orient_reads_as_it_is_and_adds_the_profile_route():
    import inspect
    from itsxpress_amd.SeqSample import SeqSample
    from itsxpress_amd.batch import SampleBatch
    assert list(inspect.signature(SeqSample.orient_reads).parameters) == ["self", "threads"]
    assert list(inspect.signature(SampleBatch.orient_reads).parameters) == ["self", "threads", "write_seq_files"]
    assert list(inspect.signature(SeqSample.orient_reads_by_profiles).parameters) == ["self", "hmmfile", "threads"]
    assert list(inspect.signature(SampleBatch.orient_reads_by_profiles).parameters) == ["self", "hmmfile", "threads", "write_seq_files"]
