"""Host-side checks of the paired sample batch that need no GPU: which samples SampleBatch takes, the mirror of
`_merge_reads`, and that the header and the binding both know the batch merge's entry point."""
import inspect
import os
import re

import pytest

from itsxpress_amd import SeqSample, _lib
from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
from itsxpress_amd.batch import SampleBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoEngine:
    """stands where the engine would: the constructor must not need one"""


def test_batch_takes_unmerged_paired_samples_only():
    s = SeqSamplePairedNotInterleaved("a_R1.fq", "/tmp", "a_R2.fq")
    assert s.seq_file is None
    b = SampleBatch([s], engine=_NoEngine())
    assert b.samples == [s] and b.counts is None and b.n_pairs is None
    r = SeqSamplePairedNotInterleaved("a_R1.fq", "/tmp", "a_R2.fq", reversed_primers=True)
    assert (r.r1, r.fastq2) == ("a_R2.fq", "a_R1.fq")
    SampleBatch([s, r], engine=_NoEngine())
    with pytest.raises(ValueError):
        SampleBatch([], engine=_NoEngine())
    with pytest.raises(ValueError):
        SampleBatch([SeqSample("reads.fq", "/tmp")], engine=_NoEngine())      # neither a seq_file nor a pair
    half = SeqSample("reads.fq", "/tmp")
    half.r1 = "reads.fq"                                                      # one mate is not a pair
    with pytest.raises(ValueError):
        SampleBatch([s, half], engine=_NoEngine())


def test_merge_reads_mirrors_the_sample_method():
    a = inspect.signature(SampleBatch.merge_reads).parameters
    b = inspect.signature(SeqSamplePairedNotInterleaved._merge_reads).parameters
    assert list(a)[:len(b)] == list(b)
    assert "write_seq_files" in a and a["write_seq_files"].default is None
    for name in ("write_paired_trimmed", "write_trimmed"):
        assert list(inspect.signature(getattr(SampleBatch, name)).parameters)[-3:] == ["gzipped", "zstd_file", "trim_ccs"]


def test_header_and_binding_list_the_batch_merge():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert "itsx_merge_pairs_load_files" in declared
    assert "itsx_merge_pairs_load_files" in _lib.EXPORTS
    assert declared == set(_lib.EXPORTS)
    assert "#define ITSX_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6       # an additive entry point: no new version
