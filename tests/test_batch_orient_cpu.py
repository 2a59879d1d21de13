"""Host-side checks of the batch's read orientation that need no GPU: the header and the binding both know `itsx_orient_apply`
(an additive entry point: the ABI version stays), and `SampleBatch.orient_reads` takes what `SeqSample.orient_reads` takes."""
import inspect
import os
import re

import pytest

from itsxpress_amd import _lib
from itsxpress_amd.SeqSample import SeqSample, SeqSampleNotPaired
from itsxpress_amd.batch import SampleBatch
from itsxpress_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoEngine:
    """stands where the engine would: nothing below may need one"""


def test_header_and_binding_list_orient_apply():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert "itsx_orient_apply" in declared and "itsx_orient_apply" in _lib.EXPORTS
    assert declared == set(_lib.EXPORTS)
    m = re.search(r"int\s+itsx_orient_apply\s*\(([^)]*)\)", header)
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).split(",")]
    assert [p.rsplit("*", 1)[0].strip() for p in params] == ["itsx_ctx", "int8_t", "int32_t", "int32_t", "int64_t"]
    assert "#define ITSX_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6       # an additive entry point: no new version
    # the signature table: five pointers in, an int out
    src = inspect.getsource(_lib.lib)
    assert re.search(r'"itsx_orient_apply":\s*\(i32,\s*\[vp,\s*vp,\s*vp,\s*vp,\s*vp\]\)', src)
    assert callable(getattr(Engine, "orient_apply"))


def test_batch_orient_reads_mirrors_the_sample_method():
    a = inspect.signature(SampleBatch.orient_reads).parameters
    b = inspect.signature(SeqSample.orient_reads).parameters
    assert list(a)[:len(b)] == list(b) and a["threads"].default == 1
    assert list(a) == ["self", "threads", "write_seq_files"] and a["write_seq_files"].default is None


def test_batch_orient_reads_refuses_a_sample_without_fastq(tmp_path):
    good = SeqSampleNotPaired(str(tmp_path / "a.fq"), str(tmp_path))
    bad = SeqSampleNotPaired(str(tmp_path / "b.fq"), str(tmp_path))
    bad.fastq = None                                           # (its seq_file is still set: the batch itself takes it)
    b = SampleBatch([good, bad], engine=_NoEngine())
    with pytest.raises(ValueError, match="fastq"):
        b.orient_reads(threads=1)
    assert good.fastq == str(tmp_path / "a.fq") and good.seq_file == good.fastq      # nothing was touched
