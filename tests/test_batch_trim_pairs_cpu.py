"""A paired batch's trimmed R1 / R2 FASTQ from the pair records on the device (itsx_keep_pair_records,
itsx_write_trimmed_paired_samples, SampleBatch(keep_records="pairs")): what can be checked without a GPU -- the ABI declares and exports
the two entry points at version 6, the binding and the mirror carry them, and no existing signature moved."""
import inspect
import os
import re

import pytest

from itsxpress_amd import _lib
from itsxpress_amd.batch import SampleBatch
from itsxpress_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _types(proto):
    return [" ".join(a.split()[:-1]) + ("*" * a.split()[-1].count("*")) for a in re.sub(r"\s+", " ", proto).split(",")]


def test_abi_declares_and_exports_the_paired_batch_trim():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert {"itsx_keep_pair_records", "itsx_write_trimmed_paired_samples"} <= declared
    assert re.search(r"int itsx_keep_pair_records\(itsx_ctx \*ctx, int on\);", header)
    proto = re.search(r"int itsx_write_trimmed_paired_samples\(([^;]*)\);", header).group(1)
    assert _types(proto) == ["itsx_ctx*", "const char *const*", "const char *const*", "int32_t", "int", "int", "const char*", "const char*",
                             "const int32_t*", "const int32_t*", "const int32_t*", "int64_t*"]
    # the calls of the single-end batch are what they were
    assert re.search(r"int itsx_keep_records\(itsx_ctx \*ctx, int on\);", header)
    proto = re.search(r"int itsx_write_trimmed_samples\(([^;]*)\);", header).group(1)
    assert _types(proto) == ["itsx_ctx*", "const char *const*", "int32_t", "int", "int", "const char*", "const char*", "const int32_t*",
                             "const int32_t*", "int64_t*", "int64_t*"]
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header)
    assert {"itsx_keep_pair_records", "itsx_write_trimmed_paired_samples"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert hasattr(L, "itsx_keep_pair_records") and hasattr(L, "itsx_write_trimmed_paired_samples")
    assert L.itsx_abi_version() == _lib.ABI_VERSION == 6
    src = inspect.getsource(_lib.lib)
    assert re.search(r'"itsx_keep_pair_records":\s*\(i32,\s*\[vp,\s*i32\]\)', src)
    assert re.search(r'"itsx_write_trimmed_paired_samples":\s*\(i32,\s*\[vp,\s*vp,\s*vp,\s*i32,\s*i32,\s*i32,\s*cp,\s*cp,\s*vp,\s*vp,\s*vp,\s*vp\]\)', src)


def test_the_stats_record_keeps_its_layout():
    """the plan's and the copy's times took the place of two padding words"""
    names = list(_lib.STATS_DTYPE.names)
    assert names[names.index("ms_merge") + 1] == "ms_trim_plan" and names[names.index("ms_pack") + 1] == "ms_trim_copy"
    assert _lib.STATS_DTYPE.fields["ms_trim_plan"][1] == _lib.STATS_DTYPE.fields["ms_merge"][1] + 4
    assert _lib.STATS_DTYPE.fields["ms_trim_copy"][1] == _lib.STATS_DTYPE.fields["ms_pack"][1] + 4
    assert _lib.STATS_DTYPE.fields["cl_certified"][1] == _lib.STATS_DTYPE.fields["ms_merge"][1] + 8


def test_engine_carries_the_two_calls():
    p = inspect.signature(Engine.keep_pair_records).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    p = inspect.signature(Engine.write_trimmed_paired_samples).parameters
    assert list(p) == ["self", "paths1", "paths2", "region_prefixes", "start", "stop", "tlen", "gzipped", "zstd_file", "trim_ccs"]
    assert [p[k].default for k in list(p)[3:]] == [None, None, None, None, False, False, False]


class _StubEngine:
    read_set = 0


class _Sample:
    def __init__(self, d):
        self.r1, self.fastq2, self.seq_file, self.tempdir = "a_R1.fq", "a_R2.fq", None, d


def test_batch_takes_the_pairs_mode_and_moves_no_signature(tmp_path):
    p = inspect.signature(SampleBatch.__init__).parameters
    assert list(p) == ["self", "samples", "engine", "subdirs", "keep_records"] and p["keep_records"].default is False
    assert list(inspect.signature(SampleBatch.write_paired_trimmed).parameters) == ["self", "outfiles1", "outfiles2", "region", "gzipped", "zstd_file",
                                                                                    "trim_ccs"]
    assert list(inspect.signature(SampleBatch.write_trimmed).parameters) == ["self", "outfiles", "region", "gzipped", "zstd_file", "trim_ccs"]
    assert list(inspect.signature(SampleBatch.orient_reads).parameters) == ["self", "threads", "write_seq_files"]
    assert list(inspect.signature(SampleBatch.merge_reads).parameters) == ["self", "threads", "stagger", "write_seq_files"]
    objs = [_Sample(str(tmp_path))]
    b = SampleBatch(objs, engine=_StubEngine(), keep_records="pairs")
    assert b.keep_records is True and b.keep_pair_records is True
    b = SampleBatch(objs, engine=_StubEngine(), keep_records=True)
    assert b.keep_records is True and b.keep_pair_records is False
    b = SampleBatch(objs, engine=_StubEngine())
    assert b.keep_records is False and b.keep_pair_records is False
    with pytest.raises(ValueError):
        SampleBatch(objs, engine=_StubEngine(), keep_records="reads")

