"""The batch's trimmed FASTQ from the records on the device (itsx_keep_records, itsx_write_trimmed_samples): what can be checked
without a GPU -- the ABI declares and exports the two entry points at version 6, the binding and the mirror carry them, and no
existing signature moved."""
import inspect
import os
import re

from itsxpress_amd import _lib
from itsxpress_amd.batch import SampleBatch
from itsxpress_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_exports_the_batch_trim():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert {"itsx_keep_records", "itsx_write_trimmed_samples"} <= declared
    assert re.search(r"int itsx_keep_records\(itsx_ctx \*ctx, int on\);", header)
    proto = re.search(r"int itsx_write_trimmed_samples\(([^;]*)\);", header).group(1)
    types = [" ".join(a.split()[:-1]) + ("*" * a.split()[-1].count("*")) for a in re.sub(r"\s+", " ", proto).split(",")]
    assert types == ["itsx_ctx*", "const char *const*", "int32_t", "int", "int", "const char*", "const char*", "const int32_t*", "const int32_t*",
                     "int64_t*", "int64_t*"]
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header)
    assert {"itsx_keep_records", "itsx_write_trimmed_samples"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert hasattr(L, "itsx_keep_records") and hasattr(L, "itsx_write_trimmed_samples")
    assert L.itsx_abi_version() == _lib.ABI_VERSION == 6
    src = inspect.getsource(_lib.lib)
    assert re.search(r'"itsx_write_trimmed_samples":\s*\(i32,\s*\[vp,\s*vp,\s*i32,\s*i32,\s*i32,\s*cp,\s*cp,\s*vp,\s*vp,\s*vp,\s*vp\]\)', src)


def test_engine_carries_the_two_calls():
    assert list(inspect.signature(Engine.keep_records).parameters)[:2] == ["self", "on"]
    p = inspect.signature(Engine.write_trimmed_samples).parameters
    assert list(p) == ["self", "paths", "region_prefixes", "start", "stop", "gzipped", "zstd_file", "trim_ccs"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, False, False, False]


def test_batch_takes_keep_records_last_and_moves_no_other_signature():
    p = inspect.signature(SampleBatch.__init__).parameters
    assert list(p) == ["self", "samples", "engine", "subdirs", "keep_records"] and p["keep_records"].default is False
    for name in ("write_paired_trimmed", "write_trimmed"):
        assert list(inspect.signature(getattr(SampleBatch, name)).parameters)[-3:] == ["gzipped", "zstd_file", "trim_ccs"]
    assert list(inspect.signature(SampleBatch.write_trimmed).parameters) == ["self", "outfiles", "region", "gzipped", "zstd_file", "trim_ccs"]
    assert list(inspect.signature(SampleBatch.orient_reads).parameters) == ["self", "threads", "write_seq_files"]
    assert list(inspect.signature(SampleBatch.merge_reads).parameters) == ["self", "threads", "stagger", "write_seq_files"]


def test_the_kernel_file_is_built():
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "Makefile")) as f:
        assert "k_trim.o" in f.read()
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "k_api.h")) as f:
        api = f.read()
    assert "launch_trim_plan" in api and "launch_trim_copy" in api
