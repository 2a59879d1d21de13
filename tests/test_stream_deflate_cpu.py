"""The streamed writers' device deflate (itsx_twriter_set_device, StreamEngine.deflate): what can be checked without a GPU -- the
setting's validation, the refusal of zstd and plain output at plan time, the NULL-context argument check, the new symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _stream_engine():
    from itsxpress_amd.stream import StreamEngine
    return StreamEngine(device=0)


def test_deflate_setting_is_validated(monkeypatch):
    monkeypatch.delenv("ITSX_DEVICE_DEFLATE", raising=False)
    se = _stream_engine()
    assert se.deflate == "host"
    for bad in ("gpu", "", None, 3, "Device"):
        with pytest.raises(ValueError):
            se.deflate = bad
    assert se.deflate == "host"
    se.deflate = "device"
    assert se.deflate == "device"
    se.deflate = "host"
    assert se.deflate == "host"
    # nothing set: the environment's switch selects the device; a value that was set stays
    monkeypatch.setenv("ITSX_DEVICE_DEFLATE", "1")
    assert _stream_engine().deflate == "device" and se.deflate == "host"
    monkeypatch.setenv("ITSX_DEVICE_DEFLATE", "0")
    assert _stream_engine().deflate == "host"


def test_device_deflate_goes_with_gzip_output_only(tmp_path, monkeypatch):
    monkeypatch.delenv("ITSX_DEVICE_DEFLATE", raising=False)
    se = _stream_engine()
    se.deflate = "device"
    o1, o2 = str(tmp_path / "a"), str(tmp_path / "b")
    for kw in ({}, {"zstd_file": True}, {"gzipped": True, "zstd_file": True}):
        with pytest.raises(ValueError):
            se.plan_output(o1, "3_", "4_", **kw)
        with pytest.raises(ValueError):
            se.plan_output_paired(o1, o2, "3_", "4_", **kw)
    assert se._plan is None
    se.plan_output(o1, "3_", "4_", gzipped=True)
    assert se._plan["deflate"] == "device" and se._plan["kind"] == 1          # (the plan's kind is still gzip)
    se.plan_output_paired(o1, o2, "3_", "4_", gzipped=True)
    assert se._plan["deflate"] == "device" and se._plan["kind"] == 1
    se.deflate = "host"
    se.plan_output(o1, "3_", "4_", zstd_file=True)
    assert se._plan["deflate"] == "host" and se._plan["kind"] == 2
    # the environment's switch is about gzip output, as in the library: other outputs are planned as ever
    monkeypatch.setenv("ITSX_DEVICE_DEFLATE", "1")
    se2 = _stream_engine()
    se2.plan_output(o1, "3_", "4_")
    assert se2._plan["deflate"] == "host"
    se2.plan_output(o1, "3_", "4_", gzipped=True)
    assert se2._plan["deflate"] == "device"


def test_set_device_refuses_a_null_context(tmp_path):
    from itsxpress_amd import _lib
    L = _lib.lib()
    w = C.c_void_p()
    out = tmp_path / "o.gz"
    assert L.itsx_twriter_open(os.fsencode(str(out)), 1, 0, C.byref(w)) == 0
    assert L.itsx_twriter_set_device(w, None) == -1
    assert b"itsx_twriter_set_device" in L.itsx_trim_last_error()
    assert L.itsx_twriter_set_device(None, None) == -1
    # the writer is as usable as before
    text = b"@a\nACGT\n+\nIIII\n"
    buf = C.create_string_buffer(text, len(text))
    a, b = np.zeros(1, np.int32), np.full(1, 3, np.int32)
    assert L.itsx_twriter_text(w, C.addressof(buf), len(text), 1) == 0
    assert L.itsx_twriter_coords(w, 0, 1, a.ctypes.data, b.ctypes.data, None) == 0
    nw, tot = C.c_int64(), C.c_int64()
    assert L.itsx_twriter_close(w, C.byref(nw), C.byref(tot)) == 0 and (nw.value, tot.value) == (1, 3)
    import gzip
    assert gzip.decompress(out.read_bytes()) == b"@a\nACG\n+\nIII\n"
    # compression 3 is still refused at open: the device path is a setting of a gzip writer
    assert L.itsx_twriter_open(os.fsencode(str(tmp_path / "x")), 3, 0, C.byref(w)) == -1


def test_symbol_is_declared_exported_and_bound():
    from itsxpress_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "itsx_hip.h")).read()
    assert re.search(r"^int itsx_twriter_set_device\(itsx_twriter \*w, itsx_ctx \*ctx\);", hdr, re.M)
    assert "itsx_twriter_set_device" in _lib.EXPORTS
    L = _lib.lib()
    assert L.itsx_twriter_set_device.argtypes == [C.c_void_p, C.c_void_p] and L.itsx_twriter_set_device.restype is C.c_int
    # the forced fallback is a registered test hook
    n = L.itsx_switch_registry(None, 0)
    b = C.create_string_buffer(int(n))
    L.itsx_switch_registry(b, n)
    reg = {line.split("\t")[0]: line.split("\t")[1] for line in b.value.decode().strip().split("\n")}
    assert reg.get("ITSX_TWRITER_HOST_SLICE") == "hook"
