"""Sample sharing in the lazy and compact rows modes (itsx_set_sample_sharing_lazy) without a GPU: the entry in every layer, the
switch, and the two properties -- a setting of its own beside share_samples, which keeps governing the full rows mode.  The engine
is held to the unshared searches and to the plain-text model of the classes in tests/test_gpu_sample_sharing_lazy.py."""
import ctypes as C
import os
import re

import pytest

from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "itsx_set_sample_sharing_lazy"


def test_abi_names_the_new_symbol():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert NEW in declared and NEW in _lib.EXPORTS
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6          # additive: no new version
    assert re.search(r"int itsx_set_sample_sharing_lazy\(itsx_ctx \*ctx, int on\);", header)
    L = _lib.lib()
    assert hasattr(L, NEW)
    fn = getattr(L, NEW)
    assert fn.restype is C.c_int32 or fn.restype is C.c_int
    assert len(fn.argtypes) == 2
    at = header.index("int %s(" % NEW)
    comment = header[header.rindex("/*", 0, at):at]
    assert "q2_itsxpress.py:273-333" in comment                     # the loop of the reference it stands for
    assert "itsx_set_domz" in comment                               # ... and what it leaves as it is: counters exchanged between ranks at S > 1


def test_the_switch_is_a_mode_with_its_row():
    L = _lib.lib()
    n = L.itsx_switch_registry(None, 0)
    b = C.create_string_buffer(int(n))
    L.itsx_switch_registry(b, n)
    reg = {line.split("\t")[0]: line.split("\t")[1] for line in b.value.decode().strip().split("\n")}
    assert reg["ITSX_SHARE_SAMPLES_LAZY"] == "mode" and reg["ITSX_SHARE_SAMPLES"] == "mode"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\| `ITSX_SHARE_SAMPLES_LAZY` \| mode \|", doc)


def test_both_properties_behave_like_share_samples():
    from itsxpress_amd.engine import Engine
    from itsxpress_amd.batch import SampleBatch
    e = Engine.__new__(Engine)                  # no context: the setting is remembered by the Python layer
    assert e.share_samples_lazy is False
    e.share_samples_lazy = True
    assert e.share_samples_lazy is True
    for bad in ("device", 1, 0, None, "on"):
        with pytest.raises(ValueError):
            e.share_samples_lazy = bad
    assert e.share_samples_lazy is True
    e.share_samples_lazy = False
    assert isinstance(SampleBatch.share_samples_lazy, property) and isinstance(Engine.share_samples_lazy, property)
    bt = SampleBatch.__new__(SampleBatch)
    bt.engine = e
    assert bt.share_samples_lazy is False
    bt.share_samples_lazy = True
    assert e.share_samples_lazy is True and bt.share_samples_lazy is True
    with pytest.raises(ValueError):
        bt.share_samples_lazy = "yes"
    e.share_samples_lazy = False

    class _S:
        seq_file, tempdir = "x.fq", "."
    b2 = SampleBatch([_S()], engine=e)
    assert b2.share_samples_lazy is False and e.share_samples_lazy is False      # off by default: making a batch leaves the engine's setting alone
    b2.share_samples_lazy = True
    assert b2.share_samples_lazy is True and e.share_samples_lazy is True
    with pytest.raises(ValueError):
        b2.share_samples_lazy = "device"
    e.share_samples_lazy = False
    import inspect
    assert "share_samples_lazy" not in inspect.signature(SampleBatch.__init__).parameters      # a property, not a constructor keyword


def test_the_two_settings_are_independent():
    from itsxpress_amd.engine import Engine
    from itsxpress_amd.batch import SampleBatch
    e = Engine.__new__(Engine)
    bt = SampleBatch.__new__(SampleBatch)
    bt.engine = e
    for obj in (e, bt):
        assert (obj.share_samples, obj.share_samples_lazy) == (False, False)
        obj.share_samples_lazy = True
        assert (e.share_samples, e.share_samples_lazy) == (False, True)
        obj.share_samples = True
        assert (e.share_samples, e.share_samples_lazy) == (True, True)
        obj.share_samples_lazy = False
        assert (e.share_samples, e.share_samples_lazy) == (True, False)
        obj.share_samples = False
        assert (e.share_samples, e.share_samples_lazy) == (False, False)
