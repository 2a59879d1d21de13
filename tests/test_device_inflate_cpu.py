"""The device inflate (csrc/k_inflate.hip, itsx_inflate_device, Engine.inflate = "device"): what can be checked without a device.  The
decoder's logic is csrc/inflate_codes.h, the header one lane of the kernel runs per member; here it runs on the host through
itsx_debug_inflate_host, and once more in a stand-alone program under AddressSanitizer and UBSan with exact-size buffers.  Truth is
Python's gzip / zlib on the same bytes (tests/inflate_cases.py)."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import inflate_cases as ic
from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_inflate_device", "itsx_inflate_fetch", "itsx_debug_inflate_host", "itsx_set_device_inflate", "itsx_debug_inflate_candidates",
       "itsx_debug_inflate_where"]
SENTINEL = 0xA5


def host_inflate(gz, cap):
    """(rc, reason, text_len, n_members, the whole output buffer of cap + 64 bytes, handed over full of the sentinel)"""
    out = np.full(cap + 64, SENTINEL, np.uint8)
    tl, nm, why = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    rc = _lib.lib().itsx_debug_inflate_host(gz, len(gz), out.ctypes.data, cap, C.byref(tl), C.byref(nm), C.byref(why))
    return rc, why.value, tl.value, nm.value, out


# ------------------------------------------------------------------ ABI
def test_abi_names_the_new_symbols():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6          # additive: no new version
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert re.search(r"int itsx_inflate_device\(itsx_ctx \*ctx, const char \*gz, int64_t nbytes, int64_t \*text_len, int64_t \*n_members\);", header)
    assert re.search(r"int itsx_inflate_fetch\(itsx_ctx \*ctx, char \*out, int64_t out_cap\);", header)
    assert re.search(r"int itsx_set_device_inflate\(itsx_ctx \*ctx, int on\);", header)
    f = _lib.STATS_DTYPE.fields
    new = ("ms_inflate", "n_inflate_members", "n_inflate_device", "n_inflate_declined")
    old_end = max(f[k][1] + f[k][0].itemsize for k in f if k not in new)
    assert f["ms_inflate"][1] >= old_end                                      # after every existing field: no earlier offset moved
    assert f["ms_deflate"][1] == f["ms_ensemble"][1] + 4
    assert all(f[k][1] >= f["ms_inflate"][1] for k in new)


def test_the_switches_are_registered_and_the_setting_is_a_property():
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "switches.cpp")) as f:
        src = f.read()
    assert re.search(r'\{"ITSX_DEVICE_INFLATE", SW_TUNING, ', src) and re.search(r'\{"ITSX_INFLATE_MEMBER_KB", SW_TUNING, ', src) and re.search(r'\{"ITSX_INFLATE_GRID", SW_TUNING, ', src)
    from itsxpress_amd.engine import Engine
    e = Engine.__new__(Engine)                  # no context: the setting is remembered by the Python layer
    assert e.inflate == "host"
    e.inflate = "device"
    assert e.inflate == "device"
    with pytest.raises(ValueError):
        e.inflate = "gpu"
    assert e.inflate == "device"
    e.inflate = "host"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "file_run.py"), "--inflate", "device", "--stream"], capture_output=True, text=True)
    assert r.returncode == 2 and "--stream" in r.stderr


# ------------------------------------------------------------------ the decoder on the host
def test_every_good_case_equals_gzip():
    for name, gz, text in ic.good():
        assert gzip.decompress(gz) == text, name
        rc, why, tl, nm, out = host_inflate(gz, len(text))
        assert (rc, why, tl, nm) == (0, 0, len(text), ic.n_members(name)), (name, rc, why, tl, nm)
        assert out[:tl].tobytes() == text, name
        assert (out[tl:] == SENTINEL).all(), name


def test_the_whole_corpus_as_one_file():
    gz, text, members = ic.concatenation()
    assert gzip.decompress(gz) == text
    rc, why, tl, nm, out = host_inflate(gz, len(text))
    assert (rc, why, tl, nm) == (0, 0, len(text), members)
    assert out[:tl].tobytes() == text and (out[tl:] == SENTINEL).all()


@pytest.mark.parametrize("k", range(len(ic.bad())), ids=[re.sub(r"[^A-Za-z0-9]+", "_", c[0]) for c in ic.bad()])
def test_every_bad_case_is_refused_with_a_reason(k):
    name, gz, verified, reasons = ic.bad()[k]
    assert ic.zlib_refuses(gz), name                                          # zlib refuses it too
    rc, why, tl, nm, out = host_inflate(gz, len(verified) + (1 << 17))
    print(name, "->", rc, why)
    assert rc == -5 and why in [ic.REASON[r][0] for r in reasons], (name, rc, why, reasons)      # refused, and for what it was built to meet
    assert tl == len(verified) and out[:tl].tobytes() == verified, name       # the members that did verify, and
    assert (out[tl:] == SENTINEL).all(), name                                 # not one byte of the one that did not


def test_nested_gzip_is_declined_not_misdecoded():
    gz, inner = ic.nested()
    rc, why, tl, nm, out = host_inflate(gz, len(inner) + 4096)
    assert rc == -5 and why > 0 and tl == 0 and (out == SENTINEL).all()


# ------------------------------------------------------------------ the member-start test
def _candidates(buf):
    pos = np.full(16, -1, np.int64)
    n = int(_lib.lib().itsx_debug_inflate_candidates(buf, len(buf), pos.ctypes.data, 16))
    return [int(x) for x in pos[:min(n, 16)]]


def test_candidates():
    text = b"ACGT" * 50
    first = ic.member(text, 6, 0)
    for name, h in ic.header_variants():
        m = ic.member(text, 6, 0, hdr=h)
        assert _candidates(first + m + first) == [0, len(first), len(first) + len(m)], name
    assert _candidates(first + ic.BGZF_EOF) == [0, len(first)]
    for name, miss in ic.near_misses():
        assert _candidates(first + miss) == [0], name
        assert _candidates(miss) == [], name
    bt3 = bytearray(first)
    bt3[10] |= 6                                                              # the first block's BTYPE: 3
    assert _candidates(first + bytes(bt3)) == [0]
    gz, _ = ic.nested()
    assert len(_candidates(gz)) == 2                                          # a real header inside a stored block: why that file is declined


# ------------------------------------------------------------------ the same code under the sanitizers
def test_sanitizer_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime: " + (p.stderr.strip().splitlines() or ["the probe did not run"])[-1])
    exe = str(tmp_path / "inflate_asan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", *san, "-I" + os.path.join(ROOT, "itsxpress_amd", "csrc"),
                            os.path.join(ROOT, "tests", "csrc", "inflate_asan.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    corpus = str(tmp_path / "corpus.bin")
    n = ic.write_corpus_file(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "%d good, %d bad, 0 failed" % (n - len(ic.bad()), len(ic.bad())) in run.stdout
