"""The device parse (csrc/k_fastq.hip, itsx_parse_device, Engine.parse = "device"): what can be checked without a device.  The rule a
record is checked by is csrc/fastq_rec.h, the header the kernels run per record; here it runs on the host through
itsx_debug_parse_host, and once more in a stand-alone program under AddressSanitizer and UBSan with exact-size buffers.  Truth is the
Python statement of the engine's host parser in tests/fastq_cases.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fastq_cases as fc
from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_parse_device", "itsx_parse_fetch", "itsx_debug_parse_host", "itsx_set_device_parse"]
SENTINEL = 0xA5
PAD = 64


def host_rule(text, cap_records=None, cap_bases=None, cap_titles=None, keep_qual=True):
    """itsx_debug_parse_host with buffers of the given room (default: the text's own size bounds them) plus PAD sentinel elements each.
    Returns rc, reason, record, (n, nb, nt) and the raw buffers off, toff, seq, qual, titles."""
    cr = len(text) // 4 + 1 if cap_records is None else cap_records
    cb = len(text) if cap_bases is None else cap_bases
    ct = len(text) if cap_titles is None else cap_titles
    off, toff = np.full(cr + 1 + PAD, -0x5A5A, np.int64), np.full(cr + 1 + PAD, -0x5A5A, np.int64)
    seq, qual, titles = (np.full(cb + PAD, SENTINEL, np.uint8), np.full(cb + PAD, SENTINEL, np.uint8), np.full(ct + PAD, SENTINEL, np.uint8))
    n, nb, nt, why, rec = C.c_int64(-9), C.c_int64(-9), C.c_int64(-9), C.c_int32(-9), C.c_int64(-9)
    rc = _lib.lib().itsx_debug_parse_host(text, len(text), off.ctypes.data, toff.ctypes.data, cr, seq.ctypes.data, qual.ctypes.data if keep_qual else None, cb,
                                          titles.ctypes.data, ct, C.byref(n), C.byref(nb), C.byref(nt), C.byref(why), C.byref(rec))
    return rc, why.value, rec.value, (n.value, nb.value, nt.value), (off, toff, seq, qual, titles)


def untouched(bufs):
    off, toff, seq, qual, titles = bufs
    return (off == -0x5A5A).all() and (toff == -0x5A5A).all() and all((b == SENTINEL).all() for b in (seq, qual, titles))


def check_against(recs, sizes, bufs, keep_qual=True):
    """the buffers hold exactly the planes of these records, and nothing was written behind them"""
    eoff, etoff, eseq, equal, etitles = fc.planes(recs)
    off, toff, seq, qual, titles = bufs
    n = len(recs)
    assert sizes == (n, len(eseq), len(etitles))
    assert off[:n + 1].tolist() == eoff and toff[:n + 1].tolist() == etoff
    assert (off[n + 1:] == -0x5A5A).all() and (toff[n + 1:] == -0x5A5A).all()
    assert seq[:len(eseq)].tobytes() == eseq and (seq[len(eseq):] == SENTINEL).all()
    if keep_qual:
        assert qual[:len(eseq)].tobytes() == equal and (qual[len(eseq):] == SENTINEL).all()
    else:
        assert (qual == SENTINEL).all()
    assert titles[:len(etitles)].tobytes() == etitles and (titles[len(etitles):] == SENTINEL).all()


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
    assert re.search(r"int itsx_parse_device\(itsx_ctx \*ctx, const char \*text, int64_t nbytes, int keep_qual, int64_t \*n_records\);", header)
    assert re.search(r"int itsx_parse_fetch\(itsx_ctx \*ctx, int32_t plane, int64_t lo, int64_t hi, void \*out\);", header)
    assert re.search(r"int itsx_set_device_parse\(itsx_ctx \*ctx, int on\);", header)
    f = _lib.STATS_DTYPE_ALL.fields                                             # the whole structure (Engine.stats reads it)
    new = ("ms_parse", "parse_reserved", "n_parse_device", "n_parse_declined")
    assert all(k in f for k in new)
    old_end = max(f[k][1] + f[k][0].itemsize for k in f if k not in new)
    assert f["ms_parse"][1] == old_end                                          # after every older field: no earlier offset moved
    assert all(f[k][1] >= old_end for k in new)
    assert f["n_inflate_declined"][1] + 8 == old_end and f["ms_inflate"][1] == 656          # the last addition is where it was
    assert f["n_parse_device"][1] == old_end + 8 and f["n_parse_declined"][1] == old_end + 16 and _lib.STATS_DTYPE_ALL.itemsize == old_end + 24
    # STATS_DTYPE names the record up to the inflate's fields (an older test holds it to that): the same offsets, the structure's full size
    h = _lib.STATS_DTYPE.fields
    assert set(h) == set(f) - set(new) and all(h[k][1] == f[k][1] and h[k][0] == f[k][0] for k in h)
    assert _lib.STATS_DTYPE.itemsize == _lib.STATS_DTYPE_ALL.itemsize
    assert re.search(r"n_inflate_declined;[^}]*ms_parse;[^}]*n_parse_device, n_parse_declined;\s*\} itsx_stats;", header)      # the header's order too


def test_the_switch_is_registered_and_the_setting_is_a_property():
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "switches.cpp")) as f:
        src = f.read()
    assert re.search(r'\{"ITSX_DEVICE_PARSE", SW_TUNING, ', src)
    from itsxpress_amd.engine import Engine
    from itsxpress_amd.batch import SampleBatch
    e = Engine.__new__(Engine)                  # no context: the setting is remembered by the Python layer
    assert e.parse == "host"
    e.parse = "device"
    assert e.parse == "device"
    with pytest.raises(ValueError):
        e.parse = "gpu"
    assert e.parse == "device"
    e.parse = "host"
    assert isinstance(SampleBatch.parse, property) and isinstance(Engine.parse, property)
    b = SampleBatch.__new__(SampleBatch)
    b.engine = e
    assert b.parse == "host"
    b.parse = "device"
    assert e.parse == "device" and b.parse == "device"
    with pytest.raises(ValueError):
        b.parse = "both"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "file_run.py"), "--parse", "device", "--stream"], capture_output=True, text=True)
    assert r.returncode == 2 and "--stream" in r.stderr


# ------------------------------------------------------------------ the rule on the host
@pytest.mark.parametrize("k", range(len(fc.accepted())), ids=[re.sub(r"[^A-Za-z0-9]+", "_", c[0]) for c in fc.accepted()])
def test_every_accepted_case_equals_the_host_parser(k):
    name, text = fc.accepted()[k]
    recs = fc.host_parse(text)
    assert isinstance(recs, list), name
    for keep_qual in (True, False):
        rc, why, rec, sizes, bufs = host_rule(text, keep_qual=keep_qual)
        assert (rc, why, rec) == (0, 0, -1), (name, rc, why, rec)
        check_against(recs, sizes, bufs, keep_qual)
    # exact room is enough, one element less of any buffer is refused and nothing is written
    n, nb, nt = sizes
    rc, why, rec, sizes2, bufs = host_rule(text, n, nb, nt)
    assert rc == 0 and sizes2 == sizes
    check_against(recs, sizes2, bufs)
    for short in ((n - 1, nb, nt), (n, nb - 1, nt), (n, nb, nt - 1)):
        if min(short) < 0:
            continue
        rc, why, rec, sizes3, bufs = host_rule(text, *short)
        assert rc == -1 and sizes3 == sizes and untouched(bufs), (name, short)


def test_the_accepted_corpus_has_what_it_was_asked_to_have():
    texts = dict(fc.accepted())
    assert texts["0 bytes"] == b"" and fc.host_parse(b"") == []
    assert [len(fc.host_parse(texts["%d records" % n])) for n in (1, 2, 3)] == [1, 2, 3]
    assert not texts["no final newline"].endswith(b"\n") and texts["CRLF"].count(b"\r\n") == 12
    assert texts["a lone CR ends the unterminated last line"].endswith(b"\r") and not texts["a lone CR ends the unterminated last line"].endswith(b"\n\r")
    assert fc.host_parse(texts["a title that is just @"])[0][0] == b"@" and fc.identifiers(fc.host_parse(texts["a title that is just @"]))[0] == b""
    assert fc.identifiers(fc.host_parse(texts["tabs and blanks in titles"])) == [b"a", b"", b""]
    quals = [r[2][:1] for r in fc.host_parse(texts["@ and + open the qualities"])]
    assert b"@" in quals and b"+" in quals
    assert [r[1] for r in fc.host_parse(texts["an empty sequence with an empty quality"])] == [b"", b"AC", b""]


@pytest.mark.parametrize("k", range(len(fc.declined())), ids=[re.sub(r"[^A-Za-z0-9]+", "_", c[0]) for c in fc.declined()])
def test_every_declined_case_is_declined_with_its_reason(k):
    name, text, reason, record, host = fc.declined()[k]
    rc, why, rec, sizes, bufs = host_rule(text)
    print("%s -> rc %d, reason %d, record %d; the host parser: %s" % (name, rc, why, rec, "%d records" % host if isinstance(host, int) else host))
    assert (rc, why, rec) == (-5, fc.REASON[reason][0], record), (name, rc, why, rec)
    assert sizes == (0, 0, 0) and untouched(bufs), name
    assert fc.host_verdict(text) == host, name                                # accepted by the host parser (a record count) or rejected (a word)


def test_the_declined_corpus_has_both_kinds():
    hosts = [c[4] for c in fc.declined()]
    assert sum(isinstance(h, int) for h in hosts) >= 5 and "malformed" in hosts and "fasta" in hosts and "neither" in hosts
    assert {c[2] for c in fc.declined()} == set(fc.REASON)


def test_arguments_of_the_host_routine():
    L = _lib.lib()
    n, nb, nt, why, rec = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
    o = np.zeros(4, np.int64)
    buf = np.zeros(64, np.uint8)
    good = (b"@a\nAC\n+\nII\n", 11, o.ctypes.data, o.ctypes.data, 2, buf.ctypes.data, buf.ctypes.data, 8, buf.ctypes.data, 8)
    tail = (C.byref(n), C.byref(nb), C.byref(nt), C.byref(why), C.byref(rec))
    assert L.itsx_debug_parse_host(*good, *tail) == 0 and n.value == 1
    assert L.itsx_debug_parse_host(None, 11, *good[2:], *tail) == -1
    assert L.itsx_debug_parse_host(good[0], -1, *good[2:], *tail) == -1
    assert L.itsx_debug_parse_host(good[0], 11, None, *good[3:], *tail) == -1
    assert L.itsx_debug_parse_host(*good[:5], None, *good[6:], *tail) == -1
    assert L.itsx_debug_parse_host(*good, *tail[:3], None, tail[4]) == -1
    assert L.itsx_debug_parse_host(None, 0, *good[2:], *tail) == 0 and n.value == 0          # no text is a text of no bytes


# ------------------------------------------------------------------ fuzz: the device rule never accepts what the host parser would not return
FUZZ_TEXTS = 2000


def _fuzz_texts():
    """random line edits of valid texts: per text a base of 1 .. 6 records (LF or CRLF, with or without the final line end) and k edits,
    k = 0 for five texts in nine: nearly every edited text is declined, so the edited share is what keeps the declines below half"""
    rng = np.random.default_rng(20260)
    junk = [b"", b"\r", b"+", b"@", b"@x y", b">f", b"ACGT", b"II", b"+\r", b" ", b"@q\tz", b"IIII\r"]
    for t in range(FUZZ_TEXTS):
        nrec = int(rng.integers(1, 7))
        eol = b"\r\n" if rng.random() < 0.3 else b"\n"
        lines = []
        for k in range(nrec):
            L = int(rng.integers(0, 9))
            lines += [b"@r%d %s" % (k, b"x" * int(rng.integers(0, 3))), bytes(rng.choice(list(b"ACGTN"), L).tolist()), b"+" if rng.random() < 0.7 else b"+r%d" % k,
                      bytes(rng.choice(list(b"@+I5#"), L).tolist())]
        nedit = int(rng.choice([0, 0, 0, 0, 0, 1, 1, 2, 3]))
        for _ in range(nedit):
            op, at = int(rng.integers(0, 5)), int(rng.integers(0, len(lines) + 1))
            if op == 0:
                lines.insert(at, junk[int(rng.integers(0, len(junk)))])
            elif op == 1 and lines:
                del lines[min(at, len(lines) - 1)]
            elif op == 2 and lines:
                lines[min(at, len(lines) - 1)] = junk[int(rng.integers(0, len(junk)))]
            elif op == 3 and lines:
                i = min(at, len(lines) - 1)
                lines[i] = lines[i][:-1] if rng.random() < 0.5 else lines[i] + b"I"
            elif op == 4 and len(lines) > 1:
                i = min(at, len(lines) - 2)
                lines[i], lines[i + 1] = lines[i + 1], lines[i]
        text = eol.join(lines)
        if lines and rng.random() < 0.8:
            text += eol
        yield text


def test_fuzz_against_the_host_parser():
    n_accept = n_decline = n_host_accepts_declined = 0
    for text in _fuzz_texts():
        host = fc.host_parse(text)
        rc, why, rec, sizes, bufs = host_rule(text)
        assert rc in (0, -5), text
        if rc == 0:
            assert isinstance(host, list), ("the device rule accepted what the host parser calls %s" % host, text)
            check_against(host, sizes, bufs)
            n_accept += 1
        else:
            assert why in (1, 2, 3, 4) and untouched(bufs), text
            n_decline += 1
            n_host_accepts_declined += isinstance(host, list)
    print("fuzz: %d texts, %d accepted, %d declined (%d of them texts the host parser accepts)" % (n_accept + n_decline, n_accept, n_decline, n_host_accepts_declined))
    assert n_accept + n_decline == FUZZ_TEXTS <= 2000
    assert 2 * n_decline <= FUZZ_TEXTS                                         # at most half declined,
    assert n_decline >= FUZZ_TEXTS // 5 and n_host_accepts_declined > 0          # and both sides are exercised


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
    exe = str(tmp_path / "fastq_asan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", *san, "-I" + os.path.join(ROOT, "itsxpress_amd", "csrc"),
                            os.path.join(ROOT, "tests", "csrc", "fastq_asan.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    corpus = str(tmp_path / "corpus.bin")
    good, bad = fc.write_corpus_file(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "%d good, %d bad, 0 failed" % (good, bad) in run.stdout
