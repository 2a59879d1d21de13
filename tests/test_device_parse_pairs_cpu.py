"""The device parse of the paired merge loaders (csrc/k_fastq.hip: k_fastq_pairs, itsx_parse_pairs_device, the merge loaders under
Engine.parse = "device"): what can be checked without a device.  The per-16-byte routines the kernel runs (csrc/fastq_rec.h: fq_upper16,
fq_qual_ok16) run here on the host through itsx_debug_parse_pairs_host and itsx_debug_pair_pass_host, and once more in a stand-alone
program under AddressSanitizer and UBSan with exact-size buffers.  Truth is the Python model in tests/fastq_pair_cases.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fastq_pair_cases as pc
from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_parse_pairs_device", "itsx_parse_pairs_fetch", "itsx_debug_parse_pairs_host", "itsx_debug_pair_pass_host"]
SENTINEL = 0xA5
OFF_SENTINEL = -0x5A5A
PAD = 64


def host_pairs(t1, t2, cap_records=None, cap_bases=None, cap_titles=None):
    """itsx_debug_parse_pairs_host with buffers of the given room per side (default: the texts' own sizes bound them) plus PAD sentinel
    elements each.  Returns rc, (reason, side, record), (n, sizes[4], flags, max_total) and per side the raw buffers off, toff, seq, qual, titles."""
    big = max(len(t1), len(t2))
    cr = big // 4 + 1 if cap_records is None else cap_records
    cb = big if cap_bases is None else cap_bases
    ct = big if cap_titles is None else cap_titles
    bufs = []
    for _ in range(2):
        bufs.append((np.full(cr + 1 + PAD, OFF_SENTINEL, np.int64), np.full(cr + 1 + PAD, OFF_SENTINEL, np.int64), np.full(cb + PAD, SENTINEL, np.uint8),
                     np.full(cb + PAD, SENTINEL, np.uint8), np.full(ct + PAD, SENTINEL, np.uint8)))
    n, mx, rec, flags, why, side = C.c_int64(-9), C.c_int64(-9), C.c_int64(-9), C.c_int32(-9), C.c_int32(-9), C.c_int32(-9)
    sizes = np.full(4, -9, np.int64)
    rc = _lib.lib().itsx_debug_parse_pairs_host(t1, len(t1), t2, len(t2), *[b.ctypes.data for b in bufs[0]], *[b.ctypes.data for b in bufs[1]], cr, cb, ct,
                                                C.byref(n), sizes.ctypes.data, C.byref(flags), C.byref(mx), C.byref(why), C.byref(side), C.byref(rec))
    return rc, (why.value, side.value, rec.value), (n.value, tuple(sizes.tolist()), flags.value, mx.value), bufs


def untouched(bufs):
    return all((b[0] == OFF_SENTINEL).all() and (b[1] == OFF_SENTINEL).all() and all((x == SENTINEL).all() for x in b[2:]) for b in bufs)


def check_against(model, result, bufs):
    """the buffers hold exactly the model's planes, and nothing was written behind them"""
    n, sizes, flags, mx = result
    assert (n, flags, mx) == (model["n"], model["flags"], model["max_total"])
    assert sizes == (len(model["sides"][0]["seq"]), len(model["sides"][0]["titles"]), len(model["sides"][1]["seq"]), len(model["sides"][1]["titles"]))
    for s, (off, toff, seq, qual, titles) in zip(model["sides"], bufs):
        nb, nt = len(s["seq"]), len(s["titles"])
        assert off[:n + 1].tolist() == s["off"] and toff[:n + 1].tolist() == s["toff"]
        assert (off[n + 1:] == OFF_SENTINEL).all() and (toff[n + 1:] == OFF_SENTINEL).all()
        assert seq[:nb].tobytes() == s["seq"] and (seq[nb:] == SENTINEL).all()
        assert qual[:nb].tobytes() == s["qual"] and (qual[nb:] == SENTINEL).all()
        assert titles[:nt].tobytes() == s["titles"] and (titles[nt:] == SENTINEL).all()


def _ids(cases):
    return [re.sub(r"[^A-Za-z0-9]+", "_", c[0]) for c in cases]


# ------------------------------------------------------------------ ABI
def test_abi_names_the_new_symbols_and_keeps_its_version_and_the_stats_record():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6 and L.itsx_abi_version() == 6          # additive: no new version
    assert re.search(r"int itsx_parse_pairs_device\(itsx_ctx \*ctx, const char \*text1, int64_t nbytes1, const char \*text2, int64_t nbytes2, "
                     r"int64_t \*n_pairs, int32_t \*flags, int64_t \*max_total\);", header)
    assert re.search(r"int itsx_parse_pairs_fetch\(itsx_ctx \*ctx, int32_t side, int32_t plane, int64_t lo, int64_t hi, void \*out\);", header)
    assert re.search(r"int itsx_parse_fetch\(itsx_ctx \*ctx, int32_t plane, int64_t lo, int64_t hi, void \*out\);", header)      # the single-text fetch is as it was
    # itsx_stats: no new field, the size and the last fields where tests/test_device_parse_cpu.py holds them
    f = _lib.STATS_DTYPE_ALL.fields
    assert _lib.STATS_DTYPE_ALL.itemsize == f["n_parse_declined"][1] + 8 == f["ms_parse"][1] + 24 and f["ms_inflate"][1] == 656
    assert _lib.STATS_DTYPE_ALL.names[-4:] == ("ms_parse", "parse_reserved", "n_parse_device", "n_parse_declined")
    assert re.search(r"n_parse_device, n_parse_declined;\s*\} itsx_stats;", header)
    from itsxpress_amd.engine import Engine
    assert callable(Engine.parse_pairs_device) and callable(Engine.parse_pairs_fetch)


def test_the_catalogue_has_what_it_was_asked_to_have():
    names = [c[0] for c in pc.cases()]
    assert len(set(names)) == len(names)
    models = {n: pc.expected(a, b) for n, a, b in pc.cases()}
    assert [models["%d pairs" % n][1]["n"] for n in (0, 1023, 1024, 1025)] == [0, 1023, 1024, 1025] and models["1 pair"][1]["n"] == 1
    texts = {n: (a, b) for n, a, b in pc.cases()}
    for nb in (4095, 4096, 4097):
        assert len(texts["texts of %d bytes" % nb][0]) == len(texts["texts of %d bytes" % nb][1]) == nb
    for nb in (16383, 16384, 16385):
        assert [len(s["seq"]) for s in models["base planes of %d bytes" % nb][1]["sides"]] == [nb, nb]
    assert texts["CRLF in R1 only"][0].count(b"\r\n") == 28 and b"\r" not in texts["CRLF in R1 only"][1]
    assert not texts["no final newline"][0].endswith(b"\n") and not texts["no final newline"][1].endswith(b"\n")
    assert models["a pair of exactly 12000 bases"][1]["max_total"] == 12000 and models["a pair of 12001 bases"][1]["max_total"] == 12001
    longest = max(len(x) for n, a, b in pc.cases() if "1200" not in n for t in (a, b) for x in t.split(b"\n")[1::4])
    assert longest <= 301
    m = models["every byte value in a sequence line of R1"][1]
    every = bytes(b for b in range(256) if b not in (10, 13))
    assert m["flags"] == pc.LOWER1 and m["sides"][0]["seq"][:len(every)] == every.upper() and every.upper() == pc.upper_az(every)
    assert sum(1 for x, y in zip(every, every.upper()) if x != y) == 26
    assert {models[n][1]["flags"] for n in names if n.startswith("quality 32 ") or n.startswith("quality 127 ")} == {pc.QUAL1, pc.QUAL2}
    assert {models[n][1]["flags"] for n in names if n.startswith("quality 33 ") or n.startswith("quality 126 ")} == {0}
    assert {models[n][1]["flags"] for n in names if n.startswith("lower case")} == {pc.LOWER1, pc.LOWER2}
    declined = {(e[1], e[2]) for e in models.values() if e[0] == "declined"}
    assert {d[0] for d in declined} == set(pc.REASON) and ("pairs", -1) in declined and {d[1] for d in declined} == {-1, 0, 1}
    offsets = [(0, 0)]
    for a, b in pc.batch_at_every_offset():
        m = pc.expected(a, b)[1]
        offsets.append((offsets[-1][0] + len(m["sides"][0]["seq"]), offsets[-1][1] + len(m["sides"][1]["seq"])))
    assert {o[0] % 16 for o in offsets[:-1]} == set(range(16)) == {o[1] % 16 for o in offsets[:-1]}


# ------------------------------------------------------------------ the host routine against the model
@pytest.mark.parametrize("k", range(len(pc.accepted())), ids=_ids(pc.accepted()))
def test_every_accepted_pair_equals_the_model(k):
    name, t1, t2 = pc.accepted()[k]
    model = pc.expected(t1, t2)[1]
    rc, bad, result, bufs = host_pairs(t1, t2)
    assert (rc, bad) == (0, (0, -1, -1)), (name, rc, bad)
    check_against(model, result, bufs)
    # exact room is enough (the caps are the larger side's), one element less of any buffer is refused and nothing is written
    n, sizes = result[0], result[1]
    cb, ct = max(sizes[0], sizes[2]), max(sizes[1], sizes[3])
    rc, bad, result2, bufs = host_pairs(t1, t2, n, cb, ct)
    assert rc == 0 and result2 == result
    check_against(model, result2, bufs)
    for short in ((n - 1, cb, ct), (n, cb - 1, ct), (n, cb, ct - 1)):
        if min(short) < 0:
            continue
        rc, bad, result3, bufs = host_pairs(t1, t2, *short)
        assert rc == -1 and bad[0] == 6 and result3[:2] == (n, sizes) and untouched(bufs), (name, short)


@pytest.mark.parametrize("k", range(len(pc.declined())), ids=_ids(pc.declined()))
def test_every_declined_pair_is_declined_with_its_reason(k):
    name, t1, t2 = pc.declined()[k]
    _, why, side = pc.expected(t1, t2)
    rc, bad, result, bufs = host_pairs(t1, t2)
    assert rc == -5 and bad[:2] == (pc.REASON[why][0], side), (name, rc, bad)
    assert result == (0, (0, 0, 0, 0), 0, 0) and untouched(bufs), name


# ------------------------------------------------------------------ the 16-byte routines
def _pass(seq, qual):
    s, q = np.frombuffer(seq, np.uint8).copy(), np.frombuffer(qual, np.uint8).copy()
    flags = C.c_int32(-9)
    assert _lib.lib().itsx_debug_pair_pass_host(s.ctypes.data, q.ctypes.data, len(seq), C.byref(flags)) == 0
    assert q.tobytes() == qual
    return s.tobytes(), flags.value


def test_every_byte_value_at_every_position_of_a_group():
    """a plane of 16 (one whole group: the dword routines) and of 48 + 7 bytes (the last group partial: the byte routines) with one byte
    of every value at every position: only a-z change, to their upper case, and only 33..126 pass as a quality"""
    for total, positions in ((16, range(16)), (55, range(32, 55))):
        for v in range(256):
            for at in positions:
                plane = bytearray(b"A" * total)
                plane[at] = v
                plane = bytes(plane)
                want = pc.upper_az(plane)
                assert want == plane.upper() and (want != plane) == (97 <= v <= 122)
                got, flags = _pass(plane, b"I" * total)
                assert (got, flags) == (want, pc.LOWER1 if want != plane else 0), (v, at)
                got, flags = _pass(b"C" * total, plane)
                assert (got, flags) == (b"C" * total, 0 if 33 <= v <= 126 else pc.QUAL1), (v, at)


def test_the_pass_on_random_planes_and_its_arguments():
    rng = np.random.default_rng(11)
    for total in (0, 1, 15, 16, 17, 31, 32, 33, 1000, 4099):
        seq = bytes(rng.integers(0, 256, total, dtype=np.uint8).tolist())
        qual = bytes(rng.integers(30, 130, total, dtype=np.uint8).tolist())
        got, flags = _pass(seq, qual)
        assert got == pc.upper_az(seq) and flags == (pc.LOWER1 if got != seq else 0) | (0 if pc.qual_ok(qual) else pc.QUAL1), total
    L = _lib.lib()
    f = C.c_int32(0)
    b = np.zeros(8, np.uint8)
    assert L.itsx_debug_pair_pass_host(None, b.ctypes.data, 4, C.byref(f)) == -1 and L.itsx_debug_pair_pass_host(b.ctypes.data, None, 4, C.byref(f)) == -1
    assert L.itsx_debug_pair_pass_host(b.ctypes.data, b.ctypes.data, -1, C.byref(f)) == -1 and L.itsx_debug_pair_pass_host(b.ctypes.data, b.ctypes.data, 4, None) == -1
    assert L.itsx_debug_pair_pass_host(None, None, 0, C.byref(f)) == 0 and f.value == 0


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
    exe = str(tmp_path / "fastq_pairs_asan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", *san, "-I" + os.path.join(ROOT, "itsxpress_amd", "csrc"),
                            os.path.join(ROOT, "tests", "csrc", "fastq_pairs_asan.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    corpus = str(tmp_path / "corpus.bin")
    good, bad = pc.write_corpus_file(corpus)
    run = subprocess.run([exe, corpus], capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "%d good, %d bad, 4096 groups, 0 failed" % (good, bad) in run.stdout
