"""FASTQ text parsed on the device (csrc/k_fastq.hip: itsx_parse_device, Engine.parse = "device").  Truth is the Python statement of the
engine's host parser (tests/fastq_cases.py), which tests/test_device_parse_cpu.py holds the per-record rule to on the host.  In every
test that expects the device to do the work the context's counters are asserted, so nothing passes by quietly taking the host path.
`pytest -m gpu`."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import fastq_cases as fc
import inflate_cases as ic
from test_device_parse_cpu import host_rule
from test_gpu_device_inflate import inputs, _load, _unique_seqs, _counters as _inflate_counters      # noqa: F401  (inputs: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counters(engine):
    s = engine.stats()
    return s["n_parse_device"], s["n_parse_declined"]


def _constants():
    """the index tile (bytes) and the plan tile (records) of csrc/k_fastq.hip, read the way _scan_tile() of test_gpu_device_deflate.py reads k_trim.hip's"""
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "k_fastq.hip")) as f:
        src = f.read()
    g = lambda name: int(re.search(name + r" = (\d+);", src).group(1))
    return g("FI_BLOCK") * 16, g("FP_BLOCK") * g("FP_ITEMS")


def _equals_truth(engine, text, tag, keep_qual=True):
    """Engine.parse_device of an accepted text equals the Python statement's planes"""
    recs = fc.host_parse(text)
    assert isinstance(recs, list), tag
    eoff, etoff, eseq, equal, etitles = fc.planes(recs)
    got = engine.parse_device(text, keep_qual=keep_qual)
    assert got["n"] == len(recs), tag
    assert got["off"].tolist() == eoff and got["toff"].tolist() == etoff, tag
    assert got["seq"] == eseq and got["titles"] == etitles, tag
    assert (got["qual"] == equal) if keep_qual else (got["qual"] is None), tag
    return got


# ------------------------------------------------------------------ 1. the corpus
def test_corpus_on_the_device(engine):
    from itsxpress_amd import EngineError
    dev0, dec0 = _counters(engine)
    for name, text in fc.accepted():
        got = _equals_truth(engine, text, name)
        rc, why, rec, sizes, bufs = host_rule(text)                           # and the host routine says the same
        assert rc == 0 and sizes == (got["n"], len(got["seq"]), len(got["titles"])), name
        assert bufs[0][:got["n"] + 1].tolist() == got["off"].tolist() and bufs[2][:sizes[1]].tobytes() == got["seq"] and bufs[3][:sizes[1]].tobytes() == got["qual"], name
        _equals_truth(engine, text, name, keep_qual=False)
    n_ok = 2 * len(fc.accepted())
    assert _counters(engine) == (dev0 + n_ok, dec0)
    assert engine.stats()["ms_parse"] > 0
    good = fc.accepted()[2][1]
    for k, (name, text, reason, record, _) in enumerate(fc.declined()):
        with pytest.raises(EngineError) as ei:
            engine.parse_device(text)
        assert ei.value.code == -5 and "declined" in ei.value.message and fc.REASON[reason][1] in ei.value.message, (name, ei.value.message)
        assert ("(record %d)" % record in ei.value.message) == (record >= 0), (name, ei.value.message)
        out = np.zeros(4, np.int64)
        for plane in range(5):                                                # nothing is left to hand out,
            assert engine.L.itsx_parse_fetch(engine.h, plane, 0, 1, out.ctypes.data) == -1, name
        _equals_truth(engine, good, name)                                     # and the next good parse succeeds
        assert _counters(engine) == (dev0 + n_ok + k + 1, dec0 + k + 1)


# ------------------------------------------------------------------ 2. the edges of the index and the plan
def _text_with_newline_at(p, eol=b"\n", more=3):
    """a title line whose line end starts at byte p, then its record and `more` records of odd lengths"""
    t = b"@" + b"t" * (p - 1)
    L = 37
    recs = t + eol + b"A" * L + eol + b"+" + eol + b"I" * L + eol
    for k in range(more):
        recs += b"@x%d y" % k + eol + b"ACGTN"[: 1 + k] * (k + 2) + eol + b"+" + eol + b"#5II+"[: 1 + k] * (k + 2) + eol
    return recs


def _text_of_length(total, final_newline=True):
    """records of mixed lengths and a last one whose title pads the text to exactly `total` bytes"""
    body = b"".join(b"@r%d\n%s\n+\n%s\n" % (k, b"ACGTTGCA"[: k % 8 + 1] * 3, b"I5#@+I5#"[: k % 8 + 1] * 3) for k in range(40))
    tail = b"\nGATTACA\n+\nIIIIIII" + (b"\n" if final_newline else b"")
    pad = total - len(body) - len(tail)
    assert pad >= 1
    return body + b"@" + b"p" * (pad - 1) + tail


def test_index_edges(engine):
    tile, T = _constants()
    assert tile == 4096
    dev0, dec0 = _counters(engine)
    n = 0
    for p in (15, 16, 17, 31, 32, 33, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile):
        _equals_truth(engine, _text_with_newline_at(p), "newline at %d" % p)
        n += 1
    for p in (tile - 1, tile, tile + 1, 15, 16):                              # "\r\n": the CR at p, the newline at p + 1 (p = tile - 1 straddles the tiles)
        text = _text_with_newline_at(p, b"\r\n")
        assert text[p:p + 2] == b"\r\n"
        _equals_truth(engine, text, "CRLF at %d" % p)
        n += 1
    for k in (1, 3):
        for d in (-1, 0, 1, 7, -9):
            for final in (True, False):
                text = _text_of_length(tile * k + d, final)
                assert len(text) == tile * k + d
                _equals_truth(engine, text, "length %d x %d %+d" % (tile, k, d), keep_qual=final)
                n += 1
    # more than 256 index tiles (the one-block sums kernel goes round its loop and carries), with T - 1, T and T + 1 records (the plan's tile)
    rng = np.random.default_rng(5)
    for nrec in (T - 1, T, T + 1):
        lens = rng.integers(500, 620, nrec)
        lens[::97] = 0
        text = b"".join(b"@read%d/%d\tx\n%s\n+\n%s\n" % (k, L, bytes(rng.choice(list(b"ACGT"), L).tolist()), bytes(rng.integers(33, 74, L, dtype=np.uint8).tolist()))
                        for k, L in enumerate(lens.tolist()))
        assert len(text) > 256 * tile + 50000
        got = _equals_truth(engine, text, "%d records" % nrec)
        assert got["n"] == nrec
        n += 1
    assert _counters(engine) == (dev0 + n, dec0)


# ------------------------------------------------------------------ 3. positions past 2^31
def test_positions_are_64_bit():
    """one text of just over 2^31 bytes: a block of 64 distinct records of 65 535 bases, repeated"""
    from itsxpress_amd import Engine
    L, B = 65535, 64
    alpha = np.frombuffer(b"ACGTNRYK", np.uint8)
    base = np.arange(L)
    seqs = [alpha[(base + 3 * k) % 8].tobytes() for k in range(B)]
    quals = [((base * (k + 1)) % 41 + 33).astype(np.uint8).tobytes() for k in range(B)]
    titles = [b"@r%02d" % k for k in range(B)]
    block = b"".join(t + b"\n" + s + b"\n+\n" + q + b"\n" for t, s, q in zip(titles, seqs, quals))
    R = len(block) // B
    assert R == 4 + 1 + L + 3 + L + 1
    reps = -(-((1 << 31) + 1) // len(block))
    n = reps * B
    try:
        text = block * reps
    except MemoryError:
        pytest.skip("the host cannot allocate the text of %d bytes" % (len(block) * reps))
    assert (1 << 31) < len(text) < (1 << 31) + len(block) + 1 and 16000 < n < 17000
    e = Engine(0)
    try:
        got_n = C.c_int64(-1)
        e._chk(e.L.itsx_parse_device(e.h, text, len(text), 1, C.byref(got_n)))
        del text
        assert got_n.value == n and _counters(e) == (1, 0)
        assert np.array_equal(e.parse_fetch("off", 0, n + 1), np.arange(n + 1, dtype=np.int64) * L)
        assert np.array_equal(e.parse_fetch("toff", 0, n + 1), np.arange(n + 1, dtype=np.int64) * 4)
        straddler = (1 << 31) // R
        assert straddler * R < (1 << 31) < (straddler + 1) * R
        for r in (0, straddler, n - 1):
            k = r % B
            assert e.parse_fetch("seq", r * L, (r + 1) * L) == seqs[k], r
            assert e.parse_fetch("qual", r * L, (r + 1) * L) == quals[k], r
            assert e.parse_fetch("titles", r * 4, (r + 1) * 4) == titles[k], r
        assert e.parse_fetch("seq", straddler * L - 8, straddler * L + 8) == seqs[(straddler - 1) % B][-8:] + seqs[straddler % B][:8]
    finally:
        e.close()


# ------------------------------------------------------------------ 4. the loaders
@pytest.fixture(scope="module")
def ways(engine, inputs, tmp_path_factory):
    """the four files of tests/test_gpu_device_inflate.py as plain text, python-gzip members, device-deflated members and host-writer files,
    and what a host / host load leaves (the reference of every arm)"""
    from itsxpress_amd.trim import write_trimmed_fastq, cache_clear
    d = str(tmp_path_factory.mktemp("parse_in"))
    texts = [open(p, "rb").read() for p in inputs["files"]]
    out = {"plain": list(inputs["files"]), "python": [], "device": [], "host": []}
    keep = {v: os.environ.pop(v, None) for v in ("ITSX_IO_BLOCK_KB", "ITSX_WRITE_MIN_MB")}
    try:
        for k, t in enumerate(texts):
            cut = [0, len(t) // 3, 2 * len(t) // 3, len(t)]
            for way in ("python", "device", "host"):
                p = os.path.join(d, "%s_%d.fq.gz" % (way, k))
                z = None
                if way == "python":
                    z = b"".join(gzip.compress(t[cut[j]:cut[j + 1]]) for j in range(3))
                elif way == "device":
                    z = engine.deflate_device(t, [0, len(t)])[0]
                elif k == 1 or inputs["sizes"][k] == 0:                       # (the writer rewrites CRLF, and writes nothing of no records: the host's codec directly)
                    z = b"".join(ic.member(t[o:o + 70000], 6, 0) for o in range(0, max(len(t), 1), 70000))
                else:
                    n = inputs["sizes"][k]
                    os.environ["ITSX_IO_BLOCK_KB"], os.environ["ITSX_WRITE_MIN_MB"] = "64", "4096"
                    write_trimmed_fastq(inputs["files"][k], p, np.zeros(n, np.int32), np.full(n, 1 << 30, np.int32), gzipped=True)
                    del os.environ["ITSX_IO_BLOCK_KB"], os.environ["ITSX_WRITE_MIN_MB"]
                if z is not None:
                    with open(p, "wb") as f:
                        f.write(z)
                assert gzip.decompress(open(p, "rb").read()) == t, (way, k)
                out[way].append(p)
    finally:
        for v, x in keep.items():
            os.environ.pop(v, None)
            if x is not None:
                os.environ[v] = x
    cache_clear()
    engine.inflate = engine.parse = "host"
    ref = _load(engine, inputs["files"], inputs, d, "ref")
    assert ref["counts"] == inputs["sizes"]
    return dict(dir=d, files=out, ref=ref)


def _clean_env(monkeypatch):
    for v in ("ITSX_DEVICE_INFLATE", "ITSX_DEVICE_PARSE", "ITSX_INFLATE_MEMBER_KB", "ITSX_INFLATE_GRID", "ITSX_IO_BLOCK_KB", "ITSX_WRITE_MIN_MB", "ITSX_DEVICE_DEFLATE"):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("way", ["plain", "python", "device", "host"])
def test_loaders(engine, inputs, ways, way, monkeypatch):
    """counts, names, unique sequences, derep arrays, the writer's return values and the written bytes (records kept) of every
    inflate x parse arm equal the host / host load's"""
    _clean_env(monkeypatch)
    files, ref, d = ways["files"][way], ways["ref"], ways["dir"]
    try:
        for inflate in ("host", "device"):
            for parse in ("host", "device"):
                engine.inflate, engine.parse = inflate, parse
                p0, i0 = _counters(engine), _inflate_counters(engine)
                got = _load(engine, files, inputs, d, "%s_%s_%s" % (way, inflate, parse))
                for key in ref:
                    assert got[key] == ref[key], (way, inflate, parse, key)
                # 4 files with records kept, then 3 dereplicated: every text went where the arm says, none was declined
                assert _counters(engine) == ((p0[0] + 7, p0[1]) if parse == "device" else p0), (way, inflate, parse)
                took = 7 if inflate == "device" and way != "plain" else 0
                assert _inflate_counters(engine) == (i0[0] + took, i0[1]), (way, inflate, parse)
    finally:
        engine.inflate = engine.parse = "host"


def test_the_switch_alone_and_neither(engine, inputs, ways, monkeypatch):
    _clean_env(monkeypatch)
    engine.inflate = engine.parse = "host"
    p0 = _counters(engine)
    monkeypatch.setenv("ITSX_DEVICE_PARSE", "1")
    got = _load(engine, ways["files"]["python"], inputs, ways["dir"], "switch")
    monkeypatch.delenv("ITSX_DEVICE_PARSE")
    assert _counters(engine) == (p0[0] + 7, p0[1]) and all(got[key] == ways["ref"][key] for key in ways["ref"])
    # with neither the setting nor the switch the counters stay where they are
    p0 = _counters(engine)
    got = _load(engine, ways["files"]["python"], inputs, ways["dir"], "default")
    assert _counters(engine) == p0 and all(got[key] == ways["ref"][key] for key in ways["ref"])


def _names_and_seqs(engine):
    engine.derep()
    return engine.read_names(), _unique_seqs(engine), [a.tolist() for a in engine.get_derep()]


def test_a_declined_file_and_a_malformed_file(engine, inputs, tmp_path, monkeypatch):
    from itsxpress_amd import EngineError
    from itsxpress_amd.trim import cache_clear
    _clean_env(monkeypatch)
    good = open(inputs["files"][0], "rb").read()
    lines = good.split(b"\n")                                                  # (LF line ends, four lines per record)
    blank = tmp_path / "blank.fq"                                              # a blank line between records: the host parser takes it, the device declines it
    blank.write_bytes(b"\n".join(lines[:20]) + b"\n\n" + b"\n".join(lines[20:]))
    assert fc.host_verdict(blank.read_bytes()) == inputs["sizes"][0]
    bad = tmp_path / "bad.fq"                                                  # one quality short: malformed for both
    bad.write_bytes(b"@a\nACGT\n+\nIII\n" + good)
    bad_text = bad.read_bytes()
    batch = [inputs["files"][0], str(blank), inputs["files"][1]]
    try:
        loads = {}
        for parse in ("host", "device"):
            engine.parse = parse
            cache_clear()
            p0 = _counters(engine)
            counts = [int(x) for x in engine.load_reads_files(batch)]
            loads[parse] = (counts, _names_and_seqs(engine))
            # the first file was parsed on the device before the second was declined; then the whole call went the host's way
            assert _counters(engine) == ((p0[0] + 1, p0[1] + 1) if parse == "device" else p0)
        assert loads["host"] == loads["device"] and loads["host"][0] == [inputs["sizes"][0], inputs["sizes"][0], inputs["sizes"][1]]
        errors = {}
        for parse in ("host", "device"):
            engine.parse = parse
            for tag, call in (("file", lambda: engine.load_reads_file(str(bad))), ("files", lambda: engine.load_reads_files([inputs["files"][0], str(bad)])),
                              ("text", lambda: engine.load_reads_text(C.cast(bad_text, C.c_void_p).value, len(bad_text)))):
                cache_clear()
                p0 = _counters(engine)
                with pytest.raises(EngineError) as ei:
                    call()
                errors[parse, tag] = (ei.value.code, ei.value.message)
                assert (_counters(engine)[1] - p0[1]) == (parse == "device"), (parse, tag)
        for tag in ("file", "files", "text"):
            assert errors["host", tag] == errors["device", tag] and errors["host", tag][0] == -3 and "malformed FASTQ record" in errors["host", tag][1], tag
    finally:
        engine.parse = "host"


def test_single_file_and_text_loads_and_the_lazy_bases(engine, inputs, ways, tmp_path, monkeypatch):
    """load_reads_file and load_reads_text under "device": the same names, uniques and rep.fa (whose sequences come back from the
    device only now: the load itself moved offsets and titles)"""
    from itsxpress_amd.trim import cache_clear
    _clean_env(monkeypatch)
    text = open(inputs["files"][1], "rb").read()                                # CRLF line ends
    results = {}
    try:
        for parse in ("host", "device"):
            engine.parse = parse
            for inflate in ("host", "device"):
                engine.inflate = inflate
                for tag, src in (("plain", inputs["files"][1]), ("gz", ways["files"]["device"][1]), ("text", None)):
                    cache_clear()
                    p0, i0 = _counters(engine), _inflate_counters(engine)
                    if src is None:
                        n = engine.load_reads_text(C.cast(text, C.c_void_p).value, len(text))
                    else:
                        n = engine.load_reads_file(src)
                    assert _counters(engine) == ((p0[0] + 1, p0[1]) if parse == "device" else p0), (parse, inflate, tag)
                    assert _inflate_counters(engine) == (i0[0] + (tag == "gz" and inflate == "device"), i0[1]), (parse, inflate, tag)
                    names, seqs, derep = _names_and_seqs(engine)
                    rep = str(tmp_path / "rep.fa")
                    engine.write_rep_fasta(rep)
                    results[parse, inflate, tag] = (n, names, seqs, derep, open(rep, "rb").read())
        want = results["host", "host", "plain"]
        assert want[0] == inputs["sizes"][1] and len(want[4]) > 1000
        for key, got in results.items():
            assert got == want, key
    finally:
        engine.inflate = engine.parse = "host"


# ------------------------------------------------------------------ 5. arguments
def test_arguments():
    from itsxpress_amd import Engine
    e = Engine(0)
    try:
        L = e.L
        text = fc.accepted()[3][1]
        recs = fc.host_parse(text)
        off, toff, seq, qual, titles = fc.planes(recs)
        n = C.c_int64(-1)
        out = np.zeros(len(text) + 8, np.uint8)
        assert _counters(e) == (0, 0) and e.stats()["ms_parse"] == 0              # a fresh context counts nothing
        assert L.itsx_parse_fetch(e.h, 2, 0, 1, out.ctypes.data) == -1            # a fetch before any parse
        assert L.itsx_parse_device(None, text, len(text), 1, C.byref(n)) == -1
        assert L.itsx_parse_device(e.h, None, len(text), 1, C.byref(n)) == -1
        assert L.itsx_parse_device(e.h, text, -1, 1, C.byref(n)) == -1
        assert L.itsx_parse_device(e.h, text, len(text), 1, None) == -1
        assert _counters(e) == (0, 0)
        assert L.itsx_parse_device(e.h, text, len(text), 0, C.byref(n)) == 0 and n.value == len(recs)
        assert L.itsx_parse_fetch(e.h, 3, 0, 1, out.ctypes.data) == -1            # qualities that were not kept
        assert L.itsx_parse_device(e.h, text, len(text), 1, C.byref(n)) == 0 and n.value == len(recs)
        assert L.itsx_parse_fetch(None, 2, 0, 1, out.ctypes.data) == -1
        for plane, size in ((0, len(recs) + 1), (1, len(recs) + 1), (2, len(seq)), (3, len(seq)), (4, len(titles))):
            assert L.itsx_parse_fetch(e.h, plane, 0, size + 1, out.ctypes.data) == -1, plane          # past the plane's end
            assert L.itsx_parse_fetch(e.h, plane, -1, size, out.ctypes.data) == -1, plane
            assert L.itsx_parse_fetch(e.h, plane, 2, 1, out.ctypes.data) == -1, plane
            assert L.itsx_parse_fetch(e.h, plane, 0, size, None) == -1, plane
            assert L.itsx_parse_fetch(e.h, plane, size, size, None) == 0, plane                       # an empty range needs no buffer
        assert L.itsx_parse_fetch(e.h, 5, 0, 1, out.ctypes.data) == -1 and L.itsx_parse_fetch(e.h, -1, 0, 1, out.ctypes.data) == -1
        assert e.parse_fetch("seq", 1, len(seq) - 1) == seq[1:-1] and e.parse_fetch("off", 1, 3).tolist() == off[1:3]
        assert L.itsx_parse_device(e.h, None, 0, 1, C.byref(n)) == 0 and n.value == 0             # no text is a text of no bytes
        assert e.parse_fetch("off", 0, 1).tolist() == [0] and e.parse_fetch("toff", 0, 1).tolist() == [0] and e.parse_fetch("seq", 0, 0) == b""
        assert _counters(e) == (3, 0)
        assert e.parse == "host"
        with pytest.raises(ValueError):
            e.parse = "gpu"
        e.parse = "device"
        assert e.parse == "device"
    finally:
        e.close()
