"""itsx_twriter_strands / itsx_write_trimmed_fastq_strands on the host: a record of strand -1 is written from its reverse complement
(the record oriented.fq would hold), sliced by the same coordinates.  The model is tests/twriter_strand_cases.py: Python slicing of
Python strings.  No GPU needed: the writer is context-free."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import twriter_strand_cases as tc
from orient_profiles_exact import revcomp
from itsxpress_amd import Dedup, EngineError
from itsxpress_amd.engine import read_fastx
from itsxpress_amd.trim import write_trimmed_fastq


@pytest.fixture(autouse=True)
def _units(monkeypatch):
    monkeypatch.setenv("ITSX_WRITE_UNIT_KB", str(tc.UNIT_KB))
    monkeypatch.setenv("ITSX_IO_THREADS", "4")


@pytest.fixture(scope="module")
def cat():
    text, recs, start, stop, strand, tags = tc.catalogue()
    ends = tc.record_ends(text)
    assert len(ends) == len(recs)
    return dict(text=text, recs=recs, start=start, stop=stop, strand=strand, tags=tags, ends=ends,
                model={ccs: tc.model(recs, start, stop, strand, ccs) for ccs in (0, 1)})


def test_the_catalogue_holds_what_it_promises(cat):
    recs, start, stop, strand = cat["recs"], cat["start"], cat["stop"], cat["strand"]
    lens = np.array([len(r[1]) for r in recs])
    written = (start >= 0) & (stop >= 0) & (start < stop)
    for flip in (-1, 1):
        seen = {(int(L) % 4, int(a) % 4, int(b) % 4) for L, a, b, d, w in zip(lens, start, stop, strand, written) if w and d == flip}
        assert len(seen) == 64, (flip, len(seen))
    for L in tc.LENGTHS + [tc.LONG]:
        assert ((lens == L) & (strand < 0) & written).any() and ((lens == L) & (strand > 0) & written).any(), L
    assert {len(r[0]) for r in recs} == set(range(1, 9))
    assert (strand == 0).any() and (~written & (strand < 0)).any() and ((stop > lens) & written & (strand < 0)).any()
    assert any(r[2][0] == "@" and d < 0 for r, d in zip(recs, strand)) and any(r[3] == "\r\n" and d < 0 for r, d in zip(recs, strand))
    assert not cat["text"].endswith(b"\n") and b"\n\n@" in cat["text"]
    # runs of one strand that are longer than a unit, and a unit boundary inside alternating records
    size, best = 0, {1: 0, -1: 0}
    for i in range(len(recs)):
        if i and strand[i] != strand[i - 1]:
            size = 0
        if strand[i] and lens[i] < 2000:                # (bytes of the run of short records that ends here)
            size += len(recs[i][0]) + 2 * int(lens[i]) + 5
            best[int(strand[i])] = max(best[int(strand[i])], size)
    assert min(best.values()) > 2 * tc.UNIT_KB * 1024
    assert len(cat["text"]) > 40 * tc.UNIT_KB * 1024
    # flipping changes the bytes of the model: the test cannot pass on a writer that ignores the strands
    assert tc.model(recs, start, stop, np.ones_like(strand), 0)[0] != cat["model"][0][0]


@pytest.mark.parametrize("pieces", [False, True])
@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("ccs", [0, 1])
def test_edge_catalogue_equals_the_model(cat, tmp_path, ccs, comp, pieces):
    out = tmp_path / "o"
    nw, tot = tc.write(out, cat["text"], cat["ends"], cat["start"], cat["stop"], cat["strand"], comp, ccs, pieces)
    got = out.read_bytes()
    if comp:
        got = gzip.decompress(got)
    want, n, t = cat["model"][ccs]
    assert (nw, tot) == (n, t)
    assert got == want


def test_single_io_thread_and_the_one_call_entry(cat, tmp_path, monkeypatch):
    """itsx_write_trimmed_fastq_strands through the writer object and through the serial walk (one I/O thread): the model's bytes"""
    src = tmp_path / "in.fq"
    src.write_bytes(cat["text"])
    want, n, t = cat["model"][0]
    for threads in ("4", "1"):
        monkeypatch.setenv("ITSX_IO_THREADS", threads)
        out = str(tmp_path / ("o" + threads))
        assert write_trimmed_fastq(str(src), out, cat["start"], cat["stop"], strand=cat["strand"]) == (n, t)
        assert open(out, "rb").read() == want
    want1, n1, t1 = tc.model(cat["recs"], cat["start"], cat["stop"], np.ones_like(cat["strand"]), 1)
    out = str(tmp_path / "ccs")
    assert write_trimmed_fastq(str(src), out, cat["start"], cat["stop"], trim_ccs=True, strand=None) == (n1, t1)
    assert open(out, "rb").read() == want1


def _golden_rows(gold):
    rows = [ln.split("\t") for ln in open(os.path.join(gold, "fungi_its2_coords.tsv")).read().strip().split("\n")[1:]]
    coords = {r[0]: (int(r[2]), int(r[3])) for r in rows}
    seq = os.path.join(gold, "seq.fq.gz")
    names, _ = read_fastx(seq)
    md = Dedup(os.path.join(gold, "fixture_uc.txt"), "", seq).matchdict
    start = np.array([coords.get(md[n], (-1, -1))[0] for n in names], np.int32)
    stop = np.array([coords.get(md[n], (-1, -1))[1] for n in names], np.int32)
    return seq, start, stop


@pytest.mark.parametrize("unit_kb", [4, 8192])
def test_flipped_fixture_gives_the_unflipped_fixtures_bytes(gold, tmp_path, monkeypatch, unit_kb):
    """the reference fixture seq.fq with every third record reverse-complemented, written with those strands at -1 and the golden
    coordinates: the bytes itsx_write_trimmed_fastq writes from the fixture as it is (226 records, 42637 bases: the reference's test)"""
    monkeypatch.setenv("ITSX_WRITE_UNIT_KB", str(unit_kb))
    seq, start, stop = _golden_rows(gold)
    plain = str(tmp_path / "today.fq")
    assert write_trimmed_fastq(seq, plain, start, stop) == (226, 42637)
    today = open(plain, "rb").read()
    lines = gzip.open(seq, "rt").read().split("\n")
    n = len(start)
    strand = np.where(np.arange(n) % 3 == 0, -1, 1).astype(np.int8)
    for i in range(0, n, 3):
        lines[4 * i + 1], lines[4 * i + 3] = revcomp(lines[4 * i + 1]), lines[4 * i + 3][::-1]
    flipped = str(tmp_path / "flipped.fq")
    with open(flipped, "w") as f:
        f.write("\n".join(lines))
    for name, kw in (("f.fq", {}), ("f.fq.gz", {"gzipped": True})):
        out = str(tmp_path / name)
        assert write_trimmed_fastq(flipped, out, start, stop, strand=strand, **kw) == (226, 42637)
        got = open(out, "rb").read()
        assert (gzip.decompress(got) if kw else got) == today
    # without the strands the flipped file gives other bytes; NULL and all +1 on the fixture give today's
    out = str(tmp_path / "unoriented.fq")
    write_trimmed_fastq(flipped, out, start, stop)
    assert open(out, "rb").read() != today
    for k, sd in enumerate((None, np.ones(n, np.int8), np.zeros(n, np.int8))):
        out = str(tmp_path / ("same%d.fq" % k))
        assert write_trimmed_fastq(seq, out, start, stop, strand=sd) == (226, 42637)
        assert open(out, "rb").read() == today


def test_errors(tmp_path):
    L = tc._lib()
    text = b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIIII\n"
    buf = C.create_string_buffer(text, len(text))
    a, b = np.array([0, 0], np.int32), np.array([4, 4], np.int32)
    sd = np.array([-1, 1], np.int8)

    def opened(name):
        w = C.c_void_p()
        assert L.itsx_twriter_open(os.fsencode(str(tmp_path / name)), 0, 0, C.byref(w)) == 0
        return w

    # strands after the coordinates of the same records
    w = opened("late")
    assert L.itsx_twriter_coords(w, 0, 1, a.ctypes.data, b.ctypes.data, None) == 0
    assert L.itsx_twriter_strands(w, 0, 2, sd.ctypes.data) == -1
    assert b"before the coordinates" in L.itsx_trim_last_error()
    # ... while the records behind them still take theirs; a gap does not
    assert L.itsx_twriter_strands(w, 2, 1, sd.ctypes.data) == -1
    assert L.itsx_twriter_strands(w, 1, 1, sd.ctypes.data) == 0
    assert L.itsx_twriter_strands(w, 3, 1, sd.ctypes.data) == -1
    assert L.itsx_twriter_coords(w, 1, 1, a.ctypes.data, b.ctypes.data, None) == 0
    assert L.itsx_twriter_text(w, C.addressof(buf), len(text), 1) == 0
    assert L.itsx_twriter_close(w, None, None) == 0
    assert (tmp_path / "late").read_bytes() == b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIIII\n"      # (record 0 had no row; record 1's was -1: ACGT is its own reverse complement)
    # a mode-1 writer
    w = opened("mode1")
    assert L.itsx_twriter_set_mode(w, 1) == 0
    assert L.itsx_twriter_strands(w, 0, 2, sd.ctypes.data) == -1
    assert b"mode 1" in L.itsx_trim_last_error()
    L.itsx_twriter_close(w, None, None)
    w = opened("mode1b")
    assert L.itsx_twriter_strands(w, 0, 2, sd.ctypes.data) == 0
    assert L.itsx_twriter_set_mode(w, 1) == -1
    L.itsx_twriter_close(w, None, None)
    # null rows, a null writer
    w = opened("null")
    assert L.itsx_twriter_strands(w, 0, 2, None) == -1
    assert L.itsx_twriter_strands(None, 0, 2, sd.ctypes.data) == -1
    L.itsx_twriter_close(w, None, None)
    # a strand count that does not match the coordinates
    src = tmp_path / "in.fq"
    src.write_bytes(text)
    with pytest.raises(EngineError) as e:
        write_trimmed_fastq(str(src), str(tmp_path / "x"), a, b, strand=np.ones(3, np.int8))
    assert e.value.code == -1 and "3 strands for 2 records" in str(e.value)
    assert not (tmp_path / "x").exists()
