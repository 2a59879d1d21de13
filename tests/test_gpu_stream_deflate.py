"""itsx_twriter_set_device / StreamEngine.deflate = "device": the streamed writers' gzip output made on the device -- a unit's raw text
and coordinates go up, its lines are indexed, its records planned, copied and deflated there (csrc/k_trim.hip, csrc/k_deflate.hip), and
only compressed bytes come back.  The model throughout is the host writer object with compression 0, fed the same text and
coordinates: the device file must inflate (under Python's CRC and ISIZE checks, over all members) to the model's file byte for byte,
with the same n_written and total_len.  `pytest -m gpu`."""
import ctypes as C
import gzip
import importlib
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
UNIT_KB = 16
HOOK = "ITSX_TWRITER_HOST_SLICE"


def _lib():
    from itsxpress_amd import _lib as m
    return m.lib()


@pytest.fixture(scope="module")
def dev():
    from itsxpress_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _units(monkeypatch):
    monkeypatch.setenv("ITSX_WRITE_UNIT_KB", str(UNIT_KB))
    monkeypatch.setenv("ITSX_IO_THREADS", "4")


def _registry():
    L = _lib()
    n = L.itsx_switch_registry(None, 0)
    b = C.create_string_buffer(int(n))
    L.itsx_switch_registry(b, n)
    return {line.split("\t")[0]: line.split("\t")[1] for line in b.value.decode().strip().split("\n")}


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
def _catalogue(tail):
    """A few hundred records that make many 16-KB units.  Returns (text, lens, tags): lens[i] = bases of record i, tags = name -> record.
    tail: "open" (the last record has no newline) or "blanks" (blank lines at the end of the text)."""
    rng = np.random.default_rng(2024)
    B = int(_lib().itsx_deflate_block_bytes())
    recs, lens, tags = [], [], {}

    def add(title, ln, nl="\n", plus="+", before=""):
        s = "".join(rng.choice(list("ACGT"), ln)) if ln < 2000 else ("".join(rng.choice(list("ACGT"), 997)) * (ln // 997 + 1))[:ln]
        q = "".join(rng.choice(list("@+IF#5~"), ln)) if ln < 2000 else ("".join(rng.choice(list("@+IF#5~"), 991)) * (ln // 991 + 1))[:ln]
        recs.append(before + title + nl + s + nl + plus + nl + q + nl)
        lens.append(ln)
        return len(recs) - 1

    def plain(k):
        for _ in range(k):
            i = len(recs)
            add("@r%d some words" % i, int(rng.integers(40, 330)))

    plain(70)
    for _ in range(25):                                     # CRLF line ends, a '+' line that repeats the title
        i = len(recs)
        add("@crlf%d x" % i, int(rng.integers(40, 300)), nl="\r\n")
        add("@rep%d y" % i, int(rng.integers(40, 300)), plus="+rep%d y" % i)
        add("@both%d" % i, int(rng.integers(1, 60)), nl="\r\n", plus="+both%d" % i)
    for _ in range(6):                                      # reads of 0 bases
        add("@empty%d" % len(recs), 0)
        add("@emptycr%d" % len(recs), 0, nl="\r\n")
        plain(3)
    plain(60)
    tags["blank0"] = len(recs)
    for k in range(40):                                     # blank lines between records (also "\r\n" ones): the host slices these units
        add("@gap%d" % len(recs), int(rng.integers(40, 300)), before="\n" if k % 3 == 0 else ("\r\n\n" if k % 7 == 0 else ""))
    tags["blank1"] = len(recs)
    plain(70)
    tags["long_unit"] = add("@longer_than_a_unit", 40000)   # one record longer than a unit
    plain(70)
    tags["big"] = add("@seventy_thousand", 70000)           # its output crosses a deflate block
    # a unit whose output is exactly B bytes, and one of B + 1: 70 records before each that are not written, then one record whose
    # output is title + 5 + 2 x 32700 (its raw text spans several units' worth: the unit ends behind it)
    for name, extra in (("exact", 0), ("plus1", 1)):
        tags[name + "_lo"] = len(recs)
        plain(70)
        tl = B + extra - 5 - 2 * 32700
        tags[name] = add("@" + name + " " + "t" * (tl - len(name) - 2), 33000)
        assert len(recs[-1].split("\n")[0]) == tl
    tags["dead_lo"] = len(recs)
    plain(200)                                              # units with no surviving record (the coordinates skip these)
    tags["dead_hi"] = len(recs)
    plain(40)
    text = "".join(recs)
    if tail == "open":
        assert text.endswith("\n")
        text = text[:-1]
    else:
        text += "\n\r\n\n"
    return text.encode(), np.array(lens, np.int64), tags


def _coords(lens, tags, mode, seed, none=False):
    """coordinates that visit every branch of itsx_twriter::work's decision in that mode"""
    rng = np.random.default_rng(seed)
    n = lens.shape[0]
    L = np.maximum(lens, 1)
    if mode == 0:
        start = rng.integers(0, 60, n)
        stop = start + rng.integers(1, 300, n)              # often past the read
        kind = rng.integers(0, 10, n)
        start = np.where(kind == 0, -rng.integers(1, 50, n), start)     # negative start
        stop = np.where(kind == 1, -rng.integers(1, 50, n), stop)       # negative stop
        stop = np.where(kind == 2, start, stop)                         # start == stop
        stop = np.where(kind == 3, start - 1 - rng.integers(0, 5, n), stop)     # start > stop
        stop = np.where(kind == 4, lens + rng.integers(1, 1000, n), stop)       # stop past the read
        start = np.where(kind == 5, lens + 5, start)                    # start past the read too (an empty slice that is still a record)
        stop = np.where(kind == 5, lens + 9, stop)
        skip = (-1, -1)
    else:
        start = rng.integers(-400, 300, n)                  # negative bounds, some below -len
        stop = rng.integers(-400, 500, n)
        kind = rng.integers(0, 10, n)
        start = np.where(kind == 0, -L - rng.integers(1, 100, n), start)        # below -len
        stop = np.where(kind == 1, I32_MAX, stop)                       # open end
        stop = np.where(kind == 2, I32_MIN, stop)                       # not written
        stop = np.where(kind == 3, start - rng.integers(1, 30, n), stop)        # stop < start: an empty slice, still a record
        start = np.where(kind == 4, I32_MIN, start)
        skip = (0, I32_MIN)
    start, stop = start.astype(np.int64), stop.astype(np.int64)
    for name in ("exact", "plus1"):
        start[tags[name + "_lo"]:tags[name]] = skip[0]; stop[tags[name + "_lo"]:tags[name]] = skip[1]
        start[tags[name]] = 0; stop[tags[name]] = 32700
    start[tags["dead_lo"]:tags["dead_hi"]] = skip[0]; stop[tags["dead_lo"]:tags["dead_hi"]] = skip[1]
    for name in ("big", "long_unit"):
        start[tags[name]] = 3; stop[tags[name]] = I32_MAX if mode == 1 else 10 ** 6
    if none:
        start[:] = skip[0]; stop[:] = skip[1]
    return start.astype(np.int32), stop.astype(np.int32)


# ---- feeding a writer ------------------------------------------------------------------------------------------------------------
def _record_ends(text):
    """byte offset behind every record, as the library's parser walks the text: blank lines are skipped before a title only"""
    ends, inside, pos = [], 0, 0
    for ln in text.split(b"\n"):
        pos += len(ln) + 1
        if inside == 0 and not ln.strip(b"\r"):
            continue
        inside += 1
        if inside == 4:
            ends.append(min(pos, len(text)))
            inside = 0
    return ends


def _write(path, text, ends, start, stop, comp, ccs, mode, rhythm, ctx=None, expect=0):
    """test_trim_cpu.py's arrival rhythm: text and coordinates in pieces in a seeded random order, some records undecided when their
    piece arrives and settled later by itsx_twriter_update.  rhythm None: everything at once.  Returns (n_written, total_len)."""
    L = _lib()
    n = len(ends)
    w = C.c_void_p()
    assert L.itsx_twriter_open(os.fsencode(str(path)), comp, ccs, C.byref(w)) == 0, L.itsx_trim_last_error()
    if mode:
        assert L.itsx_twriter_set_mode(w, mode) == 0
    if ctx is not None:
        assert L.itsx_twriter_set_device(w, ctx.h) == 0, L.itsx_trim_last_error()
    buf = C.create_string_buffer(text, len(text))
    base = C.addressof(buf)
    if rhythm is None:
        assert L.itsx_twriter_text(w, base, len(text), 1) == 0
        assert L.itsx_twriter_coords(w, 0, n, start.ctypes.data, stop.ctypes.data, None) == 0
    else:
        rng = np.random.default_rng(100 + rhythm)
        late = rng.random(n) < (0.0, 0.01, 0.08)[rhythm]
        wrong = np.where(late, 7, start).astype(np.int32)
        cuts = sorted(set(int(x) for x in rng.integers(1, n, 4 + 3 * rhythm))) + [n]
        lo = 0
        for k, hi in enumerate(cuts):
            a1, a2, a3 = np.ascontiguousarray(wrong[lo:hi]), np.ascontiguousarray(stop[lo:hi]), (~late[lo:hi]).astype(np.uint8)
            upto = len(text) if hi == n else ends[hi - 1]
            steps = [lambda: L.itsx_twriter_text(w, base, int(upto), 1 if hi == n else 0),
                     lambda: L.itsx_twriter_coords(w, lo, hi - lo, a1.ctypes.data, a2.ctypes.data, a3.ctypes.data)]
            for f in (steps if (k + rhythm) % 2 else steps[::-1]):
                assert f() == 0, L.itsx_trim_last_error()
            lo = hi
        idx = np.flatnonzero(late).astype(np.int64)
        for part in np.array_split(idx, 3):
            s1, s2 = np.ascontiguousarray(start[part]), np.ascontiguousarray(stop[part])
            assert L.itsx_twriter_update(w, part.ctypes.data, len(part), s1.ctypes.data, s2.ctypes.data) == 0
    nw, tot = C.c_int64(), C.c_int64()
    rc = L.itsx_twriter_close(w, C.byref(nw), C.byref(tot))
    assert rc == expect, (rc, L.itsx_trim_last_error())
    return nw.value, tot.value


def _members(z):
    """the inflated size of every gzip member of z, each under zlib's CRC-32 and ISIZE checks"""
    sizes = []
    while z:
        d = zlib.decompressobj(31)
        out = d.decompress(z)
        assert d.eof
        sizes.append(len(out))
        z = d.unused_data
    return sizes


_MODEL = {}


def _model(tmp_path_factory, tail, mode, ccs, none=False):
    """the catalogue text, its coordinates and the host writer's plain file for them: computed once, shared, left unchanged"""
    key = (tail, mode, ccs, none)
    if key not in _MODEL:
        text, lens, tags = _catalogue(tail)
        ends = _record_ends(text)
        assert len(ends) == lens.shape[0]
        start, stop = _coords(lens, tags, mode, 7 + mode, none)
        p = tmp_path_factory.mktemp("model") / "model.fq"
        want = _write(p, text, ends, start, stop, 0, ccs, mode, None)
        _MODEL[key] = (text, ends, start, stop, want, p.read_bytes(), tags)
    return _MODEL[key]


def _expected_paths(text, start, stop, mode):
    """The units as itsx_twriter cuts them (the first record start behind the first newline at or after every multiple of the unit size),
    and which way each must go: (units whose lines are 4 per record: the device's index, plan and copy; units with a blank line that have
    output: sliced by the host; units with output at all)."""
    import bisect
    n, U = len(text), UNIT_KB << 10
    titles, inside, pos = [], 0, 0                          # where every record's title starts
    for ln in text.split(b"\n"):
        if inside or ln.strip(b"\r"):
            if inside == 0:
                titles.append(pos)
            inside = (inside + 1) % 4
        pos += len(ln) + 1
    written = (start >= 0) & (stop >= 0) & (start < stop) if mode == 0 else stop != I32_MIN
    units, lo, cut = [], 0, 0
    while lo < n:
        want = cut + U
        cut = want
        nl = text.find(b"\n", want) if want < n else -1
        i = bisect.bisect_left(titles, nl + 1) if nl >= 0 else len(titles)
        hi = titles[i] if i < len(titles) else n
        if hi > lo:
            units.append((lo, hi))
            lo = hi
    fit = sliced = with_output = 0
    for lo, hi in units:
        r0, r1 = bisect.bisect_left(titles, lo), bisect.bisect_left(titles, hi)
        lines = text.count(b"\n", lo, hi) + (text[hi - 1:hi] != b"\n")
        out = bool(written[r0:r1].any())
        with_output += out
        if r1 > r0 and lines == 4 * (r1 - r0):
            fit += 1
        elif out:
            sliced += 1
    return len(units), fit, sliced, with_output


def _paths(dev):
    st = dev.stats()
    return np.array([st["n_tw_units_device"], st["n_tw_units_host"]])


CASES = [("open", 0, 0), ("open", 0, 1), ("blanks", 0, 0), ("open", 1, 0), ("blanks", 1, 0)]


@pytest.mark.parametrize("tail,mode,ccs", CASES)
def test_device_writer_equals_the_host_model_in_every_rhythm(tmp_path, tmp_path_factory, dev, monkeypatch, tail, mode, ccs):
    """every catalogue case and coordinate branch: the device file inflates to the model's, with its counts; the file's bytes are the
    same across three arrival rhythms, across two runs, and with every unit forced through the host slicer (which is what checks the
    index, plan and copy kernels against the host slicer).  The context's counters say which way the units went: without the hook every
    unit but those with a blank line through the device's index, plan and copy; with it none"""
    assert _registry().get(HOOK) == "hook"
    text, ends, start, stop, want, plain, tags = _model(tmp_path_factory, tail, mode, ccs)
    assert want[0] > 100 and len(text) > 30 * (UNIT_KB << 10)
    n_units, fit, sliced, with_output = _expected_paths(text, start, stop, mode)
    print("units: %d, 4 lines per record: %d, with a blank line and output: %d, with output: %d" % (n_units, fit, sliced, with_output))
    assert n_units >= 20 and fit >= n_units - 6 and 1 <= sliced <= 5 and with_output < fit
    files = {}
    for name, rhythm, hook in (("r0", 0, False), ("r1", 1, False), ("r2", 2, False), ("again", 0, False), ("host_slice", 1, True)):
        if hook:
            monkeypatch.setenv("ITSX_TEST_HOOKS", "1")
            monkeypatch.setenv(HOOK, "1")
        out = tmp_path / (name + ".fq.gz")
        before = _paths(dev)
        got = _write(out, text, ends, start, stop, 1, ccs, mode, rhythm, ctx=dev)
        assert (_paths(dev) - before).tolist() == ([0, with_output] if hook else [fit, sliced]), name
        if hook:
            monkeypatch.delenv(HOOK)
            monkeypatch.delenv("ITSX_TEST_HOOKS")
        files[name] = out.read_bytes()
        assert got == want, name
        assert gzip.decompress(files[name]) == plain, name
    sizes = _members(files["r0"])
    assert sum(sizes) == len(plain)
    for name in ("r1", "r2", "again", "host_slice"):
        assert files[name] == files["r0"], name
    B = int(_lib().itsx_deflate_block_bytes())
    print("members: %d, of a full block: %d, of one byte: %d, compressed %d of %d" % (len(sizes), sizes.count(B), sizes.count(1), len(files["r0"]), len(plain)))
    assert max(sizes) == B
    if not ccs:
        # the unit of B + 1 bytes leaves a member of one byte; full members: that unit's, the unit of exactly B, the 70 000-base read's
        assert sizes.count(1) == 1 and sizes.count(B) >= 3


def test_hook_without_the_gate_changes_nothing(tmp_path, tmp_path_factory, dev, monkeypatch):
    """the forced fallback is a test hook: set without ITSX_TEST_HOOKS=1 the run ends as well as ever"""
    text, ends, start, stop, want, plain, _ = _model(tmp_path_factory, "open", 0, 0)
    monkeypatch.setenv(HOOK, "1")
    out = tmp_path / "o.fq.gz"
    assert _write(out, text, ends, start, stop, 1, 0, 0, None, ctx=dev) == want
    assert gzip.decompress(out.read_bytes()) == plain


@pytest.mark.parametrize("mode", [0, 1])
def test_text_with_no_surviving_record(tmp_path, tmp_path_factory, dev, mode):
    """no record survives: the valid empty gzip the host writer produces, byte for byte"""
    text, ends, start, stop, want, plain, _ = _model(tmp_path_factory, "open", mode, 0, none=True)
    assert want == (0, 0) and plain == b""
    host, devf = tmp_path / "host.fq.gz", tmp_path / "dev.fq.gz"
    assert _write(host, text, ends, start, stop, 1, 0, mode, None) == (0, 0)
    assert _write(devf, text, ends, start, stop, 1, 0, mode, 1, ctx=dev) == (0, 0)
    assert devf.read_bytes() == host.read_bytes() and gzip.decompress(devf.read_bytes()) == b""


def test_two_writers_share_one_context(tmp_path, tmp_path_factory, dev):
    """a paired run's R1 and R2: two writers on one context, fed side by side"""
    L = _lib()
    m = [_model(tmp_path_factory, "open", 1, 0), _model(tmp_path_factory, "blanks", 1, 0)]
    ws, bufs = [], []
    for k in range(2):
        w = C.c_void_p()
        assert L.itsx_twriter_open(os.fsencode(str(tmp_path / ("p%d.fq.gz" % k))), 1, 0, C.byref(w)) == 0
        assert L.itsx_twriter_set_mode(w, 1) == 0
        assert L.itsx_twriter_set_device(w, dev.h) == 0, L.itsx_trim_last_error()
        ws.append(w)
        bufs.append(C.create_string_buffer(m[k][0], len(m[k][0])))
    for k in range(2):
        assert L.itsx_twriter_text(ws[k], C.addressof(bufs[k]), len(m[k][0]), 1) == 0
    for k in range(2):
        assert L.itsx_twriter_coords(ws[k], 0, len(m[k][1]), m[k][2].ctypes.data, m[k][3].ctypes.data, None) == 0
    for k in range(2):
        nw, tot = C.c_int64(), C.c_int64()
        assert L.itsx_twriter_close(ws[k], C.byref(nw), C.byref(tot)) == 0, L.itsx_trim_last_error()
        assert (nw.value, tot.value) == m[k][4]
        assert gzip.decompress((tmp_path / ("p%d.fq.gz" % k)).read_bytes()) == m[k][5]
    assert dev.stats()["ms_deflate"] > 0


def test_malformed_text_is_reported_as_the_host_writer_reports_it(tmp_path, tmp_path_factory, dev):
    text, ends, start, stop, _, _, _ = _model(tmp_path_factory, "blanks", 0, 0)
    bad = text + b"@broken\nACGT\n+\nII\n"
    n = len(ends) + 1
    a, b = np.zeros(n, np.int32), np.full(n, 10, np.int32)
    L = _lib()
    for ctx in (None, dev):
        _write(tmp_path / "bad.fq.gz", bad, ends + [len(bad)], a, b, 1, 0, 0, None, ctx=ctx, expect=-3)
        assert b"malformed FASTQ record" in L.itsx_trim_last_error()


def test_set_device_arguments(tmp_path, dev):
    """ITSX_E_ARG on a plain writer, a zstd writer and after text has arrived; the writer stays usable or closable; compression 3 is
    still refused at open"""
    L = _lib()
    w = C.c_void_p()
    assert L.itsx_twriter_open(os.fsencode(str(tmp_path / "x")), 3, 0, C.byref(w)) == -1
    text = b"@a\nACGT\n+\nIIII\n"
    buf = C.create_string_buffer(text, len(text))
    one, four = np.zeros(1, np.int32), np.full(1, 4, np.int32)
    kinds = [0] + ([2] if L.itsx_io_codecs() & 2 else [])
    for kind in kinds:
        out = tmp_path / ("k%d" % kind)
        assert L.itsx_twriter_open(os.fsencode(str(out)), kind, 0, C.byref(w)) == 0
        assert L.itsx_twriter_set_device(w, dev.h) == -1
        assert b"itsx_twriter_set_device" in L.itsx_trim_last_error()
        assert L.itsx_twriter_text(w, C.addressof(buf), len(text), 1) == 0
        assert L.itsx_twriter_coords(w, 0, 1, one.ctypes.data, four.ctypes.data, None) == 0
        nw, tot = C.c_int64(), C.c_int64()
        assert L.itsx_twriter_close(w, C.byref(nw), C.byref(tot)) == 0 and (nw.value, tot.value) == (1, 4)
        if kind == 0:
            assert out.read_bytes() == text
    out = tmp_path / "late.gz"
    assert L.itsx_twriter_open(os.fsencode(str(out)), 1, 0, C.byref(w)) == 0
    assert L.itsx_twriter_text(w, C.addressof(buf), len(text), 0) == 0
    assert L.itsx_twriter_set_device(w, dev.h) == -1
    assert b"before any text" in L.itsx_trim_last_error()
    assert L.itsx_twriter_text(w, C.addressof(buf), len(text), 1) == 0
    assert L.itsx_twriter_coords(w, 0, 1, one.ctypes.data, four.ctypes.data, None) == 0
    assert L.itsx_twriter_close(w, None, None) == 0
    assert gzip.decompress(out.read_bytes()) == text
    # a second context for a writer that has one
    assert L.itsx_twriter_open(os.fsencode(str(tmp_path / "twice.gz")), 1, 0, C.byref(w)) == 0
    assert L.itsx_twriter_set_device(w, dev.h) == 0, L.itsx_trim_last_error()
    assert L.itsx_twriter_set_device(w, dev.h) == -1
    assert L.itsx_twriter_text(w, C.addressof(buf), len(text), 1) == 0
    assert L.itsx_twriter_coords(w, 0, 1, one.ctypes.data, four.ctypes.data, None) == 0
    assert L.itsx_twriter_close(w, None, None) == 0
    assert gzip.decompress((tmp_path / "twice.gz").read_bytes()) == text


# ---- end to end through the mirror ------------------------------------------------------------------------------------------------
S = importlib.import_module("itsxpress_amd.SeqSample")
_OPEN = []


@pytest.fixture(autouse=True)
def _close_engines():
    yield
    while _OPEN:
        s = _OPEN.pop()
        if getattr(s, "_engine", None) is not None:
            s._engine.close()


def _its2(tmp, t_hmm_text):
    from bench import its2_profiles
    p = os.path.join(tmp, "its2.hmm")
    with open(p, "w") as f:
        f.write(its2_profiles(t_hmm_text))
    return p


def _planned_single(fq, d, hmm, monkeypatch, deflate):
    from itsxpress_amd import trim
    from itsxpress_amd.stream import StreamEngine
    os.makedirs(d, exist_ok=True)
    monkeypatch.setenv("ITSXPRESS_GPUS", "1"); monkeypatch.setenv("ITSXPRESS_STREAM", "1"); monkeypatch.setenv("ITSXPRESS_ARRAYS", "1")
    trim.cache_clear()
    sobj = S.SeqSampleNotPaired(fastq=fq, tempdir=d)
    _OPEN.append(sobj)
    assert isinstance(sobj.engine, StreamEngine)
    if deflate is not None:
        sobj.engine.deflate = deflate
    out = os.path.join(d, "trimmed.fq.gz")
    sobj.plan_output(out, "ITS2", gzipped=True)
    sobj.deduplicate(threads=1)
    sobj._search(hmmfile=hmm, threads=1)
    eng = sobj._engine
    assert eng.world >= 4 and eng._out is not None
    its_pos = S.ItsPosition(domtable=sobj.dom_file, region="ITS2")
    dd = S.Dedup(uc_file=sobj.uc_file, rep_file=sobj.rep_file, seq_file=sobj.seq_file, fastq=sobj.r1, fastq2=sobj.fastq2)
    dd.create_trimmed_seqs(out, gzipped=True, zstd_file=False, itspos=its_pos, wri_file=True, tempdir=d)
    assert eng._out.result is not None and eng._out.dev_eng is None
    return open(out, "rb").read(), eng._out


def test_single_end_through_the_streaming_engine(tmp_path, t_hmm_text, monkeypatch):
    """test_writer_inside_the_pipeline_writes_the_same_bytes's settings (chunks of 1.5 MB, units of 256 KB): deflate = "device" through the
    mirror, then ITSX_DEVICE_DEFLATE=1 alone: both inflate to what the default run's file inflates to"""
    from test_gpu_stream import _fastq_gz
    tmp = str(tmp_path)
    hmm = _its2(tmp, t_hmm_text)
    monkeypatch.setenv("ITSX_PINFLATE_CHUNK_KB", "32")
    monkeypatch.setenv("ITSX_STREAM_CHUNK_MB", "1.5")
    monkeypatch.setenv("ITSX_WRITE_UNIT_KB", "256")
    fq = os.path.join(tmp, "in.fq.gz")
    _fastq_gz(fq, t_hmm_text, 12000, 616)
    ref, o = _planned_single(fq, os.path.join(tmp, "host"), hmm, monkeypatch, None)
    assert o.plan["deflate"] == "host" and o.ms_deflate == 0
    want = gzip.decompress(ref)
    assert len(want) > (1 << 20)
    got, o = _planned_single(fq, os.path.join(tmp, "device"), hmm, monkeypatch, "device")
    assert o.plan["deflate"] == "device" and o.ms_deflate > 0
    assert o.units_device >= 4 and o.units_host == 0          # (well-formed text: every unit through the device's index, plan and copy)
    assert got != ref and gzip.decompress(got) == want
    monkeypatch.setenv("ITSX_DEVICE_DEFLATE", "1")
    env, o = _planned_single(fq, os.path.join(tmp, "env"), hmm, monkeypatch, None)
    assert o.plan["deflate"] == "device" and o.ms_deflate > 0
    assert env == got and gzip.decompress(env) == want


def test_paired_end_through_the_streaming_engine(tmp_path, t_hmm_text, monkeypatch):
    """test_gpu_stream.py's paired fixture with chunks of 0.02 MB, the two outputs planned as gzip: with deflate = "device" both files
    inflate to the default run's"""
    from conftest import GOLD
    from itsxpress_amd.stream import StreamEngine
    tmp = str(tmp_path)
    hmm = _its2(tmp, t_hmm_text)
    raw = []
    for fn in ("4774-1-MSITS3_R1.fastq", "4774-1-MSITS3_R2.fastq"):
        p = os.path.join(tmp, fn)
        with gzip.open(os.path.join(GOLD, fn + ".gz"), "rb") as f, open(p, "wb") as g:
            g.write(f.read())
        raw.append(p)
    monkeypatch.setenv("ITSX_STREAM_CHUNK_MB", "0.02")
    monkeypatch.setenv("ITSXPRESS_GPUS", "1"); monkeypatch.setenv("ITSXPRESS_STREAM", "1"); monkeypatch.setenv("ITSXPRESS_ARRAYS", "1")
    outs = {}
    for name in ("host", "device"):
        d = os.path.join(tmp, name)
        os.makedirs(d, exist_ok=True)
        sobj = S.SeqSamplePairedNotInterleaved(fastq=raw[0], tempdir=d, fastq2=raw[1])
        _OPEN.append(sobj)
        assert isinstance(sobj.engine, StreamEngine)
        sobj.engine.deflate = name
        o1, o2 = os.path.join(d, "r1.fq.gz"), os.path.join(d, "r2.fq.gz")
        sobj.plan_output_paired(o1, o2, "ITS2", gzipped=True)
        sobj._merge_reads(threads=1)
        sobj.deduplicate(threads=1)
        sobj._search(hmmfile=hmm, threads=1)
        its_pos = S.ItsPosition(domtable=sobj.dom_file, region="ITS2")
        dd = S.Dedup(uc_file=sobj.uc_file, rep_file=sobj.rep_file, seq_file=sobj.seq_file, fastq=sobj.r1, fastq2=sobj.fastq2)
        dd.create_paired_trimmed_seqs(o1, o2, gzipped=True, zstd_file=False, itspos=its_pos, wri_file=True)
        eng = sobj._engine
        assert eng.world >= 3 and eng._out is not None and eng._out.result is not None and eng._out.dev_eng is None
        assert eng._out.plan["deflate"] == name
        assert (eng._out.units_device > 0 and eng._out.units_host == 0) if name == "device" else eng._out.units_device == 0
        outs[name] = (open(o1, "rb").read(), open(o2, "rb").read())
    for k in range(2):
        assert len(gzip.decompress(outs["host"][k])) > 1000
        assert gzip.decompress(outs["device"][k]) == gzip.decompress(outs["host"][k])
        assert outs["device"][k] != outs["host"][k]
