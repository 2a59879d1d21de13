"""gzip input inflated on the device (csrc/k_inflate.hip: itsx_inflate_device, Engine.inflate = "device").  Truth is Python's gzip on the
same bytes (tests/inflate_cases.py).  In every test that expects the device to do the work a decline is a failure: Engine.inflate_device
raises, and the loader test asserts the context's counters, so nothing passes by quietly taking the host path.  The malformed inputs
are the ones tests/test_device_inflate_cpu.py has shown the same decoder to refuse inside exact-size buffers.  `pytest -m gpu`."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu


def _counters(engine):
    s = engine.stats()
    return s["n_inflate_device"], s["n_inflate_declined"]


def _small_good():
    return next(c for c in ic.good() if c[0] == "level9:259")


# ------------------------------------------------------------------ 1. the corpus
def test_corpus_on_the_device(engine, monkeypatch):
    monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB", raising=False)
    dev0, dec0 = _counters(engine)
    for name, gz, text in ic.good():
        assert engine.inflate_device(gz) == text, name
        assert engine.inflate_members == ic.n_members(name), name
    assert engine.stats()["ms_inflate"] > 0
    gz, text, members = ic.concatenation()
    assert gzip.decompress(gz) == text
    assert engine.inflate_device(gz) == text and engine.inflate_members == members
    s = engine.stats()
    assert s["ms_inflate"] > 0 and s["n_inflate_members"] == members
    assert engine.inflate_device(gz) == text                                  # again on the same bytes: the same text
    assert _counters(engine) == (dev0 + len(ic.good()) + 2, dec0)


# ------------------------------------------------------------------ 2. many members per workgroup, and the stale ring
GRID = 8


def _where(engine, n):
    w = np.zeros(n, np.int64)
    engine._chk(engine.L.itsx_debug_inflate_where(engine.h, w.ctypes.data, n))
    return [(int(x) >> 32, int(x) & 0xffffffff) for x in w]


def test_many_members_per_workgroup(engine, monkeypatch):
    """600 members on a launch of GRID workgroups (ITSX_INFLATE_GRID: the default launch is wider than any file a quick test can hold),
    so every workgroup decodes 75 in a row: the reset of the per-member state, the decoder begun again over the same LDS, and the ring
    that still holds the member before.  Which member ran where is what the kernel itself recorded (itsx_debug_inflate_where)."""
    monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB", raising=False)
    monkeypatch.setenv("ITSX_INFLATE_GRID", str(GRID))
    rng = np.random.default_rng(31)
    cases = [c for c in ic.good() if len(c[1]) <= 40000 and ic.n_members(c[0]) == 1]
    full = [c for c in ic.good() if len(c[2]) == 65536 and c[0].split(":")[0] in ("level1", "level9", "fixed")]
    assert len(full) == 3
    base = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))

    def reaches_back(k):
        """k literals, then a match at distance k: the largest this member's own text allows, while the ring holds the member before"""
        b, text = ic.Bits(), bytearray()
        blk = ic.fixed_block(b, text)
        blk.lits(base[:k])
        blk.match(258, k)
        blk.eob()
        return ic.wrap(b.done(), bytes(text)), bytes(text)
    parts, texts, kinds = [], [], []
    ks = [1, 2, 3, 257, 32767, 32768]
    while len(parts) < 600:
        if len(parts) % 25 == 0:                                              # a full-window member, and after it in the file one that reaches back
            _, gz, text = full[(len(parts) // 25) % 3]
            parts.append(gz)
            texts.append(text)
            kinds.append("full")
            gz, text = reaches_back(ks[(len(parts) // 25) % len(ks)])
            kinds.append("back")
        else:
            _, gz, text = cases[int(rng.integers(0, len(cases)))]
            kinds.append("other")
        parts.append(gz)
        texts.append(text)
    n = len(parts)
    gz, text = b"".join(parts), b"".join(texts)
    assert gzip.decompress(gz) == text
    assert engine.inflate_device(gz) == text and engine.inflate_members == n >= 600
    where = _where(engine, n)
    groups = {}
    for i, (wg, seq) in enumerate(where):
        groups.setdefault(wg, []).append((seq, i))
    assert sorted(groups) == list(range(GRID))
    backs = 0
    for wg, members in groups.items():
        members.sort()
        assert [seq for seq, _ in members] == list(range(len(members))) and len(members) >= n // GRID      # several in a row, none twice
        seen_full = False
        for seq, i in members:
            if kinds[i] == "back":
                assert seen_full and seq > 0, (wg, seq, i)                     # the ring it met had been filled by a 65 536-byte member
                backs += 1
            seen_full = seen_full or kinds[i] == "full"
    assert backs == kinds.count("back") >= 24
    print("600 members on %d workgroups: %d -> %d bytes, kernels %.2f ms" % (GRID, len(gz), len(text), engine.stats()["ms_inflate"]))
    # and the default launch gives the same text
    monkeypatch.delenv("ITSX_INFLATE_GRID")
    assert engine.inflate_device(gz) == text
    assert len({wg for wg, _ in _where(engine, n)}) > GRID


# ------------------------------------------------------------------ 3. the project's own files
def test_the_projects_own_files_round_trip(engine, tmp_path, monkeypatch):
    from itsxpress_amd.trim import write_trimmed_fastq
    monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB", raising=False)
    B = int(engine.L.itsx_deflate_block_bytes())
    rng = np.random.default_rng(32)
    # the seams of tests/test_gpu_device_deflate.py, its window edges (the device deflate emits distance 32768 there), and 3 B zeros
    sizes = [0, 1, 2, 3, 4, B - 1, B, B + 1, 0, 0, 2 * B + 1]
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = ic.fastq_like(rng, int(bounds[-1]))
    word = bytes(rng.integers(128, 256, 40, dtype=np.uint8))
    fill = b"abcdefg" * 6000
    edges = [fill[:100] + word + fill[:d - 40] + word + fill[:700] for d in (32768, 32769)]
    tail = bytes(rng.integers(0, 256, 1024, dtype=np.uint8))
    edges.append((fill * 2)[:B - 1024] + tail + tail + fill[:3000])
    for tag, d, b in [("seams", data, bounds), ("edges", b"".join(edges), np.concatenate([[0], np.cumsum([len(t) for t in edges])]).astype(np.int64)),
                      ("zeros", bytes(3 * B), np.array([0, 3 * B], np.int64))]:
        out = engine.deflate_device(d, b)
        for r, z in enumerate(out):
            want = d[int(b[r]):int(b[r + 1])]
            assert engine.inflate_device(z) == want, (tag, r)
            assert engine.inflate_members == max(1, -(-len(want) // B)), (tag, r)
        assert engine.inflate_device(b"".join(out)) == d, tag                   # and the ranges' files one after another
    # the host BlockWriter: 1 MB of records in 64 KiB blocks
    text = ic.fastq_like(rng, 1 << 20)
    text = text[:text.rindex(b"\n@read") + 1]
    n = text.count(b"\n") // 4
    src = tmp_path / "in.fq"
    src.write_bytes(text)
    monkeypatch.setenv("ITSX_IO_BLOCK_KB", "64")
    monkeypatch.setenv("ITSX_WRITE_MIN_MB", "4096")                            # the BlockWriter itself, not the pool of the unit writer
    dst = str(tmp_path / "out.fq.gz")
    write_trimmed_fastq(str(src), dst, np.zeros(n, np.int32), np.full(n, 1 << 30, np.int32), gzipped=True)
    z = open(dst, "rb").read()
    assert gzip.decompress(z) == text
    assert engine.inflate_device(z) == text and engine.inflate_members == -(-len(text) // 65536) == 16


# ------------------------------------------------------------------ 4. declines
def test_declines(engine, monkeypatch):
    from itsxpress_amd import EngineError
    monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB", raising=False)
    _, good_gz, good_text = _small_good()
    dev0, dec0 = _counters(engine)
    declined = 0

    def must_decline(gz, tag, reason=None):
        nonlocal declined
        with pytest.raises(EngineError) as ei:
            engine.inflate_device(gz)
        assert ei.value.code == -5 and "declined" in ei.value.message, (tag, ei.value.message)
        if isinstance(reason, tuple):                                          # the refusals the case was built to meet (inflate_cases.REASON)
            assert any(ic.REASON[r][1] in ei.value.message for r in reason), (tag, reason, ei.value.message)
        elif reason:
            assert reason in ei.value.message, (tag, ei.value.message)
        declined += 1
        assert engine.L.itsx_inflate_fetch(engine.h, None, 0) == -1, tag       # nothing half-made is left behind
        assert engine.inflate_device(good_gz) == good_text, tag                 # and the context goes on
    for name, gz, _, reasons in ic.bad():
        assert ic.zlib_refuses(gz), name
        must_decline(gz, name, reasons)
    gz, inner = ic.nested()
    must_decline(gz, "nested")
    must_decline(b"@r\nACGT\n+\nIIII\n", "plain text", "not gzip")
    big = next(g for n, g, _ in ic.good() if n == "level0:200000")
    assert engine.inflate_device(big) == next(t for n, _, t in ic.good() if n == "level0:200000")
    monkeypatch.setenv("ITSX_INFLATE_MEMBER_KB", "64")
    must_decline(big, "a 200 KB member against a cap of 64 KiB", "member too long")
    monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB")
    assert _counters(engine) == (dev0 + declined + 1, dec0 + declined)


# ------------------------------------------------------------------ 5. the loaders
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the four files of tests/test_gpu_device_deflate.py::loaded (1023, 1024, 1025 and 0 reads, the second with CRLF line ends, the third
    holding one 65 535-base read) as plain text, with the coordinates of its writer test"""
    from test_gpu_device_deflate import _sample, _scan_tile
    d = str(tmp_path_factory.mktemp("inflate_in"))
    tile = _scan_tile()
    rng = np.random.default_rng(78)
    sizes = [tile - 1, tile, tile + 1, 0]
    files, starts, stops = [], [], []
    for k, n in enumerate(sizes):
        recs, a, b = _sample(rng, n, "s%d_" % k, long_at=500 if k == 2 else None)
        eol = "\r\n" if k == 1 else "\n"
        p = os.path.join(d, "in_%d.fq" % k)
        with open(p, "w", newline="") as f:
            f.write("".join("@%s%s%s%s+%s%s%s" % (t, eol, s, eol, eol, q, eol) for t, s, q in recs))
        files.append(p)
        starts.append(a)
        stops.append(b)
    assert sizes[:3] == [1023, 1024, 1025]
    return dict(dir=d, files=files, sizes=sizes, start=np.concatenate(starts), stop=np.concatenate(stops))


def _unique_seqs(engine):
    uo = np.zeros(engine.n_unique + 1, np.int64)
    engine._chk(engine.L.itsx_get_unique_seqs(engine.h, None, 0, uo.ctypes.data))
    buf = C.create_string_buffer(int(uo[-1]) + 1)
    engine._chk(engine.L.itsx_get_unique_seqs(engine.h, buf, int(uo[-1]), uo.ctypes.data))
    return buf.raw[:int(uo[-1])], uo.tolist()


def _short(files):
    """the files without the one that holds the 65 535-base read (a dereplication with it takes seconds, whatever inflated the file)"""
    return [files[0], files[1], files[3]]


def _load(engine, files, inputs, outdir, tag):
    """everything a load leaves that the later stages read: the four files with their records kept and written out again, then the
    three without the long read once more, dereplicated"""
    from itsxpress_amd.trim import cache_clear
    cache_clear()                                                             # a cached text would be handed back without any inflate
    engine.keep_records(True)
    try:
        counts = [int(x) for x in engine.load_reads_files(files)]
    finally:
        engine.keep_records(False)
    names = engine.read_names()
    outs = [os.path.join(outdir, "%s_%d.fq" % (tag, k)) for k in range(len(files))]
    ret = engine.write_trimmed_samples(outs, start=inputs["start"], stop=inputs["stop"])
    cache_clear()
    counts3 = [int(x) for x in engine.load_reads_files(_short(files))]
    engine.derep()
    seqs = _unique_seqs(engine)
    derep = [a.tolist() for a in engine.get_derep()]
    return dict(counts=counts, counts3=counts3, names=names, seqs=seqs, derep=derep, ret=[tuple(r) for r in ret], written=[open(p, "rb").read() for p in outs])


def _member_spans(engine, gz):
    pos = np.zeros(4096, np.int64)
    n = int(engine.L.itsx_debug_inflate_candidates(gz, len(gz), pos.ctypes.data, 4096))
    assert 0 < n <= 4096
    edges = [int(x) for x in pos[:n]] + [len(gz)]
    return [b - a for a, b in zip(edges, edges[1:])]


def test_loaders(engine, inputs, tmp_path, monkeypatch):
    from itsxpress_amd.trim import write_trimmed_fastq, cache_clear
    for v in ("ITSX_DEVICE_INFLATE", "ITSX_INFLATE_MEMBER_KB", "ITSX_INFLATE_GRID", "ITSX_IO_BLOCK_KB", "ITSX_WRITE_MIN_MB", "ITSX_DEVICE_DEFLATE"):
        monkeypatch.delenv(v, raising=False)
    texts = [open(p, "rb").read() for p in inputs["files"]]
    d = str(tmp_path)
    ways = {"python": [], "device": [], "host": []}
    for k, t in enumerate(texts):
        cut = [0, len(t) // 3, 2 * len(t) // 3, len(t)]
        for way in ways:
            p = os.path.join(d, "%s_%d.fq.gz" % (way, k))
            if way == "python":
                z = b"".join(gzip.compress(t[cut[j]:cut[j + 1]]) for j in range(3))
            elif way == "device":
                z = engine.deflate_device(t, [0, len(t)])[0]
            else:
                z = None
                n = inputs["sizes"][k]
                if k == 1 or n == 0:                                          # (the writer rewrites CRLF, and writes nothing of no records:
                    z = b"".join(ic.member(t[o:o + 70000], 6, 0) for o in range(0, max(len(t), 1), 70000))          # the host's codec directly)
                else:
                    monkeypatch.setenv("ITSX_IO_BLOCK_KB", "64")
                    monkeypatch.setenv("ITSX_WRITE_MIN_MB", "4096")          # (the BlockWriter itself, not the pool of the unit writer)
                    write_trimmed_fastq(inputs["files"][k], p, np.zeros(n, np.int32), np.full(n, 1 << 30, np.int32), gzipped=True)
                    monkeypatch.delenv("ITSX_IO_BLOCK_KB")
                    monkeypatch.delenv("ITSX_WRITE_MIN_MB")
            if z is not None:
                with open(p, "wb") as f:
                    f.write(z)
            assert gzip.decompress(open(p, "rb").read()) == t, (way, k)
            ways[way].append(p)
    cache_clear()
    engine.inflate = "host"
    ref = _load(engine, inputs["files"], inputs, d, "plain")                   # plain files: untouched and uncounted
    assert ref["counts"] == inputs["sizes"]
    base = _counters(engine)
    try:
        for way, files in ways.items():
            gzs = [open(p, "rb").read() for p in files]
            engine.inflate = "device"
            dev0, dec0 = _counters(engine)
            got = _load(engine, files, inputs, d, way + "_dev")
            assert _counters(engine) == (dev0 + 4 + 3, dec0), way              # every gzip file went through the device, both times
            engine.inflate = "host"
            dev1, dec1 = _counters(engine)
            host = _load(engine, files, inputs, d, way + "_host")
            assert _counters(engine) == (dev1, dec1), way                      # and with "host" none does
            for key in ref:
                assert got[key] == host[key] == ref[key], (way, key)
            # a cap of 1 KiB: the same reads, every file with a member above it declined (and inflated by the host)
            is_long = [max(_member_spans(engine, z)) > 1024 for z in gzs]
            long_files = sum(is_long) + sum(_short(is_long))
            assert long_files >= 5
            monkeypatch.setenv("ITSX_INFLATE_MEMBER_KB", "1")
            engine.inflate = "device"
            capped = _load(engine, files, inputs, d, way + "_cap")
            monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB")
            assert _counters(engine) == (dev1 + 7 - long_files, dec1 + long_files), way
            assert all(capped[key] == ref[key] for key in ref), way
            engine.inflate = "host"
        # the switch alone takes the device path
        dev0, dec0 = _counters(engine)
        monkeypatch.setenv("ITSX_DEVICE_INFLATE", "1")
        got = _load(engine, ways["device"], inputs, d, "switch")
        monkeypatch.delenv("ITSX_DEVICE_INFLATE")
        assert _counters(engine) == (dev0 + 7, dec0) and all(got[key] == ref[key] for key in ref)
        # a plain file and a .zst file are not the device's: untouched and uncounted
        engine.inflate = "device"
        dev0, dec0 = _counters(engine)
        files = list(inputs["files"])
        if engine.L.itsx_io_codecs() & 2:
            zst = os.path.join(d, "in_0.fq.zst")
            n = inputs["sizes"][0]
            write_trimmed_fastq(inputs["files"][0], zst, np.zeros(n, np.int32), np.full(n, 1 << 30, np.int32), zstd_file=True)
            files[0] = zst
        else:
            print("no libzstd in this process: the .zst file is left out")
        got = _load(engine, files, inputs, d, "other")
        assert _counters(engine) == (dev0, dec0) and all(got[key] == ref[key] for key in ref)
        # a well-formed file the device must decline, not mis-decode: a level-0 member whose text holds a complete gzip member (here in
        # a read's title), a real header inside a stored block.  The raw call declines; the loader falls back and loads the right reads.
        from itsxpress_amd import EngineError
        inner = ic.member(b"x", 6, 0)
        assert not set(inner) & set(b"\n\r \t")
        text = b"@r1\nACGT\n+\nIIII\n@r2" + inner + b"\nTTGCA\n+\nIIIII\n"
        nested = ic.member(text, 0, 0)
        assert gzip.decompress(nested) == text and len(_member_spans(engine, nested)) == 2
        with pytest.raises(EngineError) as ei:
            engine.inflate_device(nested)
        assert ei.value.code == -5
        p = os.path.join(d, "nested.fq.gz")
        with open(p, "wb") as f:
            f.write(nested)
        loads = []
        for where in ("device", "host"):
            engine.inflate = where
            cache_clear()
            dev0, dec0 = _counters(engine)
            n = engine.load_reads_file(p)
            assert _counters(engine) == (dev0, dec0 + (where == "device"))
            engine.derep()
            loads.append((n, engine.read_names_raw()[0], _unique_seqs(engine)))
        assert loads[0] == loads[1] and loads[0][0] == 2 and loads[0][1].startswith(b"r1") and inner in loads[0][1]
    finally:
        engine.inflate = "host"
    # with neither the setting nor the switch both counters stay where they are
    dev0, dec0 = _counters(engine)
    _load(engine, ways["python"], inputs, d, "default")
    assert _counters(engine) == (dev0, dec0)


def test_a_fresh_context_counts_nothing_by_default(inputs, tmp_path):
    from itsxpress_amd import Engine
    from itsxpress_amd.trim import cache_clear
    p = str(tmp_path / "a.fq.gz")
    with open(p, "wb") as f:
        f.write(gzip.compress(open(inputs["files"][0], "rb").read()))
    e = Engine(0)
    try:
        cache_clear()
        assert e.inflate == "host" and e.load_reads_file(p) == inputs["sizes"][0]
        assert _counters(e) == (0, 0)
    finally:
        e.close()


# ------------------------------------------------------------------ 6. arguments
def test_arguments(monkeypatch):
    from itsxpress_amd import Engine
    monkeypatch.delenv("ITSX_INFLATE_MEMBER_KB", raising=False)
    e = Engine(0)
    try:
        L = e.L
        _, gz, text = _small_good()
        n, m = C.c_int64(-1), C.c_int64(-1)
        out = np.zeros(len(text) + 8, np.uint8)
        assert L.itsx_inflate_fetch(e.h, out.ctypes.data, out.size) == -1                       # a fetch before any inflate
        assert L.itsx_inflate_device(e.h, gz, 0, C.byref(n), C.byref(m)) == -5                  # no bytes: not gzip
        assert L.itsx_inflate_device(e.h, None, len(gz), C.byref(n), C.byref(m)) == -1
        assert L.itsx_inflate_device(None, gz, len(gz), C.byref(n), C.byref(m)) == -1
        assert L.itsx_inflate_device(e.h, gz, len(gz), C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (len(text), 1)
        assert L.itsx_inflate_fetch(e.h, out.ctypes.data, len(text) - 1) == -1                  # out_cap one short
        assert L.itsx_inflate_fetch(e.h, out.ctypes.data, len(text)) == 0 and out[:len(text)].tobytes() == text
        assert e.inflate == "host"
        with pytest.raises(ValueError):
            e.inflate = "gpu"
        assert e.inflate == "host"
        e.inflate = "device"
        assert e.inflate == "device"
    finally:
        e.close()
