"""gzip output deflated on the device (csrc/k_deflate.hip: itsx_deflate_device, compression == 3 of the batch writers, Engine.deflate =
"device").  Every output is checked three ways: Python's gzip takes it, the project's own reader (libdeflate / pinflate.cpp; both verify
every member's CRC-32 and ISIZE) takes it, and what comes out is the input.  `pytest -m gpu`."""
import gzip
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGTN", "TGCAN")
_ACGT = np.array(list("ACGT"))
_LENS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]
_LONG = 65535


def _B(engine):
    return int(engine.L.itsx_deflate_block_bytes())


def _members(n, B):
    return max(1, -(-n // B))


def _roundtrip(engine, tmp_path, data, bounds, tag):
    """deflate_device over the ranges; each range's bytes through both decoders; returns the compressed ranges"""
    from itsxpress_amd.trim import read_text
    out = engine.deflate_device(data, bounds)
    assert len(out) == len(bounds) - 1
    for r, z in enumerate(out):
        want = data[bounds[r]:bounds[r + 1]]
        assert z[:4] == b"\x1f\x8b\x08\x00", (tag, r)
        assert gzip.decompress(z) == want, (tag, r, len(want))
        p = str(tmp_path / ("%s_%d.gz" % (tag, r)))
        with open(p, "wb") as f:
            f.write(z)
        assert read_text(p) == want, (tag, r, len(want))
    return out


def _fastq_like(rng, nbytes):
    parts, have = [], 0
    i = 0
    while have < nbytes:
        L = int(rng.integers(50, 301))
        rec = "@read%d len=%d\n%s\n+\n%s\n" % (i, L, "".join(_ACGT[rng.integers(0, 4, L)]), "".join(chr(c) for c in rng.integers(35, 74, L)))
        parts.append(rec)
        have += len(rec)
        i += 1
    return "".join(parts).encode()[:nbytes]


def _fib(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


# ------------------------------------------------------------------ the coder by itself
def test_ranges_and_block_seams(engine, tmp_path):
    B = _B(engine)
    sizes = [0, 1, 2, 3, 4, B - 1, B, B + 1, 0, 0, 2 * B + 1]
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = _fastq_like(np.random.default_rng(1), int(bounds[-1]))
    out = _roundtrip(engine, tmp_path, data, bounds, "seams")
    for r, n in enumerate(sizes):
        if n == 0:                                                # an empty range: one member, an empty text, no more than a member's frame
            assert gzip.decompress(out[r]) == b"" and len(out[r]) <= 18 + 5
        if n > 1000:
            assert len(out[r]) < n
    # members per range: a range of n bytes is ceil(n / B) members, none across a range's end
    for r, n in enumerate(sizes):
        assert out[r].count(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff") >= _members(n, B)


def test_long_runs(engine, tmp_path):
    B = _B(engine)
    rng = np.random.default_rng(2)
    p258 = bytes(rng.integers(0, 256, 258, dtype=np.uint8))
    p259 = bytes(rng.integers(0, 256, 259, dtype=np.uint8))
    texts = [bytes(3 * B), b"q" * 259, (p258 * 40)[:258 * 39 + 17], (p259 * 40)[:259 * 39 + 5]]
    bounds = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    out = _roundtrip(engine, tmp_path, b"".join(texts), bounds, "runs")
    # runs are matches, not literals: a coder of literals alone spends a bit a byte at the least on the zeros, and on the periodic
    # texts (258 / 259 random byte values, about 7.7 bits of order-0 entropy) nearly what they are
    assert len(out[0]) < 3 * B // 16 and len(out[2]) < len(texts[2]) // 2 and len(out[3]) < len(texts[3]) // 2


def test_window_edges(engine, tmp_path):
    B = _B(engine)
    assert B > 32768 + 200
    rng = np.random.default_rng(3)
    word = bytes(rng.integers(128, 256, 40, dtype=np.uint8))                 # the filler's alphabet is disjoint: a..g
    fill = b"abcdefg" * 6000

    def block(dist):
        t = fill[:100] + word + fill[:dist - 40] + word + fill[:700]
        assert t.index(word, 101) - 100 == dist and len(t) < B
        return t
    tail = bytes(rng.integers(0, 256, 1024, dtype=np.uint8))
    first = (fill * 2)[:B - 1024] + tail                                       # a whole block ...
    second = tail + fill[:3000]                                               # ... and one that starts with a copy of its last 1 KiB
    texts = [block(32768), block(32769), first + second]
    assert len(first) == B
    bounds = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    out = _roundtrip(engine, tmp_path, b"".join(texts), bounds, "window")
    # the member after the seam cannot have used the copy before it: its 1 KiB of random bytes costs about what it is
    z2 = out[2]
    cut = z2.index(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff", 10)
    assert gzip.decompress(z2[:cut]) == first and gzip.decompress(z2[cut:]) == second and len(z2) - cut > 1000


def test_code_length_limit_on_the_device(engine, tmp_path):
    rng = np.random.default_rng(4)
    skew = np.concatenate([np.full(f, i, np.uint8) for i, f in enumerate(_fib(22))])
    rng.shuffle(skew)
    every = np.frombuffer(_fastq_like(rng, 30000), np.uint8).copy()
    every[rng.choice(every.size, 256, replace=False)] = np.arange(256, dtype=np.uint8)
    assert len(set(every.tolist())) == 256 and skew.size == sum(_fib(22)) < _B(engine)
    texts = [skew.tobytes(), every.tobytes()]
    bounds = np.array([0, len(texts[0]), len(texts[0]) + len(texts[1])], np.int64)
    out = _roundtrip(engine, tmp_path, b"".join(texts), bounds, "limit")
    assert len(out[0]) < len(texts[0]) // 2 and len(out[1]) < len(texts[1])  # coded, not stored


def test_incompressible_input_costs_the_stored_form(engine, tmp_path):
    B = _B(engine)
    n = 2 * B + 7
    data = bytes(np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8))
    out = _roundtrip(engine, tmp_path, data, np.array([0, n], np.int64), "random")
    bound = n + 5 * -(-n // 65535) + 18 * _members(n, B)
    print("incompressible: %d bytes -> %d, bound %d" % (n, len(out[0]), bound))
    assert len(out[0]) <= bound
    assert len(out[0]) <= int(engine.L.itsx_deflate_bound(n, 1))


@pytest.fixture(scope="module")
def repeats():
    """3 000 records drawn from 8 distinct complete records of 200..460 bases"""
    rng = np.random.default_rng(6)
    recs = []
    for k in range(8):
        L = int(rng.integers(200, 461))
        recs.append("@rec%d\n%s\n+\n%s\n" % (k, "".join(_ACGT[rng.integers(0, 4, L)]), "".join(chr(c) for c in rng.integers(35, 74, L))))
    return "".join(recs[k] for k in rng.integers(0, 8, 3000)).encode()


def test_matches_are_used_and_the_bytes_are_the_same_every_run(engine, tmp_path, repeats):
    B = _B(engine)
    n = len(repeats)
    bounds = np.array([0, n], np.int64)
    out = _roundtrip(engine, tmp_path, repeats, bounds, "repeats")
    a = np.frombuffer(repeats, np.uint8)
    order0 = 0.0
    for o in range(0, n, B):
        c = np.bincount(a[o:o + B], minlength=256).astype(np.float64)
        c = c[c > 0]
        order0 += float(-(c * np.log2(c / c.sum())).sum()) / 8
    print("repeats: %d bytes -> %d (%.4f of the text), order-0 bound %.0f (%.4f)" % (n, len(out[0]), len(out[0]) / n, order0, order0 / n))
    assert len(out[0]) < order0 / 2                                            # no Huffman-only coder gets below order0 itself
    again = engine.deflate_device(repeats, bounds)
    assert again[0] == out[0]


def test_arguments(engine):
    from itsxpress_amd import EngineError
    L = engine.L
    data = b"ACGT" * 100
    b = np.array([0, 400], np.int64)
    out = np.zeros(1000, np.uint8)
    ob = np.zeros(2, np.int64)
    assert L.itsx_deflate_bound(400, 1) > 400
    assert L.itsx_deflate_device(engine.h, data, 400, b.ctypes.data, 1, out.ctypes.data, int(L.itsx_deflate_bound(400, 1)) - 1, ob.ctypes.data) == -1
    with pytest.raises(EngineError):
        engine.deflate_device(data, [0, 500])
    with pytest.raises(EngineError):
        engine.deflate_device(data, [0, 300, 200, 400])
    assert engine.deflate_device(b"", [0]) == [] and [gzip.decompress(z) for z in engine.deflate_device(b"", [0, 0, 0])] == [b"", b""]


# ------------------------------------------------------------------ the batch writers
def _scan_tile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "itsxpress_amd", "csrc", "k_trim.hip")) as f:
        src = f.read()
    return int(re.search(r"TR_BLOCK = (\d+);", src).group(1)) * int(re.search(r"TR_ITEMS = (\d+);", src).group(1))


def _sample(rng, n, tag, long_at=None):
    """n records and their coordinates, as tests/test_gpu_batch_trim.py draws them: every (trimmed length, start) combination, and in
    odd blocks of 88 reads the coordinates that are clamped, empty or not written"""
    alpha = np.array(list("ACGTACGTACGTacgtNRYKMSWBDHVnrykmswbdhv"))
    recs, start, stop = [], [], []
    for i in range(n):
        tl, st = _LENS[i % 11], (i // 11) % 8
        kind = i % 7 if (i // 88) % 2 else 0
        L = st + tl + (i % 3 if kind == 0 else 0)
        a, b = st, st + tl
        if kind == 1:
            b = st + tl + 5
        elif kind == 2:
            b = a
        elif kind == 3:
            a, b = st + tl, st
        elif kind == 4:
            a = -1
        elif kind == 5:
            b = -1
        elif kind == 6:
            a, b = L + 2, L + 9
        if i == long_at:
            L, a, b = _LONG, 3, _LONG - 5
        want = 2 + (i * 7) % 79
        ident = ("%s%d" % (tag, i))[:want - 1]
        if i % 2 and want - 1 - len(ident) >= 2:
            title = ident + " " + "c" * (want - 2 - len(ident))
        else:
            title = ident + "x" * (want - 1 - len(ident))
        seq = "".join(alpha[rng.integers(0, len(alpha), L)])
        qual = "".join(chr(c) for c in rng.integers(35, 64, L))
        recs.append((title, seq, qual))
        start.append(a)
        stop.append(b)
    return recs, np.array(start, np.int32), np.array(stop, np.int32)


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """four samples whose sizes straddle the plan's tile (tile - 1, tile, tile + 1, 0 reads), the second file with CRLF line ends, the
    third holding one 65 535-base read, and per trim_ccs the host writer's output for every sample"""
    from itsxpress_amd.trim import write_trimmed_fastq
    d = str(tmp_path_factory.mktemp("deflate_in"))
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
    ref = {}
    for ccs in (0, 1):
        outs, ret = [], []
        for k, p in enumerate(files):
            o = os.path.join(d, "ref_%d_%d.fq" % (ccs, k))
            ret.append(write_trimmed_fastq(p, o, starts[k], stops[k], trim_ccs=bool(ccs)))
            outs.append(open(o, "rb").read())
        ref[ccs] = (outs, ret)
    assert b"\r" not in ref[0][0][1] and ref[0][0][3] == b"" and len(ref[0][0][2]) > 2 * _LONG and sizes[:3] == [1023, 1024, 1025]
    return dict(files=files, start=np.concatenate(starts), stop=np.concatenate(stops), sizes=sizes, ref=ref)


def _decoded(path):
    from itsxpress_amd.trim import read_text
    raw = open(path, "rb").read()
    assert raw[:3] == b"\x1f\x8b\x08"
    text = gzip.decompress(raw)
    assert text == read_text(path)
    return text


def test_batch_writer(engine, loaded, tmp_path, monkeypatch):
    monkeypatch.delenv("ITSX_DEVICE_DEFLATE", raising=False)
    engine.keep_records(True)
    try:
        counts = engine.load_reads_files(loaded["files"])
    finally:
        engine.keep_records(False)
    assert list(counts) == loaded["sizes"]
    a, b = loaded["start"], loaded["stop"]
    raw = {}
    try:
        engine.deflate = "device"
        for ccs in (0, 1):
            outs = [str(tmp_path / ("d%d_%d.fq.gz" % (ccs, k))) for k in range(4)]
            ret = engine.write_trimmed_samples(outs, start=a, stop=b, gzipped=True, trim_ccs=bool(ccs))
            exp, exp_ret = loaded["ref"][ccs]
            for k in range(4):
                assert _decoded(outs[k]) == exp[k], (ccs, k)
                assert tuple(ret[k]) == tuple(exp_ret[k]), (ccs, k)                # counts and total_len
            assert _decoded(outs[3]) == b""                                        # the empty sample: a valid gzip file of an empty text
            raw[ccs] = [open(p, "rb").read() for p in outs]
        assert engine.stats()["ms_deflate"] > 0
        # the text is smaller than its plain form, and a None path is skipped while the others are what they were
        assert sum(len(z) for z in raw[0]) < sum(len(t) for t in loaded["ref"][0][0])
        outs = [str(tmp_path / ("n_%d.fq.gz" % k)) for k in range(4)]
        engine.write_trimmed_samples([outs[0], None, outs[2], outs[3]], start=a, stop=b, gzipped=True)
        assert not os.path.exists(outs[1]) and [open(outs[k], "rb").read() for k in (0, 2, 3)] == [raw[0][k] for k in (0, 2, 3)]
        # the device makes gzip: no zstd, no plain output
        for kw in (dict(zstd_file=True), dict(), dict(gzipped=True, zstd_file=True)):
            with pytest.raises(ValueError, match="device"):
                engine.write_trimmed_samples(outs, start=a, stop=b, **kw)
    finally:
        engine.deflate = "host"
    with pytest.raises(ValueError):
        engine.deflate = "gpu"
    # the switch alone takes the same path: the same bytes
    monkeypatch.setenv("ITSX_DEVICE_DEFLATE", "1")
    outs = [str(tmp_path / ("e_%d.fq.gz" % k)) for k in range(4)]
    engine.write_trimmed_samples(outs, start=a, stop=b, gzipped=True)
    assert [open(p, "rb").read() for p in outs] == raw[0]
    monkeypatch.delenv("ITSX_DEVICE_DEFLATE")
    # and without either the host's deflate writes what it always wrote: other bytes, the same text
    engine.write_trimmed_samples(outs, start=a, stop=b, gzipped=True)
    assert [open(p, "rb").read() for p in outs] != raw[0] and [_decoded(p) for p in outs] == loaded["ref"][0][0]


# ------------------------------------------------------------------ paired
def _rc(s):
    return s[::-1].translate(_COMP)


def _overlapping_pairs(rng, frags, name):
    """one pair per fragment, as tests/test_gpu_batch_trim_pairs.py cuts them from the fixture's reads"""
    r1, r2 = [], []
    for i, frag in enumerate(frags):
        L = len(frag)
        fl, rl = int(rng.integers(L // 2 + 8, L)), int(rng.integers(L // 2 + 8, L))
        f, r = list(frag[:fl]), list(_rc(frag[L - rl:]))
        for s in (f, r):
            if rng.random() < 0.3:
                s[int(rng.integers(0, len(s)))] = str(_ACGT[rng.integers(0, 4)])
        label = "%s%05d" % (name, i)
        r1.append((label + " 1:N:0", "".join(f), "".join(chr(33 + int(x)) for x in rng.integers(25, 41, fl))))
        r2.append((label + " 2:N:0", "".join(r), "".join(chr(33 + int(x)) for x in rng.integers(25, 41, rl))))
    return r1, r2


def _write_fastq(path, recs):
    with open(path, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % r for r in recs))
    return path


def test_paired_batch(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from bench import its2_profiles
    from itsxpress_amd import EngineError
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    monkeypatch.delenv("ITSX_DEVICE_DEFLATE", raising=False)
    rng = np.random.default_rng(9)
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    seqs = [lines[k + 1].upper() for k in range(0, len(lines) - 3, 4) if set(lines[k + 1].upper()) <= set("ACGT")]
    assert len(seqs) > 150
    d = str(tmp_path / "in")
    os.makedirs(d)
    u1 = [("un%02d" % i, "".join(_ACGT[rng.integers(0, 4, 120)]), "I" * 120) for i in range(40)]          # unrelated mates: nothing merges
    u2 = [("un%02d" % i, "".join(_ACGT[rng.integers(0, 4, 110)]), "I" * 110) for i in range(40)]
    pairs = [_overlapping_pairs(rng, seqs[:70], "a"), (u1, u2), _overlapping_pairs(rng, seqs[70:150], "c")]
    files = [(_write_fastq(os.path.join(d, "m%d_R1.fq" % k), p1), _write_fastq(os.path.join(d, "m%d_R2.fq" % k), p2)) for k, (p1, p2) in enumerate(pairs)]
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    bd = str(tmp_path / "batch")
    os.makedirs(bd)

    def batch(keep, tag):
        objs = [SeqSamplePairedNotInterleaved(fastq=r1, tempdir=bd, fastq2=r2) for r1, r2 in files]
        b = SampleBatch(objs, engine=engine, subdirs=["%s%d" % (tag, k) for k in range(3)], keep_records=keep)
        b.merge_reads(threads=1)
        b.deduplicate(threads=1)
        b._search(hmmfile=str(hmm), threads=1)
        return b

    def paths(tag, ext):
        return ([os.path.join(bd, "%s_%d_R1.%s" % (tag, k, ext)) for k in range(3)], [os.path.join(bd, "%s_%d_R2.%s" % (tag, k, ext)) for k in range(3)])

    b = batch("pairs", "pairs")
    assert b.deflate == "host"
    try:
        b.deflate = "device"
        assert engine.deflate == "device"
        o1, o2 = paths("dev", "fq.gz")
        ret = b.write_paired_trimmed(o1, o2, "ITS2", gzipped=True)
        got = [(_decoded(p), _decoded(q)) for p, q in zip(o1, o2)]
        # an unwritable second path: neither file of that pair is left
        x1, x2 = paths("bad", "fq.gz")
        x2[0] = os.path.join(bd, "no_such_directory", "bad_0_R2.fq.gz")
        with pytest.raises(EngineError) as ei:
            b.write_paired_trimmed(x1, x2, "ITS2", gzipped=True)
        assert ei.value.code == -2 and not os.path.exists(x1[0]) and not os.path.exists(x2[0])
        with pytest.raises(ValueError, match="device"):
            b.write_paired_trimmed(x1, x2, "ITS2", zstd_file=True)
    finally:
        b.deflate = "host"
    h = batch(False, "files")                                     # the host writer, from the files
    e1, e2 = paths("host", "fq")
    exp_ret = h.write_paired_trimmed(e1, e2, "ITS2")
    exp = [(open(p, "rb").read(), open(q, "rb").read()) for p, q in zip(e1, e2)]
    assert got == exp and [int(x) for x in ret] == [int(x) for x in exp_ret]
    assert exp[1] == (b"", b"") and ret[0] > 20 and ret[2] > 20 and len(exp[0][0]) > 1000 and len(exp[2][1]) > 1000
