"""R1 / R2 parsed on the device for the paired merge loaders (csrc/k_fastq.hip: k_fastq_pairs; itsx_parse_pairs_device; merge_pairs_load,
merge_pairs_load_text and merge_pairs_load_files under Engine.parse = "device").  Truth for the raw entry is the Python model of
tests/fastq_pair_cases.py, which tests/test_device_parse_pairs_cpu.py holds the host twin to; truth for the loaders is the host / host arm of
the same call.  Every comparison is exact.  Where the device is expected to do the work the context's counters are asserted, so nothing
passes by quietly taking the host path.  `pytest -m gpu`."""
import ctypes as C
import gzip
import importlib
import os

import numpy as np
import pytest

import fastq_pair_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_SWITCHES = ("ITSX_DEVICE_INFLATE", "ITSX_DEVICE_PARSE", "ITSX_INFLATE_MEMBER_KB", "ITSX_INFLATE_GRID", "ITSX_IO_BLOCK_KB", "ITSX_WRITE_MIN_MB", "ITSX_DEVICE_DEFLATE")


def _parse_counters(engine):
    s = engine.stats()
    return s["n_parse_device"], s["n_parse_declined"]


def _inflate_counters(engine):
    s = engine.stats()
    return s["n_inflate_device"], s["n_inflate_declined"]


def _clean_env(monkeypatch):
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _unique_seqs(engine):
    uo = np.zeros(engine.n_unique + 1, np.int64)
    engine._chk(engine.L.itsx_get_unique_seqs(engine.h, None, 0, uo.ctypes.data))
    buf = C.create_string_buffer(int(uo[-1]) + 1)
    engine._chk(engine.L.itsx_get_unique_seqs(engine.h, buf, int(uo[-1]), uo.ctypes.data))
    return buf.raw[:int(uo[-1])], uo.tolist()


def _pairs(rng, n, tag, unmerged=7):
    """n pairs as records (title, bases, qualities) per side: overlapping mates of unlike lengths that merge, a few with a substitution,
    then `unmerged` unrelated mates; one empty read on either side"""
    r1, r2 = [], []
    for i in range(n):
        if i < n - unmerged:
            L = int(rng.integers(150, 261))
            frag = bytes(rng.choice(list(b"ACGT"), L).tolist())
            fl, rl = int(rng.integers(L // 2 + 8, L)), int(rng.integers(L // 2 + 8, L))
            f, r = bytearray(frag[:fl]), bytearray(frag[L - rl:][::-1].translate(_COMP))
            if rng.random() < 0.3:
                f[int(rng.integers(0, fl))] = b"ACGT"[int(rng.integers(0, 4))]
        else:
            f, r = bytes(rng.choice(list(b"ACGT"), 100 + i % 7).tolist()), bytes(rng.choice(list(b"ACGT"), 90 + i % 5).tolist())
        if i == 3:
            f = b""
        if i == 5:
            r = b""
        q = lambda k: bytes(rng.integers(58, 74, k, dtype=np.uint8).tolist())
        r1.append((b"%s%d 1:N:0" % (tag, i), bytes(f), q(len(f))))
        r2.append((b"%s%d\t2:N:0" % (tag, i), bytes(r), q(len(r))))
    return r1, r2


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def _merged_state(engine, tmp, tag):
    """what a merge load leaves for the later stages: names, the pair index, the unique sequences, the derep arrays and rep.fa"""
    names = engine.read_names()
    pidx = engine.merge_pair_index().tolist()
    engine.derep()
    rep = os.path.join(tmp, "%s_rep.fa" % tag)
    engine.write_rep_fasta(rep)
    return names, pidx, _unique_seqs(engine), [a.tolist() for a in engine.get_derep()], open(rep, "rb").read()


# ------------------------------------------------------------------ 1. the raw entry
def test_the_raw_entry_equals_the_model(engine):
    from itsxpress_amd import EngineError
    dev0, dec0 = _parse_counters(engine)
    for k, (name, t1, t2) in enumerate(pc.accepted()):
        model = pc.expected(t1, t2)[1]
        got = engine.parse_pairs_device(t1, t2)
        assert (got["n"], got["flags"], got["max_total"]) == (model["n"], model["flags"], model["max_total"]), name
        for side in (0, 1):
            g, m = got["sides"][side], model["sides"][side]
            assert g["off"].tolist() == m["off"] and g["toff"].tolist() == m["toff"], (name, side)
            assert g["seq"] == m["seq"] and g["qual"] == m["qual"] and g["titles"] == m["titles"], (name, side)
        assert _parse_counters(engine) == (dev0 + 2 * (k + 1), dec0), name
    assert engine.stats()["ms_parse"] > 0
    dev0, dec0 = _parse_counters(engine)
    good = next(c for c in pc.accepted() if c[0] == "lower case in R2 only")
    out = np.zeros(4, np.int64)
    for name, t1, t2 in pc.declined():
        _, why, side = pc.expected(t1, t2)
        with pytest.raises(EngineError) as ei:
            engine.parse_pairs_device(t1, t2)
        assert ei.value.code == -5 and "declined" in ei.value.message and pc.REASON[why][1] in ei.value.message, (name, ei.value.message)
        for s in (0, 1):                                                      # nothing is left to hand out,
            for plane in range(5):
                assert engine.L.itsx_parse_pairs_fetch(engine.h, s, plane, 0, 1, out.ctypes.data) == -1, name
        d1, c1 = _parse_counters(engine)                                      # the texts before the declined one were parsed, the declined one counted
        assert (d1 - dev0, c1 - dec0) == ((2, 0) if side < 0 else (side, 1)), name
        got = engine.parse_pairs_device(good[1], good[2])                     # and the context goes on to parse a good pair
        assert got["flags"] == pc.LOWER2 and got["sides"][1]["seq"] == pc.expected(good[1], good[2])[1]["sides"][1]["seq"]
        dev0, dec0 = _parse_counters(engine)


def test_the_raw_entrys_arguments():
    from itsxpress_amd import Engine
    e = Engine(0)
    try:
        L = e.L
        _, t1, t2 = next(c for c in pc.accepted() if c[0] == "R1 and R2 of unlike lengths")
        m = pc.expected(t1, t2)[1]
        n, fl, mx = C.c_int64(-1), C.c_int32(-1), C.c_int64(-1)
        tail = (C.byref(n), C.byref(fl), C.byref(mx))
        out = np.zeros(len(t1) + len(t2) + 8, np.uint8)
        assert L.itsx_parse_pairs_fetch(e.h, 0, 2, 0, 1, out.ctypes.data) == -1   # a fetch before any parse
        assert L.itsx_parse_pairs_device(None, t1, len(t1), t2, len(t2), *tail) == -1
        assert L.itsx_parse_pairs_device(e.h, None, len(t1), t2, len(t2), *tail) == -1
        assert L.itsx_parse_pairs_device(e.h, t1, len(t1), None, len(t2), *tail) == -1
        assert L.itsx_parse_pairs_device(e.h, t1, -1, t2, len(t2), *tail) == -1
        assert L.itsx_parse_pairs_device(e.h, t1, len(t1), t2, len(t2), None, tail[1], tail[2]) == -1
        assert L.itsx_parse_pairs_device(e.h, t1, len(t1), t2, len(t2), tail[0], None, tail[2]) == -1
        assert L.itsx_parse_pairs_device(e.h, t1, len(t1), t2, len(t2), tail[0], tail[1], None) == -1
        assert _parse_counters(e) == (0, 0)
        assert L.itsx_parse_pairs_device(e.h, t1, len(t1), t2, len(t2), *tail) == 0 and (n.value, fl.value, mx.value) == (m["n"], 0, m["max_total"])
        assert L.itsx_parse_fetch(e.h, 2, 0, 1, out.ctypes.data) == -1            # the single-text fetch has nothing of it
        assert L.itsx_parse_pairs_fetch(None, 0, 2, 0, 1, out.ctypes.data) == -1
        for side in (0, 1):
            s = m["sides"][side]
            for plane, size in ((0, m["n"] + 1), (1, m["n"] + 1), (2, len(s["seq"])), (3, len(s["seq"])), (4, len(s["titles"]))):
                assert L.itsx_parse_pairs_fetch(e.h, side, plane, 0, size + 1, out.ctypes.data) == -1, plane      # past the plane's end
                assert L.itsx_parse_pairs_fetch(e.h, side, plane, -1, size, out.ctypes.data) == -1, plane
                assert L.itsx_parse_pairs_fetch(e.h, side, plane, 2, 1, out.ctypes.data) == -1, plane
                assert L.itsx_parse_pairs_fetch(e.h, side, plane, 0, size, None) == -1, plane
                assert L.itsx_parse_pairs_fetch(e.h, side, plane, size, size, None) == 0, plane                    # an empty range needs no buffer
            assert L.itsx_parse_pairs_fetch(e.h, side, 5, 0, 1, out.ctypes.data) == -1 and L.itsx_parse_pairs_fetch(e.h, side, -1, 0, 1, out.ctypes.data) == -1
            assert e.parse_pairs_fetch(side, "seq", 1, len(s["seq"]) - 1) == s["seq"][1:-1] and e.parse_pairs_fetch(side, "off", 1, 3).tolist() == s["off"][1:3]
        assert L.itsx_parse_pairs_fetch(e.h, 2, 2, 0, 1, out.ctypes.data) == -1 and L.itsx_parse_pairs_fetch(e.h, -1, 2, 0, 1, out.ctypes.data) == -1
        assert L.itsx_parse_pairs_device(e.h, None, 0, None, 0, *tail) == 0 and (n.value, fl.value, mx.value) == (0, 0, 0)      # no text is a text of no bytes
        assert e.parse_pairs_fetch(1, "off", 0, 1).tolist() == [0] and e.parse_pairs_fetch(0, "seq", 0, 0) == b""
        assert _parse_counters(e) == (4, 0)
    finally:
        e.close()


# ------------------------------------------------------------------ 2. the single-sample loader
@pytest.fixture(scope="module")
def sample(engine, tmp_path_factory):
    """one paired sample (CRLF in R2) as plain text, python-gzip members and device-deflated members"""
    d = str(tmp_path_factory.mktemp("pairs_in"))
    rng = np.random.default_rng(41)
    r1, r2 = _pairs(rng, 300, b"q")
    texts = (pc.text_of(r1), pc.text_of(r2, b"\r\n"))
    files = {"plain": [], "python": [], "device": []}
    for side, t in enumerate(texts):
        cut = [0, len(t) // 3, 2 * len(t) // 3, len(t)]
        files["plain"].append(_write(os.path.join(d, "R%d.fq" % (side + 1)), t))
        files["python"].append(_write(os.path.join(d, "py_R%d.fq.gz" % (side + 1)), b"".join(gzip.compress(t[cut[j]:cut[j + 1]]) for j in range(3))))
        files["device"].append(_write(os.path.join(d, "dev_R%d.fq.gz" % (side + 1)), engine.deflate_device(t, [0, len(t)])[0]))
        for way in ("python", "device"):
            assert gzip.decompress(open(files[way][side], "rb").read()) == t
    return dict(dir=d, files=files, texts=texts, n=300)


def test_single_sample_loader(engine, sample, tmp_path, monkeypatch):
    from itsxpress_amd.trim import cache_clear
    _clean_env(monkeypatch)
    results = {}
    try:
        for way in ("plain", "python", "device"):
            for inflate in ("host", "device"):
                for parse in ("host", "device"):
                    engine.inflate, engine.parse = inflate, parse
                    cache_clear()                                             # a cached text would be handed back without any inflate
                    p0, i0 = _parse_counters(engine), _inflate_counters(engine)
                    n, m = engine.merge_pairs_load(*sample["files"][way])
                    # both texts went where the arm says, none was declined
                    assert _parse_counters(engine) == ((p0[0] + 2, p0[1]) if parse == "device" else p0), (way, inflate, parse)
                    took = 2 if inflate == "device" and way != "plain" else 0
                    assert _inflate_counters(engine) == (i0[0] + took, i0[1]), (way, inflate, parse)
                    results[way, inflate, parse] = (n, m) + _merged_state(engine, str(tmp_path), "%s_%s_%s" % (way, inflate, parse))
        want = results["plain", "host", "host"]
        assert want[0] == sample["n"] and sample["n"] - 40 < want[1] <= sample["n"] - 7 and len(want[6]) > 1000
        assert want[3].count(-1) == sample["n"] - want[1]
        for key, got in results.items():
            assert got == want, key
    finally:
        engine.inflate = engine.parse = "host"


# ------------------------------------------------------------------ 3. the batch loader, through a batch's stages to its files
def _batch_inputs(gold, d):
    """four samples of 1 023 / 1 024 / 1 025 / 0 pairs cut from the fixture's reads (so that the stand-in profiles find their ITS2), the
    second with CRLF line ends"""
    tp = importlib.import_module("test_gpu_batch_trim_pairs")
    rng = np.random.default_rng(12)
    seqs = [s.upper() for _, s, _ in tp._fixture_records(gold) if set(s.upper()) <= set("ACGT")]
    files = []
    for k, n in enumerate((1023, 1024, 1025, 0)):
        frags = []
        for i in range(n):
            s = list(seqs[(i * 7 + k) % len(seqs)])
            s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
            frags.append("".join(s))
        p1, p2 = tp._overlapping_pairs(rng, frags, "b%d_" % k) if n else ([], [])
        eol = "\r\n" if k == 1 else "\n"
        paths = []
        for side, recs in ((1, p1), (2, p2)):
            text = "".join("@%s%s%s%s+%s%s%s" % (t, eol, s, eol, eol, q, eol) for t, s, q in recs).encode()
            paths.append(_write(os.path.join(d, "b%d_R%d.fq" % (k, side)), text))
        files.append(tuple(paths))
    return files


def _run_batch(engine, files, hmm, bd, tag, inflate, parse, keep="pairs", seq_files=None):
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.trim import cache_clear
    S = len(files)
    cache_clear()
    objs = [SeqSamplePairedNotInterleaved(fastq=r1, tempdir=bd, fastq2=r2) for r1, r2 in files]
    b = SampleBatch(objs, engine=engine, subdirs=["%s%d" % (tag, k) for k in range(S)], keep_records=keep)
    b.inflate, b.parse = inflate, parse
    p0 = _parse_counters(engine)
    b.merge_reads(threads=1, write_seq_files=seq_files)
    moved = tuple(x - y for x, y in zip(_parse_counters(engine), p0))
    out = dict(moved=moved, n_pairs=[int(x) for x in b.n_pairs], counts=[int(x) for x in b.counts])
    if seq_files:
        out["seq"] = [open(o.seq_file, "rb").read() for o in objs]
        return out
    b.deduplicate(threads=1)
    b._search(hmmfile=hmm, threads=1)
    for kind, gz in (("plain", False), ("gz", True)):
        outs = [os.path.join(bd, "%s_%s_m%d.fq" % (tag, kind, k)) for k in range(S)]
        o1s = [os.path.join(bd, "%s_%s_%d_R1.fq" % (tag, kind, k)) for k in range(S)]
        o2s = [os.path.join(bd, "%s_%s_%d_R2.fq" % (tag, kind, k)) for k in range(S)]
        out["merged_" + kind] = ([tuple(int(v) for v in x) for x in b.write_trimmed(outs, "ITS2", gzipped=gz)], [open(p, "rb").read() for p in outs])
        out["paired_" + kind] = ([int(x) for x in b.write_paired_trimmed(o1s, o2s, "ITS2", gzipped=gz)], [(open(p, "rb").read(), open(q, "rb").read()) for p, q in zip(o1s, o2s)])
        out["ms_trim_copy"] = engine.stats()["ms_trim_copy"]
    return out


def test_batch_loader_through_the_batch_writers(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    from bench import its2_profiles
    _clean_env(monkeypatch)
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    d, bd = str(tmp_path / "in"), str(tmp_path / "batch")
    os.makedirs(d)
    os.makedirs(bd)
    files = _batch_inputs(gold, d)
    hmm = _write(str(tmp_path / "its2.hmm"), its2_profiles(t_hmm_text).encode())
    try:
        host = _run_batch(engine, files, hmm, bd, "h", "host", "host")
        dev = _run_batch(engine, files, hmm, bd, "d", "device", "device")
        assert host["moved"] == (0, 0) and dev["moved"] == (8, 0)
        assert host["n_pairs"] == [1023, 1024, 1025, 0] and all(c > 800 for c in host["counts"][:3]) and host["counts"][3] == 0
        assert dev["ms_trim_copy"] > 0                                        # the paired writer cut from the pair records on the device
        for key in host:
            if key not in ("moved", "ms_trim_copy"):
                assert dev[key] == host[key], key
        assert all(r > 300 for r in host["paired_plain"][0][:3]) and len(host["paired_plain"][1][1][0]) > 30000
        hs = _run_batch(engine, files, hmm, bd, "hs", "host", "host", seq_files=True)
        ds = _run_batch(engine, files, hmm, bd, "ds", "device", "device", seq_files=True)
        assert ds["moved"] == (8, 0) and ds["seq"] == hs["seq"] and ds["counts"] == hs["counts"] == host["counts"] and len(hs["seq"][0]) > 100000
    finally:
        engine.inflate = engine.parse = "host"


def test_a_batch_whose_samples_start_at_every_plane_offset(engine, tmp_path, monkeypatch):
    """17 samples whose bases end 1 (R1) and 3 (R2) past a multiple of 16: the gather writes every later sample from an unaligned byte"""
    from itsxpress_amd.trim import cache_clear
    _clean_env(monkeypatch)
    files = [(_write(str(tmp_path / ("o%d_R1.fq" % k)), a), _write(str(tmp_path / ("o%d_R2.fq" % k)), b)) for k, (a, b) in enumerate(pc.batch_at_every_offset())]
    got = {}
    try:
        for parse in ("host", "device"):
            engine.parse = parse
            cache_clear()
            p0 = _parse_counters(engine)
            engine.keep_pair_records(True)
            try:
                n, m = engine.merge_pairs_load_files([f[0] for f in files], [f[1] for f in files])
            finally:
                engine.keep_pair_records(False)
            assert _parse_counters(engine) == ((p0[0] + 34, p0[1]) if parse == "device" else p0)
            z = np.zeros(engine.n_reads, np.int32)
            o1, o2 = [str(tmp_path / ("%s_%d_1.fq" % (parse, k))) for k in range(17)], [str(tmp_path / ("%s_%d_2.fq" % (parse, k))) for k in range(17)]
            ret = engine.write_trimmed_paired_samples(o1, o2, start=z + 1, stop=z + 90, tlen=z + 100)      # the kept planes, cut on the device
            got[parse] = (n.tolist(), m.tolist(), _merged_state(engine, str(tmp_path), parse), list(ret), [(open(p, "rb").read(), open(q, "rb").read()) for p, q in zip(o1, o2)])
        assert got["host"] == got["device"] and got["host"][0] == [3] * 17 and sum(got["host"][1]) > 40 and sum(got["host"][3]) > 40
    finally:
        engine.parse = "host"


# ------------------------------------------------------------------ 4. lower case, and the fallbacks
def test_lower_case_in_one_r2_keeps_no_pair_records(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    import itsxpress_amd.trim as trim
    from bench import its2_profiles
    _clean_env(monkeypatch)
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    tp = importlib.import_module("test_gpu_batch_trim_pairs")
    rng = np.random.default_rng(13)
    seqs = [s.upper() for _, s, _ in tp._fixture_records(gold) if set(s.upper()) <= set("ACGT")]
    d, bd = str(tmp_path / "in"), str(tmp_path / "batch")
    os.makedirs(d)
    os.makedirs(bd)
    files = []
    for k, (lo, hi) in enumerate(((0, 60), (60, 120))):
        p1, p2 = tp._overlapping_pairs(rng, seqs[lo:hi], "l%d_" % k)
        if k == 1:                                                           # one lower-case base in one R2
            t, s, q = p2[17]
            p2[17] = (t, s[:30] + s[30].lower() + s[31:], q)
        files.append((tp._write_fastq(os.path.join(d, "l%d_R1.fq" % k), p1), tp._write_fastq(os.path.join(d, "l%d_R2.fq" % k), p2)))
    hmm = _write(str(tmp_path / "its2.hmm"), its2_profiles(t_hmm_text).encode())
    calls = []
    host_writer = trim.write_trimmed_paired

    def counted(*a, **kw):
        calls.append(1)
        return host_writer(*a, **kw)
    monkeypatch.setattr(trim, "write_trimmed_paired", counted)
    try:
        host = _run_batch(engine, files, hmm, bd, "h", "host", "host")
        assert len(calls) == 4                                               # the host loop: one call per sample, plain and gzipped
        del calls[:]
        dev = _run_batch(engine, files, hmm, bd, "d", "host", "device")
        assert dev["moved"] == (4, 0) and len(calls) == 4                    # parsed on the device all the same; no pair records, so the host writer
        for key in host:
            if key not in ("moved", "ms_trim_copy"):
                assert dev[key] == host[key], key
        assert host["paired_plain"][0][1] > 20 and len(host["paired_plain"][1][1][1]) > 1000
    finally:
        engine.parse = "host"


def test_fallbacks_give_the_host_paths_results_and_errors(engine, tmp_path, monkeypatch):
    from itsxpress_amd import EngineError
    from itsxpress_amd.trim import cache_clear
    _clean_env(monkeypatch)
    rng = np.random.default_rng(14)
    r1, r2 = _pairs(rng, 40, b"f")
    good = (_write(str(tmp_path / "good_R1.fq"), pc.text_of(r1)), _write(str(tmp_path / "good_R2.fq"), pc.text_of(r2)))

    def variant(tag, e1=None, e2=None, raw1=None, raw2=None):
        a, b = list(r1), list(r2)
        if e1:
            e1(a)
        if e2:
            e2(b)
        return (_write(str(tmp_path / (tag + "_R1.fq")), raw1(pc.text_of(a)) if raw1 else pc.text_of(a)), _write(str(tmp_path / (tag + "_R2.fq")), raw2(pc.text_of(b)) if raw2 else pc.text_of(b)))

    def blank_line(t):
        lines = t.split(b"\n")
        return b"\n".join(lines[:8]) + b"\n\n" + b"\n".join(lines[8:])

    def long_pair(side_len):
        return lambda recs: recs.__setitem__(2, (recs[2][0], b"A" * side_len, b"]" * side_len))

    # (the pair, what the device arm's counters move by, the error both arms raise or None)
    cases = [("blank", variant("blank", raw2=blank_line), (1, 1), None),
             ("unequal", variant("unequal", e2=lambda recs: recs.pop()), (2, 0), (-3, "different numbers of records")),
             ("qual32", variant("qual32", e1=lambda recs: recs.__setitem__(1, (recs[1][0], recs[1][1], b" " + recs[1][2][1:]))), (2, 0), (-3, "forward quality outside")),
             ("long", variant("long", e1=long_pair(6000), e2=long_pair(6001)), (2, 0), (-5, "longer than 12000")),
             ("malformed", variant("malformed", raw1=lambda t: b"@a\nACGT\n+\nIII\n" + t), (0, 1), (-3, "malformed FASTQ record"))]
    try:
        engine.parse = "host"
        cache_clear()
        n, m = engine.merge_pairs_load_files([good[0]], [good[1]])
        want_good = (n.tolist(), m.tolist(), _merged_state(engine, str(tmp_path), "good"))
        for tag, (p1, p2), moved, err in cases:
            seen = {}
            for parse in ("host", "device"):
                engine.parse = parse
                cache_clear()
                p0 = _parse_counters(engine)
                if err is None:
                    n, m = engine.merge_pairs_load_files([p1], [p2])
                    seen[parse] = (n.tolist(), m.tolist(), _merged_state(engine, str(tmp_path), tag + parse))
                else:
                    with pytest.raises(EngineError) as ei:
                        engine.merge_pairs_load_files([p1], [p2])
                    seen[parse] = (ei.value.code, ei.value.message)
                    assert seen[parse][0] == err[0] and err[1] in seen[parse][1], (tag, parse, seen[parse])
                    assert engine.n_reads == 0 and engine.read_names() == []          # the context is left empty
                got = tuple(x - y for x, y in zip(_parse_counters(engine), p0))
                assert got == (moved if parse == "device" else (0, 0)), (tag, parse, got)
                # ... and usable: a good load follows, on the device where the arm says so
                p0 = _parse_counters(engine)
                n, m = engine.merge_pairs_load_files([good[0]], [good[1]])
                assert (n.tolist(), m.tolist(), _merged_state(engine, str(tmp_path), tag + "_after_" + parse)) == want_good, (tag, parse)
                assert _parse_counters(engine) == ((p0[0] + 2, p0[1]) if parse == "device" else p0), (tag, parse)
            assert seen["host"] == seen["device"], tag
            if err is None:
                assert seen["host"][0] == [40] and seen["host"][1] == want_good[1]
    finally:
        engine.parse = "host"


# ------------------------------------------------------------------ 5. text slices
def test_text_slices(engine, sample, tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    t1, t2 = sample["texts"]
    got = {}
    try:
        for parse in ("host", "device"):
            engine.parse = parse
            p0 = _parse_counters(engine)
            n, m, idx = engine.merge_pairs_load_text(C.cast(t1, C.c_void_p).value, len(t1), C.cast(t2, C.c_void_p).value, len(t2))
            assert _parse_counters(engine) == ((p0[0] + 2, p0[1]) if parse == "device" else p0)
            got[parse] = (n, m, idx.tolist()) + _merged_state(engine, str(tmp_path), "text_" + parse)
            # a slice of no bytes on either side: no pairs, no reads
            p0 = _parse_counters(engine)
            assert engine.merge_pairs_load_text(C.cast(t1, C.c_void_p).value, 0, C.cast(t2, C.c_void_p).value, 0)[:2] == (0, 0)
            assert _parse_counters(engine) == ((p0[0] + 2, p0[1]) if parse == "device" else p0)
        assert got["host"] == got["device"] and got["host"][0] == sample["n"] and got["host"][1] > 250
    finally:
        engine.parse = "host"


# ------------------------------------------------------------------ 6. the streamed paired run
def test_streamed_paired_run_under_the_switch(tmp_path, t_hmm_text, gold, monkeypatch):
    """tests/test_gpu_stream.py's arrays-mode scenario on the reference's paired fixture (R1 / R2 streamed side by side, every pair of slices
    merged by its chunk's context through merge_pairs_load_text): the same two files with and without ITSX_DEVICE_PARSE=1"""
    from bench import its2_profiles
    S = importlib.import_module("itsxpress_amd.SeqSample")
    _clean_env(monkeypatch)
    tmp = str(tmp_path)
    hmm = _write(os.path.join(tmp, "its2.hmm"), its2_profiles(t_hmm_text).encode())
    raw = []
    for fn in ("4774-1-MSITS3_R1.fastq", "4774-1-MSITS3_R2.fastq"):
        with gzip.open(os.path.join(gold, fn + ".gz"), "rb") as f:
            raw.append(_write(os.path.join(tmp, fn), f.read()))
    monkeypatch.setenv("ITSX_STREAM_CHUNK_MB", "0.02")
    monkeypatch.setenv("ITSXPRESS_GPUS", "1")
    monkeypatch.setenv("ITSXPRESS_STREAM", "1")
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "1")
    outs = {}
    for name in ("host", "device"):
        if name == "device":
            monkeypatch.setenv("ITSX_DEVICE_PARSE", "1")
        d = os.path.join(tmp, name)
        os.makedirs(d)
        sobj = S.SeqSamplePairedNotInterleaved(fastq=raw[0], tempdir=d, fastq2=raw[1])
        try:
            o1, o2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
            sobj._merge_reads(threads=1)
            sobj.deduplicate(threads=1)
            sobj._search(hmmfile=hmm, threads=1)
            its_pos = S.ItsPosition(domtable=sobj.dom_file, region="ITS2")
            dd = S.Dedup(uc_file=sobj.uc_file, rep_file=sobj.rep_file, seq_file=sobj.seq_file, fastq=sobj.r1, fastq2=sobj.fastq2)
            dd.create_paired_trimmed_seqs(o1, o2, gzipped=False, zstd_file=False, itspos=its_pos, wri_file=True)
            outs[name] = (open(o1, "rb").read(), open(o2, "rb").read(), [np.asarray(c).tolist() for c in sobj.trim_coordinates("ITS2")], sobj._engine.n_pairs, sobj._engine.n_reads)
            assert sobj._engine.world >= 3
        finally:
            if getattr(sobj, "_engine", None) is not None:
                sobj._engine.close()
    assert outs["host"] == outs["device"] and outs["host"][3] == 250 and len(outs["host"][0]) > 1000


# ------------------------------------------------------------------ 7. the switch alone, and neither
def test_the_switch_alone_and_neither(engine, sample, tmp_path, monkeypatch):
    from itsxpress_amd.trim import cache_clear
    _clean_env(monkeypatch)
    engine.inflate = engine.parse = "host"
    cache_clear()
    p0 = _parse_counters(engine)
    n, m = engine.merge_pairs_load(*sample["files"]["python"])
    want = (n, m) + _merged_state(engine, str(tmp_path), "neither")
    assert _parse_counters(engine) == p0                                      # with neither the setting nor the switch no parse counter moves
    monkeypatch.setenv("ITSX_DEVICE_PARSE", "1")
    cache_clear()
    n, m = engine.merge_pairs_load(*sample["files"]["python"])
    got = (n, m) + _merged_state(engine, str(tmp_path), "switch")
    monkeypatch.delenv("ITSX_DEVICE_PARSE")
    assert _parse_counters(engine) == (p0[0] + 2, p0[1]) and got == want
