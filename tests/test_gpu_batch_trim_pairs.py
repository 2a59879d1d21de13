"""The trimmed R1 / R2 FASTQ of every paired sample of a batch cut on the device from the ORIGINAL pair records the context keeps
(itsx_keep_pair_records, itsx_write_trimmed_paired_samples, SampleBatch(keep_records="pairs")).  The reference in every case is the
host writer itsxpress_amd.trim.write_trimmed_paired on the sample's own R1 / R2 files with that sample's slice of the merged reads'
labels and coordinates, exactly as SampleBatch.write_paired_trimmed slices them.  `pytest -m gpu`."""
import gzip
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
_COMP = str.maketrans("ACGTN", "TGCAN")
_ACGT = np.array(list("ACGT"))
_LENS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]          # trimmed lengths; with start 0..7: every source / destination misalignment
_UNMERGED = 60                                               # unrelated mates at the end of every sample
_LONG = (6000, 5990)                                         # one pair near the merge kernel's limit of 12 000 bases in total


def _rc(s):
    return s[::-1].translate(_COMP)


def _scan_tile():
    """pairs per block of the plan's scan, from the kernel source (k_trim.hip: TR_BLOCK threads x TR_ITEMS items)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "itsxpress_amd", "csrc", "k_trim.hip")) as f:
        src = f.read()
    return int(re.search(r"TR_BLOCK = (\d+);", src).group(1)) * int(re.search(r"TR_ITEMS = (\d+);", src).group(1))


def _have_zstd(engine):
    return bool(engine.L.itsx_io_codecs() & 2)


def _random_bases(rng, n):
    return "".join(_ACGT[rng.integers(0, 4, n)])


def _quals(rng, n):
    return (rng.integers(25, 41, n) + 33).astype(np.uint8).tobytes().decode()


def _titles(i, tag):
    """the two title lines of pair i, 2..80 bytes with the '@'; every other one with a comment, after a blank or (one in three) a TAB"""
    want = 2 + (i * 7) % 79
    ident = ("%s%d" % (tag, i))[:want - 1]
    rest = want - 1 - len(ident)
    if i % 2 and rest >= 2:
        sep = "\t" if i % 6 == 1 else " "
        return ident + sep + "c" * (rest - 1), ident + sep + "d" * (rest - 1)
    return ident + "x" * rest, ident + "x" * rest


def _sample_pairs(rng, n, k):
    """n pairs of sample k: overlapping mates that merge (R1 and R2 of different lengths, both long enough for every trimmed length),
    then _UNMERGED unrelated mates.  Planted: pairs 40 and 41 share an identifier; two unmerged pairs reuse the identifiers of the merged
    pairs 5 and 17; sample 0's pair 9 has an identifier that an UNMERGED pair of sample 1 carries too; sample 2's pair 500 is the long one."""
    tag = "p%d_" % k
    r1, r2 = [], []
    nm = n - _UNMERGED
    for i in range(n):
        t1, t2 = _titles(i, tag)
        if i < nm:
            if k == 2 and i == 500:
                fl, rl = _LONG
                L = 11000
            else:
                L = int(rng.integers(560, 601))
                fl, rl = int(rng.integers(L // 2 + 8, L)), int(rng.integers(L // 2 + 8, L))
            frag = _random_bases(rng, L)
            f, r = list(frag[:fl]), list(_rc(frag[L - rl:]))
            for s in (f, r):
                if rng.random() < 0.3:
                    s[int(rng.integers(0, len(s)))] = str(_ACGT[rng.integers(0, 4)])
            f, r = "".join(f), "".join(r)
        else:
            f, r = _random_bases(rng, 300 + i % 7), _random_bases(rng, 290 + i % 5)
        planted = {5: "reuseA", 17: "reuseB", 40: "twin", 41: "twin", nm + 10: "reuseA", nm + 20: "reuseB"}
        if k == 0:
            planted[9] = "only_in_s0"
        if k == 1:
            planted[nm + 30] = "only_in_s0"
        if i in planted:
            t1, t2 = planted[i] + " planted 1", planted[i] + "\tplanted 2"
        if (len(f), len(r)) == _LONG:                       # (11 000 merged bases stay under the merge's expected-error limit only at a high quality)
            r1.append((t1, f, "]" * len(f)))
            r2.append((t2, r, "]" * len(r)))
            continue
        r1.append((t1, f, _quals(rng, len(f))))
        r2.append((t2, r, _quals(rng, len(r))))
    return r1, r2


def _coords(i, l1, l2):
    """(start, stop, tlen) of the i-th merged read of a sample whose pair has l1 / l2 bases.  Blocks of 88 reads walk every (trimmed
    length, start) combination, tlen - stop taking every residue mod 4; even blocks are written as they are, odd blocks interleave the
    edges of the two slices."""
    tl, st = _LENS[i % 11], (i // 11) % 8
    s, e = st, st + tl
    t = e + (i // 176) % 4 + 4 * ((i // 88) % 3)
    kind = i % 13 if (i // 88) % 2 else 0
    if kind == 1:                                            # stop > tlen: R1 open, R2 from a small negative start
        t = e - 3
    elif kind == 2:                                          # stop > tlen, |tlen - stop| > len2: R2's start clamped at 0
        s, t, e = 1, 2, l2 + 100 + st
    elif kind == 3:                                          # stop == tlen
        t = e
    elif kind == 4:                                          # tlen - start > len2: R2's end clamped
        t = l2 + 50 + s
        e = t - (l2 - 10)
    elif kind == 5:                                          # tlen < start: R2's end negative
        s = st + 3
        e, t = s + tl, s - 2
    elif kind == 6:                                          # start >= len1: written, R1's slice empty
        s, e = l1 + 2, l1 + 9
        t = e + 1
    elif kind == 7:                                          # not written: start == stop, start > stop, -1 on either side
        e = s
    elif kind == 8:
        s, e = e, s
    elif kind == 9:
        s = -1
    elif kind == 10:
        e = -1
    elif kind == 11:                                         # stop > tlen, |tlen - stop| < len2, R2's end past its length: the last 5 bases
        e = l2 + 40
        t = e - 5
    return s, e, t


def _ident(title):
    return re.split(r"[ \t]", title)[0]


def _model(r1, r2, names, start, stop, tlen, seen):
    """Dedup.create_paired_trimmed_seqs in Python's own slices (SeqSample.py:564-790): the two texts and the pairs written; `seen`
    counts the cases the coordinates were laid out to reach"""
    first = {}
    for k, nm in enumerate(names):
        first.setdefault(nm, k)
    o1, o2, n = [], [], 0
    for (t1, s1, q1), (t2, s2, q2) in zip(r1, r2):
        k = first.get(_ident(t1))
        if k is None:
            continue
        s, e, t = int(start[k]), int(stop[k]), int(tlen[k])
        if s < 0 or e < 0 or not s < e:
            seen["skipped_%s" % ("minus" if s < 0 or e < 0 else "equal" if s == e else "reversed")] += 1
            continue
        a1 = slice(s, None) if e > t else slice(s, e)
        a2 = slice(t - e, None) if (t - s) > t else slice(t - e, t - s)
        seen["open_r1"] += e > t
        seen["neg_small"] += t - e < 0 and e - t < len(s2)
        seen["neg_big"] += t - e < 0 and e - t > len(s2)
        seen["stop_is_tlen"] += e == t
        seen["r2_end_clamped"] += t - s > len(s2)
        seen["r2_end_negative"] += t < s
        seen["start_past_r1"] += s >= len(s1)
        seen["residue_%d" % ((t - e) % 4)] += 0 <= t - e < 16 and len(s2[a2]) > 200
        o1.append("@%s\n%s\n+\n%s\n" % (t1, s1[a1], q1[a1]))
        o2.append("@%s\n%s\n+\n%s\n" % (t2, s2[a2], q2[a2]))
        n += 1
    return "".join(o1).encode(), "".join(o2).encode(), n


_CASES = ["skipped_minus", "skipped_equal", "skipped_reversed", "open_r1", "neg_small", "neg_big", "stop_is_tlen", "r2_end_clamped",
          "r2_end_negative", "start_past_r1", "residue_0", "residue_1", "residue_2", "residue_3"]


def _write_pairs(d, k, r1, r2):
    """sample k's two files: the second sample with CRLF line ends, the third gzipped"""
    eol = "\r\n" if k == 1 else "\n"
    out = []
    for side, recs in ((1, r1), (2, r2)):
        text = "".join("@%s%s%s%s+%s%s%s" % (t, eol, s, eol, eol, q, eol) for t, s, q in recs).encode()
        p = os.path.join(d, "in%d_R%d.fq%s" % (k, side, ".gz" if k == 2 else ""))
        with (gzip.open(p, "wb", compresslevel=1) if k == 2 else open(p, "wb")) as f:
            f.write(text)
        out.append(p)
    return out


def _merge_with_pairs(engine, r1s, r2s):
    engine.keep_records(True)
    engine.keep_pair_records(True)
    try:
        return engine.merge_pairs_load_files(r1s, r2s)
    finally:
        engine.keep_pair_records(False)
        engine.keep_records(False)


def _sample_names(engine, first):
    """per sample its slice of read_names_raw(), as SampleBatch.write_paired_trimmed cuts it"""
    blob, offs = engine.read_names_raw()
    return [(blob[int(offs[lo]):int(offs[hi])], offs[lo:hi + 1] - offs[lo]) for lo, hi in zip(first[:-1], first[1:])]


@pytest.fixture(scope="module")
def merged(engine, tmp_path_factory):
    """four samples whose PAIR counts straddle the plan's tile (tile - 1, tile, tile + 1, 0), their files, the coordinates of every
    merged read and, per trim_ccs, the host writer's two outputs and count for every sample"""
    from collections import Counter
    from itsxpress_amd.trim import write_trimmed_paired
    d = str(tmp_path_factory.mktemp("trim_pairs_in"))
    tile = _scan_tile()
    rng = np.random.default_rng(99)
    sizes = [tile - 1, tile, tile + 1, 0]
    pairs = [_sample_pairs(rng, n, k) if n else ([], []) for k, n in enumerate(sizes)]
    files = [_write_pairs(d, k, r1, r2) for k, (r1, r2) in enumerate(pairs)]
    r1s, r2s = [f[0] for f in files], [f[1] for f in files]
    n, m = _merge_with_pairs(engine, r1s, r2s)
    assert list(n) == sizes and all(sizes[k] - _UNMERGED - 40 < m[k] <= sizes[k] - _UNMERGED for k in range(3)) and m[3] == 0
    first = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    pidx = engine.merge_pair_index()
    pfirst = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    start, stop, tlen = (np.zeros(int(first[-1]), np.int32) for _ in range(3))
    for k in range(3):
        for p in range(sizes[k]):
            g = int(pidx[pfirst[k] + p])
            if g < 0:
                continue
            l1, l2 = len(pairs[k][0][p][1]), len(pairs[k][1][p][1])
            start[g], stop[g], tlen[g] = _coords(g - int(first[k]), l1, l2)
            if (l1, l2) == _LONG:
                start[g], stop[g], tlen[g] = 3, 5903, 5905
    names = _sample_names(engine, first)
    ref, seen = {}, Counter()
    for ccs in (0, 1):
        outs, ret = [], []
        for k in range(4):
            lo, hi = int(first[k]), int(first[k + 1])
            o1, o2 = os.path.join(d, "ref_%d_%d_R1.fq" % (ccs, k)), os.path.join(d, "ref_%d_%d_R2.fq" % (ccs, k))
            ret.append(write_trimmed_paired(r1s[k], r2s[k], o1, o2, names[k], start[lo:hi], stop[lo:hi], tlen[lo:hi], trim_ccs=bool(ccs)))
            outs.append((open(o1, "rb").read(), open(o2, "rb").read()))
        ref[ccs] = (outs, ret)
    # ---- every case the coordinates were laid out for occurs in the reference outputs: they are what Python's own slices give, and
    # that model counts the cases
    outs, ret = ref[0]
    for k in range(4):
        nb, no = names[k]
        nl = [nb[int(no[j]):int(no[j + 1])].decode() for j in range(len(no) - 1)]
        lo, hi = int(first[k]), int(first[k + 1])
        e1, e2, cnt = _model(pairs[k][0], pairs[k][1], nl, start[lo:hi], stop[lo:hi], tlen[lo:hi], seen)
        assert (e1, e2, cnt) == (outs[k][0], outs[k][1], ret[k]), k
    assert all(seen[c] >= 1 for c in _CASES), {c: seen[c] for c in _CASES}
    assert b"\r" not in outs[1][0] + outs[1][1] and outs[3] == (b"", b"") and ret[3] == 0
    assert all(0 < ret[k] < sizes[k] and len(outs[k][0]) > 1000 and len(outs[k][1]) > 1000 for k in range(3))
    assert b"\n\n+\n\n" in outs[0][0] and b"\n\n+\n\n" in outs[0][1]                        # written with an empty slice
    assert any(b"\t" in o for o in outs[0]) and max(len(x) for x in outs[2][0].split(b"\n")) == 5900
    for k in range(3):                                                                      # an unmerged pair under a merged pair's identifier
        assert outs[k][0].count(b"@reuseA planted 1\n") == 2 and outs[k][1].count(b"@reuseB\tplanted 2\n") == 2
        twins = [x.split(b"\n")[0] for x in outs[k][0].split(b"@twin planted 1\n")[1:]]
        assert len(twins) == 2 and len(twins[0]) == len(twins[1]) > 0                       # both under the FIRST twin's coordinates
        g40, g41 = int(pidx[pfirst[k] + 40]), int(pidx[pfirst[k] + 41])                   # (both merged, and their own coordinates differ)
        assert 0 <= g40 < g41 and int(stop[g40] - start[g40]) != int(stop[g41] - start[g41]) and len(twins[0]) == int(stop[g40] - start[g40])
    assert outs[0][0].count(b"@only_in_s0 planted 1\n") == 1 and b"only_in_s0" not in outs[1][0] + outs[1][1]      # not across samples
    return dict(dir=d, r1s=r1s, r2s=r2s, sizes=sizes, merged=list(m), first=first, start=start, stop=stop, tlen=tlen, ref=ref, tile=tile)


def _decoded(path, kind):
    from itsxpress_amd.trim import read_text
    raw = open(path, "rb").read()
    if kind == "plain":
        return raw
    assert raw                                               # an empty gzip / zstd file is still a valid empty member
    if kind == "gzip":
        text = gzip.decompress(raw)                          # Python's own reader must accept it
        assert text == read_text(path)
        return text
    return read_text(path)


@pytest.mark.parametrize("ccs,kind", [(0, "plain"), (1, "plain"), (0, "gzip"), (1, "zstd")])
def test_explicit_coordinates_on_merged_pairs(engine, merged, tmp_path, ccs, kind):
    if kind == "zstd" and not _have_zstd(engine):
        kind = "gzip"
    n, m = _merge_with_pairs(engine, merged["r1s"], merged["r2s"])
    assert list(n) == merged["sizes"] and list(m) == merged["merged"]
    o1 = [str(tmp_path / ("o%d_R1.%s" % (k, kind))) for k in range(4)]
    o2 = [str(tmp_path / ("o%d_R2.%s" % (k, kind))) for k in range(4)]
    ret = engine.write_trimmed_paired_samples(o1, o2, start=merged["start"], stop=merged["stop"], tlen=merged["tlen"], gzipped=kind == "gzip",
                                              zstd_file=kind == "zstd", trim_ccs=bool(ccs))
    exp, exp_ret = merged["ref"][ccs]
    for k in range(4):
        for side, paths in enumerate((o1, o2)):
            assert os.path.exists(paths[k])
            got = _decoded(paths[k], kind)
            assert got == exp[k][side], (k, side, len(got), len(exp[k][side]))
        assert ret[k] == exp_ret[k], k
    if kind != "plain" or ccs:
        return
    # a sample given None for both paths is skipped, and the others are what they were
    p1 = [str(tmp_path / ("p%d_R1.fq" % k)) for k in range(4)]
    p2 = [str(tmp_path / ("p%d_R2.fq" % k)) for k in range(4)]
    ret2 = engine.write_trimmed_paired_samples([p1[0], None, p1[2], p1[3]], [p2[0], None, p2[2], p2[3]], start=merged["start"], stop=merged["stop"],
                                               tlen=merged["tlen"])
    assert not os.path.exists(p1[1]) and not os.path.exists(p2[1]) and ret2 == exp_ret
    for k in (0, 2, 3):
        assert (open(p1[k], "rb").read(), open(p2[k], "rb").read()) == exp[k], k


# ------------------------------------------------------------------ the mirror: a paired batch from raw files to trimmed files
def _fixture_records(gold):
    lines = gzip.open(os.path.join(gold, "seq.fq.gz"), "rt").read().split("\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]


def _overlapping_pairs(rng, frags, name):
    """one pair per fragment (the fixture's reads, so that the stand-in profiles find their ITS2): a few substitutions, qualities 25..40"""
    r1, r2 = [], []
    for i, frag in enumerate(frags):
        L = len(frag)
        fl, rl = int(rng.integers(L // 2 + 8, L)), int(rng.integers(L // 2 + 8, L))
        f, r = list(frag[:fl]), list(_rc(frag[L - rl:]))
        for s in (f, r):
            if rng.random() < 0.3:
                s[int(rng.integers(0, len(s)))] = str(_ACGT[rng.integers(0, 4)])
        label = "%s%05d" % (name, i)
        r1.append((label + " 1:N:0", "".join(f), _quals(rng, fl)))
        r2.append((label + " 2:N:0", "".join(r), _quals(rng, rl)))
    return r1, r2


def _write_fastq(path, recs):
    with open(path, "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % r for r in recs))
    return path


def test_paired_batch_writes_from_the_pair_records(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    import itsxpress_amd.trim as trim
    from bench import its2_profiles
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    rng = np.random.default_rng(6)
    seqs = [s.upper() for _, s, _ in _fixture_records(gold) if set(s.upper()) <= set("ACGT")]
    assert len(seqs) > 150
    d = str(tmp_path / "in")
    os.makedirs(d)
    u1 = [("un%02d" % i, _random_bases(rng, 120), "I" * 120) for i in range(40)]            # unrelated mates: nothing merges
    u2 = [("un%02d" % i, _random_bases(rng, 110), "I" * 110) for i in range(40)]
    a1, a2 = _overlapping_pairs(rng, seqs[:70], "a")
    a1.append((a1[3][0].split(" ")[0] + " again", u1[0][1], u1[0][2]))                      # an unmerged pair under a merged pair's identifier
    a2.append((a2[3][0].split(" ")[0] + " again", u2[0][1], u2[0][2]))
    pairs = [(a1, a2), (u1, u2), _overlapping_pairs(rng, seqs[70:150], "c")]
    files = [(_write_fastq(os.path.join(d, "m%d_R1.fq" % k), p1), _write_fastq(os.path.join(d, "m%d_R2.fq" % k), p2)) for k, (p1, p2) in enumerate(pairs)]
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    host_calls = []
    host_writer = trim.write_trimmed_paired

    def run(keep, tag, host_allowed):
        def guarded(*a, **kw):
            if not host_allowed:
                raise AssertionError("the host writer was called in a batch that keeps the pair records")
            host_calls.append(tag)
            return host_writer(*a, **kw)
        monkeypatch.setattr(trim, "write_trimmed_paired", guarded)
        objs = [SeqSamplePairedNotInterleaved(fastq=r1, tempdir=bd, fastq2=r2) for r1, r2 in files]
        b = SampleBatch(objs, engine=engine, subdirs=["%s%d" % (tag, k) for k in range(3)], keep_records=keep)
        b.merge_reads(threads=1)
        seq_there = [os.path.exists(o.seq_file) for o in objs]
        b.deduplicate(threads=1)
        b._search(hmmfile=str(hmm), threads=1)
        got = {}
        for ccs in (False, True):
            o1s = [os.path.join(bd, "%s_%d_%d_R1.fq" % (tag, ccs, k)) for k in range(3)]
            o2s = [os.path.join(bd, "%s_%d_%d_R2.fq" % (tag, ccs, k)) for k in range(3)]
            ret = b.write_paired_trimmed(o1s, o2s, "ITS2", trim_ccs=ccs)
            got[ccs] = ([(open(p, "rb").read(), open(q, "rb").read()) for p, q in zip(o1s, o2s)], [int(x) for x in ret])
        merged_out = None
        if keep or all(seq_there):
            outs = [os.path.join(bd, "%s_m_%d.fq" % (tag, k)) for k in range(3)]
            merged_out = ([tuple(x) for x in b.write_trimmed(outs, "ITS2")], [open(p, "rb").read() for p in outs])
        return seq_there, got, merged_out, list(b.counts)

    seq_there, got, merged_out, counts = run("pairs", "pairs", False)
    assert seq_there == [False, False, False] and host_calls == []          # no seq.fq, and the host writer was not called
    seq_there2, exp, merged_exp, counts2 = run(False, "files", True)
    assert seq_there2 == [True, True, True] and counts == counts2 and counts[1] == 0 and counts[0] > 50 and counts[2] > 50
    assert len(host_calls) == 6
    assert got[False] == exp[False] and got[True] == exp[True] and got[False] != got[True]
    texts, ret = got[False]
    assert texts[1] == (b"", b"") and ret[1] == 0 and ret[0] > 20 and ret[2] > 20 and len(texts[0][0]) > 1000 and len(texts[2][1]) > 1000
    assert texts[0][0].count(b" again\n") == 1                              # the unmerged pair under a merged pair's identifier is written
    # write_trimmed on a batch that keeps the pairs still works, from the merged records
    assert merged_out == merged_exp and len(merged_out[1][0]) > 1000
    # keep_records=True (not "pairs") keeps no pair records: write_paired_trimmed takes the host path, the same bytes
    del host_calls[:]
    seq_there3, got3, _, _ = run(True, "kept", True)
    assert seq_there3 == [False, False, False] and len(host_calls) == 6 and got3 == exp


def test_lower_case_inputs_keep_no_pair_records_and_take_the_host_writer(engine, gold, t_hmm_text, tmp_path, monkeypatch):
    """the merge reads its bases in upper case, so slices of its upload would not be the input's bytes: such pairs keep no pair records,
    the engine call says so, and the batch writes the host writer's bytes, lower case included"""
    import itsxpress_amd.trim as trim
    from bench import its2_profiles
    from itsxpress_amd import EngineError
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    monkeypatch.setenv("ITSXPRESS_ARRAYS", "0")
    monkeypatch.setenv("ITSXPRESS_STREAM", "0")
    monkeypatch.delenv("ITSXPRESS_GPUS", raising=False)
    rng = np.random.default_rng(8)
    seqs = [s.upper() for _, s, _ in _fixture_records(gold) if set(s.upper()) <= set("ACGT")]
    d = str(tmp_path / "in")
    os.makedirs(d)
    files = []
    for k, (lo, hi) in enumerate(((0, 60), (60, 120))):
        p1, p2 = _overlapping_pairs(rng, seqs[lo:hi], "l%d_" % k)
        if k == 1:                                               # one sample with lower-case bases on both sides, every third pair
            p1 = [(t, s.lower() if i % 3 == 0 else s, q) for i, (t, s, q) in enumerate(p1)]
            p2 = [(t, s[:20] + s[20:].lower() if i % 3 == 1 else s, q) for i, (t, s, q) in enumerate(p2)]
        files.append((_write_fastq(os.path.join(d, "l%d_R1.fq" % k), p1), _write_fastq(os.path.join(d, "l%d_R2.fq" % k), p2)))
    n, m = _merge_with_pairs(engine, [f[0] for f in files], [f[1] for f in files])
    assert m[0] > 40 and m[1] > 40
    z = np.zeros(engine.n_reads, np.int32)
    with pytest.raises(EngineError, match="itsx_keep_pair_records") as ei:
        engine.write_trimmed_paired_samples([str(tmp_path / "x1a"), str(tmp_path / "x1b")], [str(tmp_path / "x2a"), str(tmp_path / "x2b")],
                                            start=z, stop=z + 5, tlen=z + 9)
    assert ei.value.code == -1 and not os.path.exists(str(tmp_path / "x1a"))
    hmm = tmp_path / "its2.hmm"
    hmm.write_text(its2_profiles(t_hmm_text))
    bd = str(tmp_path / "batch")
    os.makedirs(bd)
    calls = []
    host_writer = trim.write_trimmed_paired

    def counted(*a, **kw):
        calls.append(1)
        return host_writer(*a, **kw)
    monkeypatch.setattr(trim, "write_trimmed_paired", counted)

    def run(keep, tag):
        objs = [SeqSamplePairedNotInterleaved(fastq=r1, tempdir=bd, fastq2=r2) for r1, r2 in files]
        b = SampleBatch(objs, engine=engine, subdirs=["%s%d" % (tag, k) for k in range(2)], keep_records=keep)
        b.merge_reads(threads=1)
        b.deduplicate(threads=1)
        b._search(hmmfile=str(hmm), threads=1)
        o1s = [os.path.join(bd, "%s_%d_R1.fq" % (tag, k)) for k in range(2)]
        o2s = [os.path.join(bd, "%s_%d_R2.fq" % (tag, k)) for k in range(2)]
        ret = b.write_paired_trimmed(o1s, o2s, "ITS2")
        return [(open(p, "rb").read(), open(q, "rb").read()) for p, q in zip(o1s, o2s)], [int(x) for x in ret]

    got = run("pairs", "pairs")
    assert len(calls) == 2                                       # the host loop, one call per sample
    exp = run(False, "files")
    assert got == exp and got[1][0] > 20 and got[1][1] > 20
    seq_lines = lambda text: b"".join(text.split(b"\n")[1::4])
    assert any(c in seq_lines(got[0][1][0]) for c in (b"a", b"c", b"g", b"t")) and seq_lines(got[0][0][0]).isupper()


# ------------------------------------------------------------------ errors
def test_errors_and_what_survives_them(merged, tmp_path):
    from itsxpress_amd import Engine, EngineError
    eng = Engine(0)                                             # its own context: no profiles, nothing finalized
    r1s, r2s, a, b, t = merged["r1s"], merged["r2s"], merged["start"], merged["stop"], merged["tlen"]
    o1 = [str(tmp_path / ("e%d_R1.fq" % k)) for k in range(4)]
    o2 = [str(tmp_path / ("e%d_R2.fq" % k)) for k in range(4)]
    eng.keep_records(True)                                      # the single-end flag alone keeps no pairs
    eng.merge_pairs_load_files(r1s, r2s)
    with pytest.raises(EngineError, match="itsx_keep_pair_records") as ei:
        eng.write_trimmed_paired_samples(o1, o2, start=a, stop=b, tlen=t)
    assert ei.value.code == -1
    eng.keep_records(False)
    eng.keep_pair_records(True)
    eng.merge_pairs_load_files(r1s, r2s)
    for bad in (dict(p1=o1[:3], p2=o2[:3], start=a, stop=b, tlen=t), dict(p1=o1 + [o1[0]], p2=o2 + [o2[0]], start=a, stop=b, tlen=t),
                dict(p1=[o1[0], None, o1[2], o1[3]], p2=o2, start=a, stop=b, tlen=t), dict(p1=o1, p2=[o2[0], o2[1], o2[2], None], start=a, stop=b, tlen=t),
                dict(p1=o1, p2=o2), dict(p1=o1, p2=o2, region_prefixes=("3_", "4_"), start=a, stop=b, tlen=t),
                dict(p1=o1, p2=o2, start=a, stop=b), dict(p1=o1, p2=o2, tlen=t)):
        with pytest.raises(EngineError) as ei:
            eng.write_trimmed_paired_samples(bad.pop("p1"), bad.pop("p2"), **bad)
        assert ei.value.code == -1
    with pytest.raises(EngineError, match="itsx_search_finalize") as ei:
        eng.write_trimmed_paired_samples(o1, o2, region_prefixes=("3_", "4_"))
    assert ei.value.code == -1
    assert not any(os.path.exists(p) for p in o1 + o2)
    # the records survived all that, and the single-end writer has none to write from
    ret = eng.write_trimmed_paired_samples(o1, o2, start=a, stop=b, tlen=t)
    exp, exp_ret = merged["ref"][0]
    assert [(open(p, "rb").read(), open(q, "rb").read()) for p, q in zip(o1, o2)] == exp and ret == exp_ret
    with pytest.raises(EngineError, match="itsx_keep_records"):
        eng.write_trimmed_samples(o1, start=a, stop=b)
    # any other read set replaces the pairs: their records are gone
    eng.load_reads_files([r1s[0]])
    with pytest.raises(EngineError, match="itsx_keep_pair_records") as ei:
        eng.write_trimmed_paired_samples(o1[:1], o2[:1], start=np.zeros(eng.n_reads, np.int32), stop=np.ones(eng.n_reads, np.int32),
                                         tlen=np.ones(eng.n_reads, np.int32))
    assert ei.value.code == -1
    # and with the flag off again a merge keeps none
    eng.keep_pair_records(False)
    eng.merge_pairs_load_files(r1s, r2s)
    with pytest.raises(EngineError, match="itsx_keep_pair_records"):
        eng.write_trimmed_paired_samples(o1, o2, start=a, stop=b, tlen=t)
    eng.close()
