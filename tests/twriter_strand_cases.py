"""The streamed writers' strands (itsx_twriter_strands): the edge catalogue, its model in plain Python and the driver that feeds a
writer object.  TEST INFRASTRUCTURE ONLY, shared by tests/test_twriter_strands_cpu.py and tests/test_gpu_twriter_strands.py.

The model: a record of strand -1 is `orient_profiles_exact.revcomp` of its bases and `[::-1]` of its qualities, every other record is
as it is; a record is written iff start >= 0, stop >= 0 and start < stop, as title, [primer] bases[start:stop] [primer], '+',
[17 x '~'] qualities[start:stop] [17 x '~'] -- Python's slicing, the CCS primers of the reference."""
import ctypes as C
import os

import numpy as np

from orient_profiles_exact import revcomp

UNIT_KB = 4
LENGTHS = list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 255, 256, 257]
LONG = 65535
SYMBOLS = "ACGTURYMKSWHBVDNacgturymkswhbvdn"
CCS_FWD, CCS_REV = "GACAGGTACAAGAAGGA", "TTAACCCAGTCTCCAGT"


def _lib():
    from itsxpress_amd import _lib as m
    return m.lib()


def _slices(L):
    """(start, stop) pairs for a read of L bases: every (start mod 4, stop mod 4), written inside the read where the read is long
    enough (and clamped by Python where it is not), then the ends and the records that are not written"""
    out = []
    for sm in range(4):
        for em in range(4):
            a = sm + (4 if L > 40 else 0)
            b = a + 1 + (em - a - 1) % 4
            if L > 40:                      # a long slice whose end keeps its residue: whole dwords in the middle, seams at both ends
                b += (L - 12 - b) // 4 * 4
            out.append((a, b))
    out += [(0, L), (0, L + 5), (1, L), (L - 1, L), (0, 1), (L, L + 3),      # start = 0, stop = L, stop > L, an empty slice that IS written
            (3, 3), (5, 2), (-1, 4), (2, -1), (-1, -1)]                      # not written
    return out


def catalogue():
    """records (title, bases, qualities, line end, text before the title), their coordinates and strands.  Sections 1 and 3 alternate flipped
    and unflipped records (every seventh of strand 0; section 3 the other way round, so that every slice is seen on both strands);
    section 2 repeats the records in runs of 37 of one strand: at 4-KB units both a flipped and an unflipped run cross unit boundaries."""
    rng = np.random.default_rng(77)
    recs, start, stop, strand = [], [], [], []
    tags = {}

    def add(bases, quals, a, b, s, nl="\n", before="", tl=None):
        tl = 1 + len(recs) % 8 if tl is None else tl                     # title lengths 1 .. 8 ('@' alone is a title)
        title = "@" + "".join(rng.choice(list("abcXYZ019_"), tl - 1))
        recs.append((title, bases, quals, nl, before))
        start.append(a); stop.append(b); strand.append(s)

    def rnd(L, alphabet):
        if L < 2000:
            return "".join(rng.choice(list(alphabet), L))
        return ("".join(rng.choice(list(alphabet), 997)) * (L // 997 + 1))[:L]

    for section in range(3):
        k = 0
        for L in LENGTHS:
            for a, b in _slices(L):
                if section != 1:
                    s = 0 if k % 7 == 6 else (-1 if (k + section // 2) % 2 else 1)
                else:
                    s = -1 if (k // 37) % 2 == 0 else 1
                q = rnd(L, "@+IF#5~!")
                if k % 5 == 0:
                    q = "@" + q[1:]                                      # a quality line that looks like a title
                add(rnd(L, "ACGT"), q, a, b, s, nl="\r\n" if k % 11 == 3 else "\n")
                k += 1
    # every IUPAC symbol, lower case and U at both ends of a flipped read, whole and cut one base short at either end
    for c in SYMBOLS + "X-.*":
        for a, b in ((0, 10), (1, 9), (0, 1), (9, 10)):
            add(c + rnd(8, "ACGTNacgtn") + c, rnd(10, "@+IF#5~!"), a, b, -1)
    add(SYMBOLS + rnd(33, "ACGT") + SYMBOLS[::-1], rnd(97, "@+IF#5~!"), 0, 97, -1)
    add(SYMBOLS + rnd(33, "ACGT") + SYMBOLS[::-1], rnd(97, "@+IF#5~!"), 2, 95, -1)
    # a blank line between two records: the device leaves that unit to the host, which honours the strands
    tags["blank"] = len(recs)
    add(rnd(64, "ACGT"), rnd(64, "@+IF#5~!"), 3, 61, -1, before="\n")
    for i in range(6):
        add(rnd(65, "ACGT"), rnd(65, "@+IF#5~!"), i, 60 + i, -1 if i % 2 else 1)
    # one read of 65 535 bases, flipped, then the same shape unflipped: a record that is many units long
    tags["long"] = len(recs)
    add(rnd(LONG, "ACGTN"), rnd(LONG, "@+IF#5~!"), 5, LONG - 2, -1)
    add(rnd(LONG, "ACGTN"), rnd(LONG, "@+IF#5~!"), 2, LONG - 5, 1)
    # the last line has no newline
    add(rnd(17, "ACGTRYacgt"), rnd(17, "@+IF#5~!"), 1, 16, -1)
    parts = []
    for i, (t, s, q, nl, before) in enumerate(recs):
        last = i == len(recs) - 1
        parts.append(before + t + nl + s + nl + "+" + nl + q + ("" if last else nl))
    text = "".join(parts).encode()
    return text, recs, np.array(start, np.int32), np.array(stop, np.int32), np.array(strand, np.int8), tags


def model(recs, start, stop, strand, ccs):
    """(text, records written, summed length) of the trimmed file"""
    out, n, tot = [], 0, 0
    for (t, s, q, _, _), a, b, d in zip(recs, start, stop, strand):
        a, b = int(a), int(b)
        if a < 0 or b < 0 or not a < b:
            continue
        if d < 0:
            s, q = revcomp(s), q[::-1]
        s, q = s[a:b], q[a:b]
        if ccs:
            s, q = CCS_FWD + s + CCS_REV, "~" * 17 + q + "~" * 17
        out.append(t + "\n" + s + "\n+\n" + q + "\n")
        n += 1
        tot += len(s)
    return "".join(out).encode(), n, tot


def record_ends(text):
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


def write(path, text, ends, start, stop, strand, comp, ccs, pieces, ctx=None):
    """the writer object fed in one piece (pieces False), or in pieces of 7 records: a piece's strands, then its text and coordinates,
    every fifth record undecided (decided = 0 beside a wrong start) until itsx_twriter_update names it.  strand None: no strands.
    Returns (records written, summed length)."""
    L = _lib()
    n = len(ends)
    w = C.c_void_p()
    assert L.itsx_twriter_open(os.fsencode(str(path)), comp, ccs, C.byref(w)) == 0, L.itsx_trim_last_error()
    if ctx is not None:
        assert L.itsx_twriter_set_device(w, ctx.h) == 0, L.itsx_trim_last_error()
    buf = C.create_string_buffer(text, len(text))
    base = C.addressof(buf)
    if not pieces:
        if strand is not None:
            assert L.itsx_twriter_strands(w, 0, n, strand.ctypes.data) == 0, L.itsx_trim_last_error()
        assert L.itsx_twriter_text(w, base, len(text), 1) == 0
        assert L.itsx_twriter_coords(w, 0, n, start.ctypes.data, stop.ctypes.data, None) == 0
    else:
        late = np.arange(n) % 5 == 2
        wrong = np.where(late, 7, start).astype(np.int32)
        for lo in range(0, n, 7):
            hi = min(n, lo + 7)
            if strand is not None:
                sd = np.ascontiguousarray(strand[lo:hi])
                assert L.itsx_twriter_strands(w, lo, hi - lo, sd.ctypes.data) == 0, L.itsx_trim_last_error()
            a1, a2, a3 = np.ascontiguousarray(wrong[lo:hi]), np.ascontiguousarray(stop[lo:hi]), (~late[lo:hi]).astype(np.uint8)
            assert L.itsx_twriter_text(w, base, len(text) if hi == n else ends[hi - 1], 1 if hi == n else 0) == 0
            assert L.itsx_twriter_coords(w, lo, hi - lo, a1.ctypes.data, a2.ctypes.data, a3.ctypes.data) == 0, L.itsx_trim_last_error()
        idx = np.flatnonzero(late).astype(np.int64)
        for part in np.array_split(idx, 3):
            s1, s2 = np.ascontiguousarray(start[part]), np.ascontiguousarray(stop[part])
            assert L.itsx_twriter_update(w, part.ctypes.data, len(part), s1.ctypes.data, s2.ctypes.data) == 0
    nw, tot = C.c_int64(), C.c_int64()
    rc = L.itsx_twriter_close(w, C.byref(nw), C.byref(tot))
    assert rc == 0, (rc, L.itsx_trim_last_error())
    return nw.value, tot.value
