"""Pairs of FASTQ texts (R1, R2) for the device parse of the paired merge loaders (csrc/k_fastq.hip: k_fastq_pairs, itsx_parse_pairs_device)
and a Python statement of what the host path makes of them between its parser and the merge kernel.  Each text is parsed as
tests/fastq_cases.py states the host parser (host_parse, planes); then, per side, bases 'a'..'z' become upper case and nothing else
(parse_fastx_range's toupper in the C locale), a quality byte outside 33..126 is flagged (merge_core's check), and the longest pair is
the largest sum of an R1 and its R2 length (merge_core's 12 000-base limit is held against it).  A pair is DECLINED when either text is
(fastq_cases' reasons) or when the two hold different numbers of records (reason "pairs", code 7)."""
import struct

import numpy as np

import fastq_cases as fc

REASON = dict(fc.REASON, pairs=(7, "R1 and R2 hold different numbers of records"))
LOWER1, LOWER2, QUAL1, QUAL2 = 1, 2, 4, 8
_LOWER = bytes(range(ord("a"), ord("z") + 1))
_UPPER = bytes(range(ord("A"), ord("Z") + 1))
_TABLE = bytes.maketrans(_LOWER, _UPPER)


def upper_az(b):
    """bytes.upper restricted to a-z (which is what it is for bytes: stated here without relying on it)"""
    return bytes(b).translate(_TABLE)


def qual_ok(b):
    return all(33 <= c <= 126 for c in b)


def expected(t1, t2):
    """the model: ("ok", dict(n, flags, max_total, sides=[dict(off, toff, seq, qual, titles)] x 2)), or ("declined", reason word, side)
    with side 0 / 1 for a text the rule declines (the lower side first) and -1 for unequal record counts"""
    recs = []
    for side, t in enumerate((t1, t2)):
        why = fc_decline_reason(t)
        if why is not None:
            return ("declined", why, side)
        recs.append(fc.host_parse(t))
    if len(recs[0]) != len(recs[1]):
        return ("declined", "pairs", -1)
    flags, sides = 0, []
    for side, rr in enumerate(recs):
        off, toff, seq, qual, titles = fc.planes(rr)
        up = upper_az(seq)
        flags |= (LOWER1 << side) if up != seq else 0
        flags |= (QUAL1 << side) if not qual_ok(qual) else 0
        sides.append(dict(off=off, toff=toff, seq=up, qual=qual, titles=titles))
    mx = max([len(a[1]) + len(b[1]) for a, b in zip(*recs)] or [0])
    return ("ok", dict(n=len(recs[0]), flags=flags, max_total=mx, sides=sides))


def fc_decline_reason(text):
    """the reason word csrc/fastq_rec.h declines a text for, None where it accepts: the rule restated on fastq_cases' lines"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        return "lines"
    lines = [x[:-1] if x.endswith(b"\r") else x for x in lines]
    for r in range(0, len(lines), 4):
        t, s, p, q = lines[r:r + 4]
        if t[:1] != b"@":
            return "title"
        if p[:1] != b"+":
            return "plus"
        if len(q) != len(s):
            return "qual"
    return None


# ------------------------------------------------------------------ building blocks
def text_of(recs, eol=b"\n", final=True):
    t = b"".join(b"@" + ti + eol + s + eol + b"+" + eol + q + eol for ti, s, q in recs)
    return t if final or not t else t[:-len(eol)]


def _bases(rng, L):
    return bytes(rng.choice(list(b"ACGTN"), L).tolist()) if L else b""


def _quals(rng, L):
    return bytes(rng.integers(33, 127, L, dtype=np.uint8).tolist()) if L else b""


def rand_recs(rng, lens, tag):
    """records of the given base counts; titles of mixed lengths, every third with a comment"""
    return [(b"%s%d" % (tag, k) + (b" c%d" % (k % 7) if k % 3 == 0 else b"\tx" if k % 3 == 1 else b""), _bases(rng, int(L)), _quals(rng, int(L))) for k, L in enumerate(lens)]


def _lens_summing_to(rng, total, lmax=301):
    lens = []
    while total > 0:
        L = min(int(rng.integers(0, lmax + 1)), total)
        lens.append(L)
        total -= L
    return lens


def _pad_text_to(rng, nbytes, tag):
    """records whose text (LF, final newline) has exactly nbytes bytes: the last record's title and bases make up the rest"""
    recs, used = [], 0
    while nbytes - used > 500:
        r = rand_recs(rng, [int(rng.integers(0, 120))], tag + b"%d_" % len(recs))[0]
        recs.append(r)
        used += len(text_of([r]))
    rest = nbytes - used - 6                      # '@' + 4 newlines + '+'
    tl = 1 if (rest - 1) % 2 == 0 else 2
    s = (rest - tl) // 2
    assert 0 <= s <= 301
    recs.append((b"z" * tl, _bases(rng, s), _quals(rng, s)))
    assert len(text_of(recs)) == nbytes
    return recs


def _set(side_recs, k, seq=None, qual=None):
    t, s, q = side_recs[k]
    side_recs[k] = (t, s if seq is None else seq, q if qual is None else qual)


_CASES = None


def cases():
    """[(name, R1 text, R2 text)], seeded: the same list on every call"""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(20261019)
    c = []

    def pair(name, n=None, lens1=None, lens2=None, eol1=b"\n", eol2=b"\n", final1=True, final2=True, edit=None):
        l1 = lens1 if lens1 is not None else rng.integers(0, 302, n).tolist()
        l2 = lens2 if lens2 is not None else rng.integers(0, 302, len(l1)).tolist()
        r1, r2 = rand_recs(rng, l1, b"p"), rand_recs(rng, l2, b"p")
        if edit:
            edit(r1, r2)
        c.append((name, text_of(r1, eol1, final1), text_of(r2, eol2, final2)))

    # ---- sample sizes around the plan's 1 024-record tile (short reads keep the big ones small; one of 301-base reads)
    c.append(("0 pairs", b"", b""))
    pair("1 pair", 1)
    for n in (1023, 1024, 1025):
        pair("%d pairs" % n, lens1=rng.integers(0, 24, n).tolist(), lens2=rng.integers(0, 24, n).tolist())
    pair("reads of 301 bases", lens1=[301] * 40, lens2=[301, 300] * 20)
    # ---- texts around the index's 4 096-byte tile
    for nb in (4095, 4096, 4097):
        r1 = _pad_text_to(rng, nb, b"a")
        r2 = rand_recs(rng, [len(r[1]) for r in r1], b"b")
        r2 = [(t1, s, q) for (t1, _, _), (_, s, q) in zip(r1, r2)]
        assert len(text_of(r2)) == nb
        c.append(("texts of %d bytes" % nb, text_of(r1), text_of(r2)))
    # ---- base planes around the gather's 16 384-byte tile
    for nb in (16383, 16384, 16385):
        l1 = _lens_summing_to(rng, nb)
        l2 = _lens_summing_to(rng, nb)
        n = max(len(l1), len(l2))
        l1 += [0] * (n - len(l1))
        l2 += [0] * (n - len(l2))
        assert sum(l1) == sum(l2) == nb
        pair("base planes of %d bytes" % nb, lens1=l1, lens2=l2)
    # ---- line ends
    pair("CRLF in R1 only", 7, eol1=b"\r\n")
    pair("CRLF in R2 only", 7, eol2=b"\r\n")
    pair("no final newline", 5, final1=False, final2=False)
    pair("no final newline in R2, CRLF", 5, eol2=b"\r\n", final2=False)
    pair("an empty read with an empty quality in R1", lens1=[9, 0, 20, 0], lens2=[9, 5, 20, 7])
    pair("an empty read with an empty quality in R2", lens1=[9, 5, 20, 7], lens2=[0, 5, 0, 0])
    pair("an empty read on both sides", lens1=[0, 0], lens2=[0, 0])
    pair("R1 and R2 of unlike lengths", lens1=[301, 1, 150, 17], lens2=[1, 301, 16, 250])
    # ---- lower case
    low = lambda side, k, at: (lambda r1, r2: _set((r1, r2)[side], k, seq=_lowered((r1, r2)[side][k][1], at)))
    pair("lower case in R1 only", lens1=[40, 33, 50], lens2=[41, 30, 17], edit=low(0, 1, 7))
    pair("lower case in R2 only", lens1=[40, 33, 50], lens2=[41, 30, 17], edit=low(1, 2, 16))
    pair("lower case at the first byte of R1's plane", lens1=[40, 33, 50], lens2=[41, 30, 17], edit=low(0, 0, 0))
    pair("lower case at the last byte of R1's plane", lens1=[40, 33, 50], lens2=[41, 30, 17], edit=low(0, 2, 49))
    pair("lower case at the first byte of R2's plane", lens1=[40, 33, 50], lens2=[41, 30, 17], edit=low(1, 0, 0))
    pair("lower case at the last byte of R2's plane", lens1=[40, 33, 50], lens2=[41, 30, 17], edit=low(1, 2, 16))
    pair("lower case in the last, partial group only (16 n + 1 bases)", lens1=[16, 17], lens2=[5, 5], edit=low(0, 1, 16))
    pair("all lower case, both sides", lens1=[64, 64], lens2=[63, 65],
         edit=lambda r1, r2: [_set(r, k, seq=r[k][1].lower()) for r in (r1, r2) for k in range(2)])
    # ---- every byte value in a sequence line except CR and LF: only a-z change
    every = bytes(b for b in range(256) if b not in (10, 13))
    for side in (0, 1):
        pair("every byte value in a sequence line of R%d" % (side + 1), lens1=[len(every), 5], lens2=[len(every), 5],
             edit=(lambda sd: lambda r1, r2: _set((r1, r2)[sd], 0, seq=every))(side))
    # ---- quality bytes at the edges of the range, at the first byte, the last byte and a 16-byte seam of the plane
    for v in (32, 33, 126, 127):
        for where, (k, at) in (("first byte", (0, 0)), ("last byte", (2, 29)), ("byte 15", (0, 15)), ("byte 16", (0, 16))):
            side = (v + at) % 2
            pair("quality %d at the %s of R%d's plane" % (v, where, side + 1), lens1=[20, 10, 30], lens2=[20, 10, 30],
                 edit=(lambda sd, kk, aa, vv: lambda r1, r2: _set((r1, r2)[sd], kk, qual=_with_byte((r1, r2)[sd][kk][2], aa, vv)))(side, k, at, v))
    pair("quality 200 in R2", lens1=[20, 10], lens2=[20, 10], edit=lambda r1, r2: _set(r2, 1, qual=_with_byte(r2[1][2], 3, 200)))
    # ---- the merge kernel's limit of 12 000 bases a pair (the one place where a read is longer than 301)
    pair("a pair of exactly 12000 bases", lens1=[30, 6000, 12], lens2=[25, 6000, 14])
    pair("a pair of 12001 bases", lens1=[30, 6000, 12], lens2=[25, 6001, 14])
    # ---- declined
    pair("unequal record counts: R2 one short", lens1=[5, 6, 7], lens2=[5, 6])
    pair("unequal record counts: R1 empty", lens1=[], lens2=[4])
    good = text_of(rand_recs(rng, [12, 9], b"g"))
    bad = {"lines": good + b"\n", "title": good.replace(b"@g1", b"g1"), "plus": good.replace(b"\n+\n", b"\n-\n", 1), "qual": good[:-2] + b"\n"}
    for k, (why, t) in enumerate(sorted(bad.items())):
        c.append(("R%d declined: %s" % (k % 2 + 1, why), t if k % 2 == 0 else good, good if k % 2 == 0 else t))
    c.append(("both declined: R1's reason is named", bad["plus"], bad["title"]))
    _CASES = c
    return c


def _lowered(s, at):
    assert 65 <= s[at] <= 90
    return s[:at] + bytes([s[at] + 32]) + s[at + 1:]


def _with_byte(q, at, v):
    return q[:at] + bytes([v]) + q[at + 1:]


def accepted():
    return [(n, a, b) for n, a, b in cases() if expected(a, b)[0] == "ok"]


def declined():
    return [(n, a, b) for n, a, b in cases() if expected(a, b)[0] == "declined"]


def batch_at_every_offset():
    """17 samples (R1 text, R2 text) whose base counts are 1 mod 16 on R1 and 3 mod 16 on R2: in a batch's joined planes sample k starts at
    k mod 16 on R1 and 3 k mod 16 on R2 -- every plane offset mod 16 on either side.  Mates overlap, so most pairs merge."""
    rng = np.random.default_rng(77)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = []
    for k in range(17):
        r1, r2 = [], []
        for i in range(3):
            frag = bytes(rng.choice(list(b"ACGT"), 200).tolist())
            fl, rl = 112 + 16 * i + (1 if i == 0 else 0), 128 + 16 * i + (3 if i == 0 else 0)
            r1.append((b"s%d_%d 1" % (k, i), frag[:fl], bytes(rng.integers(60, 74, fl, dtype=np.uint8).tolist())))
            r2.append((b"s%d_%d 2" % (k, i), frag[200 - rl:][::-1].translate(comp), bytes(rng.integers(60, 74, rl, dtype=np.uint8).tolist())))
        assert sum(len(r[1]) for r in r1) % 16 == 1 and sum(len(r[1]) for r in r2) % 16 == 3
        out.append((text_of(r1, b"\r\n" if k == 5 else b"\n"), text_of(r2)))
    return out


# ------------------------------------------------------------------ the catalogue as one file, for the stand-alone sanitizer program
def write_corpus_file(path):
    """per case: int32 expected reason (0: accepted), int32 expected side, int64 nbytes1, text1, int64 nbytes2, text2; for an accepted case
    then int64 n, int32 flags, int64 max_total and per side off[n + 1], toff[n + 1] (int64), int64 nb, seq, qual, int64 nt, titles.
    Returns (accepted, declined)."""
    good = bad = 0
    with open(path, "wb") as f:
        for _, t1, t2 in cases():
            e = expected(t1, t2)
            ok = e[0] == "ok"
            f.write(struct.pack("<ii", 0 if ok else REASON[e[1]][0], -1 if ok else e[2]))
            f.write(struct.pack("<q", len(t1)) + t1 + struct.pack("<q", len(t2)) + t2)
            if not ok:
                bad += 1
                continue
            good += 1
            m = e[1]
            f.write(struct.pack("<qiq", m["n"], m["flags"], m["max_total"]))
            for s in m["sides"]:
                f.write(np.array(s["off"], "<i8").tobytes() + np.array(s["toff"], "<i8").tobytes())
                f.write(struct.pack("<q", len(s["seq"])) + s["seq"] + s["qual"] + struct.pack("<q", len(s["titles"])) + s["titles"])
    return good, bad
