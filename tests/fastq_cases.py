"""FASTQ texts for the device parse (csrc/fastq_rec.h, csrc/k_fastq.hip) and an independent statement of what the engine's host parser
(parse_fastx_range in csrc/engine.hip) makes of a text.  The host parser reads line by line (a newline ends a line, a last line without
one counts, one '\\r' before the end of a non-empty line is dropped), skips blank lines ONLY where it expects a title, and takes the
three lines after an '@' title as bases, '+' line and qualities whatever they look like.  The device rule accepts less -- exactly 4
lines per record throughout -- and where it accepts, the records must be these."""
import struct

import numpy as np

# the decline reasons of csrc/fastq_rec.h: code, and the words the message names it by
REASON = {"lines": (1, "line count is not a multiple of four"), "title": (2, "title line is empty or lacks '@'"),
          "plus": (3, "third line is empty or lacks '+'"), "qual": (4, "quality and sequence differ in length")}


def lines_of(text):
    """the host parser's lines: split at newlines, a last line without a newline counts, one trailing CR dropped"""
    parts = text.split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def host_parse(text):
    """the records [(title line, bases, qualities)] the host parser returns for FASTQ text, or "malformed" where it raises on a record,
    "fasta" where it takes the FASTA branch, "neither" where a line that should start a record starts with neither '@' nor '>'"""
    lines = lines_of(text)
    recs, i = [], 0
    while i < len(lines):
        title = lines[i]
        i += 1
        if title == b"":
            continue
        if title[:1] == b"@":
            if i + 3 > len(lines):
                return "malformed"
            seq, plus, qual = lines[i:i + 3]
            i += 3
            if plus == b"" or plus[:1] != b"+" or len(qual) != len(seq):
                return "malformed"
            recs.append((title, seq, qual))
        elif title[:1] == b">":
            return "fasta"
        else:
            return "neither"
    return recs


def planes(recs):
    """what the parse leaves for these records: off, toff (lists of n + 1), seq, qual, titles (bytes)"""
    off, toff = [0], [0]
    for t, s, _ in recs:
        off.append(off[-1] + len(s))
        toff.append(toff[-1] + len(t))
    return off, toff, b"".join(r[1] for r in recs), b"".join(r[2] for r in recs), b"".join(r[0] for r in recs)


def identifiers(recs):
    """the read names: the title after its '@' up to the first blank or tab"""
    out = []
    for t, _, _ in recs:
        name = t[1:]
        for k, c in enumerate(name):
            if c in b" \t":
                name = name[:k]
                break
        out.append(name)
    return out


def _rec(k, L, eol=b"\n"):
    seq = bytes(b"ACGTN"[(k * 7 + j * 3) % 5] for j in range(L))
    qual = bytes(33 + (k + j) % 40 for j in range(L))
    return b"@r%d len=%d" % (k, L) + eol + seq + eol + b"+" + eol + qual + eol


def accepted():
    """(name, text): the device rule accepts each, and the host parser returns the same records"""
    c = [("0 bytes", b"")]
    for n in (1, 2, 3):
        c.append(("%d records" % n, b"".join(_rec(k, 5 + 3 * k) for k in range(n))))
    c.append(("no final newline", b"".join(_rec(k, 4 + k) for k in range(3))[:-1]))
    c.append(("CRLF", b"".join(_rec(k, 6 + k, b"\r\n") for k in range(3))))
    c.append(("CRLF, no final line end", b"".join(_rec(k, 6 + k, b"\r\n") for k in range(2))[:-2]))
    c.append(("a lone CR ends the unterminated last line", _rec(0, 7) + _rec(1, 9)[:-1] + b"\r"))
    c.append(("a title that is just @", b"@\nACGT\n+\nIIII\n" + _rec(1, 3)))
    c.append(("a title that is just @, CRLF", b"@\r\nACGT\r\n+\r\nIIII\r\n"))
    c.append(("tabs and blanks in titles", b"@a b\tc  d\nAC\n+\nII\n@\te f\nG\n+\nI\n@ lead\nTT\n+\nII\n"))
    c.append(("@ and + open the qualities", b"@a\nACG\n+\n@II\n@b\nGT\n+\n+I\n@c\nA\n+c again\n@\n@d\nC\n+\n+\n"))
    c.append(("an empty sequence with an empty quality", b"@a\n\n+\n\n@b\nAC\n+\nII\n@c\n\n+\n\n"))
    c.append(("only empty sequences, CRLF", b"@a\r\n\r\n+\r\n\r\n"))
    c.append(("lower case and IUPAC", b"@x\nacgtnRYKM\n+x\nIIIIIIIII\n"))
    c.append(("a CR inside a line stays", b"@a\rb\nAC\n+\nI\rI\n".replace(b"AC", b"A\rC")))
    return c


def declined():
    """(name, text, reason, record, what the host parser makes of it): the device rule declines each for `reason` at `record` (-1: the text
    as a whole); the last entry is the number of records the host parser returns, or the word host_parse gives"""
    a, b = _rec(0, 5), _rec(1, 7)
    c = [("FASTA", b">a\nACGT\n>b\nGG\n", "title", 0, "fasta"),
         ("FASTA of an odd line count", b">a\nACGT\nAC\n", "lines", -1, "fasta"),
         ("a leading blank line", b"\n" + a + b, "lines", -1, 2),
         ("a blank line between records", a + b"\n" + b, "lines", -1, 2),
         ("four blank lines between records", a + b"\n\n\n\n" + b, "title", 1, 2),
         ("a trailing blank line", a + b + b"\n", "lines", -1, 2),
         ("four trailing blank lines, CRLF", _rec(0, 5, b"\r\n") + b"\r\n\r\n\r\n\r\n", "title", 1, 1),
         ("4n + 1 lines", a + b + b"@c\n", "lines", -1, "malformed"),
         ("4n + 3 lines: the qualities are missing", a + b"@c\nAC\n+\n", "lines", -1, "malformed"),
         ("a missing +", a + b"@c\nAC\n-\nII\n", "plus", 1, "malformed"),
         ("an empty third line", b"@c\nAC\n\nII\n" + a, "plus", 0, "malformed"),
         ("the quality one shorter", a + b + b"@c\nACG\n+\nII\n", "qual", 2, "malformed"),
         ("the quality one longer", b"@c\nACG\n+\nIIII\n" + a, "qual", 0, "malformed"),
         ("the quality one longer by a CR inside", a + b"@c\nACG\n+\nII\rI\n", "qual", 1, "malformed"),
         ("a title without @", a + b"c\nAC\n+\nII\n", "title", 1, "neither"),
         ("two bad records: the lower one is named", a + b"@c\nAC\n-\nII\n" + b"d\nAC\n+\nII\n" + b, "plus", 1, "malformed"),
         ("only a newline", b"\n", "lines", -1, 0),
         ("only CRLF", b"\r\n", "lines", -1, 0),
         ("four blank lines", b"\n\n\n\n", "title", 0, 0)]
    return c


def host_verdict(text):
    h = host_parse(text)
    return len(h) if isinstance(h, list) else h


# ------------------------------------------------------------------ the corpus as one file, for the stand-alone sanitizer program
def write_corpus_file(path):
    """per case: int32 expected reason (0: accepted), int64 expected record (-1), int64 nbytes, the text; for an accepted case then int64 n,
    off[n + 1], toff[n + 1] (int64), int64 nb, seq, qual, int64 nt, titles.  Returns (accepted, declined)."""
    with open(path, "wb") as f:
        for _, text in accepted():
            off, toff, seq, qual, titles = planes(host_parse(text))
            f.write(struct.pack("<iqq", 0, -1, len(text)) + text)
            f.write(struct.pack("<q", len(off) - 1) + np.array(off, "<i8").tobytes() + np.array(toff, "<i8").tobytes())
            f.write(struct.pack("<q", len(seq)) + seq + qual + struct.pack("<q", len(titles)) + titles)
        for _, text, reason, record, _ in declined():
            f.write(struct.pack("<iqq", REASON[reason][0], record, len(text)) + text)
    return len(accepted()), len(declined())
