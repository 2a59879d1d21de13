"""The inputs of the device-inflate tests (tests/test_device_inflate_cpu.py, tests/test_gpu_device_inflate.py): gzip members made by
zlib at every setting that changes the block type, and members written bit by bit for what zlib never emits (the window's edge, every
first and last length and distance, the corners of the code-length alphabet, and every malformation the decoder refuses).  A shared
helper, not a test.  Truth is Python's zlib / gzip on the same bytes: every hand-made good member is checked against gzip.decompress
where it is built, every bad one against zlib.decompressobj(31)."""
import gzip
import struct
import zlib

import numpy as np

_ACGT = np.array(list("ACGT"))
SETTINGS = [("level0", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("level1", 1, zlib.Z_DEFAULT_STRATEGY),
            ("level9", 9, zlib.Z_DEFAULT_STRATEGY), ("rle", 6, zlib.Z_RLE), ("huffman", 6, zlib.Z_HUFFMAN_ONLY)]
FIRST_BTYPE = {"level0": 0, "fixed": 1, "level1": 2, "level9": 2, "rle": 2, "huffman": 2}
LENGTHS = [0, 1, 2, 3, 4, 257, 258, 259, 32767, 32768, 32769, 65535, 65536, 200000]


def fastq_like(rng, nbytes):
    """as tests/test_gpu_device_deflate.py::_fastq_like draws them"""
    parts, have = [], 0
    i = 0
    while have < nbytes:
        L = int(rng.integers(50, 301))
        rec = "@read%d len=%d\n%s\n+\n%s\n" % (i, L, "".join(_ACGT[rng.integers(0, 4, L)]), "".join(chr(c) for c in rng.integers(35, 74, L)))
        parts.append(rec)
        have += len(rec)
        i += 1
    return "".join(parts).encode()[:nbytes]


# ------------------------------------------------------------------ gzip framing
def header(fname=None, fcomment=None, fextra=None, fhcrc=False, mtime=0, xfl=0, os_=255, cm=8, reserved=0, fhcrc_xor=0):
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0) | reserved
    h = bytes([0x1f, 0x8b, cm, flg]) + struct.pack("<I", mtime) + bytes([xfl, os_])
    if fextra is not None:
        h += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", ((zlib.crc32(h) & 0xffff) ^ fhcrc_xor))
    return h


def wrap(deflate, text, hdr=None, crc=None, isize=None):
    return ((header() if hdr is None else hdr) + deflate + struct.pack("<II", zlib.crc32(text) & 0xffffffff if crc is None else crc,
                                                                       len(text) & 0xffffffff if isize is None else isize))


def member(data, level, strategy, hdr=None, flush_at=None, flush_mode=None):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    if flush_at is None:
        z = co.compress(data) + co.flush()
    else:
        z = co.compress(data[:flush_at]) + co.flush(flush_mode) + co.compress(data[flush_at:]) + co.flush()
    return z if hdr is None else hdr + z[10:]


def first_btype(gz):
    """BTYPE of the first block of a member whose header has no optional field"""
    return (gz[10] >> 1) & 3


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ------------------------------------------------------------------ a deflate stream bit by bit
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def canon(lens):
    """symbol -> (code, length), RFC 1951 3.2.2"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lens):
    """the code's Kraft sum scaled by 2^15"""
    return sum(1 << (15 - l) for l in lens if l)


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, val, nbits):
        self.acc |= val << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):
        c, l = cl
        self.put(int(format(c, "0%db" % l)[::-1], 2), l)           # Huffman codes go in MSB first

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


class Block:
    """tokens of one coded block; text keeps what a decoder should have produced"""

    def __init__(self, bits, ll, d, text):
        self.b, self.ll, self.d, self.text = bits, canon(ll), canon(d), text

    def lit(self, x):
        self.b.code(self.ll[x])
        self.text.append(x)

    def lits(self, data):
        for x in data:
            self.lit(x)

    def match(self, length, dist, apply=True):
        k = max(i for i in range(29) if _LBASE[i] <= length) if length < 258 else 28
        self.b.code(self.ll[257 + k])
        self.b.put(length - _LBASE[k], _LEXT[k])
        j = max(i for i in range(30) if _DBASE[i] <= dist)
        self.b.code(self.d[j])
        self.b.put(dist - _DBASE[j], _DEXT[j])
        if apply:
            for _ in range(length):
                self.text.append(self.text[-dist])

    def eob(self):
        self.b.code(self.ll[256])


def block_header(b, final, btype):
    b.put(1 if final else 0, 1)
    b.put(btype, 2)


def fixed_block(b, text, final=True):
    block_header(b, final, 1)
    return Block(b, FIXED_LL, FIXED_D, text)


def complete_lengths(k):
    """k >= 2 code lengths of a complete code"""
    m = max(1, (k - 1).bit_length())
    short = (1 << m) - k
    return [m - 1] * short + [m] * (k - short)


def dynamic_header(b, hlit, hdist, seq, final=True, cl_lens=None):
    """BTYPE 2 and its header from the code-length symbols seq = [(symbol, value of its extra bits)]"""
    block_header(b, final, 2)
    used = sorted({s for s, _ in seq})
    if cl_lens is None:
        names = used if len(used) > 1 else used + [(used[0] + 1) % 19]
        cl_lens = [0] * 19
        for s, l in zip(names, complete_lengths(len(names))):
            cl_lens[s] = l
    hclen = max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1
    hclen = max(hclen, 4)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl_lens[CL_ORDER[i]], 3)
    cl = canon(cl_lens)
    for s, e in seq:
        b.code(cl[s])
        b.put(e, {16: 2, 17: 3, 18: 7}.get(s, 0))


def expand_seq(seq):
    out = []
    for s, e in seq:
        if s < 16:
            out.append(s)
        elif s == 16:
            out.extend([out[-1]] * (3 + e))
        elif s == 17:
            out.extend([0] * (3 + e))
        else:
            out.extend([0] * (11 + e))
    return out


def dynamic_block(b, hlit, hdist, seq, text, final=True, cl_lens=None):
    dynamic_header(b, hlit, hdist, seq, final, cl_lens)
    lens = expand_seq(seq)
    assert len(lens) == hlit + hdist, (len(lens), hlit, hdist)
    return Block(b, lens[:hlit], lens[hlit:], text)


def _checked(name, gz, text):
    assert gzip.decompress(gz) == text, name
    return (name, gz, text)


# ------------------------------------------------------------------ the corpora
def _hand_fixed(rng):
    out = []
    base = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))

    def one(name, build):
        b, text = Bits(), bytearray()
        blk = fixed_block(b, text)
        build(blk)
        blk.eob()
        out.append(_checked("fixed:" + name, wrap(b.done(), bytes(text)), bytes(text)))

    def far(blk, length):
        blk.lits(base[:32768])
        blk.match(length, 32768)
    one("distance 32768 length 3 as byte 32769", lambda k: far(k, 3))
    one("distance 32768 length 258 as byte 32769", lambda k: far(k, 258))
    one("distance 1 length 258 after one literal", lambda k: (k.lit(0x61), k.match(258, 1)))

    def lengths(blk):
        blk.lits(base[:300])
        for i in range(29):
            for L in sorted({_LBASE[i], 257 if i == 27 else _LBASE[i] + (1 << _LEXT[i]) - 1}):          # (258 is code 285's)
                blk.match(L, 7 + i)
    one("first and last length of every length code", lengths)

    def distances(blk):
        blk.lits(base[:32768])
        for j in range(30):
            for D in sorted({_DBASE[j], _DBASE[j] + (1 << _DEXT[j]) - 1}):
                blk.match(3 + j % 5, D)
    one("first and last distance of every distance code", distances)

    def wraps(blk):
        blk.lits(base[:65536 - 100])
        blk.match(258, 32768)                                      # source crosses 32768, destination crosses 65536
        blk.match(258, 32700)
    one("source and destination wrap the ring", wraps)
    one("match ends on the last byte", lambda k: (k.lits(b"abc"), k.match(3, 3)))
    return out


def _hand_dynamic():
    out = []

    def one(name, hlit, hdist, seq, build, cl_lens=None):
        b, text = Bits(), bytearray()
        blk = dynamic_block(b, hlit, hdist, seq, text, cl_lens=cl_lens)
        assert kraft(expand_seq(seq)[:hlit]) == 1 << 15, name
        build(blk)
        blk.eob()
        out.append(_checked("dynamic:" + name, wrap(b.done(), bytes(text)), bytes(text)))

    # literals a..o and 256, 4 bits each; no distance code at all
    seq = [(18, 97 - 11), (4, 0), (16, 3), (16, 3), (4, 0), (4, 0), (18, 127), (17, 3), (4, 0), (0, 0)]
    assert len(expand_seq(seq)) == 258
    one("literals only, no distance code", 257, 1, seq, lambda k: k.lits(b"abcdefghijklmno" * 20))
    # literals a..n, 256 and length 3, and a single distance code of one bit
    seq = [(18, 97 - 11), (4, 0), (16, 3), (16, 3), (4, 0), (18, 127), (17, 4), (4, 0), (4, 0), (1, 0)]
    assert len(expand_seq(seq)) == 259
    one("a single 1-bit distance code", 258, 1, seq, lambda k: (k.lits(b"nml"), k.match(3, 1), k.lits(b"abc"), k.match(3, 1)))
    # every repeat code at its shortest and its longest run; 16 literals' worth of 4-bit codes: 138..144, 156..159, 170..173, 256
    seq = [(18, 127), (4, 0), (16, 3), (18, 0), (4, 0), (16, 0), (17, 7), (4, 0), (4, 0), (4, 0), (4, 0), (17, 0), (18, 79 - 11), (4, 0), (0, 0)]
    lens = expand_seq(seq)
    assert len(lens) == 258 and [i for i, l in enumerate(lens) if l] == list(range(138, 145)) + list(range(156, 160)) + list(range(170, 174)) + [256]
    one("repeats 16, 17 and 18 at their shortest and longest", 257, 1, seq, lambda k: k.lits(bytes(list(range(138, 145)) + list(range(156, 160)) + list(range(170, 174))) * 9))
    # a run of 16 that starts in the literal lengths and ends in the distance lengths
    seq = [(18, 97 - 11), (4, 0), (16, 3), (4, 0), (18, 127), (18, 2), (2, 0), (16, 2)]
    lens = expand_seq(seq)
    assert len(lens) == 262 and lens[256:] == [2] * 6 and lens[97:105] == [4] * 8
    one("a run from the literal lengths into the distance lengths", 258, 4, seq,
        lambda k: (k.lits(b"abcdefgh"), k.match(3, 1), k.match(3, 2), k.lits(b"hg"), k.match(3, 3), k.match(3, 4)))
    # literal codes of 1..15 bits (118..132 and 256), a code-length code with 7-bit codes, one 1-bit distance code
    seq = [(18, 118 - 11)] + [(l, 0) for l in range(1, 16)] + [(18, 123 - 11), (15, 0), (1, 0)]
    lens = expand_seq(seq)
    assert len(lens) == 258 and lens[118:133] == list(range(1, 16)) and lens[256] == 15
    cl_lens = [0] * 19
    for s, l in zip([18, 1, 15, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], [2, 2, 3, 4, 5, 6, 7, 7] + [5] * 8):
        cl_lens[s] = l
    assert kraft(cl_lens) == 1 << 15 and max(cl_lens) == 7
    one("a 15-bit literal code and a 7-bit code-length code", 257, 1, seq, lambda k: k.lits(bytes(range(118, 133)) * 3), cl_lens)
    return out


_GOOD = None


def good():
    """[(name, gzip bytes, text)]; built once"""
    global _GOOD
    if _GOOD is not None:
        return _GOOD
    rng = np.random.default_rng(20)
    out = []
    for n in LENGTHS:
        text = fastq_like(rng, n)
        for tag, level, strategy in SETTINGS:
            gz = member(text, level, strategy)
            if n >= 257:
                assert first_btype(gz) == FIRST_BTYPE[tag], (tag, n)
            if tag == "level0" and n == 200000:
                assert gz.count(b"\xff\xff\x00\x00") >= 1 and len(gz) > n      # several stored blocks
            out.append(("%s:%d" % (tag, n), gz, text))
    text = fastq_like(rng, 50000)
    out.append(("sync flush", member(text, 6, zlib.Z_DEFAULT_STRATEGY, flush_at=20001, flush_mode=zlib.Z_SYNC_FLUSH), text))
    out.append(("full flush", member(text, 6, zlib.Z_DEFAULT_STRATEGY, flush_at=30001, flush_mode=zlib.Z_FULL_FLUSH), text))
    noise = bytes(rng.integers(0, 256, 65536, dtype=np.uint8))
    out.append(("random 64 KiB", member(noise, 6, zlib.Z_DEFAULT_STRATEGY), noise))
    text = fastq_like(rng, 3000)
    bc = b"BC" + struct.pack("<HH", 2, 4000)
    for name, h in header_variants(bc):
        out.append(("header:" + name, member(text, 6, zlib.Z_DEFAULT_STRATEGY, hdr=h), text))
    out.append(("header:BGZF EOF member", BGZF_EOF, b""))
    out.append(("an empty member between two full ones", member(text, 6, 0) + member(b"", 6, 0) + member(text[::-1], 1, 0), text + text[::-1]))
    out.extend(_hand_fixed(rng))
    out.extend(_hand_dynamic())
    for name, gz, text in out:
        assert gzip.decompress(gz) == text, name
    _GOOD = out
    return out


def header_variants(bc=b"BC\x02\x00\xa0\x0f"):
    return [("FNAME", header(fname=b"reads.fastq")), ("FCOMMENT", header(fcomment=b"a comment")), ("FEXTRA BGZF", header(fextra=bc)),
            ("FHCRC", header(fhcrc=True)), ("all four flags", header(fname=b"n", fcomment=b"c", fextra=bc, fhcrc=True)),
            ("MTIME", header(mtime=1700000000, xfl=2, os_=3))]


def n_members(name):
    return 3 if name.startswith("an empty member") else 1


def concatenation(seed=5):
    """the whole good corpus as one file in a seeded shuffled order: (gzip bytes, text, members)"""
    cases = good()
    order = np.random.default_rng(seed).permutation(len(cases))
    return (b"".join(cases[i][1] for i in order), b"".join(cases[i][2] for i in order), sum(n_members(cases[i][0]) for i in order))


def zlib_refuses(gz):
    """zlib.decompressobj(31), member after member: an error, a member that does not end, or bytes no member starts at"""
    buf = gz
    while buf:
        d = zlib.decompressobj(31)
        try:
            d.decompress(buf)
        except zlib.error:
            return True
        if not d.eof:
            return True
        buf = d.unused_data
    return False


def _bad_fixed(build):
    b, text = Bits(), bytearray()
    blk = fixed_block(b, text)
    build(blk, b)
    blk.eob()
    return wrap(b.done(), bytes(text))


# csrc/inflate_codes.h: IcReason, and the words itsx_last_error uses for each
REASON = {"header": (2, "bad gzip header"), "fhcrc": (3, "header CRC mismatch"), "btype": (4, "block type 3"), "stored": (5, "stored LEN is not ~NLEN"),
          "oversubscribed": (7, "over-subscribed code"), "incomplete": (8, "incomplete code"), "repeat": (9, "bad repeat in the code lengths"),
          "no_eob": (10, "no code for end of block"), "lsymbol": (11, "literal/length symbol 286 or 287"), "dsymbol": (12, "invalid distance symbol"),
          "distance": (13, "distance beyond the member's start"), "output": (14, "output beyond ISIZE"), "input": (15, "input beyond the member's end"),
          "trailer": (16, "deflate data does not end 8 bytes before the member's end"), "short": (17, "fewer bytes than ISIZE"), "crc": (18, "CRC-32 mismatch"),
          "expansion": (21, "more text than deflate expands to")}
# the refusal each bad case is built to meet.  A member cut short also loses its ISIZE: the plan reads four bytes of what is left, so the
# decoder runs out of input, or, where those bytes happen to name fewer bytes than the text, out of output first -- or, on the device,
# the plan refuses them before any decoding because they name more text than deflate can expand the span to.  Garbage after the last
# member is that member's trailer as far as the plan can tell: the same refusal there, or the deflate data not ending where it should.
_WHY = [("distance", ("distance",)), ("BTYPE 3", ("btype",)), ("NLEN", ("stored",)), ("over-subscribed", ("oversubscribed",)), ("incomplete", ("incomplete",)),
        ("repeat", ("repeat",)), ("no code for 256", ("no_eob",)), ("symbol 286", ("lsymbol",)), ("cut ", ("input", "output", "expansion")), ("wrong CRC", ("crc",)),
        ("ISIZE one too small", ("output",)), ("ISIZE one too large", ("short",)), ("garbage", ("trailer", "expansion")), ("reserved FLG", ("header",)),
        ("wrong FHCRC", ("fhcrc",))]


def _why(name):
    if name.startswith("distance symbol 30"):
        return ("dsymbol",)
    hits = [w for key, w in _WHY if key in name]
    assert len(hits) == 1, name
    return hits[0]


_BAD = None


def bad():
    """[(name, gzip bytes, verified: the text of the members before the one that is refused, the REASON keys it may be refused for)]"""
    global _BAD
    if _BAD is not None:
        return _BAD
    rng = np.random.default_rng(21)
    base = bytes(rng.integers(0, 256, 40000, dtype=np.uint8))
    text = fastq_like(rng, 5000)
    okm = member(text, 6, 0)
    out = []
    # a distance one larger than the bytes produced: 1 with none, 2 with one, 32768 (the largest there is) with 32767
    out.append(("distance 1 with nothing produced", _bad_fixed(lambda k, b: k.match(3, 1, apply=False)), b""))
    out.append(("distance 2 with one byte produced", _bad_fixed(lambda k, b: (k.lit(65), k.match(3, 2, apply=False))), b""))
    out.append(("distance 32768 with 32767 bytes produced", _bad_fixed(lambda k, b: (k.lits(base[:32767]), k.match(3, 32768, apply=False))), b""))
    # the same in the second member, where the bytes reached for would be the first member's
    out.append(("distance into the member before", okm + _bad_fixed(lambda k, b: (k.lit(65), k.match(3, 2, apply=False))), text))
    out.append(("distance reaching 32768 back into the member before", member(base[:32768], 0, 0) + _bad_fixed(lambda k, b: (k.lits(b"xy"), k.match(258, 32768, apply=False))), base[:32768]))

    def dsym30(k, b):
        k.lits(b"abcdef")
        b.code(k.ll[257])
        b.put(int(format(30, "05b")[::-1], 2), 5)
    out.append(("distance symbol 30", _bad_fixed(dsym30), b""))
    out.append(("literal/length symbol 286", _bad_fixed(lambda k, b: (k.lits(b"abc"), b.code(canon(FIXED_LL)[286]))), b""))
    b = Bits()
    block_header(b, False, 0)
    b.align()
    b.out += struct.pack("<HH", 5, 0xffff ^ 5) + b"hello"
    block_header(b, True, 3)
    out.append(("BTYPE 3 in the second block", wrap(b.done(), b"hello"), b""))
    b = Bits()
    block_header(b, True, 0)
    b.align()
    b.out += struct.pack("<HH", 5, (0xffff ^ 5) ^ 0x100) + b"hello"
    out.append(("NLEN mismatch", wrap(b.done(), b"hello"), b""))

    def dyn(name, hlit, hdist, seq, lits=b""):
        b = Bits()
        dynamic_header(b, hlit, hdist, seq)
        b.put(0, 40)
        out.append((name, wrap(b.done(), lits), b""))
    dyn("an over-subscribed code", 257, 1, [(18, 97 - 11), (1, 0), (1, 0), (1, 0), (18, 127), (18, 256 - 100 - 138 - 11), (1, 0), (0, 0)])
    dyn("an incomplete literal code", 257, 1, [(18, 97 - 11), (2, 0), (18, 127), (18, 256 - 98 - 138 - 11), (2, 0), (0, 0)])
    dyn("repeat-16 first", 257, 1, [(16, 0), (18, 127)])
    dyn("a repeat past HLIT + HDIST", 257, 1, [(18, 127), (18, 127)])
    dyn("no code for 256", 257, 1, [(18, 97 - 11), (1, 0), (1, 0), (18, 127), (18, 258 - 99 - 138 - 11)])
    for cut in (1, 8, 9):
        out.append(("cut %d short" % cut, okm[:-cut], b""))
    out.append(("cut mid-block", okm[:len(okm) // 2], b""))
    out.append(("cut short after a whole member", okm + okm[:-9], text))
    out.append(("wrong CRC", okm[:-8] + struct.pack("<I", (zlib.crc32(text) ^ 0x10) & 0xffffffff) + okm[-4:], b""))
    out.append(("ISIZE one too small", okm[:-4] + struct.pack("<I", len(text) - 1), b""))
    out.append(("ISIZE one too large", okm[:-4] + struct.pack("<I", len(text) + 1), b""))
    out.append(("3 bytes of garbage after the last member", okm + okm + b"\x00\x01\x02", text))
    out.append(("reserved FLG bit in the first header", member(text, 6, 0, hdr=header(reserved=0x20)), b""))
    out.append(("wrong FHCRC", member(text, 6, 0, hdr=header(fhcrc=True, fhcrc_xor=1)), b""))
    for name, gz, _ in out:
        assert zlib_refuses(gz), name
    _BAD = [(name, gz, verified, _why(name)) for name, gz, verified in out]
    return _BAD


def nested():
    """well-formed, and the device must decline it: a level-0 member whose text is itself a complete .gz file"""
    inner = member(fastq_like(np.random.default_rng(22), 4000), 6, 0)
    gz = member(inner, 0, 0)
    assert gzip.decompress(gz) == inner and gz.count(b"\x1f\x8b\x08") == 2
    return gz, inner


def near_misses():
    """positions that are no member start: [(name, bytes)] -- each a good small member but for one thing"""
    text = b"ACGT" * 10
    ok = member(text, 6, 0, hdr=header())
    cut_hdr = header(fname=b"a-long-name-that-the-buffer-cuts")
    return [("1f 8b 09", ok[:2] + b"\x09" + ok[3:]), ("reserved FLG bit", ok[:3] + b"\x80" + ok[4:]), ("XFL 1", ok[:8] + b"\x01" + ok[9:]),
            ("OS 14", ok[:9] + b"\x0e" + ok[10:]), ("a header cut by the buffer's end", cut_hdr[:-3]), ("a header and no block after it", header())]


# ------------------------------------------------------------------ the sanitizer program's input
def write_corpus_file(path):
    """every good case (flag 1, its text) and every bad one (flag 0, the text of the members that verify): u32 count, then per case
    u32 name length, name, u8 flag, u64 gzip length, bytes, u64 text length, text"""
    cases = [(n, g, t, 1) for n, g, t in good()] + [(n, g, t, 0) for n, g, t, _ in bad()]
    cat = concatenation()
    cases.append(("the whole corpus as one file", cat[0], cat[1], 1))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for name, gz, text, flag in cases:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<BQ", flag, len(gz)) + gz + struct.pack("<Q", len(text)) + text)
    return len(cases)
