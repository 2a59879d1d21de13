"""Read orientation (vsearch --orient restated) as a plain statement on Python strings and sets, the catalogue
of edge cases that the oracle (oracle/orc_cluster.c: orc_orient) and the engine (k_orient, k_orient_long, itsx_orient_load_db) are
held to, and a seeded sweep of chimeric reads.  Helper module: no test functions.  tests/test_orient_edges_cpu.py holds the oracle
to it, tests/test_gpu_orient_edges.py the kernels and the database loader.

The procedure.  A read is upper-cased and its U read as T.  A position is usable when its symbol is one of A C G T and DUST
(tests/dust_exact.py) does not mask it.  The read's words are the distinct 12-mers whose twelve positions are all usable; the
database's words are the union over its sequences.  f = the read's words that are database words, v = the read's words whose
reverse complement is a database word (a palindromic word counts on both sides).  The read is forward (+1) when f >= 1 and
f >= 4 v, reverse (-1) when v >= 1 and v >= 4 f, otherwise undetermined (0) and not written.

Documented choices (none of them can be settled without vsearch's sources; the engine and the oracle agree on every one):
 - DUST treats every symbol outside A C G T U as A, so a run of N is a homopolymer to it;
 - a FASTA record starts at a '>' that begins a line and its header runs to the end of that line; a '>' anywhere else in a
   sequence line is an ordinary character outside the alphabet;
 - carriage returns and line feeds never break a word: a sequence folded over several lines is one sequence;
 - every other character of a sequence line that is not an IUPAC nucleotide letter, U or X (either case) -- gaps '-', '.', blanks,
   digits, '*' -- breaks words exactly as N does (vsearch may strip some of these silently instead; parse_fasta spells them N);
 - text before the first header is outside this statement: no case places any.

Nothing here packs bits, rolls a word or calls C: the statement is meant to be read, and to be wrong in other ways than the code.
"""
import collections
import functools
import os
import re

import numpy as np

from dust_exact import py_dust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 12
_COMP = str.maketrans("ACGT", "TGCA")
_RC_ALL = str.maketrans("ACGTURYMKSWHBVDNacgturymkswhbvdn", "TGCAAYRKMSWDVBHNtgcaayrkmswdvbhn")
_ALPHABET = frozenset("ACGTURYMKSWHBVDNX")


def rc(word):
    """reverse complement of a string of A C G T"""
    return word[::-1].translate(_COMP)


def revcomp_read(read):
    """a read as the oriented output writes a reverse one: IUPAC symbols complemented, case kept"""
    return read[::-1].translate(_RC_ALL)


# ---------------------------------------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def words(seq, dust=True):
    s = seq.upper().replace("U", "T")
    masked = py_dust(s) if dust else None
    unusable = [0]                                    # unusable[i] = the unusable positions before i
    for i, c in enumerate(s):
        unusable.append(unusable[-1] + (1 if (c not in "ACGT" or (dust and masked[i])) else 0))
    return frozenset(s[i:i + W] for i in range(len(s) - W + 1) if unusable[i + W] == unusable[i])


@functools.lru_cache(maxsize=64)
def _db_words(seqs, dust):
    out = set()
    for s in seqs:
        out |= words(s, dust)
    return frozenset(out)


def db_words(seqs, dust=True):
    return _db_words(tuple(seqs), dust)


def decide(f, v):
    return 1 if (f >= 1 and f >= 4 * v) else -1 if (v >= 1 and v >= 4 * f) else 0


def orient(db_seqs, reads, dust=True):
    """[(strand, count_fwd, count_rev)] of the reads against the database sequences"""
    db = db_words(db_seqs, dust)
    memo, out = {}, []
    for r in reads:
        if r not in memo:
            ws = words(r, dust)
            f = sum(1 for x in ws if x in db)
            v = sum(1 for x in ws if rc(x) in db)
            memo[r] = (decide(f, v), f, v)
        out.append(memo[r])
    return out


def parse_fasta(data):
    """bytes of a FASTA file -> [(header, sequence)], the sequence as the database loader reads it (see the choices above): line
    ends dropped, letters as they are, every character outside the alphabet spelled N"""
    recs = []
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            recs.append([line[1:].rstrip(b"\r").decode("latin-1"), []])
        elif recs:
            for ch in line.decode("latin-1"):
                if ch != "\r":
                    recs[-1][1].append(ch if ch.upper() in _ALPHABET else "N")
    return [(h, "".join(s)) for h, s in recs]


# ---------------------------------------------------------------------------------------------------------------- the kernels' hash
_HASH_MULT = 2654435761
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _constant(path, name):
    src = open(os.path.join(ROOT, "itsxpress_amd", "csrc", path)).read()
    m = re.search(r"constexpr int %s = (\d+);" % name, src)
    if not m:
        raise AssertionError("%s not found in %s: the orientation edge cases cannot be placed" % (name, path))
    v = int(m.group(1))
    return v


def table_sizes():
    """(OTAB, OL_TAB, OL_BLOCKS): k_orient's LDS set, k_orient_long's set per block, its blocks -- read from the sources"""
    otab, oltab, olb = _constant("k_cluster.hip", "OTAB"), _constant("k_orient.hip", "OL_TAB"), _constant("k_orient.hip", "OL_BLOCKS")
    for t in (otab, oltab):
        if t & (t - 1) or t < 4:
            raise AssertionError("a hash table of %d slots: not a power of two" % t)
    return otab, oltab, olb


def word_value(word):
    """a word's 24-bit value: first base in the low bits, A0 C1 G2 T3"""
    return sum(_CODE[c] << (2 * i) for i, c in enumerate(word))


def value_word(k):
    return "".join("ACGT"[(k >> (2 * i)) & 3] for i in range(W))


def home_slot(word, table):
    return ((word_value(word) * _HASH_MULT) & 0xffffffff) >> (32 - (table.bit_length() - 1))


def words_homed(table, slots, count, rng, exclude=()):
    """`count` distinct words whose home slot is one of `slots`: no palindromes, no word together with its reverse complement.
    The multiplier is odd, so the hash is a bijection of 32-bit values: every value that lands in a slot is k = h / mult mod 2^32,
    and one in 256 of those is a 24-bit word."""
    shift = 32 - (table.bit_length() - 1)
    inv = pow(_HASH_MULT, -1, 1 << 32)
    cand = []
    for slot in slots:
        h = (np.uint64(slot) << np.uint64(shift)) + np.arange(1 << shift, dtype=np.uint64)
        k = (h * np.uint64(inv)) & np.uint64(0xffffffff)
        cand += [int(x) for x in k[k < (1 << 24)]]
    cand = [cand[i] for i in rng.permutation(len(cand))]
    out, taken = [], set(exclude)
    for k in cand:
        w = value_word(k)
        if w == rc(w) or w in taken or rc(w) in taken:
            continue
        taken.add(w)
        out.append(w)
        if len(out) == count:
            return out
    raise AssertionError("only %d of %d words homed in slots %s of a %d-slot table" % (len(out), count, list(slots), table))


# ---------------------------------------------------------------------------------------------------------------- the catalogue
# A case: a database (list of sequences), reads, the masking settings it is compared under, and `check(on, off)`: the property the
# case must show in the MODEL's output (on / off = orient(..., dust=True / False), None for a setting outside `modes`).  The tests
# run every check before anything is compared with the model, so a case that no longer hits its target fails instead of passing idly.
Case = collections.namedtuple("Case", "name db reads modes check")
BOTH, OFF_ONLY = (True, False), (False,)


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), n)) if n else ""


def _join(ws):
    return "N".join(ws)


class _Pools:
    """the words of the shared database and the fillers around them, drawn once"""

    def __init__(self):
        rng = self.rng = np.random.default_rng(20240611)
        self.otab, self.oltab, self.olblocks = table_sizes()
        taken = set()

        def fresh(n):
            out = []
            while len(out) < n:
                w = _rnd(rng, W)
                if w == rc(w) or w in taken or rc(w) in taken:
                    continue
                taken.add(w)
                out.append(w)
            return out

        def palindromes(n):
            out = []
            while len(out) < n:
                h = _rnd(rng, W // 2)
                w = h + rc(h)
                if w not in taken:
                    taken.add(w)
                    out.append(w)
            return out

        self.F, self.R, self.X = fresh(20), fresh(20), fresh(6)
        self.P_in, self.P_out = palindromes(3), palindromes(3)
        self.word, self.both = fresh(1)[0], fresh(1)[0]
        self.S = words_homed(self.otab, (self.otab - 2, self.otab - 1), 64, rng, taken)
        taken |= set(self.S) | {rc(w) for w in self.S}
        self.L = words_homed(self.oltab, range(self.oltab - 4, self.oltab), 64, rng, taken)
        taken |= set(self.L)
        self.word_a = "A" + fresh(1)[0][1:]            # a database word that a rolled 11-mer padded with zero bits would equal
        self.word_aa = "AAAA" + fresh(1)[0][4:]         # ... and one that 8 bases behind a symbol that zeroes the rolled word would equal
        assert self.word_a != rc(self.word_a) and self.word_aa != rc(self.word_aa)
        self.in_db = set(self.F) | {rc(w) for w in self.R} | set(self.P_in) | {self.word, self.both, self.word_a, self.word_aa} | set(self.S[::2]) | set(self.L[::2])
        self.db = [_join(self.F), _join(rc(w) for w in self.R), _join(self.P_in + [self.word, self.both, self.word_a, self.word_aa]), _join(self.S[::2]),
                   _join(self.L[::2])]
        # words joined by a single N: DUST masks none of them, and nothing else becomes a word
        assert db_words(self.db, True) == db_words(self.db, False) == frozenset(self.in_db)
        self.either = self.in_db | {rc(w) for w in self.in_db}

    def filler(self, n):
        """n random bases none of whose words is a database word on either strand"""
        while True:
            s = _rnd(self.rng, n)
            if not (words(s, False) & self.either):
                return s


@functools.lru_cache(maxsize=1)
def pools():
    return _Pools()


def _expect(pairs):
    """check(on, off): the model's output is exactly `pairs` (a list of triples) under every setting compared"""
    def check(on, off):
        for got in (on, off):
            if got is not None:
                assert got == pairs, [(i, g, e) for i, (g, e) in enumerate(zip(got, pairs)) if g != e][:5]
    return check


GRID = 21
NAMED_CELLS = {(0, 0): 0, (1, 0): 1, (0, 1): -1, (4, 1): 1, (3, 1): 0, (1, 4): -1, (1, 3): 0}


def grid_read(f, v):
    p = pools()
    parts = p.F[:f] + p.R[:v] + [p.X[(f + 2 * v) % len(p.X)]]
    k = (7 * f + 3 * v) % len(parts)                 # the words in a different order from cell to cell
    return _join(parts[k:] + parts[:k])


def case_rule_grid():
    p = pools()
    cells = [(f, v) for f in range(GRID) for v in range(GRID)]
    reads = [grid_read(f, v) for f, v in cells]

    def check(on, off):
        for got in (on, off):
            res = dict(zip(cells, got))
            for (f, v), (s, cf, cv) in res.items():
                assert (cf, cv) == (f, v), ((f, v), (cf, cv))
            for cell, s in NAMED_CELLS.items():
                assert res[cell][0] == s, cell
            for k in range(1, 5):                     # both sides of f = 4 v and of v = 4 f
                assert res[(4 * k, k)][0] == 1 and res[(4 * k - 1, k)][0] == 0 and res[(4 * k + 1, k)][0] == 1, k
                assert res[(k, 4 * k)][0] == -1 and res[(k, 4 * k - 1)][0] == 0 and res[(k, 4 * k + 1)][0] == -1, k
            strands = [s for s, _, _ in got]
            assert min(strands.count(x) for x in (1, 0, -1)) >= 60
    return Case("rule_grid", p.db, reads, BOTH, check)


def case_distinct_words():
    p = pools()
    reads = [_join([p.word] * k) for k in (2, 50, 1000)]
    reads += [_join([p.word, p.X[0]] * k) for k in (2, 50, 500)]
    return Case("distinct_words", p.db, reads, OFF_ONLY, _expect([(1, 1, 0)] * len(reads)))


def case_distinct_words_masked():
    """the same reads with the masking on: a word repeated at a period of 13 is a tandem repeat to DUST, which takes the word away
    from the long runs -- the property is the masking's, the comparison with the model is the point"""
    p = pools()
    reads = [_join([p.word] * k) for k in (2, 50, 1000)]

    def check(on, off):
        assert on[0] == (1, 1, 0) and all(t in ((1, 1, 0), (0, 0, 0)) for t in on)
    return Case("distinct_words_masked", p.db, reads, (True,), check)


def case_tandem():
    p = pools()
    reads = [p.word * k for k in (2, 50, 1001)]       # 12 distinct rotations of the word, each counted once
    rot = {(p.word * 2)[i:i + W] for i in range(W)}
    f = len(rot & p.in_db)
    v = len({rc(w) for w in rot} & p.in_db)
    assert len(rot) == W and f == 1 and v == 0

    def check(on, off):
        assert off == [(1, 1, 0)] * 3
    return Case("distinct_words_tandem", p.db, reads, OFF_ONLY, check)


def case_palindromes():
    p = pools()
    reads = [p.P_in[0], _join(p.P_in), p.P_out[0], _join(p.P_out), _join(p.P_in[:1] + p.P_out[:1]), _join(p.P_in[:1] + p.F[:3]),
             _join(p.P_in[:1] + p.F[:4]), _join(p.P_in[:2] + p.R[:6]), _join(p.P_in[:2] + p.R[:5])]
    exp = [(0, 1, 1), (0, 3, 3), (0, 0, 0), (0, 0, 0), (0, 1, 1), (1, 4, 1), (1, 5, 1), (-1, 2, 8), (0, 2, 7)]
    return Case("palindromes", p.db, reads, BOTH, _expect(exp))


def case_both_strands():
    p = pools()
    reads = [_join([p.both, p.X[0], rc(p.both)]), _join([rc(p.both), p.both]), _join([p.F[0], rc(p.F[0]), p.F[1]]),
             _join([p.R[0], rc(p.R[0])]), _join(p.F[:8] + [rc(p.F[0]), rc(p.F[1])]), _join(p.F[:7] + [rc(p.F[0]), rc(p.F[1])])]
    exp = [(0, 1, 1), (0, 1, 1), (0, 2, 1), (0, 1, 1), (1, 8, 2), (0, 7, 2)]
    return Case("both_strands", p.db, reads, BOTH, _expect(exp))


def case_positions():
    p = pools()
    rng = np.random.default_rng(31)
    reads = [_rnd(rng, a) + p.word + _rnd(rng, b) for a in range(34) for b in range(18)]
    exp = [(1, 1, 0)] * len(reads)
    reads += [p.word[:11], p.word, p.word + "A", p.word[1:] + "A", p.word[:1], "ACGTACGTAC", p.word_a, p.word_a[1:], "N" + p.word_a[1:],
              rc(p.word_a), rc(p.word_a)[:11]]
    exp += [(0, 0, 0), (1, 1, 0), (1, 1, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 0), (0, 0, 0), (0, 0, 0), (-1, 0, 1), (0, 0, 0)]
    return Case("positions", p.db, reads, BOTH, _expect(exp))


def case_positions_long():
    """the word at the last twelve bases of reads just past k_orient's 12 011 bases"""
    p = pools()
    reads = [p.filler(12000 + e) + p.word for e in range(16)]
    assert [len(r) for r in reads] == list(range(12012, 12028))
    return Case("positions_long", p.db, reads, BOTH, _expect([(1, 1, 0)] * 16))


def case_spoilers():
    p = pools()
    rng = np.random.default_rng(32)
    reads, exp = [], []

    def spoil(read, pos, sym):
        return read[:pos] + sym + read[pos + 1:]
    for off in range(20, 33):                         # the spoiled positions cross position 32 of the kernels' `bad` bitmap
        base = _rnd(rng, off) + p.word + _rnd(rng, 20)
        for sym in "NRYn":
            for pos in range(off - 1, off + W + 1):
                reads.append(spoil(base, pos, sym))
                exp.append((1, 1, 0) if pos in (off - 1, off + W) else (0, 0, 0))
    for sym in "NRYn":                                # the read's first and last position
        a, b = p.word + _rnd(rng, 9), "A" + p.word + _rnd(rng, 9)
        c, d = _rnd(rng, 9) + p.word, _rnd(rng, 9) + p.word + "A"
        reads += [spoil(a, 0, sym), spoil(b, 0, sym), spoil(c, len(c) - 1, sym), spoil(d, len(d) - 1, sym)]
        exp += [(0, 0, 0), (1, 1, 0), (0, 0, 0), (1, 1, 0)]
    # the tail of a database word right behind a spoiler, in a read that has had twelve good symbols before: A is the zero code, so
    # a word that is cleared but whose run length is kept would be read as the database word
    for sym in "NRYn":
        reads += [_rnd(rng, 15) + sym + p.word_a[1:], _rnd(rng, 20) + sym + p.word_aa[4:] + sym + _rnd(rng, 10), _rnd(rng, 14) + sym + p.word_aa[4:],
                  _rnd(rng, 15) + "A" + p.word_a[1:], _rnd(rng, 20) + "AAAA" + p.word_aa[4:] + sym + _rnd(rng, 10)]
        exp += [(0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 0), (1, 1, 0)]
    return Case("spoilers", p.db, reads, BOTH, _expect(exp))


def _respell(s, how):
    return {0: s.lower(), 1: s.replace("T", "U"), 2: s.lower().replace("t", "u"), 3: s}[how % 4]


def case_case_and_u():
    p = pools()
    db = [_respell(s, i) for i, s in enumerate(p.db)]
    cells = [(1, 0), (0, 1), (4, 1), (3, 1), (1, 4), (1, 3), (8, 2), (7, 2), (20, 5), (5, 20), (0, 0), (20, 20)]
    reads = [_respell(grid_read(f, v), i + k) for k in range(3) for i, (f, v) in enumerate(cells)]
    exp = [(decide(f, v), f, v) for _ in range(3) for f, v in cells]
    assert any("u" in s for s in db) and any("U" in s for s in db) and any("u" in r for r in reads)
    # the same counts as the upper-case T spelling
    assert orient(p.db, [grid_read(f, v) for f, v in cells]) == exp[:len(cells)]
    return Case("case_and_u", db, reads, BOTH, _expect(exp))


_STRETCHES = ("A", "T", "AC", "AT", "GA", "ACG", "TTG", "AAC", "CCG")


def case_dust():
    """low-complexity stretches beside database words, in reads and in database sequences"""
    rng = np.random.default_rng(33)
    low = lambda unit, n: (unit * n)[:n]
    D = [_rnd(rng, W) for _ in range(40)]
    micro = low("AC", 60)
    tail = _rnd(rng, 30)
    # database: words beside stretches; window-edge lengths; a microsatellite; a long sequence with stretches up to its last base
    db = [_rnd(rng, 30) + D[0] + low("A", 40) + D[1] + _rnd(rng, 30), micro, tail + low("A", 40) + _rnd(rng, 30)]
    edge_lens = (7, 8, 63, 64, 65, 95, 96, 97)
    for k, n in enumerate(edge_lens):
        db.append((D[2 + k] + low(_STRETCHES[k % len(_STRETCHES)], n))[:n] if n >= 20 else low("ACGTTGCA", n))
    big = list(_rnd(rng, 70000))
    marks = ((1000, 40, "A"), (31990, 70, "AT"), (32000 + 64 * 300 - 5, 31, "ACG"), (50000, 7, "T"), (60000, 12, "GA"), (70000 - 55, 55, "AC"))
    for pos, n, unit in marks:
        big[pos:pos + n] = low(unit, n)
    big = "".join(big)
    db.append(big)
    reads = []
    # stretches of 7..70 bases that end 0, 1, 11 and 12 bases before a database word
    for n in (7, 8, 12, 20, 31, 32, 33, 45, 64, 70):
        for k, gap in enumerate((0, 1, 11, 12)):
            unit = _STRETCHES[(n + k) % len(_STRETCHES)]
            reads.append(_rnd(rng, 5 + (n % 3)) + low(unit, n) + _rnd(rng, gap) + D[0] + _rnd(rng, 14))
            reads.append(D[1] + _rnd(rng, gap) + low(unit, n))
    # a forward word and the microsatellite's other strand: undetermined without the masking, forward with it
    n_flip = len(reads)
    for n in (24, 30, 40, 41, 52, 60):
        reads.append(_rnd(rng, 20) + D[0] + _rnd(rng, 15) + rc(low("AC", n)))
        reads.append(rc(low("AC", n)) + _rnd(rng, 15) + D[1] + _rnd(rng, 7))
    flips = range(n_flip, len(reads))
    # a word that straddles the end of the database's A run: masked there, unmasked in a read that holds four A's only
    straddle = tail[-8:] + "AAAA"
    i_straddle = len(reads)
    reads.append(_rnd(rng, 25) + straddle + "C" + _rnd(rng, 25))
    # the window-edge lengths as reads, and probes of the database sequences of those lengths
    for k, n in enumerate(edge_lens):
        reads.append(low(_STRETCHES[(k + 3) % len(_STRETCHES)], n))
        reads.append((low(_STRETCHES[k % len(_STRETCHES)], n - W) + D[0]) if n >= 20 else low("ACGTTGCA", n))
        if n >= 20:
            reads += [D[2 + k], db[3 + k][:24], db[3 + k]]
    # probes of the long sequence around every stretch, its last bases included
    for pos, n, unit in marks:
        for a in (pos - 30, pos - 12, pos - 6, pos + n - 6, pos + n, pos + n + 1):
            a = max(0, min(len(big) - 40, a))
            reads.append(big[a:a + 40])
    reads += [big[-12:], big[-40:], big[-100:], rc(big[-100:]), big[31900:32200]]

    def check(on, off):
        differ = [i for i in range(len(reads)) if on[i][0] != off[i][0]]
        assert len(differ) >= 5 and sum(1 for i in flips if on[i][0] == 1 and off[i][0] == 0) >= 5, differ
        # a database word removed by database masking alone: the read keeps it, the unmasked database holds it
        gone = db_words(db, False) - db_words(db, True)
        assert straddle in gone and straddle in words(reads[i_straddle], True) and on[i_straddle][1] == 0 and off[i_straddle][1] == 1
        assert sum(1 for t in on if t[1] > 0) > 40 and any(t[0] == -1 for t in on)
    return Case("dust", db, reads, BOTH, check)


def case_short_table():
    """k_orient's set: a probe chain that wraps from the table's last slots to slot 0, and the fullest legal load"""
    p = pools()
    reads = [_join(p.S), _join(p.S[::-1]), _join(p.S[1::2]), _join(p.S[::2]), _join([rc(w) for w in p.S]),
             p.filler(12011 - W - 1) + "N" + p.word]
    assert len(reads[-1]) == 12011
    exp = [(1, 32, 0), (1, 32, 0), (0, 0, 0), (1, 32, 0), (-1, 0, 32), (1, 1, 0)]

    def check(on, off):
        assert len(p.S) >= 64 and all(home_slot(w, p.otab) in (p.otab - 2, p.otab - 1) for w in p.S)
        assert sum(1 for w in p.S if w in p.in_db) == len(p.S) // 2
        _expect(exp)(on, off)
        assert len(words(reads[-1], False)) > 11900    # (random bases: next to no repeats)
    return Case("short_table", p.db, reads, BOTH, check)


def long_table_reads():
    """(the table read, two long reads that share words with it, short reads that do)"""
    p = pools()
    t = _join(p.L) + "N" + p.filler(12500 - 13 * len(p.L))
    s1 = p.filler(12100) + "N" + _join(p.L[16:48])
    s2 = _join(p.L[32:]) + "N" + p.filler(13000 - 13 * 32)
    assert len(t) == 12500 and len(s2) == 13000 and 12012 <= len(s1) <= 13000
    return t, s1, s2, [_join(p.L[:8]), _join(p.L[40:]), _join([rc(w) for w in p.L[:10]])]


def case_long_table():
    p = pools()
    t, s1, s2, short = long_table_reads()
    reads = [t, short[0], s1, short[1], t, s2, short[2], t]
    exp = [(1, 32, 0), (1, 4, 0), (1, 16, 0), (1, 12, 0), (1, 32, 0), (1, 16, 0), (-1, 0, 5), (1, 32, 0)]

    def check(on, off):
        assert len(p.L) >= 64 and all(home_slot(w, p.oltab) >= p.oltab - 4 for w in p.L)
        _expect(exp)(on, off)
    return Case("long_table", p.db, reads, BOTH, check)


CASE_NAMES = ("rule_grid", "distinct_words", "distinct_words_masked", "distinct_words_tandem", "palindromes", "both_strands",
              "positions", "positions_long", "spoilers", "case_and_u", "dust", "short_table", "long_table")


@functools.lru_cache(maxsize=1)
def catalogue():
    """the cases, in the order of CASE_NAMES"""
    return [case_rule_grid(), case_distinct_words(), case_distinct_words_masked(), case_tandem(), case_palindromes(),
            case_both_strands(), case_positions(), case_positions_long(), case_spoilers(), case_case_and_u(), case_dust(),
            case_short_table(), case_long_table()]


# ---------------------------------------------------------------------------------------------------------------- the sweep
SWEEP_SEED, SWEEP_READS = 6, 2000
EDGE_CLASSES = ("f == 4v", "f == 4v - 1", "v == 4f", "v == 4f - 1", "(1, 0)", "(0, 1)", "(0, 0)")


def edge_classes(out):
    """how many reads of a model output sit in each class of EDGE_CLASSES"""
    n = dict.fromkeys(EDGE_CLASSES, 0)
    for _, f, v in out:
        n["f == 4v"] += f == 4 * v and v >= 1
        n["f == 4v - 1"] += f == 4 * v - 1 and v >= 1
        n["v == 4f"] += v == 4 * f and f >= 1
        n["v == 4f - 1"] += v == 4 * f - 1 and f >= 1
        n["(1, 0)"] += (f, v) == (1, 0)
        n["(0, 1)"] += (f, v) == (0, 1)
        n["(0, 0)"] += (f, v) == (0, 0)
    return n


@functools.lru_cache(maxsize=1)
def sweep():
    """seeded chimeras: a slice of a database sequence of 0..69 bases, then the reverse complement of another slice of 0..69"""
    rng = np.random.default_rng(SWEEP_SEED)
    runs = "".join(_rnd(rng, 40) + ("AT" * 20, "A" * 25, "AT" * 9, "A" * 14)[k % 4] for k in range(12))
    db = [_rnd(rng, 2000), runs]
    reads = []
    for i in range(SWEEP_READS):
        parts = []
        for _ in range(2):
            src = db[int(rng.integers(0, 4) == 0)]
            n = int(rng.integers(0, 70))
            a = int(rng.integers(0, len(src) - n + 1))
            parts.append(src[a:a + n])
        s = parts[0] + rc(parts[1])
        if i % 7 == 0 and s:
            k = int(rng.integers(0, len(s)))
            s = s[:k] + "NRYacgtuU"[int(rng.integers(0, 9))] + s[k + 1:]
        if i % 11 == 0:
            s = s.lower()
        reads.append(s)

    def check(on, off):
        n = edge_classes(on)
        assert all(n[c] >= 3 for c in EDGE_CLASSES), n
        strands = [s for s, _, _ in on]
        assert min(strands.count(x) for x in (1, 0, -1)) >= 400, [strands.count(x) for x in (1, 0, -1)]
    return Case("sweep", db, reads, BOTH, check)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "sweep":
        return sweep()
    cases = catalogue()
    assert tuple(c.name for c in cases) == CASE_NAMES
    return cases[CASE_NAMES.index(name)]


def model_outputs(case):
    """(on, off) of a case: the model under the settings the case is compared under, None for the others"""
    return tuple(orient(case.db, case.reads, d) if d in case.modes else None for d in (True, False))


@functools.lru_cache(maxsize=None)
def outputs(name):
    """model_outputs of a case by name, computed once per process"""
    return model_outputs(case(name))
