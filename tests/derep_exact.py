"""Exact dereplication as plain text, and ONE catalogue of the cases at which the engine's packed form can go wrong, shared by
tests/test_derep_edges_cpu.py and tests/test_gpu_derep_edges.py.

The model shares nothing with the engine (csrc/k_derep.hip) or the oracle (oracle/orc_derep.c): no 2-bit packing, no hash, no
residue codes.  One pass in input order over a dict from text to first index; a read joins its own text first (+1), then its reverse
complement (-1), else it seeds.

Every case is named and seeded: Case(name, seqs, strand_both, minlen, sample); GROUPS[name]() -> [Case].  Every builder checks its
own premise with the model and asserts it, so a case list cannot degenerate without a test turning red.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name seqs strand_both minlen sample")

_COMP = str.maketrans("ACGTRYMKSWHBVDN", "TGCAYRKMSWDVBHN")
AMBIG = "NRYSWKMBDHV"
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 95, 96, 97, 111, 112, 113, 127, 128, 129, 255, 256, 257)


# ---------------------------------------------------------------- the model
def norm(s):
    return s.upper().replace("U", "T")


def rc(s):
    """reverse complement of normalised text"""
    return s[::-1].translate(_COMP)


def derep(seqs, strand_both=True, minlen=1, sample=None):
    """-> (n_unique, rep_of int64[n], strand int8[n], uniq_of int64[n], seed_read int64[U], abundance int64[U])"""
    n = len(seqs)
    rep_of = np.full(n, -1, np.int64)
    strand = np.zeros(n, np.int8)
    first = {}
    for i, s in enumerate(seqs):
        if len(s) < minlen:
            continue
        d = first.setdefault(0 if sample is None else int(sample[i]), {})
        t = norm(s)
        if t in d:
            rep_of[i], strand[i] = d[t], 1
        elif strand_both and rc(t) in d:
            rep_of[i], strand[i] = d[rc(t)], -1
        else:
            d[t] = i
            rep_of[i], strand[i] = i, 1
    seed_read = np.nonzero(rep_of == np.arange(n))[0].astype(np.int64)
    rank = np.full(n + 1, -1, np.int64)
    rank[seed_read] = np.arange(len(seed_read))
    uniq_of = rank[rep_of]                                   # (rep_of == -1 reads rank[n] = -1)
    abundance = np.bincount(uniq_of[uniq_of >= 0], minlength=len(seed_read)).astype(np.int64)
    return len(seed_read), rep_of, strand, uniq_of, seed_read, abundance


def global_derep(shards, strand_both=True, minlen=1):
    """the same pass over the concatenation of the shards, and per shard what its own derep gives"""
    whole = derep([s for sh in shards for s in sh], strand_both, minlen)
    return whole, [derep(sh, strand_both, minlen) for sh in shards]


def n_minus(case):
    return int((derep(case.seqs, case.strand_both, case.minlen, case.sample)[2] == -1).sum())


def n_key_words(s):
    """words of the engine's key for this text: packed words + exceptions + the length word (what the xxh_shapes group walks)"""
    t = norm(s)
    return (len(t) + 15) // 16 + sum(c not in "ACGT" for c in t) + 1


# ---------------------------------------------------------------- helpers
def _rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), int(n)))


def _other(rng, base):
    return str(rng.choice([b for b in "ACGT" if b != base]))


def _put(s, p, c):
    return s[:p] + c + s[p + 1:]


def _expect(seqs, n_unique, minus, strand_both=True, what=""):
    nu, _, strand, _, _, _ = derep(seqs, strand_both)
    assert (nu, int((strand == -1).sum())) == (n_unique, minus), (what, nu, int((strand == -1).sum()), n_unique, minus)


# ---------------------------------------------------------------- word_edges
def _word_reads(rng, L):
    """the reads of one length, the reverse complement before the forward read"""
    t = _rnd(rng, L)
    while rc(t) == t:
        t = _rnd(rng, L)
    last = t[:-1] + _other(rng, t[-1])
    reads = [rc(t), t, t + "A", rc(t + "A"), last, rc(last), "A" + t, rc("A" + t), t.lower(), rc(t).replace("T", "u"), t + "T", rc(t + "T")]
    return t, reads


def word_edges():
    rng = np.random.default_rng(301)
    out, every = [], []
    for L in LENGTHS:
        t, reads = _word_reads(rng, L)
        # the zero-padding pairs stand apart whatever else happens at a tiny length
        _, rep, _, _, _, _ = derep(reads)
        assert rep[2] != rep[1] and rep[6] != rep[1] and rep[10] != rep[1], L        # t+"A", "A"+t, t+"T" never join t
        if L >= 15:                                                                 # five sequences, each once per strand; t three times more
            _expect(reads, 5, 6, what="word_edges L%d" % L)
            _expect(reads, 10, 0, strand_both=False, what="word_edges+ L%d" % L)
        out.append(Case("L%d" % L, reads, True, 1, None))
        every += reads
    order = rng.permutation(len(every))
    shuffled = [every[i] for i in order]
    out.append(Case("all_lengths_shuffled", shuffled, True, 1, None))
    out.append(Case("all_lengths_shuffled_plus", shuffled, False, 1, None))
    return out


# ---------------------------------------------------------------- exceptions
def _exc_positions(L):
    return sorted({min(max(p, 0), L - 1) for p in (0, 15, 16, L // 2, L - 17, L - 16, L - 1)})


def _exc_reads(rng, L):
    pos = _exc_positions(L)
    t = list(_rnd(rng, L))
    for p in pos:                                            # no A at the probed positions: "A at p" is then always another read
        t[p] = str(rng.choice(list("CGT")))
    t = "".join(t)
    reads, nu, minus = [], 0, 0

    def both(x, flip):
        nonlocal nu, minus
        reads.extend([rc(x), x] if flip else [x, rc(x)])
        nu += 1
        minus += 1

    k = 0
    for p in pos:
        for c in AMBIG:
            both(_put(t, p, c), k % 2 == 1)
            k += 1
        reads.append(_put(t, p, "A"))                        # differs from "N at p" only by the exception list
        nu += 1
    for m in (2, 3, 7):                                      # several exceptions of different codes: their order flips under reversal
        ps = {0, L - 1}
        while len(ps) < m:
            ps.add(int(rng.integers(L)))
        x = t
        for p, c in zip(sorted(ps), rng.permutation(list(AMBIG))):
            x = _put(x, p, str(c))
        both(x, m == 3)
    nw = (L + 15) // 16
    w = int(rng.choice([j for j in range(nw) if min(16, L - 16 * j) >= 5]))
    x = t
    for p, c in zip(16 * w + rng.choice(min(16, L - 16 * w), 5, replace=False), rng.permutation(list(AMBIG))):
        x = _put(x, int(p), str(c))
    both(x, True)                                            # five exceptions, all in one word
    if nw >= 3:                                              # one exception in every word (with one or two words it would repeat a read above)
        x = t
        for j in range(nw):
            x = _put(x, 16 * j + int(rng.integers(min(16, L - 16 * j))), AMBIG[(j + L) % len(AMBIG)])
        both(x, False)
    return reads, nu, minus


def exceptions():
    rng = np.random.default_rng(302)
    out = []
    for L in LENGTHS:
        if L < 15:
            continue
        reads, nu, minus = _exc_reads(rng, L)
        _expect(reads, nu, minus, what="exceptions L%d" % L)
        _expect(reads, nu + minus, 0, strand_both=False, what="exceptions+ L%d" % L)
        out.append(Case("L%d" % L, reads, True, 1, None))
        if L in (16, 33, 129):
            out.append(Case("L%d_plus" % L, reads, False, 1, None))
    return out


# ---------------------------------------------------------------- xxh_shapes
def xxh_shapes():
    """key-word counts 2..18 (the stripe loop from 8, the two-word and the one-word tail), reached by length and by exceptions"""
    rng = np.random.default_rng(303)
    reads, seen = [], set()
    for n in range(2, 19):
        shapes = [(16 * (n - 1) - int(rng.integers(0, 16)), 0)]                     # by length alone
        if n >= 3:
            nw = max(1, (n - 1) // 2)
            shapes.append((16 * nw - int(rng.integers(0, 8)), n - 1 - nw))          # by exceptions
        for L, ne in shapes:
            x = _rnd(rng, L)
            ps = sorted(int(p) for p in rng.choice(L, ne, replace=False))
            for p in ps:
                x = _put(x, p, str(rng.choice(list(AMBIG))))
            free = [p for p in range(L) if p not in ps]
            q = free[len(free) // 2]
            nb = _put(x, q, _other(rng, x[q]))
            assert n_key_words(x) == n and n_key_words(nb) == n, (n, L, ne)
            seen.add((n, ne > 0))
            four = [x, x, rc(x), nb]
            _expect(four, 2, 1, what="xxh n=%d" % n)
            reads += four
    assert seen == {(n, False) for n in range(2, 19)} | {(n, True) for n in range(3, 19)}
    return [Case("n2_to_n18", reads, True, 1, None), Case("n2_to_n18_plus", reads, False, 1, None)]


# ---------------------------------------------------------------- palindromes
PALINDROMES = ["ACGT" * 4, "ACGT" * 8, "ACGT" * 9, "ACGTSACGT", "ACGTWACGT", "ACGTNACGT", "N" * 400, "N" * 399]
RC_PAIR = ["ACGTRACGT", "ACGTYACGT"]


def palindromes():
    for p in PALINDROMES:
        assert rc(p) == p
    assert rc(RC_PAIR[0]) == RC_PAIR[1] != RC_PAIR[0]
    seqs = (PALINDROMES + RC_PAIR) * 2
    n = len(PALINDROMES)
    nu, rep, strand, _, _, _ = derep(seqs, True)
    assert nu == n + 1 and all(strand[i] == 1 for i in range(len(seqs)) if seqs[i] in PALINDROMES)      # every join of a palindrome is +1
    assert list(strand[n:n + 2]) == [1, -1] and list(strand[2 * n + 2:]) == [1, -1]
    nu, rep, strand, _, _, _ = derep(seqs, False)
    assert nu == n + 2 and (strand == 1).all()
    return [Case("both", seqs, True, 1, None), Case("plus", seqs, False, 1, None)]


# ---------------------------------------------------------------- first_occurrence
def first_occurrence():
    """20 000 reads of 40 sequences in random orientation.  Sequence k < 20 first stands at index k; the other twenty stand nowhere
    before index 15 000 (so those indices hold other sequences only), and their first occurrences lie wherever the draw puts them
    behind it.  The early ones fill [20, 15 000) (about 750 copies each), the late ones [15 000, 20 000) (250 each)."""
    rng = np.random.default_rng(305)
    uniq = [_rnd(rng, rng.integers(150, 301)) for _ in range(40)]
    pick = np.concatenate([np.arange(20), rng.integers(0, 20, 15000 - 20), rng.integers(20, 40, 5000)])
    flip = rng.random(20000) < 0.5
    seqs = [rc(uniq[k]) if f else uniq[k] for k, f in zip(pick, flip)]
    nu, rep, strand, _, seed, ab = derep(seqs)
    assert nu == 40 and list(seed[:20]) == list(range(20)) and (seed[20:] >= 15000).all() and ab.min() > 150
    assert 0.4 < (strand == -1).mean() < 0.6
    return [Case("forty_sequences", seqs, True, 1, None), Case("forty_sequences_plus", seqs, False, 1, None)]


# ---------------------------------------------------------------- minlen
def minlen():
    rng = np.random.default_rng(306)
    out = []
    for m in (1, 16, 17, 32):
        seqs = [""]
        for L in (m - 1, m, m + 1):
            t = _rnd(rng, L)
            seqs += [t, rc(t), t, ""]
        nu, rep, strand, uq, _, ab = derep(seqs, True, m)
        dropped = sum(len(s) < m for s in seqs)
        assert int((rep < 0).sum()) == dropped == 7 and ab.sum() == len(seqs) - dropped      # three of length m - 1 and four ""
        out.append(Case("minlen%d" % m, seqs, True, m, None))
    out.append(Case("minlen17_plus", out[2].seqs, False, 17, None))
    return out


# ---------------------------------------------------------------- table_edges
def table_edges():
    """the engine's table has the power of two >= 2n + 16 slots, 1 024 at least: n = 504 fills a 1 024-slot table to the last read it
    may hold, n = 505 is the first to take 2 048.  n = 0: the engine accepts an empty read set (derep() == 0)."""
    rng = np.random.default_rng(307)
    out = []
    for n in (0, 1, 504, 505):
        seqs = [_rnd(rng, 40) for _ in range(n)]
        assert derep(seqs)[0] == n
        out.append(Case("n%d" % n, seqs, True, 1, None))
    return out


# ---------------------------------------------------------------- samples
def samples():
    rng = np.random.default_rng(308)
    shared = [_rnd(rng, rng.integers(100, 201)) for _ in range(200)]
    seqs, sample = [], []
    for s in range(3):
        own = [_rnd(rng, rng.integers(100, 201)) for _ in range(50)]
        block = [rc(x) if rng.random() < 0.5 else x for x in shared] + own + [rc(x) for x in own[:10]] + shared[:20]
        block = [block[i] for i in rng.permutation(len(block))]
        seqs += block
        sample += [s] * len(block)
    sample = np.array(sample, np.int32)
    nu, rep, strand, _, seed, _ = derep(seqs, True, 1, sample)
    assert nu == 750 and (sample[rep] == sample).all() and [int((sample[seed] == s).sum()) for s in range(3)] == [250] * 3
    assert derep(seqs, True, 1, None)[0] == 350                  # without samples the shared ones meet
    return [Case("three_samples", seqs, True, 1, sample), Case("three_samples_plus", seqs, False, 1, sample)]


# ---------------------------------------------------------------- length_order
def _with_copies(rng, uniq):
    """the uniques in order, a reverse-complement copy of an earlier one after every 16th: the seed reads are not 0..U-1"""
    seqs = []
    for i, x in enumerate(uniq):
        seqs.append(x)
        if i % 16 == 15:
            seqs.append(rc(uniq[int(rng.integers(i + 1))]))
    return seqs


def length_order():
    """what decides the path of the length sort: the longest read (counters in LDS up to 8 191 bases, 64 KiB of them exactly there;
    the ballot kernels above) and the number of uniques against the 4 096-unique tile"""
    rng = np.random.default_rng(309)
    out = []

    def add(name, uniq):
        seqs = _with_copies(rng, uniq)
        assert derep(seqs)[0] == len(uniq), name
        out.append(Case(name, seqs, True, 1, None))

    add("all_equal", [_rnd(rng, 50) for _ in range(300)])
    add("all_distinct", [_rnd(rng, L) for L in rng.permutation(np.arange(20, 320))])
    for U in (1, 4095, 4096, 4097, 8193):
        add("U%d" % U, [_rnd(rng, rng.integers(40, 61)) for _ in range(U)])
    for Lmax in (8191, 8192, 65535):
        short = [_rnd(rng, rng.integers(40, 61)) for _ in range(4200)]
        add("longest_%d" % Lmax, short[:3000] + [_rnd(rng, Lmax)] + short[3000:] + [_rnd(rng, Lmax - 1)])
    return out


GROUPS = {"word_edges": word_edges, "exceptions": exceptions, "xxh_shapes": xxh_shapes, "palindromes": palindromes,
          "first_occurrence": first_occurrence, "minlen": minlen, "table_edges": table_edges, "samples": samples,
          "length_order": length_order}

_BUILT = {}


def group(name):
    """the cases of a group, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = GROUPS[name]()
    return _BUILT[name]


def expected(case):
    """the model's answer for a case, computed once per process"""
    key = ("model", id(case.seqs), case.strand_both, case.minlen, case.sample is not None)
    if key not in _BUILT:
        _BUILT[key] = derep(case.seqs, case.strand_both, case.minlen, case.sample)
    return _BUILT[key]


# ---------------------------------------------------------------- shards
def cross_shards(n_shards, seed=310):
    """read sets of n_shards shards whose uniques meet across them only: a reverse complement that seeds shard 0 with its forward read
    in shard 1, a palindrome in every shard, t against t + "A", N against A at one position, a sequence present three times in mixed
    orientation, one whose representative's orientation only one shard holds, and duplicates of both strands inside the shards"""
    rng = np.random.default_rng(seed)
    sh = [[] for _ in range(n_shards)]
    last = n_shards - 1
    a, t, c, e = (_rnd(rng, L) for L in (97, 111, 128, 257))
    p = 16
    if t[p] == "A":
        t = _put(t, p, "C")
    tn, ta = _put(t, p, "N"), _put(t, p, "A")
    pal = "ACGT" * 8
    sh[0] += [rc(a), pal, t, tn, c, rc(e), "ACGTSACGT"]
    sh[1] += [a, pal, t + "A", ta, rc(c), e, "N" * 40]
    sh[last] += [c, pal.lower(), e, "A" + t, rc(tn), "ACGTSACGT", "N" * 40]
    for r in range(n_shards):                                # fillers: some shared between neighbours, copies of both strands inside
        own = [_rnd(rng, rng.integers(30, 130)) for _ in range(40)]
        sh[r] += own + [rc(x) for x in own[:10]] + own[5:15]
        sh[(r + 1) % n_shards] += [rc(x) for x in own[20:30]] + own[25:35]
    for r in range(n_shards):
        sh[r] = [sh[r][i] for i in rng.permutation(len(sh[r]))]
    if n_shards >= 2:
        sh[0].insert(0, rc(a))                               # the representative of a is its reverse complement, at global index 0
    return sh


def canonical(s):
    t = norm(s)
    return min(t, rc(t))
