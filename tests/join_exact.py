"""A plain-Python model of the join of read pairs that do not overlap (Engine.merge_join, itsx_set_merge_join): strings in,
strings out, with its own upper-case and complement tables -- nothing here calls the engine or the oracle.

The rule (include/itsx_hip.h): with the setting on, a pair the merge rejects with reason 1 (no shared 5-mers), 3 (score < 16)
or 5 (overlap < 10) is kept as

    bases      upper(R1) + "NNNNNNNN" + revcomp(upper(R2))     (a symbol outside ACGTU complements to N, U to A)
    qualities  Q1        + "IIIIIIII" + reversed(Q2)

which is vsearch --fastq_join's padding as its manual gives it.  Reasons 0 (merged), 2, 4, 6, 7 and 8 are not joined; a joined
read gets no expected-error filter.  The reference's paired slicing (Dedup._get_paired_seq_generator) cuts R1[start:stop] and
R2[tlen - stop : tlen - start] -- `paired_slices` is that arithmetic on Python strings."""

PAD = 8
PAD_BASES = "N" * PAD
PAD_QUALS = "I" * PAD
JOIN_REASONS = (1, 3, 5)
JOIN_REASON_NAMES = ("nokmers", "minscore", "minovlen")        # orc.MERGE_REASONS[1], [3], [5]

_UPPER = {}
for _lo, _up in zip("abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ"):
    _UPPER[_lo] = _up
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A"}


def upper(s):
    """ASCII upper case, as the merge reads a base"""
    return "".join(_UPPER.get(c, c) for c in s)


def revcomp_as_merged(r):
    """R2 as the merge holds it: upper case, reversed, complemented; whatever is not A C G T U becomes N"""
    return "".join(_COMPLEMENT.get(c, "N") for c in reversed(upper(r)))


def is_joined(reason):
    """reason: the merge's code 0..8, or the oracle's name for it"""
    return reason in JOIN_REASONS or reason in JOIN_REASON_NAMES


def join_pair(f, fq, r, rq):
    """(bases, qualities) of the joined read of R1 = (f, fq) and R2 = (r, rq), both as they are in their files"""
    assert len(f) == len(fq) and len(r) == len(rq)
    return upper(f) + PAD_BASES + revcomp_as_merged(r), fq + PAD_QUALS + rq[::-1]


def joined_len(f, r):
    return len(f) + PAD + len(r)


def read_of_pair(reason, merged, f, fq, r, rq):
    """the read a pair leaves with the setting on: the merged one (reason 0; merged = (bases, quals)), the joined one, or None"""
    if reason in (0, "ok"):
        return merged
    if is_joined(reason):
        return join_pair(f, fq, r, rq)
    return None


def fastq_text(records):
    """seq.fq as the engine writes it: records = [(label, bases, quals)]"""
    return "".join("@%s\n%s\n+\n%s\n" % rec for rec in records)


def paired_slices(s1, q1, s2, q2, start, stop, tlen):
    """the reference's paired cut of one pair with its read's coordinates: ((R1 bases, R1 quals), (R2 bases, R2 quals))"""
    a, b = tlen - stop, tlen - start
    return (s1[start:stop], q1[start:stop]), (s2[a:b], q2[a:b])


def trimmed_pair_files(pairs, coords):
    """both trimmed files' text: pairs = [(title1, s1, q1, title2, s2, q2)] (titles with their '@'), coords = per pair
    (start, stop, tlen) or None; a pair is written when its read has 0 <= start < stop"""
    o1, o2 = [], []
    for (t1, s1, q1, t2, s2, q2), c in zip(pairs, coords):
        if c is None:
            continue
        start, stop, tlen = c
        if start < 0 or stop < 0 or start >= stop:
            continue
        (a, aq), (b, bq) = paired_slices(s1, q1, s2, q2, start, stop, tlen)
        o1.append("%s\n%s\n+\n%s\n" % (t1, a, aq))
        o2.append("%s\n%s\n+\n%s\n" % (t2, b, bq))
    return "".join(o1), "".join(o2)
