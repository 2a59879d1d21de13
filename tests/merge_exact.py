"""An independent high-precision model of the paired-end merge, and a named, seeded catalogue of pairs that
stand at its decision edges.  Shared by tests/test_merge_edges_cpu.py and tests/test_gpu_merge_edges.py.

The model is written from the procedure text in the header of oracle/orc_merge.c, not from that file's code, and imports nothing
from the oracle's binding or from the engine.  Arithmetic is mpmath at 70 digits (the standard library's decimal where mpmath is
missing): error probabilities are exact powers of ten (0.75 below Q2); log-odds, posterior qualities and expected errors are
computed at that precision.  Candidate diagonals come from a 5-mer dictionary of the forward read.

Besides the answer, merge() returns every decision it took with its distance to the threshold (the margin) and a bound on the
error of the same sum taken sequentially in double:

    bound = (n + 4) * 2^-52 * sum |term_i|       over the n terms of the sum

(n - 1 roundings of the running sum at 2^-53 relative each, doubled; the 4 covers a few ulp of libm in each table entry).  A
decision with margin <= bound is THIN: double arithmetic may legitimately take the other side.  The decisions: each candidate's
score against 16, its maximal running drop against 16, the best candidate against the second best, the expected errors against
maxee.  The drop is the difference of two partial sums, each within the bound, so that decision is held to twice the bound.  A sum
whose terms are all exactly zero is exact in double too (bound 0); two such sums that tie are not thin -- the order rule decides.

Choices where the procedure text is silent: bases are upper-cased first; A C G T U are the bases of a 5-mer
(U as T); the complement of anything else is N; symbols are compared as they are (U differs from T, N equals N, an IUPAC
symbol differs from every base); of equal scores the diagonal evaluated first (the largest shift) is reported; a diagonal discarded
by the drop rule scores -1000; a pair with an empty read is `empty`.
"""
from collections import namedtuple

import numpy as np

try:
    import mpmath as _mp
    _mp.mp.dps = 70
    F = _mp.mpf

    def _log2(x):
        return _mp.log(x, 2)

    def _log10(x):
        return _mp.log10(x)

    def _floor(x):
        return int(_mp.floor(x))
except ImportError:                                             # the same arithmetic on the standard library
    import decimal as _dec
    _dec.getcontext().prec = 70
    F = _dec.Decimal
    _LN2 = F(2).ln()

    def _log2(x):
        return x.ln() / _LN2

    def _log10(x):
        return x.log10()

    def _floor(x):
        return int(x.to_integral_value(rounding=_dec.ROUND_FLOOR))

REASONS = ["ok", "nokmers", "repeat", "minscore", "maxdiffs", "minovlen", "staggered", "maxee", "empty"]
U52 = F(2) ** -52
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A"}
_CODE = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T"}

Result = namedtuple("Result", "reason seq qual shift score diffs candidates decisions ee")
Candidate = namedtuple("Candidate", "shift score diffs overlap raw dropped bound")
Decision = namedtuple("Decision", "kind margin bound")


class FormatError(ValueError):
    """a quality byte outside ASCII 33..126"""


# ---------------------------------------------------------------- per-quality quantities, computed once each
_P, _MATCH, _MISM, _QSAME, _QDIFF = {}, {}, {}, {}, {}


def err_p(q):
    """error probability of quality byte q (33..126)"""
    if q not in _P:
        x = q - 33
        _P[q] = F(3) / 4 if x < 2 else F(10) ** (F(-x) / 10)
    return _P[q]


def match_term(qa, qb):
    k = (qa, qb)
    if k not in _MATCH:
        px, py = err_p(qa), err_p(qb)
        _MATCH[k] = _log2((1 - px - py + 4 * px * py / 3) * 4)
    return _MATCH[k]


def mism_term(qa, qb):
    k = (qa, qb)
    if k not in _MISM:
        px, py = err_p(qa), err_p(qb)
        _MISM[k] = _log2(((px + py) / 3 - 4 * px * py / 9) * 4)
    return _MISM[k]


def _round_q(p):
    """(quality byte, distance of -10 log10 p to the nearest half-integer)"""
    x = -10 * _log10(p)
    half = abs(x - _floor(x) - F(1) / 2)
    q = _floor(x + F(1) / 2)
    return 33 + max(0, min(41, q)), half


def q_same(qa, qb):
    """merged quality byte of two agreeing bases"""
    k = (qa, qb)
    if k not in _QSAME:
        px, py = err_p(qa), err_p(qb)
        _QSAME[k] = _round_q(px * py / 3 / (1 - px - py + 4 * px * py / 3))
    return _QSAME[k][0]


def q_diff(qhi, qlo):
    """merged quality byte of two disagreeing bases; qhi is the kept base's quality (the smaller error)"""
    k = (qhi, qlo)
    if k not in _QDIFF:
        px, py = err_p(qhi), err_p(qlo)
        _QDIFF[k] = _round_q(px * (1 - py / 3) / (px + py - 4 * px * py / 3))
    return _QDIFF[k][0]


def tables():
    """The 94 x 94 tables, indexed [qa - 33][qb - 33]: match and mismatch log-odds (F), the two posterior-quality tables (bytes) and,
    for each of their entries, the distance of -10 log10 p to the nearest half-integer (F)."""
    R = range(33, 127)
    for a in R:
        for b in R:
            q_same(a, b); q_diff(a, b)
    return dict(match=[[match_term(a, b) for b in R] for a in R], mism=[[mism_term(a, b) for b in R] for a in R],
                qsame=[[_QSAME[(a, b)][0] for b in R] for a in R], qdiff=[[_QDIFF[(a, b)][0] for b in R] for a in R],
                same_half=[[_QSAME[(a, b)][1] for b in R] for a in R], diff_half=[[_QDIFF[(a, b)][1] for b in R] for a in R],
                q2p=[err_p(a) for a in R])


# ---------------------------------------------------------------- the procedure
def revcomp(r):
    return "".join(_COMP.get(c, "N") for c in reversed(r.upper()))


def shared_5mers(f, r):
    """{shift: 5-mers shared on that diagonal} of the forward read and the reverse-complemented reverse read"""
    f, rc = f.upper(), revcomp(r)
    pos = {}
    for i in range(len(f) - 4):
        w = f[i:i + 5]
        if all(c in _CODE for c in w):
            pos.setdefault("".join(_CODE[c] for c in w), []).append(i)
    diag = {}
    for j in range(len(rc) - 4):
        w = rc[j:j + 5]
        if all(c in _CODE for c in w):
            for i in pos.get("".join(_CODE[c] for c in w), ()):
                diag[i - j] = diag.get(i - j, 0) + 1
    return diag


_GIVE_UP = 18          # a walk whose drop has passed 18 is discarded whatever follows (2 above the rule, far over any bound)


def _walk(f, fq, rc, rcq, shift):
    a, b = max(0, shift), min(len(f), shift + len(rc))
    score = high = drop = sabs = F(0)
    diffs = n = 0
    for p in range(b - 1, a - 1, -1):
        qa, qb = fq[p], rcq[p - shift]
        if f[p] == rc[p - shift]:
            t = match_term(qa, qb)
        else:
            t = mism_term(qa, qb)
            diffs += 1
        score += t
        sabs += abs(t)
        n += 1
        if score > high:
            high = score
        if high - score > drop:
            drop = high - score
            if drop > _GIVE_UP:
                break
    bound = (n + 4) * U52 * sabs
    dropped = drop >= 16
    return Candidate(shift, F(-1000) if dropped else score, diffs, b - a, score, dropped, F(0) if dropped else bound), drop, bound


def merge(f, fq, r, rq, maxdiffs=40, maxee=2.0, allow_stagger=False):
    """One pair (str; the reverse read as it is in the file).  Returns a Result: reason (a word of REASONS), merged bases and
    qualities (None unless ok), shift and score of the reported diagonal (0, 0 without one), its mismatches, every candidate
    (largest shift first) and every decision with its margin and bound."""
    fqb, rqb = [ord(c) for c in fq], [ord(c) for c in rq]
    if len(fqb) != len(f) or len(rqb) != len(r):
        raise ValueError("one quality per base")
    if any(q < 33 or q > 126 for q in fqb + rqb):
        raise FormatError("quality outside ASCII 33..126")
    if len(f) < 1 or len(r) < 1:
        return Result("empty", None, None, 0, F(0), 0, [], [], None)
    f, rc, rcq = f.upper(), revcomp(r), rqb[::-1]
    fl, rl = len(f), len(rc)
    diag = shared_5mers(f, r)
    cands, dec = [], []
    for shift in sorted((d for d, c in diag.items() if c >= 4), reverse=True):
        c, drop, bound = _walk(f, fqb, rc, rcq, shift)
        cands.append(c)
        dec.append(Decision("drop@%d" % shift, abs(drop - 16), 2 * bound))
        if not c.dropped:
            dec.append(Decision("score@%d" % shift, abs(c.score - 16), bound))
    if not cands:
        return Result("nokmers", None, None, 0, F(0), 0, cands, dec, None)
    best = cands[0]
    for c in cands[1:]:
        if c.score > best.score:
            best = c
    rest = [c for c in cands if c is not best]
    if rest:
        second = max(rest, key=lambda c: c.score)
        b2 = best.bound + second.bound
        if not (b2 == 0 and best.score == second.score):        # two exact sums that tie: the order rule decides
            dec.append(Decision("best@%d/%d" % (best.shift, second.shift), best.score - second.score, b2))
    hits = sum(c.score >= 16 for c in cands)
    shift = best.shift
    a, b = max(0, shift), min(fl, shift + rl)
    reason = "ok"
    if hits > 1:
        reason = "repeat"
    elif best.score < 16:
        reason = "minscore"
    elif best.diffs > maxdiffs:
        reason = "maxdiffs"
    elif b - a < 10:
        reason = "minovlen"
    elif shift < 0 and not allow_stagger:
        reason = "staggered"
    if reason != "ok":
        return Result(reason, None, None, shift, best.score, best.diffs, cands, dec, None)
    seq, qual = list(f[:a]), list(fqb[:a])
    for p in range(a, b):
        fs, rs, qa, qb = f[p], rc[p - shift], fqb[p], rcq[p - shift]
        if rs == "N":
            s, q = fs, qa
        elif fs == "N":
            s, q = rs, qb
        elif fs == rs:
            s, q = fs, q_same(qa, qb)
        elif qa > qb:
            s, q = fs, q_diff(qa, qb)
        else:
            s, q = rs, q_diff(qb, qa)
        seq.append(s)
        qual.append(q)
    if shift + rl >= fl:                                        # else the reverse read ends inside the forward read: its 3' rest is dropped
        seq += list(rc[b - shift:])
        qual += rcq[b - shift:]
    ee = sum((err_p(q) for q in qual), F(0))
    dec.append(Decision("maxee", abs(ee - F(maxee)), (len(qual) + 4) * U52 * ee))
    if ee > F(maxee):
        return Result("maxee", None, None, shift, best.score, best.diffs, cands, dec, ee)
    return Result("ok", "".join(seq), "".join(chr(q) for q in qual), shift, best.score, best.diffs, cands, dec, ee)


def thin(res):
    """the decisions of a Result whose margin does not exceed their bound"""
    return [d for d in res.decisions if d.margin <= d.bound]


def min_ratio(res):
    """the smallest margin / bound over a Result's decisions with a non-zero bound (None without one)"""
    rs = [d.margin / d.bound for d in res.decisions if d.bound > 0]
    return min(rs) if rs else None


def score_bound(res):
    """the bound of the reported diagonal's score (0 for a discarded one: -1000 is a constant)"""
    for c in res.candidates:
        if c.shift == res.shift:
            return c.bound
    return F(0)


# ================================================================ the catalogue
Case = namedtuple("Case", "name group f fq r rq kw expect")
Q41, Q2, Q0, Q1 = "J", "#", "!", '"'
_NEXT = str.maketrans("ACGT", "CGTA")


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), int(n)))


def _geom(rng, fl, rl, shift):
    """a forward read of fl bases and a reverse read of rl whose reverse complement lies on diagonal `shift` of it; what does not
    overlap is random"""
    f = _rnd(rng, fl)
    rc = list(_rnd(rng, rl))
    for j in range(rl):
        if 0 <= shift + j < fl:
            rc[j] = f[shift + j]
    return f, revcomp("".join(rc))


def _put(s, pos, ch):
    return s[:pos] + ch + s[pos + 1:]


def _rput(r, j, ch):
    """set position j of the reverse read's reverse complement view (ch is what the forward strand shows there)"""
    return _put(r, len(r) - 1 - j, ch)


_DEFAULTS = dict(maxdiffs=40, maxee=2.0, allow_stagger=False)


def _case(name, group, f, fq, r, rq, expect=None, **kw):
    return Case(name, group, f, fq, r, rq, {k: v for k, v in kw.items() if v != _DEFAULTS[k]}, expect)


_FT = {}


def _fmatch(qa, qb):
    k = (0, qa, qb)
    if k not in _FT:
        _FT[k] = float(match_term(qa, qb))
    return _FT[k]


def _fmism(qa, qb):
    k = (1, qa, qb)
    if k not in _FT:
        _FT[k] = float(mism_term(qa, qb))
    return _FT[k]


def _search_sum(rng, n, term, lo, hi, qlo=35, qhi=74):
    """n quality-byte pairs whose terms sum into (lo, hi): a seeded random search in double, confirmed by the caller in the model"""
    for _ in range(200000):
        qs = [(int(rng.integers(qlo, qhi + 1)), int(rng.integers(qlo, qhi + 1))) for _ in range(n)]
        s = sum(term(a, b) for a, b in qs)
        if lo < s < hi:
            return qs
    raise AssertionError("no quality bytes found for a sum in (%g, %g)" % (lo, hi))


def _lengths(rng):
    out = []
    L = (1, 4, 5, 6, 8, 9, 10, 13)
    k = 0
    for fl in L:
        for rl in L:
            ov = min(fl, rl) - (1 if min(fl, rl) > 8 else 0)
            f, r = _geom(rng, fl, rl, fl - ov)
            out.append(_case("len_%d_%d" % (fl, rl), "lengths", f, Q41 * fl, r, Q41 * rl))
            k += 1
            if k in (20, 40, 60):                              # an empty read between pairs that merge (13 + 13 just before and after)
                g, s = _geom(rng, 30, 30, 10)
                out.append(_case("len_merging_before_%d" % k, "lengths", g, Q41 * 30, s, Q41 * 30, "ok"))
                e = {20: ("", s), 40: (g, ""), 60: ("", "")}[k]
                out.append(_case("len_empty_%d" % k, "lengths", e[0], Q41 * len(e[0]), e[1], Q41 * len(e[1]), "empty"))
                out.append(_case("len_merging_after_%d" % k, "lengths", g, Q41 * 30, s, Q41 * 30, "ok"))
    return out


def _overlap(rng):
    out = []
    for ov, expect in ((8, "minscore"), (9, "minovlen"), (10, "ok"), (11, "ok")):
        f, r = _geom(rng, 40, 40, 40 - ov)
        out.append(_case("overlap_%d" % ov, "overlap", f, Q41 * 40, r, Q41 * 40, expect))
    return out


def _kmers(rng):
    """an N at offset t of the overlap's first 5-mer removes the 5-mers that start at 0..t; the overlap is as long as leaves the true
    diagonal `count` of them (starts t+1..t+count)"""
    out = []
    for count in (3, 4):
        for t in range(5):
            for side in "fr":
                x = t
                ov = count + t + 5
                fl = rl = 30
                shift = fl - ov
                f, r = _geom(rng, fl, rl, shift)
                fq = rq = Q41 * 30
                if side == "f":
                    f, fq = _put(f, shift + x, "N"), _put(fq, shift + x, Q2)
                else:
                    r, rq = _rput(r, x, "N"), _rput(rq, x, Q2)
                d = shared_5mers(f, r)
                assert d.get(shift, 0) == count and all(v < 4 for s, v in d.items() if s != shift), (count, t, side, d)
                out.append(_case("kmers_%d_N%d_%s" % (count, t, side), "kmers", f, fq, r, rq, "nokmers" if count == 3 else None, maxee=50.0))
    return out


def _with_overlap_quals(f, r, shift, qs):
    """Q41 everywhere but the overlap's first len(qs) positions, which take the byte pairs qs (forward, reverse)"""
    fq, rq = Q41 * len(f), Q41 * len(r)
    for k, (a, b) in enumerate(qs):
        fq = _put(fq, shift + k, chr(a))
        rq = _rput(rq, k, chr(b))
    return fq, rq


def _score16(rng):
    out = []
    for name, lo, hi, expect in (("score_below_16", 15.95, 15.9999, "minscore"), ("score_above_16", 16.0001, 16.05, "ok")):
        f, r = _geom(rng, 40, 40, 28)
        qs = _search_sum(rng, 12, _fmatch, lo, hi)
        fq, rq = _with_overlap_quals(f, r, 28, qs)
        out.append(_case(name, "score16", f, fq, r, rq, expect, maxee=50.0))
    return out


def _drop16(rng):
    """three mismatches at the forward read's 3' end, where the walk starts: the running drop is minus their sum"""
    out = []
    for name, lo, hi, expect in (("drop_below_16", -15.9999, -15.95, "ok"), ("drop_above_16", -16.05, -16.0001, "minscore")):
        f, r = _geom(rng, 60, 60, 20)
        f = f[:57] + f[57:].translate(_NEXT)
        qs = _search_sum(rng, 3, _fmism, lo, hi, 40, 74)
        fq, rq = Q41 * 60, Q41 * 60
        for k, (a, b) in enumerate(qs):
            fq = _put(fq, 57 + k, chr(a))
            rq = _rput(rq, 37 + k, chr(b))
        out.append(_case(name, "drop16", f, fq, r, rq, expect, maxee=50.0))
    return out


def _second16(rng):
    """forward = A W B W, reverse complement = W B W E: the long diagonal is strong, the one that lays the reverse read's W on the
    forward read's last W overlaps 12 bases, whose forward qualities put it next to 16"""
    out = []
    for name, lo, hi, expect in (("second_below_16", 15.95, 15.9999, "ok"), ("second_above_16", 16.0001, 16.05, "repeat")):
        A, W, B, E = _rnd(rng, 15), _rnd(rng, 12), _rnd(rng, 20), _rnd(rng, 15)
        f, r = A + W + B + W, revcomp(W + B + W + E)
        qs = _search_sum(rng, 12, lambda a, b: _fmatch(a, 74), lo, hi, 35, 45)
        fq = Q41 * (len(f) - 12) + "".join(chr(a) for a, _ in qs)
        out.append(_case(name, "second16", f, fq, r, Q41 * len(r), expect, maxee=50.0))
    return out


def _diffs(rng):
    out = []
    for m, expect in ((40, "ok"), (41, "maxdiffs")):
        f, r = _geom(rng, 170, 170, 10)                        # overlap 160: 20 clean bases, then a Q2 mismatch every third base
        fq = Q41 * 170
        for k in range(m):
            p = 10 + 20 + 3 * k
            f, fq = _put(f, p, f[p].translate(_NEXT)), _put(fq, p, Q2)
        out.append(_case("diffs_%d_of_40" % m, "diffs", f, fq, r, Q41 * 170, expect, maxee=50.0))
    for m, expect in ((0, "ok"), (1, "maxdiffs")):
        f, r = _geom(rng, 50, 50, 20)
        if m:
            f = _put(f, 40, f[40].translate(_NEXT))
        out.append(_case("diffs_%d_of_0" % m, "diffs", f, Q41 * 50, r, Q41 * 50, expect, maxdiffs=0))
    return out


def _maxee(rng):
    """the forward read's first bases take Q10 / Q20 / Q30 until the merged read's expected errors stand within 0.001 of maxee"""
    out = []
    for maxee in (2.0, 0.5):
        f, r = _geom(rng, 80, 40, 60)
        base = merge(f, Q41 * 80, r, Q41 * 40, maxee=1e9).ee
        assert base < maxee
        for over in (0, 1):
            rem, ks = F(maxee) - base, []
            for q in (10, 20, 30):
                inc = err_p(33 + q) - err_p(74)                 # a Q41 base of the forward-only part becomes a Qq base
                k = _floor(rem / inc)
                ks.append(k)
                rem -= k * inc
            ks[2] += over
            assert sum(ks) <= 38
            fq = chr(43) * ks[0] + chr(53) * ks[1] + chr(63) * ks[2]
            fq += Q41 * (80 - len(fq))
            out.append(_case("maxee_%s_%s" % (maxee, "over" if over else "under"), "maxee", f, fq, r, Q41 * 40, "maxee" if over else "ok", maxee=maxee))
    return out


def _ties(rng):
    """every quality Q0 or Q1: every term is log2(0.25 / 0.25) = 0 exactly and every candidate scores 0.0"""
    out = []
    for name, period, fl, rl in (("ties_period7_other_lanes", 7, 60, 60), ("ties_period64_same_lane", 64, 200, 200), ("ties_period8_both", 8, 150, 150)):
        unit = _rnd(rng, period)
        frag = (unit * (2 + (fl + rl) // period))
        f, rc = frag[:fl], frag[period:period + rl]
        r = revcomp(rc)
        fq = "".join(rng.choice([Q0, Q1], fl))
        rq = "".join(rng.choice([Q0, Q1], rl))
        out.append(_case(name, "ties", f, fq, r, rq, "minscore"))
    return out


def _lanes(rng):
    out = []
    for ndiag in (63, 64, 65, 71, 72, 128, 129):
        fl = (ndiag + 1) // 2 + 1
        rl = ndiag + 1 - fl
        for idx in sorted({63, 64, ndiag - 8}):
            shift = fl - 1 - idx
            if idx > ndiag - 8 or min(fl, shift + rl) - max(0, shift) < 8:
                continue
            f, r = _geom(rng, fl, rl, shift)
            out.append(_case("lanes_%d_idx%d" % (ndiag, idx), "lanes", f, Q41 * fl, r, Q41 * rl, None, allow_stagger=True))
    return out


def _posterior(rng):
    """every pair of quality bytes in an overlap, agreeing and disagreeing.  A disagreement whose term is -16 or less discards its
    diagonal on its own, so no merged read can show it: those pairs are left out.  After a disagreement come enough agreeing Q41
    bases for the running score to pass its old maximum, so that every drop is one term (a part that ends inside a padding only
    loses padding that nothing needs: the walk starts there)."""
    out = []
    R = range(33, 127)
    cols = [("s", a, b) for a in R for b in R]
    dis = []
    for a in R:
        for b in R:
            t = _fmism(a, b)
            if t > -15.9:
                dis += [("s", 74, 74)] * (int(-t / 1.99) + 1) + [("d", a, b)]     # (the walk runs from the 3' end: the padding follows)
    cols += dis
    V = 5990
    k = 0
    while cols:
        part, cols = cols[:V], cols[V:]
        n = len(part) + 10
        f, r = _geom(rng, n, n, 0)
        fq, rq = [Q41] * n, [Q41] * n
        for j, (kind, a, b) in enumerate(part):
            p = 5 + j
            fq[p], rq[n - 1 - p] = chr(a), chr(b)
            if kind == "d":
                f = _put(f, p, f[p].translate(_NEXT))
        out.append(_case("posterior_%d" % k, "posterior", f, "".join(fq), r, "".join(rq), "ok", maxee=1e6, maxdiffs=100000))
        k += 1
    # symbols: N in either read, N opposite N, U, IUPAC R / Y, each in a 40-base overlap of two 60-base reads
    f, r = _geom(rng, 60, 60, 20)
    for name, edits in (("posterior_N_forward", [("f", 30, "N")]), ("posterior_N_reverse", [("r", 12, "N")]),
                        ("posterior_N_both", [("f", 33, "N"), ("r", 13, "N")]), ("posterior_U_forward", [("f", 35, "U")]),      # (r: positions of the reverse complement)
                        ("posterior_U_reverse", [("r", 18, "U")]), ("posterior_R_forward", [("f", 36, "R")]),
                        ("posterior_Y_reverse", [("r", 20, "Y")]), ("posterior_N_low_quality", [("f", 31, "N"), ("r", 25, "N")])):
        g, s = f, r
        for side, p, ch in edits:
            if side == "f":
                g = _put(g, p, ch)
            else:
                s = _rput(s, p, ch)
        fq = Q41 * 60 if "low" not in name else _put(Q41 * 60, 31, Q2)
        out.append(_case(name, "posterior", g, fq, s, "I" * 60, None, maxee=50.0))
    return out


def _qbytes(rng):
    f, r = _geom(rng, 70, 70, 30)
    cyc = [33, 34, 35, 74, 126]
    fq = "".join(chr(cyc[i % 5]) for i in range(70))
    rq = "".join(chr(cyc[(i // 5) % 5]) for i in range(70))
    return [_case("qbytes_cycle", "qbytes", f, fq, r, rq, None, maxee=1e3),
            _case("qbytes_126_everywhere", "qbytes", f, "~" * 70, r, "~" * 70, "ok")]


def format_cases():
    """pairs with a quality byte just outside 33..126: (name, f, fq, r, rq); the whole call is refused"""
    rng = np.random.default_rng(1207)
    f, r = _geom(rng, 40, 40, 10)
    q = Q41 * 40
    return [("format_32_forward", f, _put(q, 7, " "), r, q), ("format_127_forward", f, _put(q, 39, "\x7f"), r, q),
            ("format_32_reverse", f, q, r, _put(q, 0, " ")), ("format_127_reverse", f, q, r, _put(q, 20, "\x7f"))]


def _geometry(rng):
    out = []
    rl = 40
    for name, fl, shift in (("geom_shift_minus1", 50, -1), ("geom_shift_minus_rl_plus_10", 50, -(rl - 10)),
                            ("geom_reverse_ends_inside", 90, 20), ("geom_reverse_ends_at_forward_end", 60, 20),
                            ("geom_forward_inside_reverse", 20, -10)):
        f, r = _geom(rng, fl, rl, shift)
        for st in (False, True):
            out.append(_case(name + ("_stagger" if st else ""), "geometry", f, Q41 * fl, r, Q41 * rl,
                             ("ok" if st or shift >= 0 else "staggered"), allow_stagger=st))
    return out


def _repeats(rng):
    d = "AC" * 150
    return [_case("repeat_homopolymer_300", "repeats", "A" * 300, Q41 * 300, "T" * 300, Q41 * 300, "repeat"),
            _case("repeat_dinucleotide_300", "repeats", d, Q41 * 300, revcomp(d), Q41 * 300, "repeat")]


def _lower(rng):
    f, r = _geom(rng, 60, 60, 25)
    lo = lambda s, ps: "".join(c.lower() if i in ps else c for i, c in enumerate(s))
    return [_case("lower_forward", "lower", lo(f, {3, 4, 30, 31, 32, 59}), Q41 * 60, r, Q41 * 60, "ok"),
            _case("lower_reverse", "lower", f, Q41 * 60, lo(r, {0, 1, 28, 29, 30, 58}), Q41 * 60, "ok"),
            _case("lower_both_whole", "lower", f.lower(), Q41 * 60, r.lower(), Q41 * 60, "ok")]


GROUPS = (("lengths", _lengths), ("overlap", _overlap), ("kmers", _kmers), ("score16", _score16), ("drop16", _drop16),
          ("second16", _second16), ("diffs", _diffs), ("maxee", _maxee), ("ties", _ties), ("lanes", _lanes), ("posterior", _posterior),
          ("qbytes", _qbytes), ("geometry", _geometry), ("repeats", _repeats), ("lower", _lower))
SEED = 20261
_CAT = {}


def model_of(case):
    return merge(case.f, case.fq, case.r, case.rq, **case.kw)


def catalogue():
    """[(Case, Result)], built once: every case's expectation holds in the model and none of its decisions is thin"""
    if "all" not in _CAT:
        out = []
        for gi, (group, build) in enumerate(GROUPS):
            for c in build(np.random.default_rng(SEED + gi)):
                assert c.group == group
                res = model_of(c)
                assert c.expect is None or res.reason == c.expect, (c.name, res.reason, c.expect)
                assert not thin(res), (c.name, thin(res))
                out.append((c, res))
        assert len({c.name for c, _ in out}) == len(out)
        _CAT["all"] = out
    return _CAT["all"]


def short_cases(limit=50):
    """the catalogue's first `limit` pairs of at most 200 bases in total at the default parameters, one per distinct text and at most 28
    of a group (for the grid-stride and file tests)"""
    seen, out, per = set(), [], {}
    for c, res in catalogue():
        key = (c.f, c.fq, c.r, c.rq)
        if len(c.f) + len(c.r) <= 200 and not c.kw and key not in seen and per.get(c.group, 0) < 28:
            seen.add(key)
            per[c.group] = per.get(c.group, 0) + 1
            out.append((c, res))
    return out[:limit]


def filler(total, seed=5):
    """a pair of `total` bases in all that merges at the defaults (Q41, 200-base overlap): what selects the kernel variant of a batch"""
    rng = np.random.default_rng(seed + total)
    fl = (total + 1) // 2
    rl = total - fl
    f, r = _geom(rng, fl, rl, fl - 200)
    return _case("filler_%d" % total, "variant", f, Q41 * fl, r, Q41 * rl, "ok")


def sweep(n=300, seed=77):
    """[(Case, Result)] of n seeded random short pairs: fragments 30..120, reads 10..80, qualities weighted toward Q2..Q20; thin ones
    are kept in the list (the caller skips and counts them)"""
    key = ("sweep", n, seed)
    if key not in _CAT:
        rng = np.random.default_rng(seed)
        qv = np.array([2, 3, 5, 8, 10, 12, 15, 18, 20, 25, 30, 38, 41])
        qp = np.array([8, 8, 8, 9, 9, 9, 9, 9, 9, 6, 6, 5, 5], float)
        qp /= qp.sum()
        out = []
        for i in range(n):
            L = int(rng.integers(30, 121))
            frag = _rnd(rng, L)
            if i % 9 == 0:
                frag = (_rnd(rng, int(rng.integers(6, 14))) * 30)[:L]
            fl, rl = min(L, int(rng.integers(10, 81))), min(L, int(rng.integers(10, 81)))
            f, r = list(frag[:fl]), list(revcomp(frag[L - rl:]))
            if i % 7 == 0:                                      # staggered: the forward read starts inside the fragment
                f = list(frag[L // 3:][:fl])
            fq = rng.choice(qv, len(f), p=qp)
            rq = rng.choice(qv, len(r), p=qp)
            for s, q in ((f, fq), (r, rq)):
                for k in range(len(s)):
                    if rng.random() < 0.6 * 10 ** (-q[k] / 10.0):
                        s[k] = str(rng.choice(list("ACGT")))
                    if rng.random() < 0.01:
                        s[k] = "N"
            kw = {} if i % 3 else dict(maxee=[0.5, 5.0, 50.0][i % 9 // 3], allow_stagger=bool(i % 2), maxdiffs=[2, 40][i % 2])
            c = Case("sweep_%03d" % i, "sweep", "".join(f), "".join(chr(33 + int(x)) for x in fq), "".join(r),
                     "".join(chr(33 + int(x)) for x in rq), kw, None)
            out.append((c, model_of(c)))
        _CAT[key] = out
    return _CAT[key]
