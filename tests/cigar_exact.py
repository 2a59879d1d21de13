"""An exact model of the alignment PATH behind an H row of a clustering's uc.txt (column 8).  TEST INFRASTRUCTURE ONLY.

The definition is tests/align_exact.py's (global alignment; +2 / -4 between unambiguous symbols, 0 for a pair with an IUPAC code,
which counts as a match when the two sets intersect; a gap run that consumes k centroid symbols is terminal iff it lies at query
position 0 or Lq, one that consumes k query symbols iff it lies at centroid position 0 or Lt; a terminal run costs 2 + k and its
columns are not counted, every other run costs 20 + 2k and its columns are counted; the optimum is the lexicographic maximum of
(score, matches, -counted columns)).  Many paths share the optimal triple; the reported one is fixed by a rule in query / centroid
terms.  Walking back from the end:
  1. in a match state take the diagonal if it reproduces the cell's value;
  2. otherwise take the gap that consumes a centroid symbol;
  3. otherwise take the gap that consumes a query symbol;
  4. inside a gap, extend in preference to closing.
Text: run-length encoded, M a column with a symbol of each read, I a centroid symbol opposite a gap in the query, D a query symbol
opposite a gap in the centroid, a run of one without its count; "=" alone for a query that equals the centroid.

Nothing here is shared with the engine: parse() is a grammar, rescore() walks a path with three plain counters, traceback() fills
full H / E / F matrices one anti-diagonal per numpy step with score, matches and columns as three separate arrays (no packed word)
and walks them by the rule above.  The query is given on the strand it is aligned on.
"""
import re

import numpy as np

from align_exact import _SETS

_NEG = -10 ** 9
_RUN = re.compile(r"([0-9]*)([MID])")


def parse(cigar):
    """[(letter, count)] of a text of the grammar: "=" alone, or runs of M / I / D with counts >= 2 (a run of one has none) and no
    two adjacent runs of one letter.  ValueError for anything else."""
    if cigar == "=":
        return [("=", 0)]
    if not cigar:
        raise ValueError("empty alignment text")
    runs, pos = [], 0
    while pos < len(cigar):
        m = _RUN.match(cigar, pos)
        if not m:
            raise ValueError("not a run at %d: %r" % (pos, cigar[pos:pos + 12]))
        digits, letter = m.groups()
        if digits and (digits[0] == "0" or int(digits) < 2):
            raise ValueError("a count below 2 at %d: %r" % (pos, m.group(0)))
        if runs and runs[-1][0] == letter:
            raise ValueError("two adjacent %s runs at %d" % (letter, pos))
        runs.append((letter, int(digits) if digits else 1))
        pos = m.end()
    return runs


def _sets(s):
    return [_SETS[c] for c in s.upper()]


def rescore(q, t, cigar):
    """(score, matches, counted columns) of the path `cigar` through q (the query on its strand) and t (the centroid); ValueError
    unless the path consumes exactly len(q) and len(t) symbols.  A run is terminal by its POSITION, not by being first or last."""
    Lq, Lt = len(q), len(t)
    runs = parse(cigar)
    if runs == [("=", 0)]:
        if Lq != Lt:
            raise ValueError("'=' between reads of %d and %d symbols" % (Lq, Lt))
        runs = [("M", Lq)] if Lq else []
    qa, ta = _sets(q), _sets(t)
    one = (1, 2, 4, 8)
    i = j = score = matches = cols = 0
    for letter, k in runs:
        if letter == "M":
            if i + k > Lq or j + k > Lt:
                raise ValueError("the path leaves the reads")
            for d in range(k):
                x, y = qa[i + d], ta[j + d]
                if x in one and y in one:
                    score += 2 if x == y else -4
                    matches += x == y
                else:
                    matches += (x & y) != 0
            cols += k
            i += k
            j += k
        elif letter == "I":                                  # k centroid symbols opposite a gap in the query, at query position i
            if j + k > Lt:
                raise ValueError("the path leaves the centroid")
            if i == 0 or i == Lq:
                score -= 2 + k
            else:
                score -= 20 + 2 * k
                cols += k
            j += k
        else:                                                # k query symbols opposite a gap in the centroid, at centroid position j
            if i + k > Lq:
                raise ValueError("the path leaves the query")
            if j == 0 or j == Lt:
                score -= 2 + k
            else:
                score -= 20 + 2 * k
                cols += k
            i += k
    if (i, j) != (Lq, Lt):
        raise ValueError("the path consumes %d / %d symbols of %d / %d" % (i, j, Lq, Lt))
    return score, matches, cols


def _best(s1, m1, c1, s2, m2, c2):
    """the better of two candidates, element by element: higher score; then more matches; then fewer counted columns (ties: 1)"""
    w = (s2 > s1) | ((s2 == s1) & ((m2 > m1) | ((m2 == m1) & (c2 < c1))))
    return np.where(w, s2, s1), np.where(w, m2, m1), np.where(w, c2, c1)


def matrices(q, t):
    """H, E, F as (score, matches, columns) triples of (Lq + 1) x (Lt + 1) arrays; E[i][j]: the best path to (i, j) that ends in a run
    consuming centroid symbols (from the left), F[i][j]: in a run consuming query symbols (from above)"""
    Lq, Lt = len(q), len(t)
    qa, ta = np.array(_sets(q), np.int64), np.array(_sets(t), np.int64)
    unq, unt = np.isin(qa, (1, 2, 4, 8)), np.isin(ta, (1, 2, 4, 8))
    shape = (Lq + 1, Lt + 1)
    H, E, F = ([np.full(shape, _NEG, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64)] for _ in range(3))
    H[0][0, 0] = 0
    rows = np.arange(Lq + 1)
    rterm = (rows == 0) | (rows == Lq)
    oE, xE, cE = np.where(rterm, -3, -22), np.where(rterm, -1, -2), np.where(rterm, 0, 1)
    colsi = np.arange(Lt + 1)
    cterm = (colsi == 0) | (colsi == Lt)
    oF, xF, cF = np.where(cterm, -3, -22), np.where(cterm, -1, -2), np.where(cterm, 0, 1)
    for d in range(1, Lq + Lt + 1):
        lo, hi = max(0, d - Lt), min(Lq, d)
        # E from (i, j - 1): rows with j >= 1
        i = np.arange(lo, min(hi, d - 1) + 1)
        if i.size:
            j = d - i
            s, m, c = _best(H[0][i, j - 1] + oE[i], H[1][i, j - 1], H[2][i, j - 1] + cE[i],
                            E[0][i, j - 1] + xE[i], E[1][i, j - 1], E[2][i, j - 1] + cE[i])
            E[0][i, j], E[1][i, j], E[2][i, j] = s, m, c
        # F from (i - 1, j): rows with i >= 1
        i = np.arange(max(lo, 1), hi + 1)
        if i.size:
            j = d - i
            s, m, c = _best(H[0][i - 1, j] + oF[j], H[1][i - 1, j], H[2][i - 1, j] + cF[j],
                            F[0][i - 1, j] + xF[j], F[1][i - 1, j], F[2][i - 1, j] + cF[j])
            F[0][i, j], F[1][i, j], F[2][i, j] = s, m, c
        i = np.arange(lo, hi + 1)
        j = d - i
        s, m, c = _best(E[0][i, j], E[1][i, j], E[2][i, j], F[0][i, j], F[1][i, j], F[2][i, j])
        H[0][i, j], H[1][i, j], H[2][i, j] = s, m, c
        # the diagonal from (i - 1, j - 1)
        i = np.arange(max(lo, 1), min(hi, d - 1) + 1)
        if i.size:
            j = d - i
            x, y = qa[i - 1], ta[j - 1]
            una = unq[i - 1] & unt[j - 1]
            same = x == y
            ds = np.where(una, np.where(same, 2, -4), 0)
            dm = np.where(una, same, (x & y) != 0).astype(np.int64)
            s, m, c = _best(H[0][i, j], H[1][i, j], H[2][i, j], H[0][i - 1, j - 1] + ds, H[1][i - 1, j - 1] + dm, H[2][i - 1, j - 1] + 1)
            H[0][i, j], H[1][i, j], H[2][i, j] = s, m, c
    return H, E, F, (qa, ta, unq, unt, (oE, xE, cE), (oF, xF, cF))


def traceback(q, t):
    """the alignment text of q (the query on its strand) with t (the centroid) by the rule of the module's docstring"""
    if len(q) == len(t) and q.upper().replace("U", "T") == t.upper().replace("U", "T"):
        return "="
    H, E, F, (qa, ta, unq, unt, (oE, xE, cE), (oF, xF, cF)) = matrices(q, t)

    def at(X, i, j):
        return int(X[0][i, j]), int(X[1][i, j]), int(X[2][i, j])
    i, j, state, ops = len(q), len(t), "H", []
    while i > 0 or j > 0:
        if state == "H":
            here = at(H, i, j)
            if i > 0 and j > 0:
                una = bool(unq[i - 1] and unt[j - 1])
                x, y = int(qa[i - 1]), int(ta[j - 1])
                ds = (2 if x == y else -4) if una else 0
                dm = int(x == y) if una else int((x & y) != 0)
                p = at(H, i - 1, j - 1)
                if (p[0] + ds, p[1] + dm, p[2] + 1) == here:
                    ops.append("M")
                    i, j = i - 1, j - 1
                    continue
            if j > 0 and at(E, i, j) == here:
                state = "E"
            else:
                assert i > 0 and at(F, i, j) == here, (i, j)
                state = "F"
        elif state == "E":
            here = at(E, i, j)
            p = at(E, i, j - 1)
            ext = (p[0] + int(xE[i]), p[1], p[2] + int(cE[i])) == here
            if not ext:
                p = at(H, i, j - 1)
                assert (p[0] + int(oE[i]), p[1], p[2] + int(cE[i])) == here, (i, j)
                state = "H"
            ops.append("I")
            j -= 1
        else:
            here = at(F, i, j)
            p = at(F, i - 1, j)
            ext = (p[0] + int(xF[j]), p[1], p[2] + int(cF[j])) == here
            if not ext:
                p = at(H, i - 1, j)
                assert (p[0] + int(oF[j]), p[1], p[2] + int(cF[j])) == here, (i, j)
                state = "H"
            ops.append("D")
            i -= 1
    assert state == "H"
    ops.reverse()
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append(ops[k] if e - k == 1 else "%d%s" % (e - k, ops[k]))
        k = e
    return "".join(out)
