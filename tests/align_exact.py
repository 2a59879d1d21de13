"""An exact model of the clustering alignment that is fast enough for long reads.  TEST INFRASTRUCTURE ONLY.

The definition is py_align's (tests/test_cluster_cpu.py): global alignment; +2 / -4 between unambiguous symbols, 0 for a pair
with an IUPAC code, which counts as a match when the two sets intersect; an interior gap of k columns costs 20 + 2k and its
columns are counted, a terminal gap costs 2 + k and its columns are not; among the optimal scores the most matches, then the
fewest counted columns.

It shares nothing with the oracle (tests/orc.py, oracle/orc_cluster.c) or the engine: score, matches and columns are three
separate integer arrays and the lexicographic maximum is spelled out in _better(); nothing is packed into one word.  The cells
of one anti-diagonal (i + j = d) depend on the two diagonals before it only, so one numpy step per diagonal computes them all;
the vector runs over the rows.  The recurrences are symmetric under transposition (E and F swap, the terminal flags swap with
them), so align() puts the shorter read on the rows: the cost is (Lq + Lt) steps on vectors of min(Lq, Lt) + 1.  dp() takes the
arguments as given; tests/test_cluster_edges_cpu.py holds both to py_align in both argument orders.
"""
import numpy as np

_SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "M": 3, "K": 12, "S": 6, "W": 9, "H": 11, "B": 14, "V": 7, "D": 13,
         "N": 15}
_NEG = -10 ** 9


def _sets(s):
    return np.array([_SETS[c] for c in s.upper()], np.int64)


def _better(s1, m1, c1, s2, m2, c2):
    """where candidate 2 beats candidate 1: higher score; then more matches; then fewer counted columns"""
    return (s2 > s1) | ((s2 == s1) & ((m2 > m1) | ((m2 == m1) & (c2 < c1))))


def _pick(out, sl, s1, m1, c1, s2, m2, c2):
    w = _better(s1, m1, c1, s2, m2, c2)
    out[0][sl] = np.where(w, s2, s1)
    out[1][sl] = np.where(w, m2, m1)
    out[2][sl] = np.where(w, c2, c1)


def dp(q, t):
    """(score, matches, counted columns) of the best global alignment of q (rows) with t (columns)"""
    Lq, Lt = len(q), len(t)
    n = Lq + 1
    qa = _sets(q)
    tr = _sets(t)[::-1].copy()                              # t[j - 1] = tr[Lt - j]
    unq = (qa == 1) | (qa == 2) | (qa == 4) | (qa == 8)
    unt = (tr == 1) | (tr == 2) | (tr == 4) | (tr == 8)
    ii = np.arange(n)
    rterm = (ii == 0) | (ii == Lq)                          # a gap in the query's row 0 or Lq is terminal
    oE, xE, cE = np.where(rterm, -3, -22), np.where(rterm, -1, -2), np.where(rterm, 0, 1)
    jj = np.arange(Lt + 1)[::-1]                            # index Lt - j
    cterm = (jj == 0) | (jj == Lt)
    oF, xF, cF = np.where(cterm, -3, -22), np.where(cterm, -1, -2), np.where(cterm, 0, 1)

    def fresh():
        return [np.full(n, _NEG, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)]
    H = [fresh(), fresh(), fresh()]
    E = [fresh(), fresh()]
    F = [fresh(), fresh()]
    H[0][0][0] = 0
    for d in range(1, Lq + Lt + 1):
        lo, hi = max(0, d - Lt), min(Lq, d)
        Hd, H1, H2 = H[d % 3], H[(d - 1) % 3], H[(d - 2) % 3]
        Ed, E1 = E[d % 2], E[(d - 1) % 2]
        Fd, F1 = F[d % 2], F[(d - 1) % 2]
        # E[i][j] from (i, j - 1): rows lo .. min(hi, d - 1); the cell (d, 0) has none
        if hi == d:
            Ed[0][d], Ed[1][d], Ed[2][d] = _NEG, 0, 0
        a, b = lo, min(hi, d - 1) + 1
        if b > a:
            sl = slice(a, b)
            _pick(Ed, sl, H1[0][sl] + oE[sl], H1[1][sl], H1[2][sl] + cE[sl], E1[0][sl] + xE[sl], E1[1][sl], E1[2][sl] + cE[sl])
        # F[i][j] from (i - 1, j): rows max(lo, 1) .. hi; the cell (0, d) has none
        if lo == 0:
            Fd[0][0], Fd[1][0], Fd[2][0] = _NEG, 0, 0
        a, b = max(lo, 1), hi + 1
        if b > a:
            sl, up, cs = slice(a, b), slice(a - 1, b - 1), slice(Lt - d + a, Lt - d + b)
            _pick(Fd, sl, H1[0][up] + oF[cs], H1[1][up], H1[2][up] + cF[cs], F1[0][up] + xF[cs], F1[1][up], F1[2][up] + cF[cs])
        sl = slice(lo, hi + 1)
        _pick(Hd, sl, Ed[0][sl], Ed[1][sl], Ed[2][sl], Fd[0][sl], Fd[1][sl], Fd[2][sl])
        # the diagonal move from (i - 1, j - 1): rows max(lo, 1) .. min(hi, d - 1)
        a, b = max(lo, 1), min(hi, d - 1) + 1
        if b > a:
            sl, up, cs = slice(a, b), slice(a - 1, b - 1), slice(Lt - d + a, Lt - d + b)
            x, y = qa[up], tr[cs]
            una = unq[up] & unt[cs]
            same = x == y
            ds = np.where(una, np.where(same, 2, -4), 0)
            dm = np.where(una, same, (x & y) != 0).astype(np.int64)
            _pick(Hd, sl, Hd[0][sl], Hd[1][sl], Hd[2][sl], H2[0][up] + ds, H2[1][up] + dm, H2[2][up] + 1)
    Hl = H[(Lq + Lt) % 3]
    return int(Hl[0][Lq]), int(Hl[1][Lq]), int(Hl[2][Lq])


def align(q, t):
    """dp() with the shorter read on the rows (the definition is symmetric under transposition)"""
    return dp(q, t) if len(q) <= len(t) else dp(t, q)
