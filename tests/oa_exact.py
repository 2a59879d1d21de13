"""An INDEPENDENT float64 statement of the optimal-accuracy alignment of one reported domain, for tests only: the model that
itsx_align_domains (csrc/k_float.hip: k_env_align) is held to.  hmmsearch's source is not part of this repository, so this is a
restatement (parity unpinned); the rules are the ones written out in DESIGN.md section 2.

For the envelope x_1..x_Ld (Ld = jenv - ienv + 1) of a target of length L: unihit local mode, the length model at L -- the setting
of hmm_generic.domain_bits, whose Forward / Backward matrices are restated here (that file is not edited).  Posteriors:
    pM(i,k) = exp(fM + bM - envsc)    pI(i,k) likewise, k < M    pN(i) = exp(fN(i-1) + lloop + bN(i) - envsc)    pC(i) likewise
A transition is allowed iff its probability in the HMMER3/f text is > 0; B -> M_k iff its entry probability is > 0.
    A_N(0) = A_B(0) = 0, everything else -inf at row 0
    A_M(i,k) = pM(i,k) + max{A_B(i-1), A_M(i-1,k-1), A_I(i-1,k-1), A_D(i-1,k-1)}      A_I(i,k) = pI(i,k) + max{A_M(i-1,k), A_I(i-1,k)}
    A_D(i,k) = max{A_M(i,k-1), A_D(i,k-1)}   A_E(i) = max_k A_M(i,k)   A_N(i) = A_N(i-1) + pN(i) = A_B(i)   A_C(i) = max{A_C(i-1) + pC(i), A_E(i)}
oasc = A_C(Ld).  Traceback from C(Ld), the FIRST of equal candidates wins: at C stay before E; at E the smallest k; at M the order
M, I, D, B; at I: M, I; at D: M, D.  hmm_from / hmm_to = the first / last match node, ali_from / ali_to = ienv - 1 + their rows,
acc = oasc / (1 + |jenv - ienv|)."""
import math

import numpy as np

NEG = -1e300
NINF = -math.inf
MM, MI, MD, IM, II, DM, DD = range(7)
_CODE = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
         "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}


def eps(Ld, M, oasc):
    """the float32 engine against this model: its log-quantities are held to 6 (L + M) 2^-24 relative (generic_check.tol without the
    floor), a posterior is a product of three of them, and oasc sums posteriors along one path"""
    return 18.0 * (Ld + M) * 2.0 ** -24 * max(1.0, oasc)


def _lse(a, b):
    if a < b:
        a, b = b, a
    if b <= NEG / 2:
        return a
    return a + math.log1p(math.exp(b - a))


def cut(h, M):
    """the profile cut down to its first M nodes (the transitions out of the last node are never read)"""
    return dict(name=h["name"], M=M, mat=h["mat"][:M + 1].copy(), t=h["t"][:M + 1].copy(), compo=h.get("compo"), stats=h.get("stats", {}))


class Posteriors:
    """pM[i][k], pI[i][k] (1-based, row 0 and column 0 unused), pN[i], pC[i]; allowed transitions; envsc"""

    def __init__(self, h, seq, ienv, jenv):
        M, mat, t = h["M"], h["mat"], h["t"]
        L = len(seq)
        sub = seq[ienv - 1:jenv]
        Ld = len(sub)
        assert Ld >= 1 and 1 <= ienv <= jenv <= L
        ln = lambda x: math.log(x) if x > 0 else NEG
        occ = np.zeros(M + 1)
        occ[1] = t[0][MI] + t[0][MM]
        for k in range(2, M + 1):
            occ[k] = occ[k - 1] * (t[k - 1][MM] + t[k - 1][MI]) + (1.0 - occ[k - 1]) * t[k - 1][DM]
        Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
        bm = [NEG] + [ln(occ[k] / Z) for k in range(1, M + 1)]
        lt = [[ln(x) for x in row] for row in t]
        pmove = 2.0 / (L + 2.0)
        lmove, lloop = math.log(pmove), math.log(1.0 - pmove)
        sc = np.log(mat / 0.25, where=mat > 0, out=np.full(mat.shape, NEG))
        em = [[NEG] * (M + 2)]
        for ch in sub:
            xs = _CODE.get(ch.upper(), _CODE["N"])
            row = sc[:, xs[0]] if len(xs) == 1 else sc[:, list(xs)].mean(axis=1)
            em.append([float(v) for v in row] + [NEG])
        fM = [[NEG] * (M + 2) for _ in range(Ld + 1)]; fI = [[NEG] * (M + 2) for _ in range(Ld + 1)]; fD = [[NEG] * (M + 2) for _ in range(Ld + 1)]
        fN = [NEG] * (Ld + 1); fB = [NEG] * (Ld + 1); fC = [NEG] * (Ld + 1)
        fN[0] = 0.0; fB[0] = lmove
        for i in range(1, Ld + 1):
            xE = NEG
            for k in range(1, M + 1):
                s = fB[i - 1] + bm[k]
                if k > 1:
                    s = _lse(s, _lse(_lse(fM[i - 1][k - 1] + lt[k - 1][MM], fI[i - 1][k - 1] + lt[k - 1][IM]), fD[i - 1][k - 1] + lt[k - 1][DM]))
                fM[i][k] = s + em[i][k]
                if k < M:
                    fI[i][k] = _lse(fM[i - 1][k] + lt[k][MI], fI[i - 1][k] + lt[k][II])
                if k > 1:
                    fD[i][k] = _lse(fM[i][k - 1] + lt[k - 1][MD], fD[i][k - 1] + lt[k - 1][DD])
                xE = _lse(xE, _lse(fM[i][k], fD[i][k]))
            fC[i] = _lse(fC[i - 1] + lloop, xE)
            fN[i] = fN[i - 1] + lloop
            fB[i] = fN[i] + lmove
        envsc = fC[Ld] + lmove
        bM = [[NEG] * (M + 2) for _ in range(Ld + 2)]; bI = [[NEG] * (M + 2) for _ in range(Ld + 2)]; bD = [[NEG] * (M + 2) for _ in range(Ld + 2)]
        bN = [NEG] * (Ld + 2); bC = [NEG] * (Ld + 2); bE = [NEG] * (Ld + 2)
        bC[Ld] = lmove
        bE[Ld] = bC[Ld]
        for k in range(M, 0, -1):
            bM[Ld][k] = bE[Ld] if k == M else _lse(bE[Ld], lt[k][MD] + bD[Ld][k + 1])
            bD[Ld][k] = bE[Ld] if k == M else _lse(bE[Ld], lt[k][DD] + bD[Ld][k + 1])
        for i in range(Ld - 1, -1, -1):
            xB = NEG
            for k in range(1, M + 1):
                xB = _lse(xB, bm[k] + em[i + 1][k] + bM[i + 1][k])
            bC[i] = bC[i + 1] + lloop
            bE[i] = bC[i]
            bN[i] = _lse(bN[i + 1] + lloop, xB + lmove)
            if i == 0:
                break
            for k in range(M, 0, -1):
                nm = em[i + 1][k + 1] + bM[i + 1][k + 1] if k < M else NEG
                bM[i][k] = bE[i]
                bD[i][k] = bE[i]
                if k < M:
                    bM[i][k] = _lse(bM[i][k], _lse(_lse(lt[k][MM] + nm, lt[k][MI] + bI[i + 1][k]), lt[k][MD] + bD[i][k + 1]))
                    bI[i][k] = _lse(lt[k][IM] + nm, lt[k][II] + bI[i + 1][k])
                    bD[i][k] = _lse(bD[i][k], _lse(lt[k][DM] + nm, lt[k][DD] + bD[i][k + 1]))
        assert abs(bN[0] - envsc) < 1e-6 * max(1.0, abs(envsc)), (bN[0], envsc)
        ex = lambda v: math.exp(v) if v > -700.0 else 0.0
        self.M, self.Ld, self.envsc = M, Ld, envsc
        self.pM = [[0.0] * (M + 1) for _ in range(Ld + 1)]
        self.pI = [[0.0] * (M + 1) for _ in range(Ld + 1)]
        self.pN = [0.0] * (Ld + 1); self.pC = [0.0] * (Ld + 1)
        for i in range(1, Ld + 1):
            for k in range(1, M + 1):
                self.pM[i][k] = ex(fM[i][k] + bM[i][k] - envsc)
                if k < M:
                    self.pI[i][k] = ex(fI[i][k] + bI[i][k] - envsc)
            self.pN[i] = ex(fN[i - 1] + lloop + bN[i] - envsc)
            self.pC[i] = ex(fC[i - 1] + lloop + bC[i] - envsc)
        # allowed[k][X]: the transition X out of node k; enter[k]: B -> M_k
        self.allowed = [[x > 0 for x in row] for row in t]
        self.enter = [False] + [occ[k] / Z > 0 for k in range(1, M + 1)]


def _gap(vals):
    """winner minus runner-up of the candidates of one max (inf when there is only one finite candidate)"""
    v = sorted((x for x in vals if x > NINF), reverse=True)
    return math.inf if len(v) < 2 else v[0] - v[1]


def _m_cands(P, AM, AI, AD, AB, i, k):
    """the candidates of A_M(i,k), in traceback order M, I, D, B (-inf where the transition is not allowed)"""
    al = P.allowed
    c = [NINF, NINF, NINF, AB[i - 1] if P.enter[k] else NINF]
    if k > 1:
        if al[k - 1][MM]: c[0] = AM[i - 1][k - 1]
        if al[k - 1][IM]: c[1] = AI[i - 1][k - 1]
        if al[k - 1][DM]: c[2] = AD[i - 1][k - 1]
    return c


def _fill(P, first=None):
    """the OA matrices.  first = (i1, k1): only paths whose first match state is that cell (no other entry from B, N up to i1 - 1)"""
    M, Ld, al = P.M, P.Ld, P.allowed
    AM = [[NINF] * (M + 1) for _ in range(Ld + 1)]; AI = [[NINF] * (M + 1) for _ in range(Ld + 1)]; AD = [[NINF] * (M + 1) for _ in range(Ld + 1)]
    AN = [0.0] * (Ld + 1); AB = [0.0] * (Ld + 1)
    for i in range(1, Ld + 1):
        AN[i] = AN[i - 1] + P.pN[i]
        AB[i] = AN[i]
    for i in range(1, Ld + 1):
        for k in range(1, M + 1):
            c = _m_cands(P, AM, AI, AD, AB, i, k)
            if first is not None:
                c[3] = NINF
                if (i, k) == first:
                    c = [NINF, NINF, NINF, AB[i - 1] if P.enter[k] else NINF]
            AM[i][k] = P.pM[i][k] + max(c)
            if k < M:
                AI[i][k] = P.pI[i][k] + max(AM[i - 1][k] if al[k][MI] else NINF, AI[i - 1][k] if al[k][II] else NINF)
            if k > 1:
                AD[i][k] = max(AM[i][k - 1] if al[k - 1][MD] else NINF, AD[i][k - 1] if al[k - 1][DD] else NINF)
    return AM, AI, AD, AN, AB


def align(h, seq, ienv, jenv):
    """dict(hmm_from, hmm_to, ali_from, ali_to, oasc, acc, margin, constrained, M, Ld, P)"""
    P = Posteriors(h, seq, ienv, jenv)
    M, Ld, al = P.M, P.Ld, P.allowed
    AM, AI, AD, AN, AB = _fill(P)
    AE = [NINF] * (Ld + 1); AC = [NINF] * (Ld + 1)
    for i in range(1, Ld + 1):
        AE[i] = max(max(AM[i][k], AD[i][k]) for k in range(1, M + 1))
        AC[i] = max(AC[i - 1] + P.pC[i], AE[i])
    oasc = AC[Ld]
    margin = math.inf
    i = Ld
    while True:                                   # C: stay before E
        stay, enter = AC[i - 1] + P.pC[i], AE[i]
        margin = min(margin, _gap([stay, enter]))
        if stay >= enter:
            i -= 1
            continue
        break
    k = next(k for k in range(1, M + 1) if AM[i][k] == AE[i])
    margin = min(margin, _gap([AM[i][kk] for kk in range(1, M + 1)]))
    i2, k2 = i, k
    st = "M"
    while True:
        if st == "M":
            i1, k1 = i, k
            c = _m_cands(P, AM, AI, AD, AB, i, k)
            margin = min(margin, _gap(c))
            w = c.index(max(c))
            if w == 3:
                break
            i, k, st = i - 1, k - 1, "MID"[w]
        elif st == "I":
            c = [AM[i - 1][k] if al[k][MI] else NINF, AI[i - 1][k] if al[k][II] else NINF]
            margin = min(margin, _gap(c))
            i, st = i - 1, "MI"[c.index(max(c))]
        else:
            c = [AM[i][k - 1] if al[k - 1][MD] else NINF, AD[i][k - 1] if al[k - 1][DD] else NINF]
            margin = min(margin, _gap(c))
            k, st = k - 1, "MD"[c.index(max(c))]

    def constrained(hf, ht, af, at):
        """the best OA total over the paths whose first and last match states are (af, hf) and (at, ht): the N residues before, the
        best match-to-match path, the C residues after (-inf: there is no such path)"""
        a, b = af - ienv + 1, at - ienv + 1
        if not (1 <= a <= b <= Ld and 1 <= hf <= ht <= M):
            return NINF
        CM = _fill(P, first=(a, hf))[0]
        return CM[b][ht] + sum(P.pC[b + 1:Ld + 1])

    return dict(hmm_from=k1, hmm_to=k2, ali_from=ienv - 1 + i1, ali_to=ienv - 1 + i2, oasc=oasc, acc=oasc / (1.0 + abs(jenv - ienv)),
                margin=margin, constrained=constrained, M=M, Ld=Ld, P=P)


def brute_force(P):
    """every valid unihit local path of the envelope: (best total, the set of (k1, k2, i1, i2) of the paths within 1e-12 of it)"""
    M, Ld, al = P.M, P.Ld, P.allowed
    best, coords = [NINF], [set()]
    cN = [0.0] * (Ld + 1)
    for i in range(1, Ld + 1):
        cN[i] = cN[i - 1] + P.pN[i]
    tail = lambda i: sum(P.pC[i + 1:Ld + 1])

    def finish(total, i, first, last):
        total += tail(i)
        if total > best[0] + 1e-12:
            best[0] = total; coords[0] = set()
        if total >= best[0] - 1e-12:
            coords[0].add((first[1], last[1], first[0], last[0]))

    def walk(st, i, k, total, first, last):
        if st in "MD":
            finish(total, i, first, last)                          # local: every exit is free
        if st == "M":
            if k < M and i < Ld and al[k][MM]: walk("M", i + 1, k + 1, total + P.pM[i + 1][k + 1], first, (i + 1, k + 1))
            if k < M and i < Ld and al[k][MI]: walk("I", i + 1, k, total + P.pI[i + 1][k], first, last)
            if k < M and al[k][MD]: walk("D", i, k + 1, total, first, last)
        elif st == "I":
            if i < Ld and al[k][IM]: walk("M", i + 1, k + 1, total + P.pM[i + 1][k + 1], first, (i + 1, k + 1))
            if i < Ld and al[k][II]: walk("I", i + 1, k, total + P.pI[i + 1][k], first, last)
        else:
            if k < M and i < Ld and al[k][DM]: walk("M", i + 1, k + 1, total + P.pM[i + 1][k + 1], first, (i + 1, k + 1))
            if k < M and al[k][DD]: walk("D", i, k + 1, total, first, last)

    for i in range(1, Ld + 1):
        for k in range(1, M + 1):
            if P.enter[k]:
                walk("M", i, k, cN[i - 1] + P.pM[i][k], (i, k), (i, k))
    return best[0], coords[0]


def check_row(h, seq, ienv, jenv, got, what=""):
    """one aligned row of the engine against the model.  got: hmm_from, hmm_to, ali_from, ali_to, oasc.
    Returns (model, |oasc deviation|, eps, skipped for the coordinate check, list of failures)."""
    m = align(h, seq, ienv, jenv)
    e = eps(m["Ld"], m["M"], m["oasc"])
    fails = []
    dev = abs(float(got["oasc"]) - m["oasc"])
    if not dev <= e:
        fails.append("%s: oasc %.9g, model %.9g (off %.3g, eps %.3g)" % (what, float(got["oasc"]), m["oasc"], dev, e))
    c = m["constrained"](int(got["hmm_from"]), int(got["hmm_to"]), int(got["ali_from"]), int(got["ali_to"]))
    if not c >= m["oasc"] - e:
        fails.append("%s: the alignment %s is not optimal: its best total %.9g, oasc %.9g (eps %.3g)" %
                     (what, (int(got["hmm_from"]), int(got["hmm_to"]), int(got["ali_from"]), int(got["ali_to"])), c, m["oasc"], e))
    skipped = not m["margin"] > 2.0 * e
    if not skipped:
        mine = (m["hmm_from"], m["hmm_to"], m["ali_from"], m["ali_to"])
        theirs = (int(got["hmm_from"]), int(got["hmm_to"]), int(got["ali_from"]), int(got["ali_to"]))
        if mine != theirs:
            fails.append("%s: coordinates %s, model %s (margin %.3g, eps %.3g)" % (what, theirs, mine, m["margin"], e))
    return m, dev, e, skipped, fails
