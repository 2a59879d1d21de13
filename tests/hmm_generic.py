"""An INDEPENDENT statement of the Plan7 local multihit model, for tests only: HMMER3/f text -> profile (occupancy
entry distribution, local exits, length model) -> Forward in float64 log space, node by node (no striping, no odds
ratios, no rescaling).  It shares no code with oracle/ and none of its numerics; tests compare the two at 1e-3 nats,
which checks the oracle's profile configuration and recursion, not its bit patterns.
"""
import math

import numpy as np

NEG = -1e300


def parse_hmms(text):
    """list of dict(name, M, mat[M+1][4] (prob), t[M+1][7] (prob: MM MI MD IM II DM DD), node 0 = begin)"""
    out = []
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        if not lines[i].startswith("HMMER3"):
            i += 1
            continue
        name, M = None, 0
        stats = {}
        while not lines[i].startswith("HMM "):
            if lines[i].startswith("STATS LOCAL"):
                tok = lines[i].split()
                stats[tok[2]] = (float(tok[3]), float(tok[4]))
            if lines[i].startswith("NAME"):
                name = lines[i].split()[1]
            if lines[i].startswith("LENG"):
                M = int(lines[i].split()[1])
            i += 1
        i += 2                                   # header line + transition header
        p = lambda tok: 0.0 if tok == "*" else math.exp(-float(tok))
        compo = None
        if lines[i].split()[0] == "COMPO":
            compo = [p(x) for x in lines[i].split()[1:5]]
            i += 1
        mat = np.zeros((M + 1, 4))
        t = np.zeros((M + 1, 7))
        i += 1                                   # node-0 insert emissions
        t[0] = [p(x) for x in lines[i].split()[:7]]
        i += 1
        for k in range(1, M + 1):
            tok = lines[i].split()
            assert int(tok[0]) == k
            mat[k] = [p(x) for x in tok[1:5]]
            i += 2                               # match line, insert line
            t[k] = [p(x) for x in lines[i].split()[:7]]
            i += 1
        out.append(dict(name=name, M=M, mat=mat, t=t, compo=compo, stats=stats))
    return out


def forward_nats(h, seq, L_model=None, unihit=False):
    """ln P(seq | local profile at target length L) - no null model subtracted; emissions as odds vs 0.25.
    multihit (default): nj = 1, E->J and E->C at 1/2 each; unihit: nj = 0, E->C at 1 (the mode envelopes are re-scored in)"""
    M, mat, t = h["M"], h["mat"], h["t"]
    L = len(seq)
    Lm = L if L_model is None else L_model
    MM, MI, MD, IM, II, DM, DD = range(7)
    ln = lambda x: math.log(x) if x > 0 else NEG
    # entry: match occupancy (p7_hmm_CalculateOccupancy) -> B->Mk = occ[k] / sum_k occ[k] (M-k+1)
    occ = np.zeros(M + 1)
    occ[1] = t[0][MI] + t[0][MM]
    for k in range(2, M + 1):
        occ[k] = occ[k - 1] * (t[k - 1][MM] + t[k - 1][MI]) + (1.0 - occ[k - 1]) * t[k - 1][DM]
    Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
    bm = [NEG] + [ln(occ[k] / Z) for k in range(1, M + 1)]
    lt = np.vectorize(ln)(t)
    nj = 0.0 if unihit else 1.0
    pmove = (2.0 + nj) / (Lm + 2.0 + nj)
    lmove, lloop = math.log(pmove), math.log(1.0 - pmove)
    lE = 0.0 if unihit else math.log(0.5)
    code = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
            "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
    sc = np.log(mat / 0.25, where=mat > 0, out=np.full(mat.shape, NEG))
    lse = np.logaddexp
    Mv = np.full(M + 1, NEG); Iv = np.full(M + 1, NEG); Dv = np.full(M + 1, NEG)
    xN, xB, xJ, xC = 0.0, lmove, NEG, NEG
    for i in range(1, L + 1):
        xs = code[seq[i - 1].upper()]
        em = sc[:, xs[0]] if len(xs) == 1 else sc[:, list(xs)].mean(axis=1)      # a degenerate symbol scores its expected score
        Mn = np.full(M + 1, NEG); In = np.full(M + 1, NEG); Dn = np.full(M + 1, NEG)
        xE = NEG
        for k in range(1, M + 1):
            s = xB + bm[k]
            if k > 1:
                s = lse(s, lse(lse(Mv[k - 1] + lt[k - 1][MM], Iv[k - 1] + lt[k - 1][IM]), Dv[k - 1] + lt[k - 1][DM]))
            Mn[k] = s + em[k]
            if k < M:
                In[k] = lse(Mv[k] + lt[k][MI], Iv[k] + lt[k][II])      # insert emission odds = 1
            if k > 1:
                Dn[k] = lse(Mn[k - 1] + lt[k - 1][MD], Dn[k - 1] + lt[k - 1][DD])
            xE = lse(xE, lse(Mn[k], Dn[k]))                             # local exits cost nothing
        xJ = NEG if unihit else lse(xJ + lloop, xE + lE)
        xC = lse(xC + lloop, xE + lE)
        xN = xN + lloop
        xB = lse(xN + lmove, xJ + lmove)
        Mv, Iv, Dv = Mn, In, Dn
    return xC + lmove


def viterbi_filter_nats(h, seq):
    """The Viterbi filter's score in float64: the best single path of the multihit local model, exits from match states only,
    N/C/J loops at no cost and a flat -3 nats for them at the end (HMMER's ViterbiFilter approximation); no null model."""
    M, mat, t = h["M"], h["mat"], h["t"]
    L = len(seq)
    MM, MI, MD, IM, II, DM, DD = range(7)
    ln = lambda x: math.log(x) if x > 0 else NEG
    occ = np.zeros(M + 1)
    occ[1] = t[0][MI] + t[0][MM]
    for k in range(2, M + 1):
        occ[k] = occ[k - 1] * (t[k - 1][MM] + t[k - 1][MI]) + (1.0 - occ[k - 1]) * t[k - 1][DM]
    Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
    bm = [NEG] + [ln(occ[k] / Z) for k in range(1, M + 1)]
    lt = np.vectorize(ln)(t)
    lmove = math.log(3.0 / (L + 3.0))
    lE = math.log(0.5)
    code = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
            "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
    sc = np.log(mat / 0.25, where=mat > 0, out=np.full(mat.shape, NEG))
    Mv = np.full(M + 1, NEG); Iv = np.full(M + 1, NEG); Dv = np.full(M + 1, NEG)
    xN, xB, xJ, xC = 0.0, lmove, NEG, NEG
    for i in range(1, L + 1):
        xs = code[seq[i - 1].upper()]
        em = sc[:, xs[0]] if len(xs) == 1 else sc[:, list(xs)].mean(axis=1)
        Mn = np.full(M + 1, NEG); In = np.full(M + 1, NEG); Dn = np.full(M + 1, NEG)
        xE = NEG
        for k in range(1, M + 1):
            s = xB + bm[k]
            if k > 1:
                s = max(s, Mv[k - 1] + lt[k - 1][MM], Iv[k - 1] + lt[k - 1][IM], Dv[k - 1] + lt[k - 1][DM])
            Mn[k] = s + em[k]
            if k < M:
                In[k] = max(Mv[k] + lt[k][MI], Iv[k] + lt[k][II])
            if k > 1:
                Dn[k] = max(Mn[k - 1] + lt[k - 1][MD], Dn[k - 1] + lt[k - 1][DD])
            xE = max(xE, Mn[k])
        xC = max(xC, xE + lE)
        xJ = max(xJ, xE + lE)
        xB = max(xN + lmove, xJ + lmove)
        Mv, Iv, Dv = Mn, In, Dn
    return xC + lmove - 3.0


def decode_regions(h, seq):
    """Posterior decoding of begin / end / occupancy (p7_DomainDecoding) and the region scan of
    p7_domaindef_ByPosteriorHeuristics (rt1 0.25, rt2 0.10), all in float64 log space on the multihit model.
    Returns [(i1, i2), ...] (1-based, inclusive)."""
    M, mat, t = h["M"], h["mat"], h["t"]
    L = len(seq)
    MM, MI, MD, IM, II, DM, DD = range(7)
    ln = lambda x: math.log(x) if x > 0 else NEG
    occ = np.zeros(M + 1)
    occ[1] = t[0][MI] + t[0][MM]
    for k in range(2, M + 1):
        occ[k] = occ[k - 1] * (t[k - 1][MM] + t[k - 1][MI]) + (1.0 - occ[k - 1]) * t[k - 1][DM]
    Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
    bm = np.array([NEG] + [ln(occ[k] / Z) for k in range(1, M + 1)])
    lt = np.vectorize(ln)(t)
    pmove = 3.0 / (L + 3.0)
    lmove, lloop, lE = math.log(pmove), math.log(1.0 - pmove), math.log(0.5)
    code = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
            "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
    sc = np.log(mat / 0.25, where=mat > 0, out=np.full(mat.shape, NEG))
    em = np.full((L + 1, M + 1), NEG)
    for i in range(1, L + 1):
        xs = code[seq[i - 1].upper()]
        em[i] = sc[:, xs[0]] if len(xs) == 1 else sc[:, list(xs)].mean(axis=1)
    lse = np.logaddexp
    # ---- Forward, keeping the special states of every row
    fN = np.full(L + 1, NEG); fB = np.full(L + 1, NEG); fE = np.full(L + 1, NEG); fJ = np.full(L + 1, NEG); fC = np.full(L + 1, NEG)
    fN[0] = 0.0; fB[0] = lmove
    Mv = np.full(M + 1, NEG); Iv = np.full(M + 1, NEG); Dv = np.full(M + 1, NEG)
    for i in range(1, L + 1):
        Mn = np.full(M + 1, NEG); In = np.full(M + 1, NEG); Dn = np.full(M + 1, NEG)
        xE = NEG
        for k in range(1, M + 1):
            s = fB[i - 1] + bm[k]
            if k > 1:
                s = lse(s, lse(lse(Mv[k - 1] + lt[k - 1][MM], Iv[k - 1] + lt[k - 1][IM]), Dv[k - 1] + lt[k - 1][DM]))
            Mn[k] = s + em[i][k]
            if k < M:
                In[k] = lse(Mv[k] + lt[k][MI], Iv[k] + lt[k][II])
            if k > 1:
                Dn[k] = lse(Mn[k - 1] + lt[k - 1][MD], Dn[k - 1] + lt[k - 1][DD])
            xE = lse(xE, lse(Mn[k], Dn[k]))
        fE[i] = xE
        fJ[i] = lse(fJ[i - 1] + lloop, xE + lE)
        fC[i] = lse(fC[i - 1] + lloop, xE + lE)
        fN[i] = fN[i - 1] + lloop
        fB[i] = lse(fN[i] + lmove, fJ[i] + lmove)
        Mv, Iv, Dv = Mn, In, Dn
    total = fC[L] + lmove
    # ---- Backward (b*[i] = ln P(x_{i+1..L} | state at i))
    bN = np.full(L + 1, NEG); bB = np.full(L + 1, NEG); bE = np.full(L + 1, NEG); bJ = np.full(L + 1, NEG); bC = np.full(L + 1, NEG)
    bC[L] = lmove
    bE[L] = bC[L] + lE
    Mb = np.full(M + 2, NEG); Ib = np.full(M + 2, NEG); Db = np.full(M + 2, NEG)
    for k in range(M, 0, -1):                          # row L: exit directly, or through the delete states to the right
        Mb[k] = bE[L] if k == M else lse(bE[L], lt[k][MD] + Db[k + 1])
        Db[k] = bE[L] if k == M else lse(bE[L], lt[k][DD] + Db[k + 1])
    for i in range(L - 1, -1, -1):
        # B at row i enters a match state that emits residue i+1
        xB = NEG
        for k in range(1, M + 1):
            xB = lse(xB, bm[k] + em[i + 1][k] + Mb[k])
        bB[i] = xB
        bJ[i] = lse(bJ[i + 1] + lloop, xB + lmove)
        bC[i] = bC[i + 1] + lloop
        bE[i] = lse(bJ[i] + lE, bC[i] + lE)
        bN[i] = lse(bN[i + 1] + lloop, xB + lmove)
        if i == 0:
            break
        Mn = np.full(M + 2, NEG); In = np.full(M + 2, NEG); Dn = np.full(M + 2, NEG)
        for k in range(M, 0, -1):
            nm = em[i + 1][k + 1] + Mb[k + 1] if k < M else NEG           # next row's match state k+1 (emits residue i+1)
            Mn[k] = bE[i]
            Dn[k] = bE[i]
            if k < M:
                Mn[k] = lse(Mn[k], lse(lse(lt[k][MM] + nm, lt[k][MI] + Ib[k]), lt[k][MD] + Dn[k + 1]))
                In[k] = lse(lt[k][IM] + nm, lt[k][II] + Ib[k])
                Dn[k] = lse(Dn[k], lse(lt[k][DM] + nm, lt[k][DD] + Dn[k + 1]))
        Mb, Ib, Db = Mn, In, Dn
    assert abs((bN[0]) - total) < 1e-6 * max(1.0, abs(total)), (bN[0], total)
    # ---- decoding + region scan
    btot = np.zeros(L + 1); etot = np.zeros(L + 1); mocc = np.zeros(L + 1)
    for i in range(1, L + 1):
        btot[i] = btot[i - 1] + math.exp(fB[i - 1] + bB[i - 1] - total)
        etot[i] = etot[i - 1] + math.exp(fE[i] + bE[i] - total)
        njcp = math.exp(fN[i - 1] + bN[i] + lloop - total) + math.exp(fJ[i - 1] + bJ[i] + lloop - total) + math.exp(fC[i - 1] + bC[i] + lloop - total)
        mocc[i] = 1.0 - njcp
    regions = []
    i1, trig = -1, False
    for i in range(1, L + 1):
        if not trig:
            if mocc[i] - (btot[i] - btot[i - 1]) < 0.10:
                i1 = i
            elif i1 == -1:
                i1 = i
            if mocc[i] >= 0.25:
                trig = True
        elif mocc[i] - (etot[i] - etot[i - 1]) < 0.10:
            regions.append((i1, i))
            i1, trig = -1, False
    return regions


def domain_bits(h, seq, ienv, jenv):
    """Bit score of one envelope as hmmsearch reports it (column 14 of --domtblout), independently in float64:
    unihit Forward over the envelope with the length model at the full target length, + the flanks' N/C loops,
    - null1, - the null2 bias correction (p7_Null2_ByExpectation: expected state usage from posterior decoding of the
    envelope; prior omega = 1/256).  Returns (bits, domcorrection_nats, envsc_nats)."""
    M, mat, t = h["M"], h["mat"], h["t"]
    L = len(seq)
    sub = seq[ienv - 1:jenv]
    Ld = len(sub)
    MM, MI, MD, IM, II, DM, DD = range(7)
    ln = lambda x: math.log(x) if x > 0 else NEG
    occ = np.zeros(M + 1)
    occ[1] = t[0][MI] + t[0][MM]
    for k in range(2, M + 1):
        occ[k] = occ[k - 1] * (t[k - 1][MM] + t[k - 1][MI]) + (1.0 - occ[k - 1]) * t[k - 1][DM]
    Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
    bm = np.array([NEG] + [ln(occ[k] / Z) for k in range(1, M + 1)])
    lt = np.vectorize(ln)(t)
    pmove = 2.0 / (L + 2.0)                                  # unihit, length model stays at L
    lmove, lloop = math.log(pmove), math.log(1.0 - pmove)
    code = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
            "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
    odds = mat / 0.25
    sc = np.log(odds, where=mat > 0, out=np.full(mat.shape, NEG))
    em = np.full((Ld + 1, M + 1), NEG)
    for i in range(1, Ld + 1):
        xs = code[sub[i - 1].upper()]
        em[i] = sc[:, xs[0]] if len(xs) == 1 else sc[:, list(xs)].mean(axis=1)
    lse = np.logaddexp
    fM = np.full((Ld + 1, M + 2), NEG); fI = np.full((Ld + 1, M + 2), NEG); fD = np.full((Ld + 1, M + 2), NEG)
    fN = np.full(Ld + 1, NEG); fB = np.full(Ld + 1, NEG); fE = np.full(Ld + 1, NEG); fC = np.full(Ld + 1, NEG)
    fN[0] = 0.0; fB[0] = lmove
    for i in range(1, Ld + 1):
        xE = NEG
        for k in range(1, M + 1):
            s = fB[i - 1] + bm[k]
            if k > 1:
                s = lse(s, lse(lse(fM[i - 1][k - 1] + lt[k - 1][MM], fI[i - 1][k - 1] + lt[k - 1][IM]), fD[i - 1][k - 1] + lt[k - 1][DM]))
            fM[i][k] = s + em[i][k]
            if k < M:
                fI[i][k] = lse(fM[i - 1][k] + lt[k][MI], fI[i - 1][k] + lt[k][II])
            if k > 1:
                fD[i][k] = lse(fM[i][k - 1] + lt[k - 1][MD], fD[i][k - 1] + lt[k - 1][DD])
            xE = lse(xE, lse(fM[i][k], fD[i][k]))
        fE[i] = xE
        fC[i] = lse(fC[i - 1] + lloop, xE)                   # unihit: E->C with probability 1
        fN[i] = fN[i - 1] + lloop
        fB[i] = fN[i] + lmove
    envsc = fC[Ld] + lmove
    bM = np.full((Ld + 2, M + 2), NEG); bI = np.full((Ld + 2, M + 2), NEG); bD = np.full((Ld + 2, M + 2), NEG)
    bN = np.full(Ld + 2, NEG); bC = np.full(Ld + 2, NEG); bE = np.full(Ld + 2, NEG); bB = np.full(Ld + 2, NEG)
    bC[Ld] = lmove
    bE[Ld] = bC[Ld]
    for k in range(M, 0, -1):
        bM[Ld][k] = bE[Ld] if k == M else lse(bE[Ld], lt[k][MD] + bD[Ld][k + 1])
        bD[Ld][k] = bE[Ld] if k == M else lse(bE[Ld], lt[k][DD] + bD[Ld][k + 1])
    for i in range(Ld - 1, -1, -1):
        xB = NEG
        for k in range(1, M + 1):
            xB = lse(xB, bm[k] + em[i + 1][k] + bM[i + 1][k])
        bB[i] = xB
        bC[i] = bC[i + 1] + lloop
        bE[i] = bC[i]
        bN[i] = lse(bN[i + 1] + lloop, xB + lmove)
        if i == 0:
            break
        for k in range(M, 0, -1):
            nm = em[i + 1][k + 1] + bM[i + 1][k + 1] if k < M else NEG
            bM[i][k] = bE[i]
            bD[i][k] = bE[i]
            if k < M:
                bM[i][k] = lse(bM[i][k], lse(lse(lt[k][MM] + nm, lt[k][MI] + bI[i + 1][k]), lt[k][MD] + bD[i][k + 1]))
                bI[i][k] = lse(lt[k][IM] + nm, lt[k][II] + bI[i + 1][k])
                bD[i][k] = lse(bD[i][k], lse(lt[k][DM] + nm, lt[k][DD] + bD[i][k + 1]))
    # expected usage of the emitting states over the envelope
    ppM = np.zeros(M + 1); ppI = 0.0; ppX = 0.0
    for i in range(1, Ld + 1):
        for k in range(1, M + 1):
            ppM[k] += math.exp(fM[i][k] + bM[i][k] - envsc)
            if k < M:
                ppI += math.exp(fI[i][k] + bI[i][k] - envsc)
        ppX += math.exp(fN[i - 1] + lloop + bN[i] - envsc) + math.exp(fC[i - 1] + lloop + bC[i] - envsc)
    null2 = np.array([(sum(ppM[k] * odds[k][x] for k in range(1, M + 1)) + ppI + ppX) / Ld for x in range(4)])
    domcorr = 0.0
    for ch in sub:
        xs = code[ch.upper()]
        domcorr += math.log(null2[xs[0]]) if len(xs) == 1 else math.log(np.mean([null2[x] for x in xs]))
    nullsc = L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))
    dombias = math.log(1.0 + math.exp(math.log(1.0 / 256.0) + domcorr))
    bits = (envsc + (L - Ld) * math.log(L / (L + 3.0)) - (nullsc + dombias)) / math.log(2.0)
    return bits, domcorr, envsc


def msv_nats(h, seq):
    """Generic MSV score (p7_GMSV): best set of ungapped local diagonals, uniform entry 2/(M(M+1)), multihit."""
    M, mat = h["M"], h["mat"]
    L = len(seq)
    tloop, tmove = math.log(L / (L + 3.0)), math.log(3.0 / (L + 3.0))
    tbm, te = math.log(2.0 / (M * (M + 1.0))), math.log(0.5)
    code = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
            "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
    sc = np.log(mat / 0.25, where=mat > 0, out=np.full(mat.shape, NEG))
    prev = np.full(M + 1, NEG)
    xN, xB, xJ, xC = 0.0, tmove, NEG, NEG
    for ch in seq:
        xs = code[ch.upper()]
        em = sc[:, xs[0]] if len(xs) == 1 else sc[:, list(xs)].mean(axis=1)
        cur = np.full(M + 1, NEG)
        cur[1:] = em[1:] + np.maximum(prev[:-1], xB + tbm)
        xE = cur[1:].max()
        xJ = max(xJ + tloop, xE + te)
        xC = max(xC + tloop, xE + te)
        xN = xN + tloop
        xB = max(xN + tmove, xJ + tmove)
        prev = cur
    return xC + tmove


def bias_filter_nats(h, seq):
    """p7_bg_FilterScore: ln P(seq | 2-state composition HMM) as odds against the iid background, plus the null length
    model; state 0 = background (mean run 400, start 0.999, re-set to the target length), state 1 = the model's COMPO
    (mean run M/8)."""
    L = len(seq)
    p1 = L / (L + 1.0)
    L1 = h["M"] / 8.0
    t = [[p1, 1.0 - p1], [1.0 / (L1 + 1.0), L1 / (L1 + 1.0)]]
    sets = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
            "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
    e = [[0.25] * 4, list(h["compo"])]
    def eo(k, ch):
        xs = sets[ch.upper()]
        return sum(e[k][x] for x in xs) / sum(0.25 for _ in xs)
    a = [0.999 * eo(0, seq[0]), 0.001 * eo(1, seq[0])]
    logsc = 0.0
    for ch in seq[1:]:
        m = max(a)
        logsc += math.log(m)
        a = [a[0] / m, a[1] / m]
        a = [(a[0] * t[0][0] + a[1] * t[1][0]) * eo(0, ch), (a[0] * t[0][1] + a[1] * t[1][1]) * eo(1, ch)]
    logsc += math.log(a[0] + a[1])
    return logsc + L * math.log(p1) + math.log(1.0 - p1)


# ---------------------------------------------------------------------------------------------------------------------------------
# Fast forms.  The functions above are the readable definition; the ones below compute the same float64 quantities with the nodes
# of a row as one vector (and, where the read length only enters through the length model, a padded batch of reads as a second
# axis).  The delete chain D[k] = lse(M[k-1] + MD[k-1], D[k-1] + DD[k-1]) is linear in probability space, so a row's delete cells are
# one product with a fixed (M+1) x (M+1) matrix of DD products, after shifting the row by its own maximum.  Still float64, still
# nothing shared with oracle/ or the engine; tests/test_generic_cpu.py holds them to the definition at 1e-9 nats.

CODE = {"A": (0,), "C": (1,), "G": (2,), "T": (3,), "U": (3,), "R": (0, 2), "Y": (1, 3), "M": (0, 1), "K": (2, 3), "S": (1, 2),
        "W": (0, 3), "H": (0, 1, 3), "B": (1, 2, 3), "V": (0, 1, 2), "D": (0, 2, 3), "N": (0, 1, 2, 3)}
_SYMS = "ACGTURYMKSWHBVDN"
_LUT = np.full(256, 15, np.int64)
for _j, _c in enumerate(_SYMS):
    _LUT[ord(_c)] = _j
    _LUT[ord(_c.lower())] = _j


def codes_of(seq):
    """symbol indices into _SYMS (anything unknown reads as N)"""
    return _LUT[np.frombuffer(seq.encode(), np.uint8)]


def _lse_rows(x, axis=-1):
    m = x.max(axis=axis, keepdims=True)
    m = np.where(m > NEG / 2, m, 0.0)
    s = np.exp(x - m).sum(axis=axis, keepdims=True)
    out = np.where(s > 0, np.log(np.where(s > 0, s, 1.0)) + m, NEG)
    return np.squeeze(out, axis=axis)


def _safe_log(x):
    return np.where(x > 0, np.log(np.where(x > 0, x, 1.0)), NEG)


def prepare(h):
    """per-profile float64 tables of the fast forms (cached on the dict)"""
    if "_fast" in h:
        return h["_fast"]
    M, mat, t = h["M"], h["mat"], h["t"]
    occ = np.zeros(M + 1)
    occ[1] = t[0][1] + t[0][0]
    for k in range(2, M + 1):
        occ[k] = occ[k - 1] * (t[k - 1][0] + t[k - 1][1]) + (1.0 - occ[k - 1]) * t[k - 1][5]
    Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
    bm = np.full(M + 1, NEG)
    bm[1:] = _safe_log(occ[1:] / Z)
    lt = _safe_log(t)                                                  # (M+1, 7): MM MI MD IM II DM DD
    sc = _safe_log(mat / 0.25)
    sc[0] = NEG
    em = np.stack([sc[:, CODE[c][0]] if len(CODE[c]) == 1 else sc[:, list(CODE[c])].mean(axis=1) for c in _SYMS])   # (16, M+1)
    odds = mat / 0.25
    # WF[j, k] = prod_{l=j+1}^{k-1} t_l(DD) for 1 <= j < k <= M: a match cell M_j reaches D_k through M_j -> D_j+1 -> ... -> D_k
    # WB[j, k] = prod_{l=k}^{j-1} t_l(DD) for 1 <= k <= j <= M: the backward delete cell D_k collects what enters at node j
    dd = t[:, 6]
    WF = np.zeros((M + 1, M + 1))
    WB = np.zeros((M + 1, M + 1))
    for j in range(1, M + 1):
        p = 1.0
        for k in range(j + 1, M + 1):
            WF[j, k] = p
            p *= dd[k]
        p = 1.0
        for k in range(j, 0, -1):
            WB[j, k] = p
            p *= dd[k - 1] if k > 1 else 0.0
    f = dict(M=M, bm=bm, lt=lt, em=em, odds=odds, WF=WF, WB=WB)
    h["_fast"] = f
    return f


def _dchain_fwd(f, A):
    """D[:, k] = lse_{j<k} (A[:, j] + sum_{l=j+1}^{k-1} ln DD_l), A = M[:, j] + ln MD_j"""
    m = A.max(axis=-1, keepdims=True)
    return _safe_log(np.exp(A - m) @ f["WF"]) + m


def _dchain_bwd(f, c):
    """D[k] = lse_{j>=k} (c[j] + sum_{l=k}^{j-1} ln DD_l)"""
    m = c.max(axis=-1, keepdims=True)
    return _safe_log(np.exp(c - m) @ f["WB"]) + m


def _pad(seqs):
    Ls = np.array([len(s) for s in seqs], np.int64)
    X = np.full((len(seqs), max(1, int(Ls.max()))), 15, np.int64)
    for b, s in enumerate(seqs):
        X[b, :len(s)] = codes_of(s)
    return X, Ls


def forward_nats_batch(h, seqs, L_model=None, unihit=False):
    """forward_nats for a list of reads (one profile), padded into one batch; L_model: None (each read's length), a number or
    one per read"""
    f = prepare(h)
    M, bm, lt, em = f["M"], f["bm"], f["lt"], f["em"]
    X, Ls = _pad(seqs)
    B = len(seqs)
    Lm = Ls.astype(float) if L_model is None else np.broadcast_to(np.asarray(L_model, float), (B,)).copy()
    nj = 0.0 if unihit else 1.0
    pmove = (2.0 + nj) / (Lm + 2.0 + nj)
    lmove, lloop = np.log(pmove), np.log(1.0 - pmove)
    lE = 0.0 if unihit else math.log(0.5)
    Mv = np.full((B, M + 1), NEG); Iv = np.full((B, M + 1), NEG); Dv = np.full((B, M + 1), NEG)
    xN = np.zeros(B); xB = lmove.copy(); xJ = np.full(B, NEG); xC = np.full(B, NEG)
    out = np.full(B, NEG)
    MMp, IMp, DMp = lt[:-1, 0], lt[:-1, 3], lt[:-1, 5]
    for i in range(X.shape[1]):
        Mn = np.empty((B, M + 1)); Mn[:, 0] = NEG
        s = xB[:, None] + bm[None, 1:]
        s[:, 1:] = np.logaddexp(s[:, 1:], np.logaddexp(np.logaddexp(Mv[:, 1:-1] + MMp[1:], Iv[:, 1:-1] + IMp[1:]), Dv[:, 1:-1] + DMp[1:]))
        Mn[:, 1:] = s + em[X[:, i], 1:]
        In = np.full((B, M + 1), NEG)
        In[:, 1:M] = np.logaddexp(Mv[:, 1:M] + lt[1:M, 1], Iv[:, 1:M] + lt[1:M, 4])
        Dn = _dchain_fwd(f, Mn + lt[:, 2])
        xE = _lse_rows(np.concatenate([Mn[:, 1:], Dn[:, 1:]], axis=1))
        xJ = np.full(B, NEG) if unihit else np.logaddexp(xJ + lloop, xE + lE)
        xC = np.logaddexp(xC + lloop, xE + lE)
        xN = xN + lloop
        xB = np.logaddexp(xN + lmove, xJ + lmove)
        Mv, Iv, Dv = Mn, In, Dn
        done = Ls == i + 1
        out[done] = xC[done] + lmove[done]
    return out


def msv_nats_batch(h, seqs):
    """msv_nats for a list of reads (one profile)"""
    f = prepare(h)
    M, em = f["M"], f["em"]
    X, Ls = _pad(seqs)
    B = len(seqs)
    Lf = Ls.astype(float)
    tloop, tmove = np.log(Lf / (Lf + 3.0)), np.log(3.0 / (Lf + 3.0))
    tbm, te = math.log(2.0 / (M * (M + 1.0))), math.log(0.5)
    prev = np.full((B, M + 1), NEG)
    xN = np.zeros(B); xB = tmove.copy(); xJ = np.full(B, NEG); xC = np.full(B, NEG)
    out = np.full(B, NEG)
    for i in range(X.shape[1]):
        cur = np.full((B, M + 1), NEG)
        cur[:, 1:] = em[X[:, i], 1:] + np.maximum(prev[:, :-1], (xB + tbm)[:, None])
        xE = cur[:, 1:].max(axis=1)
        xJ = np.maximum(xJ + tloop, xE + te)
        xC = np.maximum(xC + tloop, xE + te)
        xN = xN + tloop
        xB = np.maximum(xN + tmove, xJ + tmove)
        prev = cur
        done = Ls == i + 1
        out[done] = xC[done] + tmove[done]
    return out


def bias_filter_nats_batch(h, seqs):
    """bias_filter_nats for a list of reads (one profile): the same 2-state HMM, in log space"""
    X, Ls = _pad(seqs)
    B = len(seqs)
    Lf = Ls.astype(float)
    p1 = Lf / (Lf + 1.0)
    L1 = h["M"] / 8.0
    l00, l01 = np.log(p1), np.log(1.0 - p1)
    l10, l11 = math.log(1.0 / (L1 + 1.0)), math.log(L1 / (L1 + 1.0))
    compo = np.asarray(h["compo"], float)
    e1 = np.log(np.array([compo[list(CODE[c])].sum() / (0.25 * len(CODE[c])) for c in _SYMS]))   # state 0 scores odds 1
    a0 = np.full(B, math.log(0.999)); a1 = math.log(0.001) + e1[X[:, 0]]
    out = np.full(B, NEG)
    done = Ls == 1
    out[done] = np.logaddexp(a0, a1)[done]
    for i in range(1, X.shape[1]):
        a0, a1 = np.logaddexp(a0 + l00, a1 + l10), np.logaddexp(a0 + l01, a1 + l11) + e1[X[:, i]]
        done = Ls == i + 1
        out[done] = np.logaddexp(a0, a1)[done]
    return out + Lf * l00 + l01


def _fb(f, x, Lm, unihit):
    """Forward and Backward of one read (codes x) with every row kept; nodes vectorised.  Returns the matrices, the special
    states and the total."""
    M, bm, lt, em = f["M"], f["bm"], f["lt"], f["em"]
    L = len(x)
    nj = 0.0 if unihit else 1.0
    pmove = (2.0 + nj) / (Lm + 2.0 + nj)
    lmove, lloop = math.log(pmove), math.log(1.0 - pmove)
    lE = 0.0 if unihit else math.log(0.5)
    E = np.full((L + 2, M + 1), NEG)
    E[1:L + 1] = em[x]
    E[:, 0] = NEG
    fM = np.full((L + 1, M + 1), NEG); fI = np.full((L + 1, M + 1), NEG); fD = np.full((L + 1, M + 1), NEG)
    fN = np.full(L + 1, NEG); fB = np.full(L + 1, NEG); fE = np.full(L + 1, NEG); fJ = np.full(L + 1, NEG); fC = np.full(L + 1, NEG)
    fN[0] = 0.0; fB[0] = lmove
    for i in range(1, L + 1):
        s = fB[i - 1] + bm[1:]
        s[1:] = np.logaddexp(s[1:], np.logaddexp(np.logaddexp(fM[i - 1, 1:-1] + lt[1:-1, 0], fI[i - 1, 1:-1] + lt[1:-1, 3]),
                                                fD[i - 1, 1:-1] + lt[1:-1, 5]))
        fM[i, 1:] = s + E[i, 1:]
        fI[i, 1:M] = np.logaddexp(fM[i - 1, 1:M] + lt[1:M, 1], fI[i - 1, 1:M] + lt[1:M, 4])
        fD[i] = _dchain_fwd(f, fM[i] + lt[:, 2])
        xE = _lse_rows(np.concatenate([fM[i, 1:], fD[i, 1:]]))
        fE[i] = xE
        fJ[i] = NEG if unihit else np.logaddexp(fJ[i - 1] + lloop, xE + lE)
        fC[i] = np.logaddexp(fC[i - 1] + lloop, xE + lE)
        fN[i] = fN[i - 1] + lloop
        fB[i] = np.logaddexp(fN[i] + lmove, fJ[i] + lmove)
    total = fC[L] + lmove
    bM = np.full((L + 2, M + 2), NEG); bI = np.full((L + 2, M + 2), NEG); bD = np.full((L + 2, M + 2), NEG)
    bN = np.full(L + 1, NEG); bB = np.full(L + 1, NEG); bE = np.full(L + 1, NEG); bJ = np.full(L + 1, NEG); bC = np.full(L + 1, NEG)
    bC[L] = lmove
    bE[L] = bC[L] + lE
    c = np.full(M + 1, NEG); c[1:] = bE[L]
    bD[L, :M + 1] = _dchain_bwd(f, c)            # row L: exit at once, or through the deletes to the right
    bM[L, 1:M] = np.logaddexp(bE[L], lt[1:M, 2] + bD[L, 2:M + 1]); bM[L, M] = bE[L]
    bD[L, 0] = NEG
    for i in range(L - 1, -1, -1):
        xB = _lse_rows(bm[1:] + E[i + 1, 1:] + bM[i + 1, 1:M + 1])
        bB[i] = xB
        bJ[i] = NEG if unihit else np.logaddexp(bJ[i + 1] + lloop, xB + lmove)
        bC[i] = bC[i + 1] + lloop
        bE[i] = np.logaddexp(bJ[i] + lE, bC[i] + lE)
        bN[i] = np.logaddexp(bN[i + 1] + lloop, xB + lmove)
        if i == 0:
            break
        nm = np.full(M + 1, NEG)
        nm[1:M] = E[i + 1, 2:M + 1] + bM[i + 1, 2:M + 1]                    # next row's match k+1
        c = np.full(M + 1, NEG)
        c[1:M] = np.logaddexp(bE[i], lt[1:M, 5] + nm[1:M]); c[M] = bE[i]
        bD[i, :M + 1] = _dchain_bwd(f, c)
        bD[i, 0] = NEG
        bM[i, 1:M] = np.logaddexp(np.logaddexp(bE[i], lt[1:M, 0] + nm[1:M]),
                                  np.logaddexp(lt[1:M, 1] + bI[i + 1, 1:M], lt[1:M, 2] + bD[i, 2:M + 1]))
        bM[i, M] = bE[i]
        bI[i, 1:M] = np.logaddexp(lt[1:M, 3] + nm[1:M], lt[1:M, 4] + bI[i + 1, 1:M])
    return dict(L=L, lmove=lmove, lloop=lloop, lE=lE, total=total, E=E, fM=fM, fI=fI, fD=fD, fN=fN, fB=fB, fE=fE, fJ=fJ, fC=fC,
                bM=bM, bI=bI, bD=bD, bN=bN, bB=bB, bE=bE, bJ=bJ, bC=bC)


def _scan(dA, dT, dZ, flip=None):
    """the region scan of p7_domaindef_ByPosteriorHeuristics on the tests' signed distances from their thresholds (row i:
    dA = mocc - pB - rt2, dT = mocc - rt1, dZ = mocc - pE - rt2); flip = (row, test) whose outcome is inverted"""
    regions = []
    i1, trig = -1, False
    for i in range(1, len(dA)):
        if not trig:
            a, t = dA[i] < 0, dT[i] >= 0
            if flip is not None and flip[0] == i:
                a, t = (not a, t) if flip[1] == "A" else (a, not t) if flip[1] == "T" else (a, t)
            if a:
                i1 = i
            elif i1 == -1:
                i1 = i
            if t:
                trig = True
        else:
            z = dZ[i] < 0
            if flip is not None and flip == (i, "Z"):
                z = not z
            if z:
                regions.append((i1, i))
                i1, trig = -1, False
    return regions


def decode_regions_fast(h, seq, tol=0.0, rt1=0.25, rt2=0.10, rt3=0.20):
    """decode_regions, nodes vectorised, plus what a knife edge needs.  Returns (regions, info), info = dict(
    near_regions: the regions whose coordinates change when any ONE threshold test that lies within tol of its threshold goes
    the other way, near_count: whether such a flip changes the number of regions, alt_regions: every region some flip produces,
    alt_counts: the region counts flips produce,
    dist: per region, the distance of the nearest test whose flip moves it (inf if none), multi: per region, the rt3 value (max
    over z of min(expected ends in i..z, expected begins in z..j)) that sends a region to the ensemble stage, total: the Forward
    score)"""
    f = prepare(h)
    x = codes_of(seq)
    L = len(x)
    r = _fb(f, x, float(L), False)
    tot, ll = r["total"], r["lloop"]
    fB, bB, fE, bE, fN, bN, fJ, bJ, fC, bC = (r[k] for k in ("fB", "bB", "fE", "bE", "fN", "bN", "fJ", "bJ", "fC", "bC"))
    pB = np.exp(fB[:-1] + bB[:-1] - tot)                      # begin posterior entering row i (i = 1..L)
    pE = np.exp(fE[1:] + bE[1:] - tot)
    njc = (np.exp(fN[:-1] + bN[1:] + ll - tot) + np.exp(fJ[:-1] + bJ[1:] + ll - tot) + np.exp(fC[:-1] + bC[1:] + ll - tot))
    mocc = np.concatenate([[0.0], 1.0 - njc])
    pB = np.concatenate([[0.0], pB]); pE = np.concatenate([[0.0], pE])
    btot = np.cumsum(pB); etot = np.cumsum(pE)
    dA, dT, dZ = mocc - pB - rt2, mocc - rt1, mocc - pE - rt2
    lists = dA.tolist(), dT.tolist(), dZ.tolist()
    regions = _scan(*lists)
    near, near_count, alt, dist, counts = set(), False, set(), {}, set()
    for kind, d in (("A", dA), ("T", dT), ("Z", dZ)):
        for i in np.flatnonzero(np.abs(d) < tol):
            if i == 0:
                continue
            other = _scan(*lists, flip=(int(i), kind))
            if other != regions:
                near_count |= len(other) != len(regions)
                counts.add(len(other))
                moved = set(regions) ^ set(other)
                near |= moved & set(regions)
                alt |= set(other)
                for rg in moved & set(regions):
                    dist[rg] = min(dist.get(rg, math.inf), abs(float(d[i])))
    multi = []
    for i1, i2 in regions:
        z = np.arange(i1, i2 + 1)
        multi.append(float(np.minimum(etot[z] - etot[i1 - 1], btot[i2] - btot[z - 1]).max()))
    return regions, dict(near_regions=near, near_count=near_count, alt_regions=alt, alt_counts=counts, dist=[dist.get(rg, math.inf) for rg in regions],
                         multi=multi, total=tot)


def domain_bits_fast(h, seq, ienv, jenv):
    """domain_bits, nodes vectorised: (bits, domcorrection_nats, envsc_nats)"""
    f = prepare(h)
    M, odds = f["M"], f["odds"]
    L = len(seq)
    x = codes_of(seq[ienv - 1:jenv])
    Ld = len(x)
    r = _fb(f, x, float(L), True)
    envsc, ll = r["total"], r["lloop"]
    ppM = np.exp(r["fM"][1:, 1:] + r["bM"][1:Ld + 1, 1:M + 1] - envsc).sum(axis=0)
    ppI = np.exp(r["fI"][1:, 1:M] + r["bI"][1:Ld + 1, 1:M] - envsc).sum()
    ppX = (np.exp(r["fN"][:-1] + ll + r["bN"][1:] - envsc) + np.exp(r["fC"][:-1] + ll + r["bC"][1:] - envsc)).sum()
    null2 = ((ppM[:, None] * odds[1:]).sum(axis=0) + ppI + ppX) / Ld
    n2 = np.log(np.array([null2[list(CODE[c])].mean() for c in _SYMS]))
    domcorr = float(n2[x].sum())
    nullsc = L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))
    dombias = math.log(1.0 + math.exp(math.log(1.0 / 256.0) + domcorr))
    bits = (envsc + (L - Ld) * math.log(L / (L + 3.0)) - (nullsc + dombias)) / math.log(2.0)
    return bits, domcorr, envsc


def report(rows, T=10.0, domE=10.0):
    """hmmsearch's reporting under the reference's flags (-T 10: a sequence is reported when its bit score is at least T; domE 10
    with domZ = the number of REPORTED sequences of the profile: a domain of a reported sequence is reported when its E-value
    P * domZ is at most domE).  rows: dicts with prof, seq, seq_score (bits), lnP (natural log of the domain's P-value); sets
    seq_reported / dom_reported on each and returns domZ per profile."""
    reported = {}
    for r in rows:
        r["seq_reported"] = r["seq_score"] >= T
        if r["seq_reported"]:
            reported.setdefault(r["prof"], set()).add(r["seq"])
    domZ = {p: len(s) for p, s in reported.items()}
    for r in rows:
        r["dom_reported"] = bool(r["seq_reported"]) and math.exp(r["lnP"]) * domZ.get(r["prof"], 0) <= domE
    return domZ


def domtbl_lines(rows, names, prof_names):
    """--domtblout lines (the columns ItsPosition reads: target, tlen, query, domain score, envelope from / to) of the reported
    rows, in hmmsearch's order: profile, then target, then domain"""
    out = []
    for r in sorted((r for r in rows if r["dom_reported"]), key=lambda r: (r["prof"], r["seq"], r["dom_idx"])):
        out.append("%s - %d %s - 0 0 0 0 0 0 0 0 %.1f 0 0 0 0 0 %d %d 0 -" % (
            names[r["seq"]], r["tlen"], prof_names[r["prof"]], r["bitscore"], r["ienv"], r["jenv"]))
    return "\n".join(out) + "\n"
