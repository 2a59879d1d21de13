"""Pass A's row state (csrc/k_lazy.hip: k_fwd_bound, k_bwd_bound) in float64, on the CPU: the folded recurrences carried as TWO
cell arrays per row -- S_k = M~_k mm_k + I^_k im_k + D^_k dm_k (what node k sends to the next row's match cell M_k+1) and
I+_k = I^_k ii_k + M~_k (the next row's insert cell) -- against the same recurrences carried as the three arrays M~, I^, D^, and
the Backward kernel's dual state (W, G) against the Forward sum: for EVERY cut row c

    score = sum_k S_k W_k + sum_k I+_k G_k + N gN + J gJ + C gC + B gB        (plus both scale logarithms)

The folded constants are computed as engine.hip's install_profiles computes them, for a 45-node model of tests/golden and the
same model stretched to 46 nodes (the last pair's second node live).  No GPU."""
import math

import numpy as np

import edge_cases
import hmm_generic as G

K = 46                       # nodes the kernels hold: 23 pairs
LENGTHS = (1, 2, 15, 16, 17, 32, 33, 65)
MM, MI, MD, IM, II, DM, DD = range(7)


def _constants(h):
    """the plain constants by SOURCE node k = 1..K (index 0 unused) and their folded forms, as install_profiles builds them"""
    M, t = h["M"], h["t"]
    occ = np.zeros(M + 1)
    occ[1] = t[0][MI] + t[0][MM]
    for k in range(2, M + 1):
        occ[k] = occ[k - 1] * (t[k - 1][MM] + t[k - 1][MI]) + (1.0 - occ[k - 1]) * t[k - 1][DM]
    Z = sum(occ[k] * (M - k + 1) for k in range(1, M + 1))
    z = lambda: np.zeros(K + 2)
    p = dict(bm=z(), mm=z(), im=z(), dm=z(), mi=z(), ii=z(), md=z(), dd=z())
    for k in range(1, M + 1):
        p["bm"][k] = occ[k] / Z
        if k < M:                                  # the local profile: nothing leaves the last node but the exit
            p["mm"][k], p["im"][k], p["dm"][k] = t[k][MM], t[k][IM], t[k][DM]
            p["mi"][k], p["ii"][k], p["md"][k], p["dd"][k] = t[k][MI], t[k][II], t[k][MD], t[k][DD]
    H = np.ones(K + 3)
    for k in range(K, 0, -1):
        H[k] = 1.0 + p["dd"][k] * H[k + 1]
    g = np.ones(K + 2); s = np.ones(K + 3); a = np.zeros(K + 2); r = np.ones(K + 2)
    for k in range(1, K + 1):
        g[k] = 1.0 + p["md"][k] * H[k + 1]
    for k in range(1, K + 1):
        if p["md"][k] > 0.0:
            s[k + 1] = p["md"][k] / g[k]
            a[k] = s[k] * p["dd"][k] / s[k + 1]
        else:
            assert not (p["dd"][k] > 0.0 and k > 1), "not foldable"
        if p["mi"][k] > 0.0:
            r[k] = p["mi"][k] / g[k]
        else:
            assert p["ii"][k] == 0.0 and p["im"][k] == 0.0, "not foldable"
    f = dict(bm=p["bm"][1:K + 1].copy(), mm=(p["mm"] / g)[1:K + 1], im=(p["im"] * r)[1:K + 1], dm=(p["dm"] * s[:K + 2])[1:K + 1],
             ii=p["ii"][1:K + 1].copy(), a=a[1:K + 1].copy(), g=g[1:K + 1].copy())
    em = np.zeros((K, 4))
    em[:M] = h["mat"][1:M + 1] / 0.25
    return p, f, em


def _odds(em, ch):
    if ch == "N":                                  # a degenerate residue: the expected score
        with np.errstate(divide="ignore"):
            return np.exp(np.log(em).mean(axis=1))
    return em[:, "ACGT".index(ch)]


def _plain_forward(p, em, seq):
    """the unfolded sum over paths (M, I, D; E adds the deletes), for the score alone"""
    L = len(seq)
    pmove = 3.0 / (L + 3.0); ploop = 1.0 - pmove
    Mv = np.zeros(K + 2); Iv = np.zeros(K + 2); Dv = np.zeros(K + 2)
    xN, xJ, xC, xB = 1.0, 0.0, 0.0, pmove
    for ch in seq:
        e = _odds(em, ch)
        send = Mv * p["mm"] + Iv * p["im"] + Dv * p["dm"]
        Mn = np.zeros(K + 2); Dn = np.zeros(K + 2)
        Mn[1:K + 1] = (xB * p["bm"][1:K + 1] + send[0:K]) * e
        In = Mv * p["mi"] + Iv * p["ii"]
        for k in range(2, K + 1):
            Dn[k] = Dn[k - 1] * p["dd"][k - 1] + Mn[k - 1] * p["md"][k - 1]
        xE = Mn.sum() + Dn.sum()
        xN *= ploop; xC = xC * ploop + 0.5 * xE; xJ = xJ * ploop + 0.5 * xE; xB = (xJ + xN) * pmove
        Mv, Iv, Dv = Mn, In, Dn
    return math.log(xC * pmove)


def _dchain(mn, a):
    """D^'_1 = 0, D^'_k+1 = D^'_k a_k + M~'_k"""
    d = np.zeros(K)
    for k in range(1, K):
        d[k] = d[k - 1] * a[k - 1] + mn[k - 1]
    return d


def _specials(sp, xE, pmove):
    xN, xJ, xC, xB = sp
    ploop = 1.0 - pmove
    xN *= ploop; xC = xC * ploop + 0.5 * xE; xJ = xJ * ploop + 0.5 * xE
    return [xN, xJ, xC, (xJ + xN) * pmove]


def _forward_three(f, em, seq, thr):
    """rows 0..L of the three-array folded recurrence: (M~, I^, D^, specials, scale)"""
    L = len(seq); pmove = 3.0 / (L + 3.0)
    Mv = np.zeros(K); Iv = np.zeros(K); Dv = np.zeros(K); sp = [1.0, 0.0, 0.0, pmove]; sc = 0.0
    rows = [(Mv, Iv, Dv, list(sp), sc)]
    for ch in seq:
        e = _odds(em, ch) * f["g"]
        S = Mv * f["mm"] + Iv * f["im"] + Dv * f["dm"]
        Mn = (sp[3] * f["bm"] + np.concatenate([[0.0], S[:-1]])) * e
        In = Iv * f["ii"] + Mv
        Dn = _dchain(Mn, f["a"])
        xE = Mn.sum()
        sp = _specials(sp, xE, pmove)
        Mv, Iv, Dv = Mn, In, Dn
        if xE > thr:
            Mv, Iv, Dv = Mv / xE, Iv / xE, Dv / xE; sp = [v / xE for v in sp]; sc += math.log(xE)
        rows.append((Mv, Iv, Dv, list(sp), sc))
    return rows


def _forward_two(f, em, seq, thr):
    """rows 0..L of the kernel's recurrence: (S, I+, specials, scale); M~ and D^ live for one row only"""
    L = len(seq); pmove = 3.0 / (L + 3.0)
    S = np.zeros(K); Ip = np.zeros(K); sp = [1.0, 0.0, 0.0, pmove]; sc = 0.0
    rows = [(S, Ip, list(sp), sc)]
    nresc = 0
    for ch in seq:
        e = _odds(em, ch) * f["g"]
        Mn = (sp[3] * f["bm"] + np.concatenate([[0.0], S[:-1]])) * e
        Dn = _dchain(Mn, f["a"])
        xE = Mn.sum()
        S = Mn * f["mm"] + Ip * f["im"] + Dn * f["dm"]
        Ip = Ip * f["ii"] + Mn
        sp = _specials(sp, xE, pmove)
        if xE > thr:
            S, Ip = S / xE, Ip / xE; sp = [v / xE for v in sp]; sc += math.log(xE); nresc += 1
        rows.append((S, Ip, list(sp), sc))
    return rows, nresc


def _backward_two(f, em, seq, every, hi):
    """gamma after rows L..0 in the kernel's dual state (W, G, gN gJ gC gB, scale): W_k = w_k+1 of the last row pulled back, G_k = the
    insert adjoint that row was entered with; a sum test every `every` rows keeps the cells small"""
    L = len(seq); pmove = 3.0 / (L + 3.0); ploop = 1.0 - pmove
    W = np.zeros(K); Gv = np.zeros(K); gN = gJ = gB = 0.0; gC = pmove; sc = 0.0
    out = {L: (W, Gv, [gN, gJ, gC, gB], sc)}
    nresc = 0
    for step, row in enumerate(range(L, 0, -1)):
        e = _odds(em, seq[row - 1]) * f["g"]
        gb0 = gB * pmove
        nJ, nN = gJ + gb0, gN + gb0
        aE = 0.5 * (nJ + gC)
        gD = f["dm"] * W
        gM = f["mm"] * W + Gv
        Gv = f["im"] * W + f["ii"] * Gv
        aD = np.zeros(K + 1)
        for k in range(K - 1, -1, -1):
            aD[k] = gD[k] + f["a"][k] * aD[k + 1]
        w = e * (gM + aE + aD[1:])
        W = np.concatenate([w[1:], [0.0]])
        gB = float((f["bm"] * w).sum())
        gN, gJ, gC = ploop * nN, ploop * nJ, ploop * gC
        if step % every == every - 1:
            tot = W.sum() + Gv.sum() + gN + gJ + gC + gB
            if tot > hi or 0.0 < tot < 1.0 / hi:
                W, Gv = W / tot, Gv / tot; gN, gJ, gC, gB = gN / tot, gJ / tot, gC / tot, gB / tot; sc += math.log(tot); nresc += 1
        out[row - 1] = (W, Gv, [gN, gJ, gC, gB], sc)
    return out, nresc


def _reads(h, rng):
    acgt = "ACGT"
    cons = "".join(acgt[int(np.argmax(h["mat"][k]))] for k in range(1, h["M"] + 1))
    out = []
    for L in LENGTHS:
        s = "".join(acgt[i] for i in rng.integers(0, 4, L))
        out.append(("acgt", s))
        n = list(s)
        for pos in (0, 15, 16, 31, 32, L - 1):      # an N at a cut: the cuts run over every row
            if pos < L:
                n[pos] = "N"
        out.append(("n", "".join(n)))
    out.append(("domains", (cons + "ACGTTGCA")[:65]))   # a whole domain: E grows by many powers of ten
    return out


def test_two_array_state_pairs_with_its_dual_at_every_cut(mini_hmm_text):
    b45 = next(b + "//\n" for b in mini_hmm_text.split("//\n") if "LENG  45" in b)
    models = G.parse_hmms(b45) + G.parse_hmms(edge_cases._stretch(b45, 46))
    assert [h["M"] for h in models] == [45, 46]
    rng = np.random.default_rng(2025)
    rel = lambda x, y: abs(x - y) / max(abs(y), 1e-300)
    for h in models:
        p, f, em = _constants(h)
        if h["M"] == 46:
            assert f["bm"][45] > 0.0 and em[45].max() > 0.0        # the last pair's second node is live
        for kind, seq in _reads(h, rng):
            L = len(seq)
            thr = 1e3 if kind == "domains" else 1e20
            three = _forward_three(f, em, seq, thr)
            two, nresc = _forward_two(f, em, seq, thr)
            bwd, nb = _backward_two(f, em, seq, 16 if kind != "domains" else 4, 1e6 if kind != "domains" else 1e2)
            if kind == "domains":
                assert nresc >= 3 and nb >= 1, (nresc, nb)
            Mv, Iv, Dv, sp, sc = three[L]
            full = sc + math.log(sp[2] * 3.0 / (L + 3.0))
            # the folded sum is the plain sum over paths
            assert abs(full - _plain_forward(p, em, seq)) <= 1e-10 * max(1.0, abs(full)), (h["M"], kind, L)
            for c in range(L + 1):
                Mv, Iv, Dv, sp3, sc3 = three[c]
                S, Ip, sp2, sc2 = two[c]
                k = math.exp(sc2 - sc3)                             # (both runs rescale at the same rows; the factor is then 1)
                S3 = Mv * f["mm"] + Iv * f["im"] + Dv * f["dm"]
                I3 = Iv * f["ii"] + Mv
                scale = max(S3.max(), I3.max(), 1e-300)
                assert np.abs(S * k - S3).max() <= 1e-12 * scale and np.abs(Ip * k - I3).max() <= 1e-12 * scale, (h["M"], kind, L, c)
                assert all(rel(x * k, y) <= 1e-12 for x, y in zip(sp2, sp3) if y > 0.0)
                W, Gv, gs, gsc = bwd[c]
                dot = float((S * W).sum() + (Ip * Gv).sum() + sum(x * y for x, y in zip(sp2, gs)))
                assert dot > 0.0
                got = sc2 + gsc + math.log(dot)
                assert abs(math.expm1(got - full)) <= 1e-10, (h["M"], kind, L, c, got, full)
