"""An INDEPENDENT float64 statement of the stage that resolves a multidomain region (p7_domaindef.c: region_trace_ensemble -- 200
stochastic tracebacks over the region's multihit Forward matrix, null2 by trace, single-linkage clustering of the sampled domains),
for tests only.  Written from the published procedure as docs/HISTORY.md section 2 and oracle/orc_search.c's header describe it:
unstriped, in log space, on hmm_generic's Forward matrix; it shares no code with oracle/ or the engine.

A sampled path cannot be repeated by another arithmetic unless every random choice falls on the same side of every boundary, so
the model REPLAYS the oracle's recorded paths (orc.ensemble_debug): at every step it forms the branch probabilities of the
state in float64, draws its own roll from its own restatement of the generator, and requires that the branch the oracle took is the
one whose cumulative interval holds the roll.  It then goes on along the oracle's path, so one excused step cannot cascade.  The
sampled tuples, the per-residue null2 scores and the envelopes are then derived from the replayed path by the model's own rules.

Band: a roll is near a boundary c of the cumulative distribution when |roll - c| <= 2 tol(Lr, M) min(c, 1 - c) + 2^-23 (the
relative error of a normalised float32 probability within generic_check's per-row budget, plus esl_vec_FNorm's float32
division).  A step is excused only if every boundary between the model's branch and the oracle's is that near, or if the step drew
fallback rolls; excused steps are counted and listed, and at most 1 roll in 1000 of a test may be excused (CAP)."""
import math

import numpy as np

import generic_check as GC
import hmm_generic as G

NSAMPLES = 200
CAP = 1e-3
M_, D_, I_, S_, N_, B_, E_, C_, T_, J_ = range(1, 11)            # state codes of the recorded steps (orc.ST_*)
_MM, _MI, _MD, _IM, _II, _DM, _DD = range(7)
_U32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------- generator
def rnd_mix3(a, b, c):
    """esl_rnd_mix3 (Bob Jenkins' mix) on 32-bit words"""
    a = (a - b - c) & _U32; a ^= c >> 13
    b = (b - c - a) & _U32; b ^= (a << 8) & _U32
    c = (c - a - b) & _U32; c ^= b >> 13
    a = (a - b - c) & _U32; a ^= c >> 12
    b = (b - c - a) & _U32; b ^= (a << 16) & _U32
    c = (c - a - b) & _U32; c ^= b >> 5
    a = (a - b - c) & _U32; a ^= c >> 3
    b = (b - c - a) & _U32; b ^= (a << 10) & _U32
    c = (c - a - b) & _U32; c ^= b >> 15
    return c


def rng_start(seed=42):
    """esl_randomness_CreateFast(seed): the state every region starts from (do_reseeding)"""
    return rnd_mix3(seed, 87654321, 12345678) or 42


def rng_step(x):
    return (69069 * x + 1) & _U32


# ---------------------------------------------------------------------------------------------------------------- replay
def estate_order(M):
    """the order in which the E state's choice walks the cells, HMMER's striped one: q = 0 .. Q-1, inside it the four match cells
    k = r Q + q + 1 (r = 0 .. 3), then the four delete cells; cells with k > M count zero"""
    Q = max(2, (M - 1) // 4 + 1)
    cells = []
    for q in range(Q):
        for st in (M_, D_):
            for r in range(4):
                cells.append((st, r * Q + q + 1))
    return cells


def _cum(logs):
    m = max(logs)
    p = [math.exp(v - m) if v > G.NEG / 2 else 0.0 for v in logs]
    s = sum(p)
    out, acc = [], 0.0
    for v in p:
        acc += v / s
        out.append(acc)
    out[-1] = 1.0
    return out


def _pick(cum, roll):
    for j, c in enumerate(cum):
        if roll < c:
            return j
    return len(cum) - 1


def _near(roll, c, t):
    return abs(roll - c) <= 2.0 * t * min(c, 1.0 - c) + 2.0 ** -23


def replay(h, seq, reg):
    """One region of one (profile, read) pair.  reg: orc.ensemble_debug's record.  Returns dict(rolls, excused [(trace, step, why)],
    contradictions [(trace, step, what)], rng_ok, doms: per trace the domains in sampling order (last first), each
    (i, j, k, m, cntM, cntI) in region coordinates)"""
    f = G.prepare(h)
    M, bm, lt = f["M"], f["bm"], f["lt"]
    ireg, jreg = reg["ireg"], reg["jreg"]
    Lr = jreg - ireg + 1
    x = G.codes_of(seq[ireg - 1:jreg])
    r = G._fb(f, x, float(len(seq)), False)
    fM, fI, fD, fN, fB, fE, fJ, fC = (r[k] for k in ("fM", "fI", "fD", "fN", "fB", "fE", "fJ", "fC"))
    lmove, lloop, lE = r["lmove"], r["lloop"], r["lE"]
    t = GC.tol(Lr, M)
    cells = estate_order(M)
    ecum = {}
    out = dict(rolls=0, excused=[], contradictions=[], rng_ok=reg["rng0"] == rng_start(), doms=[])
    bad = out["contradictions"]
    rng = rng_start()
    steps = reg["steps"]
    tr_, s0_, s1_, k_, i_, nd_ = (steps[n].tolist() for n in ("trace", "s0", "s1", "k", "i", "ndraw"))
    cur_trace = -1
    s = k = i = 0
    doms = None
    for n in range(len(tr_)):
        if tr_[n] != cur_trace:
            if cur_trace >= 0 and s != S_:
                bad.append((cur_trace, n, "path does not end in S"))
            cur_trace = tr_[n]
            s, k, i = C_, 0, Lr
            doms = []
            out["doms"].append(doms)
        where = (cur_trace, n)
        if s0_[n] != s:
            bad.append(where + ("step starts in state %d, the path stands in %d" % (s0_[n], s),))
            s = s0_[n]
        if s == N_:                                                   # N draws nothing
            want = (S_ if i == 0 else N_, k, i)
            if (s1_[n], k_[n], i_[n]) != want or nd_[n] != 0:
                bad.append(where + ("N step %s, expected %s" % ((s1_[n], k_[n], i_[n], nd_[n]), want),))
        else:
            if s == M_:
                logs = [fB[i - 1] + bm[k], fM[i - 1, k - 1] + lt[k - 1, _MM], fI[i - 1, k - 1] + lt[k - 1, _IM], fD[i - 1, k - 1] + lt[k - 1, _DM]]
                outs = [(B_, k - 1, i - 1), (M_, k - 1, i - 1), (I_, k - 1, i - 1), (D_, k - 1, i - 1)]
            elif s == D_:
                logs = [fM[i, k - 1] + lt[k - 1, _MD], fD[i, k - 1] + lt[k - 1, _DD]]
                outs = [(M_, k - 1, i), (D_, k - 1, i)]
            elif s == I_:
                logs = [fM[i - 1, k] + lt[k, _MI], fI[i - 1, k] + lt[k, _II]]
                outs = [(M_, k, i - 1), (I_, k, i - 1)]
            elif s == C_:
                logs = [fC[i - 1] + lloop, fE[i] + lE]
                outs = [(C_, k, i), (E_, k, i)]
            elif s == J_:
                logs = [fJ[i - 1] + lloop, fE[i] + lE]
                outs = [(J_, k, i), (E_, k, i)]
            elif s == B_:
                logs = [fN[i] + lmove, fJ[i] + lmove]
                outs = [(N_, k, i), (J_, k, i)]
            elif s == E_:
                logs = None
                outs = [(st, kk, i) for st, kk in cells]
            else:
                bad.append(where + ("no such state %d" % s,))
                break
            if logs is not None:
                cum = _cum(logs)
            else:
                cum = ecum.get(i)
                if cum is None:
                    cum = ecum[i] = _cum([(fM[i, kk] if st == M_ else fD[i, kk]) if kk <= M else G.NEG for st, kk in cells])
            rng = rng_step(rng)
            roll = rng / 4294967296.0
            out["rolls"] += 1
            got = (s1_[n], k_[n], i_[n])
            a = _pick(cum, roll)
            if got not in outs:
                bad.append(where + ("state %d at k %d, i %d cannot go to %s" % (s, k, i, got),))
            elif outs[a] != got:
                b = outs.index(got)
                lo, hi = min(a, b), max(a, b)
                if nd_[n] > 1:
                    out["excused"].append(where + ("fallback draws",))
                elif all(_near(roll, cum[j], t) for j in range(lo, hi)):
                    out["excused"].append(where + ("roll %.9f within the band of boundary %.9f" % (roll, cum[lo]),))
                else:
                    bad.append(where + ("state %d at k %d, i %d: roll %.9f selects %s, the path took %s (boundaries %s)"
                                        % (s, k, i, roll, outs[a], got, ["%.9f" % c for c in cum[lo:hi]]),))
            elif nd_[n] != 1:
                out["excused"].append(where + ("fallback draws",))
            for _ in range(max(0, nd_[n] - 1)):                       # keep the generator in step with the path's extra draws
                rng = rng_step(rng)
        # along the oracle's path
        s1, k, i = s1_[n], k_[n], i_[n]
        if s == E_:
            doms.append([0, 0, 0, 0, np.zeros(M + 1), np.zeros(M + 1)])  # a domain opens, read backwards: this is its end
        if s1 == M_:
            if not doms:
                bad.append(where + ("a match state outside a domain",))
            else:
                d = doms[-1]
                if d[1] == 0:
                    d[1], d[3] = i, k                                  # first seen = last match state in path order
                d[0], d[2] = i, k
                d[4][k] += 1
        elif s1 == I_ and doms:
            doms[-1][5][k] += 1
        if s1 in (N_, J_, C_) and s1 == s:
            i -= 1
        s = s1
    if cur_trace >= 0 and s != S_:
        bad.append((cur_trace, len(tr_), "path does not end in S"))
    if len(out["doms"]) != NSAMPLES:
        bad.append((-1, -1, "%d paths recorded, not %d" % (len(out["doms"]), NSAMPLES)))
    return out


# ---------------------------------------------------------------------------------------------------------------- null2 by trace
def null2_by_trace(h, seq, ireg, jreg, doms):
    """per residue of the region: ln of the mean over the paths of (null2[x] inside a domain but after its first residue, 1 otherwise),
    null2[x] = sum_k cntM_k / Ld odds_k(x) + sum_k cntI_k / Ld of that domain, a degenerate code taking the mean over its bases"""
    odds = G.prepare(h)["odds"]
    x = G.codes_of(seq[ireg - 1:jreg])
    Lr = len(x)
    acc = np.zeros(Lr + 1)
    base = np.array([[1.0 if b in G.CODE[c] else 0.0 for b in range(4)] for c in G._SYMS])
    base /= base.sum(axis=1, keepdims=True)
    for path in doms:
        row = np.ones(Lr + 1)
        for i, j, k, m, cM, cI in path:
            Ld = cM.sum() + cI.sum()
            n2 = (cM[:, None] / Ld * odds).sum(axis=0) + cI.sum() / Ld
            row[i + 1:j + 1] = (base @ n2)[x[i:j]]                 # residues i+1 .. j of the region
        acc += row
    return np.log(acc[1:] / len(doms))


# ---------------------------------------------------------------------------------------------------------------- clustering
_f32 = np.float32


def tuples_of(doms, ireg):
    """(trace, i, j, k, m) per path and domain in absolute coordinates, each path's domains last-first"""
    return [(t, d[0] + ireg - 1, d[1] + ireg - 1, d[2], d[3]) for t, path in enumerate(doms) for d in path]


def _hist_pick(vals, thr, leftmost):
    lo, hi = int(vals.min()), int(vals.max())
    cnt = np.bincount(vals - lo, minlength=hi - lo + 1)
    ok = np.flatnonzero(cnt >= thr)
    if len(ok):
        return lo + int(ok[0] if leftmost else ok[-1])
    return lo + int(np.argmax(cnt))                                   # the first maximum of the histogram


def cluster(tuples):
    """p7_spensemble_Cluster(min_overlap 0.8 of the smaller, max_diagdiff 4, min_posterior 0.25, min_endpointp 0.02) on the sampled
    tuples of 200 paths, then the removal of dominated clusters: [(i, j), ...] ordered by start.  Integer logic; the comparisons
    the published code makes in float are evaluated in np.float32."""
    if not len(tuples):
        return []
    t = np.asarray(tuples, np.int64).reshape(-1, 5)
    tr, i, j, k, m = t.T
    n = len(t)
    mn, mx = np.minimum.outer, np.maximum.outer
    nov = mn(j, j) - mx(i, i) + 1
    ln = mn(j - i + 1, j - i + 1)
    link = ~((nov.astype(_f32) / ln.astype(_f32)) < _f32(0.8))
    nov = mn(m, m) - mx(k, k)                                          # as published: no "+ 1" on the model side
    ln = mn(m - k + 1, m - k + 1)
    link &= ~((nov.astype(_f32) / ln.astype(_f32)) < _f32(0.8))
    d1, d2 = i - k, j - m
    link &= (np.abs(np.subtract.outer(d1, d1)) <= 4) | (np.abs(np.subtract.outer(d2, d2)) <= 4)
    comp = np.full(n, -1)
    nc = 0
    for h0 in range(n):                                               # single linkage; components numbered by their smallest member
        if comp[h0] >= 0:
            continue
        comp[h0] = nc
        todo = [h0]
        while todo:
            v = todo.pop()
            new = np.flatnonzero(link[v] & (comp < 0))
            comp[new] = nc
            todo.extend(new.tolist())
        nc += 1
    sig = []
    for c in range(nc):
        sel = comp == c
        trs = tr[sel]
        ninc = 1 + int((trs[1:] != trs[:-1]).sum())                   # the paths the cluster occurs in
        if _f32(ninc) / _f32(NSAMPLES) < _f32(0.25):
            continue
        thr = int(np.ceil(_f32(ninc) * _f32(0.02)))
        bi, bk = _hist_pick(i[sel], thr, True), _hist_pick(k[sel], thr, True)
        bj, bm = _hist_pick(j[sel], thr, False), _hist_pick(m[sel], thr, False)
        if bi > bj or bk > bm:
            continue
        sig.append((bi, bj, _f32(ninc) / _f32(NSAMPLES)))
    sig.sort(key=lambda s: s[0])                                      # stable
    dominated = [False] * len(sig)
    for a in range(len(sig)):
        for b in range(a + 1, len(sig)):
            nov = min(sig[a][1], sig[b][1]) - max(sig[a][0], sig[b][0]) + 1
            if nov == 0:
                break
            nn = min(sig[a][1] - sig[a][0] + 1, sig[b][1] - sig[b][0] + 1)
            if _f32(nov) / _f32(nn) >= _f32(0.8):
                if sig[a][2] > sig[b][2]:
                    dominated[b] = True
                else:
                    dominated[a] = True
    return [(s[0], s[1]) for s, d in zip(sig, dominated) if not d]


# ---------------------------------------------------------------------------------------------------------------- one region, many regions
def model_region(args):
    """(profile dict, read, oracle record) -> the model's statement of the region: dict(ireg, jreg, M, rolls, excused,
    contradictions, rng_ok, n2sc float64[Lr], envs [(i, j)], degenerate: the region holds a degenerate residue)"""
    h, seq, reg = args
    rp = replay(h, seq, reg)
    ireg, jreg = reg["ireg"], reg["jreg"]
    res = dict(ireg=ireg, jreg=jreg, M=h["M"], L=len(seq), rolls=rp["rolls"], excused=rp["excused"], contradictions=rp["contradictions"],
               rng_ok=rp["rng_ok"], degenerate=any(c.upper() not in "ACGTU" for c in seq[ireg - 1:jreg]))
    if len(rp["doms"]) == NSAMPLES and not any(c[0] < 0 for c in rp["contradictions"]):
        res["n2sc"] = null2_by_trace(h, seq, ireg, jreg, rp["doms"])
        res["envs"] = cluster(tuples_of(rp["doms"], ireg))
    else:
        res["n2sc"], res["envs"] = np.zeros(jreg - ireg + 1), []
    return res


def model_pairs(hs, hm, seqs, pairs, pool):
    """The model's statement of every multidomain region of the given (read, profile) pairs: {(read, profile): [(oracle record,
    model_region result), ...]}.  hs: orc.HmmSet and hm: hmm_generic.parse_hmms of the same profile text; the oracle's recorded
    paths are taken here (orc.ensemble_debug) and the regions fanned out over the pool."""
    import orc
    keys, tasks = [], []
    out = {}
    for s, p in sorted(set(pairs)):
        out[(s, p)] = []
        for reg in orc.ensemble_debug(hs, p, seqs[s]):
            keys.append((s, p, reg))
            tasks.append((hm[p], seqs[s], reg))
    for (s, p, reg), res in zip(keys, pool.map(model_region, tasks)):
        out[(s, p)].append((reg, res))
    return out


def verdict(results):
    """the replay's verdict over a test's regions: (rolls, excused, message or None) -- no contradiction, the generator's start state
    restated right, and at most CAP of the rolls excused"""
    rolls = sum(r["rolls"] for r in results)
    exc = [(r["ireg"], r["jreg"]) + e for r in results for e in r["excused"]]
    bad = [(r["ireg"], r["jreg"]) + c for r in results for c in r["contradictions"]]
    msg = []
    if not all(r["rng_ok"] for r in results):
        msg.append("the generator's start state is not esl_rnd_mix3(42, 87654321, 12345678) = %d" % rng_start())
    if bad:
        msg.append("%d contradictions in %d rolls:" % (len(bad), rolls))
        msg += ["  region %d-%d path %d step %d: %s" % b for b in bad[:20]]
    if len(exc) > CAP * rolls:
        msg.append("%d of %d rolls excused (cap 1 in 1000):" % (len(exc), rolls))
    if msg:
        msg += ["  excused: region %d-%d path %d step %d: %s" % e for e in exc[:20]]
    return rolls, exc, "\n".join(msg) if msg else None


# ---------------------------------------------------------------------------------------------------------------- inputs
# The smallest shapes at which the stage can go wrong, shared by tests/test_ensemble_exact_cpu.py and
# tests/test_gpu_ensemble_exact.py.  Tandem partial copies of a profile's consensus WITHOUT flanks, found by a random search
# like the reads of tests/test_gpu_caps.py, so that a multidomain region starts at residue 1 and one ends at residue L:
TANDEM_46 = ("ATTAGGCCGAGGGCACGTCTGCCTGGGCGTCACCGAAGCCATTAGGCCGAGGGCACCCGAAGCCATTAGGCCGAGGGCACGTCTGCACGTCTGCCTGGGC",      # region 1-100 = the read
             "TAGGCCGAGGGCACGTCTGCCTGGGCGTCACGCAGCCATTAGGCCGAGGGCACGTCTGCCTGGGCGCGAAGCCATTAGGCCGAGGGCACGGCACGTCTGCCTGGGCGTC",
             "GGGCACGTCTGCCTGGGCATTAGGCCGAGGGCACGTCTGCCTGGGCAGCCATTAGGCCGAGGGCACGTCTGCCTGGGCGTCACGGCCCGAAGCCATTAGGCCGAGGGCACGTCTGCCTGGGCGTCG"
             "GCCGAGGGCACGTCTGCCCCGAGGGCACGTCTGCCTGGG")
TANDEM_25 = ("GAACCTGCGGAAGGATCATTGTGAACCTGCGGAAGGTGAACCTGTGCGGAAG", "ACCTGCGGAAGGATCATTGTGCGGAAGGGTGAACCTGCGGAAGGTGCGGAAGCTGCGGAAGGATCAT",
             "CCTGCGGAAGGTGAACCTGCGGAAGGATTGCGGAAGGATCATT")
TANDEM_11 = ("AAGGATCATAAGGAAGGATCATTGGATCATTG", "AGGATCATTGAGGAATCATTAGGATCATTGATCAGATCATTG", "AGGATCAATCATTGAGGATCATTGAGGATCATTAGGATCAT")


def inputs(t_hmm_text, mini_hmm_text):
    """[(name, profile text, reads)]: the adversarial reads of tests/test_gpu_caps.py (many envelopes; the device's overflow path),
    the parity workload's ordinary regions, the node-count edges of the striping (M = 46: Q = 12 and two padding cells in the
    E state's order; M = 25, 11: Q = 7, 3 and three, one) on reads without flanks, and degenerate residues inside a region"""
    import edge_cases
    import synth
    from test_gpu_caps import READ_ENVELOPES, READ_PATH_DOMAINS, READ_TUPLES
    blob, offs = synth.make_reads(t_hmm_text, 400, seed=5, fixed_len=0, len_range=(300, 580))
    bl = edge_cases._blocks(mini_hmm_text)
    b45 = next(b for b in bl if "LENG  45" in b)
    edges = edge_cases._stretch(b45, 46) + "".join(b for b in bl if "LENG  11" in b or "LENG  25" in b)
    rng = np.random.default_rng(53)
    deg = READ_PATH_DOMAINS
    for sym in "NRY":
        deg = edge_cases._sprinkle(rng, deg, 0.02 / 3, sym)
    return [("adversarial", mini_hmm_text, [READ_PATH_DOMAINS, READ_TUPLES, READ_ENVELOPES]),
            ("parity", edge_cases._its2(t_hmm_text, 6, 6), synth.to_strings(blob, offs)),
            ("node_edges", edges, list(TANDEM_46 + TANDEM_25 + TANDEM_11)),
            ("degenerate", mini_hmm_text, [deg])]


def oracle_and_model(hmm, seqs, pool, threads=8):
    """the oracle's search of the reads, and the model's statement of every multidomain region of every pair that reached the domain
    stage: (orc.SearchResult, orc.HmmSet, parsed profiles, {(read, profile): [(oracle record, model result), ...]})"""
    import orc
    hs = orc.HmmSet(text=hmm)
    hm = G.parse_hmms(hmm)
    codes, o = orc.digitize(seqs)
    res = orc.SearchResult(hs, codes, o, keep_trace=1, threads=threads)
    pairs = [(int(r["seq"]), int(r["prof"])) for r in res.trace if r["pass_fwd"]]
    return res, hs, hm, model_pairs(hs, hm, seqs, pairs, pool)


def assert_inputs_hold_their_edges(models):
    """models: {input name: (seqs, hm, model dict)} -- a case cannot silently go empty"""
    regs = [(name, s, p, reg, r, seqs, hm) for name, (seqs, hm, md) in models.items() for (s, p), lst in md.items() for reg, r in lst]
    assert len(regs) >= 25, len(regs)
    assert any(len(r["envs"]) >= 5 for *_, r, _, _ in regs)
    assert any(r["ireg"] == 1 for *_, r, _, _ in regs) and any(r["jreg"] == r["L"] for *_, r, _, _ in regs)
    assert any(r["degenerate"] for *_, r, _, _ in regs)
    Ms = {r["M"] for *_, r, _, _ in regs}
    assert 46 in Ms and 45 in Ms and (11 in Ms or 25 in Ms), Ms
    return regs
