"""Checks of a search result (the CPU oracle's or the engine's trace and domain rows) against the independent float64 statement of
tests/hmm_generic.py, shared by tests/test_generic_cpu.py and tests/test_gpu_generic.py.

Scores must agree within tol(L) = max(2e-3, 6 (L + M) 2^-24) nats: the per-row rounding budget of a float32 Forward over L + M steps
that the lazy margin (engine.hip, lazy_c) already assumes.  A discrete outcome (a filter's pass, the number of regions, an envelope,
a reporting decision, a per-read winner) must equal the float64 decision unless the float64 value lies within tol of its threshold;
such pairs are counted and listed, never dropped silently.  The envelopes of a multidomain region take their null2 from sampled
paths: their domcorrection and the pair's seq_score are stated by tests/ensemble_exact.py's model of that stage (check(ens=...))."""
import math
import os
import tempfile

import numpy as np

import hmm_generic as G

LN2 = math.log(2.0)
F = 1e-6                                      # --F1 / --F3 of the reference
T_SEQ, DOM_E = 10.0, 10.0


def tol(L, M):
    return max(2e-3, 6.0 * (L + M) * 2.0 ** -24)


def msv_limit(L, M):
    """the byte MSV filter against the float64 MSV: every emission score is rounded to a 1/3-bit unit (at most ln 2 / 6 nats each,
    and a consensus hit repeats the same few values, so the errors add up along a full-length hit of M residues), plus HMMER's
    constant 3-nat stand-in for the N / C / J loops, which really cost 3 (L - l) / L for the l residues on the hits (up to three
    full-length hits here)"""
    return M * LN2 / 6.0 + 3.0 * min(1.0, 3.0 * M / L)


def nullsc(L):
    return L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))


def msv_threshold_bits(h):
    mu, lam = h["stats"]["MSV"]
    return mu - math.log(-math.log1p(-F)) / lam             # gumbel survival <= F


def fwd_threshold_bits(h):
    tau, lam = h["stats"]["FORWARD"]
    return tau - math.log(F) / lam                          # exponential tail <= F


def pool_size():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _task(args):
    """float64 side of one profile and a chunk of its reads"""
    h, items = args
    seqs = [s for _, s, _, _ in items]
    msv = G.msv_nats_batch(h, seqs)
    flt = G.bias_filter_nats_batch(h, seqs)
    fwd = G.forward_nats_batch(h, seqs)
    out = []
    for j, (idx, s, decode, envs) in enumerate(items):
        r = dict(msv=float(msv[j]), filt=float(flt[j]), fwd=float(fwd[j]))
        if decode:
            r["regions"], r["info"] = G.decode_regions_fast(h, s, tol=tol(len(s), h["M"]))
        r["doms"] = [G.domain_bits_fast(h, s, i, e) for i, e in envs]
        out.append((idx, r))
    return out


def float64_side(hm, seqs, pairs, pool):
    """pairs: {(seq, prof): (decode?, [(ienv, jenv), ...])} -> {(seq, prof): float64 results}"""
    tasks = []
    for p in sorted({p for _, p in pairs}):
        items = [(s, seqs[s], d, e) for (s, pp), (d, e) in sorted(pairs.items()) if pp == p]
        chunk, n = [], 0
        for it in items:
            chunk.append(it)
            n += len(it[1]) * (4 if it[2] else 1)
            if n > 6000:
                tasks.append((hm[p], chunk)); chunk, n = [], 0
        if chunk:
            tasks.append((hm[p], chunk))
    tasks.sort(key=lambda t: -sum(len(x[1]) for x in t[1]))
    out = {}
    for (h, _), res in zip(tasks, pool.map(_task, tasks)):
        for idx, r in res:
            out[(idx, h["_i"])] = r
    return out


class Report:
    def __init__(self, name, n_pairs):
        self.name, self.n_pairs = name, n_pairs
        self.worst = {}
        self.near = []
        self.fail = []
        self.unstated = 0
        self.close = 0

    def dev(self, q, d, lim, what):
        d = abs(d)
        self.worst[q] = max(self.worst.get(q, 0.0), d / lim)
        if not d <= lim:
            self.fail.append("%s: %s off by %.3g (limit %.3g) at %s" % (self.name, q, d, lim, what))

    def decide(self, q, got, want, dist, lim, what, alts=()):
        """got must equal the float64 decision `want`; a disagreement is excused (counted in `near`, capped, listed) only where the
        float64 value lies within lim of its threshold and `got` is what the other side of it gives (`alts`, or any for a yes / no
        decision); agreements within lim are only counted (`close`)"""
        same = bool(got) == bool(want) if isinstance(want, (bool, np.bool_)) else got == want
        if same:
            if dist < lim:
                self.close += 1
        elif dist < lim and (isinstance(want, (bool, np.bool_)) or got in alts):
            self.near.append((q, what, dist))
        else:
            self.fail.append("%s: %s is %s, float64 says %s (%.3g from the threshold, tol %.3g) at %s" % (self.name, q, got, want, dist, lim, what))

    def line(self):
        w = " ".join("%s=%.2f" % (k, v) for k, v in sorted(self.worst.items()))
        return "[%s] pairs=%d excused-near=%d (byte MSV band: %d; agreeing within tol: %d; ensemble seq_score not stated: %d) " \
            "worst(dev/tol): %s" % (self.name, self.n_pairs, len({x[1] for x in self.near if not x[0].startswith("msv")}),
                                    len({x[1] for x in self.near if x[0].startswith("msv")}), self.close, self.unstated, w)

    def finish(self):
        """fails on any disagreement beyond tol, and when more than 1 % of the pairs sit within tol of a threshold (outside the byte
        MSV band, which is that filter's quantisation); the near pairs are listed either way"""
        msg = self.fail[:20]
        near = sorted({x[1] for x in self.near if not x[0].startswith("msv")})
        if len(near) > 0.01 * self.n_pairs:
            msg.append("%s: %d of %d pairs within tol of a threshold (cap 1 %%)" % (self.name, len(near), self.n_pairs))
        if msg:
            msg += ["near: %s %s %.3g" % x for x in sorted(self.near, key=lambda x: x[0].startswith("msv"))[:40]]
        assert not msg, "\n".join(msg + [self.line()])
        return self.line()


def ensemble_models(hs, hm, seqs, trace, seqfield, pool):
    """the float64 model of the traceback ensemble (tests/ensemble_exact.py) for every pair of the result that reached the domain
    stage: what check() takes as `ens`.  hs: orc.HmmSet of the same profile text (the model replays the oracle's sampled paths)."""
    import ensemble_exact as EX
    pairs = [(int(r[seqfield]), int(r["prof"])) for r in trace if r["pass_fwd"] and r["nregions"] > 0]
    md = EX.model_pairs(hs, hm, seqs, pairs, pool)
    rolls, exc, msg = EX.verdict([r for lst in md.values() for _, r in lst])
    assert msg is None, msg
    return {k: [r for _, r in lst] for k, lst in md.items()}


def check(name, hm, seqs, trace, dom, seqfield, pool, sample=None, seed=0, msv_all=False, ens=None):
    """Every check of the float64 statement on one search result.  trace / dom: PairTrace / Domain rows; seqfield: "seq" (oracle) or
    "rep" (engine); sample: at most this many pairs past the Forward filter are decoded (fixed seed), None = all; ens: the float64
    model's multidomain regions per pair (ensemble_models), whose per-residue null2 scores state an ensemble envelope's
    domcorrection and the pair's seq_score.  Returns (Report, float64 domain rows) -- the rows carry float64 scores at the result's
    own envelopes and float64 reporting."""
    for i, h in enumerate(hm):
        h["_i"] = i
    rep = Report(name, len(trace))
    key = lambda r: (int(r[seqfield]), int(r["prof"]))
    pf = [key(r) for r in trace if r["pass_fwd"]]
    if sample is not None and len(pf) > sample:
        rng = np.random.default_rng(seed)
        pf = [pf[i] for i in sorted(rng.choice(len(pf), sample, replace=False))]
    decode = set(pf)
    envs = {}
    for d in dom:
        envs.setdefault(key(d), []).append((int(d["ienv"]), int(d["jenv"])))
    pairs = {key(r): (key(r) in decode, envs.get(key(r), [])) for r in trace}        # every envelope is scored: reporting needs them all
    g = float64_side(hm, seqs, pairs, pool)
    doms_by = {}
    for d in dom:
        doms_by.setdefault(key(d), []).append(d)
    rows = []
    for r in trace:
        s, p = key(r)
        h, x, L = hm[p], g[(s, p)], len(seqs[s])
        M = h["M"]
        tl = tol(L, M)
        what = "(read %d, profile %d, L %d)" % (s, p, L)
        ns = nullsc(L)
        rep.dev("nullsc", (float(r["nullsc"]) - ns) / max(1.0, abs(ns)), 1e-6, what)
        mthr = msv_threshold_bits(h) * LN2
        mq = msv_limit(L, M)
        if r["msv_xj"] < 255:
            rep.dev("msv_sc", float(r["msv_sc"]) - x["msv"], mq, what)
        else:
            rep.decide("msv_overflow", True, bool(x["msv"] - ns > mthr), abs(x["msv"] - ns - mthr), mq, what)
        rep.decide("msv_pass", int(r["pass_msv"]), bool(x["msv"] - ns >= mthr), abs(x["msv"] - ns - mthr), mq, what)
        if not r["pass_msv"]:
            continue
        rep.dev("filtersc", float(r["filtersc"]) - x["filt"], tl, what)
        v = float(r["msv_sc"]) - x["filt"] - mthr                    # the bias filter re-tests the (byte) MSV score
        rep.decide("pass_bias", int(r["pass_bias"]), bool(v >= 0), abs(v), tl, what)
        if not r["pass_bias"]:
            continue
        rep.dev("fwdsc", float(r["fwdsc"]) - x["fwd"], tl, what)
        v = x["fwd"] - x["filt"] - fwd_threshold_bits(h) * LN2
        rep.decide("pass_fwd", int(r["pass_fwd"]), bool(v >= 0), abs(v), tl, what)
        if not r["pass_fwd"]:
            continue
        rep.dev("bcksc", float(r["bcksc"]) - x["fwd"], tl, what)
        ds = doms_by.get((s, p), [])
        regs, info = x.get("regions"), x.get("info")
        if regs is not None:
            # a region counts as near only if flipping one test within tol of its threshold moves it (hmm_generic._scan)
            rep.decide("nregions", int(r["nregions"]), len(regs), 0.0 if info["near_count"] else math.inf, tl, what, info["alt_counts"])
            for (i1, i2), mu, dd in zip(regs, info["multi"], info["dist"]):
                single = [(int(d["ienv"]), int(d["jenv"])) for d in ds if i1 <= d["ienv"] and d["jenv"] <= i2 and not d["flags"] & 1]
                w2 = what + " region %d-%d" % (i1, i2)
                if abs(mu - 0.20) < tl:
                    rep.near.append(("multi", what, abs(mu - 0.20)))
                elif mu < 0.20 and not info["near_count"]:
                    rep.decide("single envelope", single, [(i1, i2)], dd, tl, w2, [[a] for a in info["alt_regions"]])
            ok = set(regs) | info["alt_regions"]
            for d in ds:                                                # every envelope lies inside one float64 region
                if any(i1 <= d["ienv"] and d["jenv"] <= i2 for i1, i2 in regs):
                    continue
                w2 = what + " envelope %d-%d outside %s" % (d["ienv"], d["jenv"], regs)
                if any(i1 <= d["ienv"] and d["jenv"] <= i2 for i1, i2 in ok):
                    rep.near.append(("envelope", w2, 0.0))
                else:
                    rep.fail.append("%s: envelope outside every float64 region at %s" % (name, w2))
        # scores at the result's own envelopes; the sequence score from the whole-sequence Forward and the reconstruction
        lnn3 = math.log(L / (L + 3.0))
        env_sc, cor_sum, ld_sum = 0.0, 0.0, 0
        cors = []
        mregs = ens.get((s, p)) if ens is not None else None           # the ensemble model's regions of this pair, or None
        stated = mregs is not None
        for d, (bits, corr, envsc) in zip(ds, x["doms"]):
            Ld = int(d["jenv"]) - int(d["ienv"]) + 1
            w2 = what + " envelope %d-%d" % (d["ienv"], d["jenv"])
            rep.dev("envsc", float(d["envsc"]) - envsc, tl, w2)
            if d["flags"] & 1:
                # an ensemble envelope: HMMER takes its null2 from the sampled traces (p7_Null2_ByTrace): the sum of the model's
                # per-residue scores over the envelope.  Where the region was not modelled (no `ens`, or a matrix that could not be
                # sampled) the bit score must still follow from the result's own correction in closed form
                mr = [m for m in mregs or () if m["ireg"] <= d["ienv"] and d["jenv"] <= m["jreg"] and (int(d["ienv"]), int(d["jenv"])) in m["envs"]]
                if mr:
                    corr = float(mr[0]["n2sc"][int(d["ienv"]) - mr[0]["ireg"]:int(d["jenv"]) - mr[0]["ireg"] + 1].sum())
                    rep.dev("ens_domcorrection", float(d["domcorrection"]) - corr, tol(Ld, M), w2)
                else:
                    if mregs is not None:
                        rep.fail.append("%s: ensemble envelope is not one of the model's at %s" % (name, w2))
                    stated = False
                    corr = float(d["domcorrection"])
                bits = (envsc + (L - Ld) * lnn3 - ns - math.log1p(math.exp(math.log(1 / 256.0) + corr))) / LN2
            else:
                rep.dev("domcorrection", float(d["domcorrection"]) - corr, tol(Ld, M), w2)
            rep.dev("bitscore", float(d["bitscore"]) - bits, tl / LN2, w2)
            tau, lam = h["stats"]["FORWARD"]
            b = float(d["bitscore"])
            lnp = -lam * (b - tau) if b > tau else 0.0
            rep.dev("lnP", (float(d["lnP"]) - lnp) / max(1.0, abs(lnp)), 1e-6, w2)
            cors.append(corr)
            if envsc - corr > 0:
                env_sc += envsc; cor_sum += corr; ld_sum += Ld
            rows.append(dict(prof=p, seq=s, dom_idx=int(d["dom_idx"]), tlen=L, ienv=int(d["ienv"]), jenv=int(d["jenv"]),
                             bitscore=bits, lnP=-lam * (bits - tau) if bits > tau else 0.0, lam=lam, tl=tl,
                             got_seq=int(d["seq_reported"]), got_dom=int(d["dom_reported"])))
        if ds:
            # the whole-sequence null2 sums the per-residue scores of every region: a single envelope's correction, and ALL of a
            # multidomain region's trace-based scores, the residues between its envelopes included
            allcor = sum(c for c, d in zip(cors, ds) if not d["flags"] & 1 or not stated) + \
                (sum(float(m["n2sc"].sum()) for m in mregs) if stated else 0.0)
            whole = (x["fwd"] - ns - math.log1p(math.exp(math.log(1 / 256.0) + allcor))) / LN2
            sc, recon = whole, -math.inf
            if ld_sum > 0:
                recon = (env_sc + (L - ld_sum) * lnn3 - ns - math.log1p(math.exp(math.log(1 / 256.0) + cor_sum))) / LN2
                sc = max(whole, recon)
            if any(d["flags"] & 1 for d in ds) and not stated:
                # without the model the trace-based per-residue scores between the envelopes are unknown (the domain rows do not
                # carry them): not stated (counted); reporting takes the result's own score for it
                rep.unstated += 1
                sc = float(ds[0]["seq_score"])
            else:
                rep.dev("seq_score", float(ds[0]["seq_score"]) - sc, tl / LN2, what)
            for rr in rows[len(rows) - len(ds):]:
                rr["seq_score"] = sc
    # reporting, from the float64 scores
    G.report(rows, T_SEQ, DOM_E)
    near_seq = {}
    for rr in rows:
        if abs(rr["seq_score"] - T_SEQ) < rr["tl"] / LN2:
            near_seq.setdefault(rr["prof"], set()).add(rr["seq"])
    for rr in rows:
        what = "(read %d, profile %d, domain %d)" % (rr["seq"], rr["prof"], rr["dom_idx"])
        rep.decide("seq_reported", rr["got_seq"], bool(rr["seq_reported"]), abs(rr["seq_score"] - T_SEQ), rr["tl"] / LN2, what)
        z = sum(1 for q in rows if q["prof"] == rr["prof"] and q["dom_idx"] == 0 and q["seq_reported"])
        zl, zh = max(1, z - len(near_seq.get(rr["prof"], ()))), z + len(near_seq.get(rr["prof"], ()))
        dist = min(abs(rr["lnP"] + math.log(zz) - math.log(DOM_E)) for zz in (zl, zh)) / rr["lam"]     # in bits of the domain score
        if (rr["lnP"] + math.log(zl) <= math.log(DOM_E)) != (rr["lnP"] + math.log(zh) <= math.log(DOM_E)):
            dist = 0.0
        rr["dom_near"] = dist < rr["tl"] / LN2
        if rr["seq_reported"] or rr["got_seq"]:
            rep.decide("dom_reported", rr["got_dom"], bool(rr["dom_reported"]), dist, rr["tl"] / LN2, what)
    return rep, rows


def winners(rows, names, prof_names, left, right):
    """per read: the float64 ItsPosition answer (start, stop, tlen; -1 = None) for the reads that have a reported row, and whether the
    float64 decision is within tol of flipping (a runner-up's score or a reporting decision near its threshold)"""
    from itsxpress_amd.SeqSample import ItsPosition
    region = {("3_", "4_"): "ITS2", ("1_", "2_"): "ITS1"}[(left, right)]
    with tempfile.NamedTemporaryFile("w", suffix=".domtbl", delete=False) as f:
        f.write(G.domtbl_lines(rows, names, prof_names))
    try:
        pos = ItsPosition(f.name, region)
    finally:
        os.unlink(f.name)
    out, shaky = {}, set()
    r10 = lambda v: math.floor(v * 10 + 0.5)
    cand = {}
    for rr in rows:
        pn = prof_names[rr["prof"]]
        side = "L" if pn.startswith(left) else "R" if pn.startswith(right) else None
        if side:
            cand.setdefault((rr["seq"], side), []).append(rr)
    for (s, side), rs in cand.items():
        t = rs[0]["tl"] / LN2
        if any(abs(r["seq_score"] - T_SEQ) < t or r["dom_near"] for r in rs):
            shaky.add(s)
        live = [r for r in rs if r["dom_reported"]]
        iv = [(r10(r["bitscore"] - t), r10(r["bitscore"] + t)) for r in live]
        for a in range(len(live)):
            for b in range(a + 1, len(live)):
                (la, ha), (lb, hb) = iv[a], iv[b]
                if (la != ha or lb != hb) and la <= hb and lb <= ha:
                    shaky.add(s)
    for s in {rr["seq"] for rr in rows if rr["dom_reported"]}:
        st, sp, tl_ = pos.get_position(names[s])
        out[s] = (-1 if st is None else st, -1 if sp is None else sp, -1 if tl_ is None else tl_)
    return out, shaky
