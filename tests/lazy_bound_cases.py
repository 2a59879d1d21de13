"""One catalogue of the edges of the lazy domain stage's bound (csrc/k_lazy.hip), shared by
tests/test_lazy_bound_cpu.py and tests/test_gpu_lazy_bound.py, with the float64 statements both hold the engine to.

The stage is exact only if, for every pair past the MSV filter and every domain of the pair,

    bits <= (fwdsc - nullsc) / ln 2 + C(n),   C(n) = 1 + (2 ln(2 (n + 3) / (3 (n + 2))) + n ln((n + 3) / (n + 2))) / ln 2

for the fwdsc pass A computes (n = target length); k_lazy_bound turns the right side, with LenTables::lazy_c = C(n) + a rounding
margin in place of C(n), into biased %.1f tenths (b10_model below restates it operation by operation).

Every case is named and seeded: case(name, ...) -> Case(hmm, seqs, F), F = the --F1 = --F2 = --F3 the searches of the case run with.
Cases are small (at most ~130 reads, at most 12 profiles: tests/golden/mini.hmm's ten -- M = 45, 25 and 11 -- plus a 3_ and a 4_
profile of the stand-in taxon stretched to the engine's 46 nodes), and every case of tests/edge_cases.py is one too.
"""
import math
from collections import namedtuple

import numpy as np

import edge_cases as EC
import hmm_generic as G
import synth

Case = namedtuple("Case", "hmm seqs F")

LN2 = math.log(2.0)
F_REF = 1e-6                # the reference's --F1 / --F3
F_LOOSE = 0.5               # nearly everything passes the filters: targets of a few residues reach pass A, weak pairs the domain stage
MMAX = 46                   # the engine's node limit (csrc/engine.h)
TENTHS_MAX = (1 << 24) - 1


# ---------------------------------------------------------------------------------------------------------- float64 statements
def c_of_n(n):
    n = float(n)
    return 1.0 + (2.0 * math.log(2.0 * (n + 3.0) / (3.0 * (n + 2.0))) + n * math.log((n + 3.0) / (n + 2.0))) / LN2


def margin_bits(n):
    """max(0.02, 6 (n + M) 2^-24 / ln 2) bits, M = the engine's node limit"""
    return max(0.02, 6.0 * (float(n) + MMAX) * 2.0 ** -24 / LN2)


def nullsc(n):
    return n * math.log(n / (n + 1.0)) + math.log(1.0 / (n + 1.0))


def bound_bits(fwd_nats, n):
    """the right side of the inequality, in float64, with no margin"""
    return (fwd_nats - nullsc(n)) / LN2 + c_of_n(n)


def b10_model(fb, nsc, lazy_c, bias):
    """k_lazy_bound's arithmetic in numpy float64, the same operations and constants in the same order: fb, nsc, lazy_c are the
    float32 values the kernel read.  NaN and +inf = no usable bound (the largest tenths: always evaluated), -inf = the smallest
    bound a pair can have (1; 0 means "no pair here")."""
    fb = np.asarray(fb, np.float32)
    f = fb.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        bits = (f - np.asarray(nsc, np.float32).astype(np.float64)) / 0.69314718055994529 + np.asarray(lazy_c, np.float32).astype(np.float64)
        t = np.floor(bits * 10.0 + 0.5) + float(bias)                       # round half UP
    t = np.where(t < 1.0, 1.0, t)
    t = np.where(t > float(TENTHS_MAX), float(TENTHS_MAX), t)
    t = np.where(np.isnan(fb) | (fb == np.inf), float(TENTHS_MAX), t)
    t = np.where(fb == -np.inf, 1.0, t)
    return t.astype(np.uint32)


def printed_tenths(x):
    """the tenths Python's "%.1f" prints for x (what ItsPosition reads from domtbl.txt's score column)"""
    s = "%.1f" % float(x)
    neg = s.startswith("-")
    a, b = s.lstrip("-").split(".")
    v = int(a) * 10 + int(b)
    return -v if neg else v


# ---------------------------------------------------------------------------------------------------------------------- profiles
def profiles(t, mini):
    """mini.hmm's ten profiles + one 3_ and one 4_ profile of the stand-in taxon, stretched from 45 to the engine's 46 nodes"""
    bl = EC._blocks(t)
    have = {EC._name(b) for b in EC._blocks(mini)}
    b3 = next(b for b in bl if EC._name(b).startswith("3_") and "LENG  45" in b and EC._name(b) not in have)
    b4 = next(b for b in bl if EC._name(b).startswith("4_") and "LENG  45" in b and EC._name(b) not in have)
    hmm = mini + EC._stretch(b3, 46) + EC._stretch(b4, 46)
    names = [EC._name(b) for b in EC._blocks(hmm)]
    assert len(names) == 12 and len(set(names)) == 12
    return hmm


def _cons(hmm):
    c = synth.consensus_motifs(hmm, "")
    assert all(c)
    return c


def _uniq(seqs):
    out, seen = [], set()
    for s in seqs:
        if s and s not in seen:
            seen.add(s); out.append(s)
    return out


# ------------------------------------------------------------------------------------------------------------------------- cases
def whole_target(t, mini, allt, fx):
    """each profile's consensus alone: the envelope is 1..n and Ld = n.  The filters run at F_LOOSE: the pairs of a consensus with
    the OTHER profiles, whose weak rows lie nearest the bound, reach the domain stage too"""
    hmm = profiles(t, mini)
    return Case(hmm, _uniq(_cons(hmm)), F_LOOSE)


def _short(kind):
    def build(t, mini, allt, fx):
        """pieces of the consensus of a 46-, the 25- and the 11-node profile, of every length from M down to 1 (the GPU test prints
        the shortest that reached pass A); the filters run at F_LOOSE, below their natural floor"""
        hmm = profiles(t, mini)
        cons = _cons(hmm)
        src = [next(c for c in cons if len(c) == m) for m in (46, 25, 11)]
        seqs = []
        for c in src:
            M = len(c)
            for k in range(M, 0, -1):
                a = {"prefix": 0, "suffix": M - k, "infix": (M - k) // 2}[kind]
                seqs.append(c[a:a + k])
        return Case(hmm, _uniq(seqs), F_LOOSE)
    return build


def degenerate_consensus(t, mini, allt, fx):
    """consensus with N and two-letter IUPAC codes at 10, 20 and 30 % of the positions, the first and the last residue among them"""
    rng = np.random.default_rng(6101)
    hmm = profiles(t, mini)
    two = {"A": "RMW", "C": "YMS", "G": "RKS", "T": "YKW"}
    seqs = []
    for c in _cons(hmm):
        for rate in (0.1, 0.2, 0.3):
            for kind in ("N", "two", "mix"):
                s = list(c)
                k = max(2, int(round(rate * len(s))))
                pos = {0, len(s) - 1} | set(int(p) for p in rng.choice(np.arange(1, len(s) - 1), k - 2, replace=False))
                for p in pos:
                    n = kind == "N" or (kind == "mix" and rng.random() < 0.5)
                    # a two-letter code that holds the consensus base, or (one time in three) one that does not
                    s[p] = "N" if n else (rng.choice(list(two.get(s[p], "RYKM"))) if rng.random() < 0.67 else rng.choice(list("RYKMSW")))
                seqs.append("".join(s))
    return Case(hmm, _uniq(seqs), F_LOOSE)      # (as whole_target: the float64 trial's smallest slack is a weak pair of this case)


def tandem(t, mini, allt, fx):
    """2, 3 and 12 back-to-back copies of every consensus, and the tandem PARTIAL copies of edge_cases.multidomain: multidomain
    regions, whose envelopes take their null2 from sampled traces, and (12 copies, and the three adversarial reads of
    tests/test_gpu_caps.py) the ensemble stage's overflow path"""
    rng = np.random.default_rng(6102)
    hmm = profiles(t, mini)
    cons = _cons(hmm)
    from test_gpu_caps import READ_ENVELOPES, READ_PATH_DOMAINS, READ_TUPLES      # mini.hmm's reads that leave the ensemble kernel's bookkeeping
    seqs = [c * k for c in cons for k in (2, 3, 12)] + [READ_PATH_DOMAINS, READ_TUPLES, READ_ENVELOPES]
    for j in range(8):
        c = cons[int(rng.integers(0, len(cons)))]
        parts = [EC._rnd(rng, int(rng.integers(0, 40)))]
        for _ in range(int(rng.integers(3, 7))):
            a = int(rng.integers(0, len(c) // 2))
            parts.append(c[a:int(rng.integers(a + len(c) // 3, len(c) + 1))])
        seqs.append("".join(parts) + EC._rnd(rng, int(rng.integers(0, 40))))
    return Case(hmm, _uniq(seqs), F_REF)


def flanked(t, mini, allt, fx):
    """every consensus inside 60 and inside 500 random bases on either side"""
    rng = np.random.default_rng(6103)
    hmm = profiles(t, mini)
    seqs = [EC._rnd(rng, f) + c + EC._rnd(rng, f) for c in _cons(hmm) for f in (60, 500)]
    return Case(hmm, seqs, F_REF)


def flanked_long(t, mini, allt, fx):
    """the two 46-node profiles alone on a CCS-shaped target of 20 kb and on one of the engine's longest, 65 535 residues"""
    rng = np.random.default_rng(6104)
    hmm = "".join(EC._blocks(profiles(t, mini))[-2:])
    c3, c4 = _cons(hmm)
    seqs = EC._ccs_reads(t, rng, [20000], per_family=1)
    seqs.append(EC._rnd(rng, 65535 - 310 - len(c3) - len(c4) - 700) + c3 + EC._rnd(rng, 310) + c4 + EC._rnd(rng, 700))
    assert len(seqs[-1]) == 65535
    return Case(hmm, seqs, F_REF)


WAVE_LENGTHS = (31, 32, 33, 63, 64, 65)       # at the 32-row block edges of the prefix / suffix trees (ITSX_SHARE_B's default)


def _waves(n):
    def build(t, mini, allt, fx):
        """n distinct near-copies of the 25-node profile's consensus in random flanks, lengths mixed inside a wave; the members of a
        family (one length) differ in their first base (the suffix is shared: a two-sided join), their last base (the prefix is
        shared: a one-sided chain), at a block boundary and next to it; n = 63 / 65 / 130 leave a ragged last wave"""
        rng = np.random.default_rng(6105)
        hmm = profiles(t, mini)
        c = next(x for x in _cons(hmm) if len(x) == 25)
        fams = []
        for L in WAVE_LENGTHS:
            a = (L - len(c)) // 2
            base = EC._rnd(rng, a) + c + EC._rnd(rng, L - len(c) - a)
            fam = [base]
            for pos in [0, L - 1, 31, 32, 1, L - 2, 30, 33, 2, L - 3]:
                if 0 <= pos < L:
                    for step in (1, 2, 3):
                        v = list(base)
                        v[pos] = "ACGT"[("ACGT".index(v[pos]) + step) % 4]
                        fam.append("".join(v))
            fams.append(_uniq(fam))
        seqs, k = [], 0
        while len(seqs) < n:                       # the families interleaved: a wave of 64 pairs holds every length
            assert any(k < len(f) for f in fams)
            for f in fams:
                if k < len(f) and len(seqs) < n and f[k] not in seqs:
                    seqs.append(f[k])
            k += 1
        assert len(seqs) == n == len(set(seqs))
        return Case(hmm, seqs, F_REF)
    return build


def _edge(name):
    def build(t, mini, allt, fx):
        hmm, seqs, _ = EC.case(name, t, mini, allt, fx)
        return Case(hmm, list(seqs), F_REF)
    build.__doc__ = "tests/edge_cases.py: %s, at its own size" % name
    return build


CASES = dict(whole_target=whole_target, short_prefix=_short("prefix"), short_suffix=_short("suffix"), short_infix=_short("infix"),
             degenerate_consensus=degenerate_consensus, tandem=tandem, flanked=flanked, flanked_long=flanked_long,
             waves_63=_waves(63), waves_64=_waves(64), waves_65=_waves(65), waves_130=_waves(130))
CASES.update({"edge_" + k: _edge(k) for k in EC.CASES})
OWN = [k for k in CASES if not k.startswith("edge_")]


def case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs):
    c = CASES[name](t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs)
    assert 0 < len(c.seqs) <= 135 and c.hmm.count("NAME  ") <= 12 or name.startswith("edge_")
    return c


# ------------------------------------------------------------------------------------------ the float64 side, one task per chunk
def forward_task(args):
    """float64 multihit Forward scores (nats) of a few reads against one profile: [(key, score)]"""
    h, items = args
    sc = G.forward_nats_batch(h, [s for _, s in items])
    return [(k, float(v)) for (k, _), v in zip(items, sc)]


def forward_float64(hm, seqs, pairs, pool):
    """{(seq, prof): float64 Forward nats} for the (seq index, profile index) pairs; reads of like length share a padded batch"""
    tasks = []
    for p in sorted({p for _, p in pairs}):
        items = sorted(((s, p), seqs[s]) for s, pp in pairs if pp == p)
        items.sort(key=lambda it: len(it[1]))
        chunk = []
        for it in items:
            if chunk and (len(chunk) >= 48 or len(it[1]) > 1.25 * len(chunk[0][1]) + 8):
                tasks.append((hm[p], chunk)); chunk = []
            chunk.append(it)
        if chunk:
            tasks.append((hm[p], chunk))
    tasks.sort(key=lambda t: -len(t[1][-1][1]))
    out = {}
    for res in pool.map(forward_task, tasks):
        out.update(res)
    return out


def inequality_task(args):
    """the inequality in float64 for one (read, profile): every envelope decode_regions_fast finds, plus the whole target.
    Returns (key, [(ienv, jenv, bits, bound, slack)]); a pair the profile cannot emit at all (Forward = 0) has no row."""
    key, h, s = args
    L = len(s)
    regs, info = G.decode_regions_fast(h, s)
    fwd = info["total"]
    if fwd < G.NEG / 2:
        return key, []
    rows = []
    for i, j in sorted(set(regs) | {(1, L)}):
        bits = G.domain_bits_fast(h, s, i, j)[0]
        b = bound_bits(fwd, L)
        rows.append((i, j, float(bits), float(b), float(b - bits)))
    return key, rows
