"""The catalogue of hand-made domain tables for the exact model of tests/position_exact.py: one seeded list of named cases, shared by
tests/test_position_exact_cpu.py (the model against the reference's golden vectors and the formatter) and tests/test_gpu_position_edges.py
(the engine against the model).  A case is a read set, a profile set, a table in physical segments, the counters and domE."""
import gzip
import json
import math
import os
import random

import numpy as np

import position_exact as X
from position_exact import Row

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINLEN = 32                       # derep(minseqlength): shorter reads are dropped
_COMP = str.maketrans("ACGT", "TGCA")


# ---------------------------------------------------------------- profiles
def _blocks(text):
    return [b + "//\n" for b in text.split("//\n") if "NAME  " in b]


def _names(text):
    return [ln[6:].strip() for ln in text.split("\n") if ln.startswith("NAME  ")]


_HMM = {}


def hmm_text(kind):
    """"mini": the 10 profiles of tests/golden/mini.hmm (3 x 3_, 2_, 3 x 4_, 3 x 1_); "wide": 20 profiles of each of the four prefixes
    out of T.hmm.gz, interleaved so that a prefix's profiles are not contiguous"""
    if kind not in _HMM:
        if kind == "mini":
            with open(os.path.join(GOLD, "mini.hmm")) as f:
                _HMM[kind] = f.read()
        else:
            with gzip.open(os.path.join(GOLD, "T.hmm.gz"), "rt") as f:
                bl = _blocks(f.read())
            by = {p: [b for b in bl if b.split("NAME  ")[1].startswith(p)][:20] for p in ("3_", "4_", "1_", "2_")}
            out = []
            for k in range(20):
                for p in ("3_", "1_", "4_", "2_"):
                    if k < len(by[p]):
                        out.append(by[p][k])
            _HMM[kind] = "".join(out)
    return _HMM[kind]


def profile_names(kind):
    return _names(hmm_text(kind))


# ---------------------------------------------------------------- reads
class ReadSet(object):
    """a few dozen distinct random reads of 20-400 bases, some of them again (plus strand and minus strand), some too short to be kept;
    the dereplication stated in plain Python: uniques in input order of their first occurrence, within a sample"""

    def __init__(self, kind):
        rng = random.Random(20240611)
        lens = [300, 301, 302, 303, 304, 305] + [32, 33, 64, 400, 399, 255, 256, 257, 100, 77] + [rng.randint(34, 398) for _ in range(20)]
        seqs = ["".join(rng.choice("ACGT") for _ in range(n)) for n in lens]
        rc = lambda s: s[::-1].translate(_COMP)
        seqs += ["".join(rng.choice("ACGT") for _ in range(n)) for n in (20, 31, 25)]        # dropped
        seqs += [seqs[0], rc(seqs[2]), seqs[7], rc(seqs[9]), rc(seqs[0]), seqs[35]]           # members of earlier reads' clusters, plus and minus strand
        self.sample_of = None
        self.S = 1
        if kind == "two":                          # the same reads as a second sample: twice the uniques, counters per sample
            self.sample_of = [0] * len(seqs) + [1] * len(seqs)
            seqs = seqs + seqs
            self.S = 2
        self.seqs = seqs
        seen, self.uniq_of, self.seed_read, self.usample = {}, [], [], []
        for i, s in enumerate(seqs):
            if len(s) < MINLEN:
                self.uniq_of.append(-1)
                continue
            k = (self.sample_of[i] if self.sample_of else 0, min(s, rc(s)))
            if k not in seen:
                seen[k] = len(self.seed_read)
                self.seed_read.append(i)
                self.usample.append(k[0])
            self.uniq_of.append(seen[k])
        self.U = len(self.seed_read)
        self.ulen = [len(seqs[r]) for r in self.seed_read]


_READS = {}


def reads(kind):
    if kind not in _READS:
        _READS[kind] = ReadSet(kind)
    return _READS[kind]


# ---------------------------------------------------------------- cases
class Case(object):
    def __init__(self, name, segments, domz=None, domE=10.0, reads="one", hmm="mini", regions=("ITS2", "ITS1", "ALL"), expect=None,
                 lazy=None, compact_refused=None):
        self.name, self.segments, self.domE, self.reads, self.hmm, self.regions = name, segments, float(domE), reads, hmm, tuple(regions)
        self.names = profile_names(hmm)
        self.P = len(self.names)
        rs = globals()["reads"](reads)
        self.domz = [int(z) for z in (domz if domz is not None else [1] * (self.P * rs.S))]
        assert len(self.domz) == self.P * rs.S
        self.expect = expect            # {region: {rep: (start, stop, tlen, in_ddict)}} from a recorded reference run
        self.lazy = lazy                # None, or dict(lb=[...], ub=[...]) of a lazy table
        self.compact_refused = compact_refused      # None, or dict(env={...}) under which finalize must refuse this case's counters / domE
        for seg in segments:
            for r in seg:
                assert r.is_padding() or (0 <= r.rep < rs.U and 0 <= r.prof < self.P and r.tlen == rs.ulen[r.rep] and -200 <= r.bitscore <= 2000), (name, r)

    @property
    def rows(self):
        return [r for seg in self.segments for r in seg]

    def usample(self):
        rs = reads(self.reads)
        return rs.usample if rs.S > 1 else None

    def __repr__(self):
        return "Case(%s)" % self.name


def pad(real=False):
    """a padding row; real=True: one that carries a winning score, which only its dom_idx < 0 keeps out"""
    if real:
        return Row(0, 0, 300, 1, 299, dom_idx=-1, bitscore=1999.0, lnP=-300.0)
    return Row(-1, -1, 0, 0, 0, dom_idx=-1)


def to_array(rows, flags=None):
    from itsxpress_amd._lib import DOMAIN_DTYPE
    a = np.zeros(len(rows), DOMAIN_DTYPE)
    for i, r in enumerate(rows):
        a[i] = (r.rep, r.prof, r.tlen, r.ienv, r.jenv, r.dom_idx, r.ndom, r.flags, 0.0, 0.0, 0.0, r.bitscore, r.lnP, r.bitscore, 0.0, r.seq_reported,
                0 if flags is None or flags[i] is None else flags[i])
    return a


def _layouts(name, rows, seed, **kw):
    """a table in table order, reversed, shuffled, and shuffled over three segments (one of them empty) with padding rows at their ends
    and in between"""
    rows = sorted(rows, key=lambda r: r.ident())
    rng = random.Random(seed)
    sh = [r.copy() for r in rows]
    rng.shuffle(sh)
    sh2 = [r.copy() for r in rows]
    rng.shuffle(sh2)
    a, b = len(sh2) // 3, 2 * len(sh2) // 3
    mid = sh2[a:b]
    mid.insert(len(mid) // 2, pad(True))
    return [Case(name + "/order", [rows], **kw), Case(name + "/reversed", [[r.copy() for r in rows[::-1]]], **kw), Case(name + "/shuffled", [sh], **kw),
            Case(name + "/split", [sh2[:a] + [pad(), pad(True)], [], [pad()] + mid + [pad()] * 3, sh2[b:]], **kw)]


def _prof(names, prefix, k=0):
    return [i for i, n in enumerate(names) if n.startswith(prefix)][k]


def _golden():
    rs = reads("one")
    names = profile_names("mini")
    out = []
    for ci, c in enumerate(json.load(open(os.path.join(GOLD, "itsposition_cases.json")))):
        order = {}
        rows = []
        for ln in c["domtbl"].split("\n"):
            if not ln or ln.startswith("#"):
                continue
            ll = ln.split()
            pre = ll[3][:2]
            seen = order.setdefault(pre, [])
            if ll[3] not in seen:
                seen.append(ll[3])
            rep = int(ll[0][1:])
            assert int(ll[2]) == rs.ulen[rep]
            rows.append(Row(rep, _prof(names, pre, seen.index(ll[3])), int(ll[2]), int(ll[19]), int(ll[20]), dom_idx=int(ll[9]) - 1, ndom=int(ll[10]),
                            bitscore=float(ll[13])))
        exp = {}
        for t, p in c["positions"].items():
            exp[int(t[1:])] = (-1, -1, -1, 0) if p == "KeyError" else tuple(-1 if v is None else int(v) for v in p) + (1,)
        rng = random.Random(1000 + ci)
        rng.shuffle(rows)
        out.append(Case("golden%02d" % ci, [rows], regions=(c["region"],), expect={c["region"]: exp}))
    return out


# scores of (the earlier row, the later row) of a pair that ties or nearly ties, and which of the two the reference ends up with
TIES = [("tenth", 34.2, 34.24, 0), ("tenth_swapped", 34.24, 34.2, 0), ("x25_x15", 34.25, 34.15, 0), ("x15_x25", 34.15, 34.25, 0),
        ("x75_x85", 34.75, 34.85, 0), ("x85_x75", 34.85, 34.75, 0), ("neg_zero", -0.04, 0.04, 0), ("zero_neg", 0.04, -0.04, 0),
        ("negative", -12.4, -12.3, 1), ("negative_swapped", -12.3, -12.4, 0), ("negative_tenth", -12.3, -12.34, 0), ("negative_tenth_swapped", -12.34, -12.3, 0),
        ("one_tenth", 34.2, 34.3, 1), ("one_tenth_swapped", 34.3, 34.2, 0), ("edge_lo", -200.0, -199.96, 0), ("edge_hi", 1999.96, 2000.0, 0)]


def _ties():
    """per tie one representative whose two candidate rows are two PROFILES of each side, and one whose candidates are two DOMAINS of
    one pair; left and right alike, for every prefix"""
    rs = reads("one")
    names = profile_names("mini")
    rows, exp = [], {"ITS2": {}, "ALL": {}}
    for k, (_, x, y, w) in enumerate(TIES):
        for how in (0, 1):
            u = 2 * k + how
            L = rs.ulen[u]
            for pre, lo in (("3_", 2), ("4_", 12), ("1_", 1)):
                p0, p1 = _prof(names, pre, 0), _prof(names, pre, 1)
                c0, c1 = (lo + k % 5, lo + 8 + k % 5), (lo + 1 + k % 5, lo + 9 + k % 5)
                if how == 0:
                    rows += [Row(u, p0, L, c0[0], c0[1], bitscore=x), Row(u, p1, L, c1[0], c1[1], bitscore=y)]
                else:
                    rows += [Row(u, p1, L, c0[0], c0[1], dom_idx=0, ndom=2, bitscore=x), Row(u, p1, L, c1[0], c1[1], dom_idx=1, ndom=2, bitscore=y)]
            # what the reference keeps, worked out by hand from TIES: ITS2 = 3_ left / 4_ right, ALL = 1_ left / 4_ right
            win = lambda lo_: ((lo_ + k % 5, lo_ + 8 + k % 5), (lo_ + 1 + k % 5, lo_ + 9 + k % 5))[w]
            exp["ITS2"][u] = (win(2)[1], win(12)[0] - 1, L, 1)
            exp["ALL"][u] = (win(1)[1], win(12)[0] - 1, L, 1)
    assert 2 * len(TIES) <= rs.U
    return _layouts("ties", rows, 7, expect=exp)


def _sides():
    rs = reads("one")
    n = profile_names("mini")
    p3, p4, p1, p2 = _prof(n, "3_"), _prof(n, "4_"), _prof(n, "1_"), _prof(n, "2_")
    L = rs.ulen
    rows = [Row(0, p3, L[0], 20, 64, bitscore=40.1), Row(0, p1, L[0], 3, 30, bitscore=20.0),                       # ITS2: left only
            Row(1, p4, L[1], 200, 240, bitscore=33.0), Row(1, p2, L[1], 100, 140, bitscore=21.0),                # ITS2: right only
            Row(2, p1, L[2], 5, 40, bitscore=50.0), Row(2, p2, L[2], 150, 190, bitscore=50.0),                   # ITS2: neither side: (None, None, None)
            Row(3, p3, L[3], 20, 64, bitscore=90.0, seq_reported=0), Row(3, p4 + 1, L[3], 200, 240, bitscore=90.0, lnP=-0.1),   # nothing reported: KeyError
            Row(4, p3, L[4], 2, 40, bitscore=30.0), Row(4, p4, L[4], 1, 45, bitscore=30.0), Row(4, p2, L[4], 1, 9, bitscore=30.0),   # ienv 1: stop 0
            Row(5, p3, L[5], 260, L[5], bitscore=30.0), Row(5, p1, L[5], 200, L[5], bitscore=30.0), Row(5, p4, L[5], L[5], L[5], bitscore=12.0),   # jenv = tlen
            Row(8, p3, L[8], 1, 1, bitscore=0.0), Row(8, p4, L[8], 64, 64, bitscore=-3.0)]
    exp = {"ITS2": {0: (64, -1, L[0], 1), 1: (-1, 199, L[1], 1), 2: (-1, -1, -1, 1), 3: (-1, -1, -1, 0), 4: (40, 0, L[4], 1), 5: (L[5], L[5] - 1, L[5], 1),
                    6: (-1, -1, -1, 0), 8: (1, 63, L[8], 1)},
           "ITS1": {0: (30, -1, L[0], 1), 1: (-1, 99, L[1], 1), 2: (40, 149, L[2], 1), 3: (-1, -1, -1, 0), 4: (-1, 0, L[4], 1), 5: (L[5], -1, L[5], 1), 8: (-1, -1, -1, 1)},
           "ALL": {0: (30, -1, L[0], 1), 1: (-1, 199, L[1], 1), 2: (40, -1, L[2], 1), 4: (-1, 0, L[4], 1), 5: (L[5], L[5] - 1, L[5], 1)}}
    z = [2] * 10
    z[p4 + 1] = 500                                  # (the second 4_ profile: its one row, P-value 0.9, is not reported)
    return _layouts("sides", rows, 11, domz=z, expect=exp)


def _thresholds():
    rs = reads("one")
    n = profile_names("mini")
    L = rs.ulen
    l0, l1, l2 = _prof(n, "3_", 0), _prof(n, "3_", 1), _prof(n, "3_", 2)
    r0, r1, r2 = _prof(n, "4_", 0), _prof(n, "4_", 1), _prof(n, "4_", 2)
    out = []
    # domE 10: lnP = 0 with Z == domE is reported, with Z == domE + 1 it is not; Z = 0 and Z = 1; an unreported target's tiny P-value;
    # rows 1e-9 (relative) either side of the edge at Z = 37; a better row that is not reported loses to a worse one that is
    z = [1] * 10
    z[l0], z[l1], z[l2], z[r0], z[r1], z[r2] = 10, 11, 0, 1, 37, 37
    e37 = math.log(10.0 / 37.0)
    rows = [Row(0, l0, L[0], 10, 50, bitscore=20.0, lnP=0.0), Row(0, l1, L[0], 12, 55, bitscore=90.0, lnP=0.0),
            Row(1, l1, L[1], 12, 55, bitscore=90.0, lnP=0.0), Row(1, l2, L[1], 14, 58, bitscore=10.0, lnP=0.0), Row(1, r0, L[1], 200, 240, bitscore=5.0, lnP=0.0),
            Row(2, l0, L[2], 10, 50, bitscore=500.0, lnP=-700.0, seq_reported=0), Row(2, l1, L[2], 11, 51, bitscore=15.0, lnP=-3.0),
            Row(3, r1, L[3], 200, 240, bitscore=70.0, lnP=e37 + 1e-9), Row(3, r2, L[3], 210, 250, bitscore=30.0, lnP=e37 - 1e-9),
            Row(4, r1, L[4], 200, 240, bitscore=30.0, lnP=e37 - 1e-9), Row(4, r2, L[4], 210, 250, bitscore=70.0, lnP=e37 + 1e-9),
            Row(5, r1, L[5], 200, 240, dom_idx=0, ndom=2, bitscore=70.0, lnP=-0.5), Row(5, r1, L[5], 100, 140, dom_idx=1, ndom=2, bitscore=12.5, lnP=-9.0),
            Row(6, l2, L[6], 1, 20, bitscore=-5.0, lnP=0.0, seq_reported=0)]
    exp = {"ITS2": {0: (50, -1, L[0], 1), 1: (58, 199, L[1], 1), 2: (51, -1, L[2], 1), 3: (-1, 209, L[3], 1), 4: (-1, 199, L[4], 1), 5: (-1, 99, L[5], 1),
                    6: (-1, -1, -1, 0), 7: (-1, -1, -1, 0)}}
    out += _layouts("thresholds_domE10", rows, 13, domz=z, domE=10.0, expect=exp)
    # domE 1e-2 at Z = 5 and Z = 1
    z = [1] * 10
    z[l0], z[r0] = 5, 1
    e5, e1 = math.log(1e-2 / 5.0), math.log(1e-2)
    rows = [Row(0, l0, L[0], 10, 50, bitscore=80.0, lnP=e5 + 1e-9), Row(0, l0, L[0], 60, 90, dom_idx=1, ndom=2, bitscore=8.0, lnP=e5 - 1e-9),
            Row(0, r0, L[0], 200, 240, bitscore=80.0, lnP=e1 + 1e-9), Row(0, r0, L[0], 250, 280, dom_idx=1, ndom=2, bitscore=8.0, lnP=e1 - 1e-9),
            Row(1, l0, L[1], 10, 50, bitscore=80.0, lnP=e5 + 1e-9), Row(1, r0, L[1], 200, 240, bitscore=80.0, lnP=e1 + 1e-9)]
    exp = {"ITS2": {0: (90, 249, L[0], 1), 1: (-1, -1, -1, 0)}}
    out += _layouts("thresholds_domE0.01", rows, 17, domz=z, domE=1e-2, expect=exp)
    # two samples whose counters differ for the same profile: the same row is reported in one and not in the other
    two = reads("two")
    U1 = two.U // 2
    assert two.usample[:U1] == [0] * U1 and two.usample[U1:] == [1] * U1 and two.ulen[:U1] == two.ulen[U1:]
    z = [1] * 20
    z[l0], z[10 + l0], z[r0], z[10 + r0] = 3, 300, 300, 3
    rows = []
    for u in (0, 1, U1, U1 + 1):
        rows += [Row(u, l0, L[u % U1], 10, 50, bitscore=60.0, lnP=-2.0), Row(u, l1, L[u % U1], 12, 52, bitscore=20.0, lnP=-40.0),
                 Row(u, r0, L[u % U1], 200, 240, bitscore=60.0, lnP=-2.0), Row(u, r1, L[u % U1], 220, 260, bitscore=20.0, lnP=-40.0)]
    exp = {"ITS2": {0: (50, 219, L[0], 1), 1: (50, 219, L[1], 1), U1: (52, 199, L[0], 1), U1 + 1: (52, 199, L[1], 1), 2: (-1, -1, -1, 0)}}
    out += _layouts("two_samples", rows, 19, domz=z, reads="two", expect=exp)
    return out


def _random_rows(rng, rs, P, pairs, maxdom=3, reps=None):
    rows = []
    seen = set()
    while len(seen) < pairs:
        u = rng.choice(reps) if reps else rng.randrange(rs.U)
        p = rng.randrange(P)
        if (u, p) in seen:
            continue
        seen.add((u, p))
        nd = rng.randint(1, maxdom)
        for d in range(nd):
            i = rng.randint(1, rs.ulen[u])
            j = rng.randint(i, rs.ulen[u])
            sc = rng.randint(-1990, 19990) / 10.0 + rng.choice([0.0, 0.0, 0.04, -0.04, 0.05, -0.05, 0.03])
            rows.append(Row(u, p, rs.ulen[u], i, j, dom_idx=d, ndom=nd, flags=rng.choice([0, 0, 0, 1, 2, 3]), bitscore=sc,
                            lnP=rng.choice([-rng.uniform(0.1, 120.0), -rng.uniform(0.1, 6.0)]), seq_reported=int(rng.random() < 0.9)))
    return rows


def _shapes():
    out = []
    rs = reads("one")
    for n in (1, 255, 256, 257):
        rng = random.Random(100 + n)
        rows = _random_rows(rng, rs, 10, n, maxdom=1)
        rng.shuffle(rows)
        z = [rng.choice([1, 2, 40, 5000]) for _ in range(10)]
        out.append(Case("shape%d" % n, [rows], domz=z))
    # 256 rows and padding up to the next block; padding between the rows too
    rng = random.Random(301)
    rows = _random_rows(rng, rs, 10, 256, maxdom=1)
    for k in (200, 130, 64, 63, 0):
        rows.insert(k, pad(k % 2 == 0))
    out.append(Case("shape256_padded", [rows + [pad()] * 59], domz=[7] * 10))
    # one representative owns every row
    rng = random.Random(302)
    rows = []
    for p in range(10):
        for d in range(30):
            rows.append(Row(7, p, rs.ulen[7], 1 + d, 30 + d, dom_idx=d, ndom=30, bitscore=rng.randint(100, 130) / 10.0, lnP=-rng.uniform(1.0, 30.0), flags=rng.choice([0, 1])))
    rng.shuffle(rows)
    out.append(Case("one_representative", [rows[:100], rows[100:]], domz=[50] * 10))
    # about 3 000 rows over many profiles of each prefix, in segments whose profiles' blocks are padded to 64 rows as a search pads them
    rng = random.Random(303)
    P = len(profile_names("wide"))
    rows = _random_rows(rng, rs, P, 1500, maxdom=3)
    segs = []
    for lo, hi in ((0, rs.U // 2), (rs.U // 2, rs.U)):
        seg = []
        for p in range(P):
            blk = [r for r in rows if r.prof == p and lo <= r.rep < hi]
            rng.shuffle(blk)
            seg += blk + [pad(len(seg) % 3 == 0)] * (-len(blk) % 64)
        segs.append(seg)
    out.append(Case("wide3000", segs, domz=[rng.choice([1, 3, 90, 20000]) for _ in range(P)], hmm="wide"))
    return out


def _compaction():
    """lnP -50: certain under the default assumptions and the tightened ones; -10: under the tightened ones only; -2: under neither"""
    rs = reads("one")
    n = profile_names("mini")
    L = rs.ulen
    l0, l1, l2, r0, r1, r2 = _prof(n, "3_", 0), _prof(n, "3_", 1), _prof(n, "3_", 2), _prof(n, "4_", 0), _prof(n, "4_", 1), _prof(n, "4_", 2)
    seg0, seg1 = [], []
    for u, lnc, lnu in ((0, -50.0, -2.0), (1, -50.0, -10.0), (2, -10.0, -2.0)):
        Lu = L[u]
        seg0 += [Row(u, l0, Lu, 10, 50, bitscore=30.0, lnP=lnc),            # the certain row
                 Row(u, l1, Lu, 11, 51, bitscore=30.04, lnP=lnu),           # equal in tenths, later: cannot win
                 Row(u, l2, Lu, 12, 52, bitscore=35.0, lnP=lnu),            # above: stays
                 Row(u, l2, Lu, 13, 53, dom_idx=1, ndom=2, bitscore=25.0, lnP=lnu),      # below: goes
                 Row(u, r1, Lu, 200, 240, bitscore=30.0, lnP=lnc), Row(u, r0, Lu, 190, 230, bitscore=30.0, lnP=lnu),   # equal in tenths, EARLIER: stays
                 Row(u, r1, Lu, 100, 140, dom_idx=1, ndom=2, bitscore=3.0, lnP=lnu, flags=2),                          # region cap: stays
                 Row(u, r2, Lu, 90, 130, bitscore=99.0, lnP=lnc, flags=2, seq_reported=0)]          # unreported target: goes
    for u, lnc, lnu in ((3, -50.0, -2.0), (4, -50.0, -10.0)):
        Lu = L[u]
        # the uncertain rows lie in the segment BEFORE their certain row (kept: nothing is known yet) and in the one after it
        seg0 += [Row(u, l1, Lu, 11, 51, bitscore=25.0, lnP=lnu), Row(u, r0, Lu, 190, 230, bitscore=29.9, lnP=lnu)]
        seg1 += [Row(u, l0, Lu, 10, 50, bitscore=30.0, lnP=lnc), Row(u, l2, Lu, 12, 52, bitscore=25.0, lnP=lnu), Row(u, l2, Lu, 13, 53, dom_idx=1, ndom=2, bitscore=30.1, lnP=lnu),
                 Row(u, r1, Lu, 200, 240, bitscore=30.0, lnP=lnc), Row(u, r1, Lu, 201, 241, dom_idx=1, ndom=2, bitscore=30.0, lnP=lnc)]
    seg1 += [Row(5, l0, L[5], 10, 50, bitscore=12.0, lnP=-2.0), Row(5, r0, L[5], 200, 240, bitscore=12.0, lnP=-10.0, flags=1)]      # no certain row at all
    rng = random.Random(23)
    rng.shuffle(seg0)
    rng.shuffle(seg1)
    tight = {"ITSX_COMPACT_ZMAX": "100", "ITSX_COMPACT_DOME_MIN": "1"}
    return [Case("compaction", [seg0 + [pad(True)], [pad()] + seg1], domz=[60] * 10),
            Case("compaction_refused_domE", [seg0, seg1], domz=[60] * 10, domE=1e-3, compact_refused=dict(env={})),
            Case("compaction_refused_domZ", [seg0, seg1], domz=[60] * 4 + [101] + [60] * 5, compact_refused=dict(env=tight)),
            Case("compaction_refused_domE_tight", [seg0, seg1], domz=[60] * 10, domE=0.5, compact_refused=dict(env=tight))]


COMPACT_ENVS = [{}, {"ITSX_COMPACT_ZMAX": "100", "ITSX_COMPACT_DOME_MIN": "1"}]


def compact_assumptions(env):
    return float(env.get("ITSX_COMPACT_ZMAX", 1e9)), float(env.get("ITSX_COMPACT_DOME_MIN", 1e-2))


def compact_combos(case, env):
    """the (counters, domE) a compacted table is finalized with: the case's own where they lie inside the assumptions, all ones at
    domE 10, and the assumptions' own limits"""
    zmax, dmin = compact_assumptions(env)
    out = [([1] * len(case.domz), 10.0), ([int(zmax)] * len(case.domz), dmin), ([min(z, int(zmax)) for z in case.domz], max(case.domE, dmin))]
    if max(case.domz) <= zmax and case.domE >= dmin:
        out.append((case.domz, case.domE))
    return out


def _lazy():
    """bounds 50 .. 5000 at domE 10: lnP -50 is reported under both (verdict 1), -3 under the lower one only (2), -0.5 under neither (0)"""
    rs = reads("one")
    n = profile_names("mini")
    L = rs.ulen
    l0, l1, l2, r0, r1 = _prof(n, "3_", 0), _prof(n, "3_", 1), _prof(n, "3_", 2), _prof(n, "4_", 0), _prof(n, "4_", 1)
    S, Un, No = -50.0, -3.0, -0.5
    base = [Row(9, l0, L[9], 10, 50, bitscore=30.0, lnP=S), Row(9, r0, L[9], 200, 240, bitscore=30.0, lnP=S), Row(9, l1, L[9], 1, 9, bitscore=99.0, lnP=No),
            Row(10, l0, L[10], 5, 40, bitscore=30.0, lnP=S), Row(10, l0, L[10], 5, 40, bitscore=30.0, lnP=S),                     # a row evaluated twice
            Row(10, r1, L[10], 50, 90, dom_idx=1, ndom=2, bitscore=44.4, lnP=S, flags=1), Row(10, r1, L[10], 50, 90, dom_idx=1, ndom=2, bitscore=44.4, lnP=S, flags=1)]
    quiet = [Row(1, l0, L[1], 10, 50, bitscore=30.0, lnP=S), Row(1, l1, L[1], 11, 51, bitscore=30.04, lnP=Un),                      # equal in tenths but later
             Row(2, l0, L[2], 10, 50, bitscore=30.0, lnP=S), Row(2, l2, L[2], 12, 52, bitscore=25.0, lnP=Un), Row(2, l2, L[2], 12, 52, bitscore=25.0, lnP=Un)]   # below (twice)
    loud = [Row(0, l0, L[0], 10, 50, bitscore=30.0, lnP=S), Row(0, l1, L[0], 11, 51, bitscore=35.0, lnP=Un),                       # above its group's sure row
            Row(3, l0, L[3], 10, 50, bitscore=20.0, lnP=Un), Row(3, r0, L[3], 200, 240, bitscore=20.0, lnP=No),                     # a sequence with no sure row
            Row(4, l0, L[4], 10, 50, bitscore=30.0, lnP=S), Row(4, r0, L[4], 200, 240, bitscore=2.0, lnP=Un),                       # a class with none
            Row(5, l1, L[5], 10, 50, bitscore=30.0, lnP=S), Row(5, l0, L[5], 11, 51, bitscore=30.0, lnP=Un),                        # equal in tenths, earlier
            Row(11, r0, L[11], 100, 150, bitscore=30.0, lnP=S), Row(11, r1, L[11], 90, 140, bitscore=30.1, lnP=Un), Row(11, r1, L[11], 90, 140, bitscore=30.1, lnP=Un)]   # above, twice
    lb, ub = [50] * 10, [5000] * 10
    out = []
    rng = random.Random(29)
    for name, rows, b in (("lazy_pending", base + quiet + loud, dict(lb=lb, ub=ub)), ("lazy_quiet", base + quiet, dict(lb=lb, ub=ub)),
                          ("lazy_exact", base + quiet + loud, dict(lb=[50] * 10, ub=[50] * 10)), ("lazy_exact_high", base + quiet + loud, dict(lb=ub, ub=ub)),
                          ("lazy_zero_bounds", base + quiet + loud, dict(lb=[0] * 10, ub=[0] * 10))):
        rows = [r.copy() for r in rows]
        rng.shuffle(rows)
        a = len(rows) // 2
        out.append(Case(name, [rows[:a] + [pad(True)], [], [pad()] + rows[a:]], domz=b["lb"], lazy=b))
    return out


_CASES = None


def catalogue():
    global _CASES
    if _CASES is None:
        _CASES = _golden() + _ties() + _sides() + _thresholds() + _shapes() + _compaction() + _lazy()
        assert len(set(c.name for c in _CASES)) == len(_CASES)
    return _CASES


def full_cases():
    """the cases whose tables name every (profile, target, domain) once: what a full or a compacted search can hold"""
    return [c for c in catalogue() if c.lazy is None]


def lazy_bounds(case):
    """the bounds a case is finalized with in lazy mode: its own, or its exact counters as both bounds"""
    return (case.lazy["lb"], case.lazy["ub"]) if case.lazy else (case.domz, case.domz)


def threshold_checks():
    """every (case name, row, counter, domE) some test compares with a threshold: full mode, the compaction's combinations, both lazy bounds"""
    for c in catalogue():
        us = c.usample()
        combos = [(c.domz, c.domE)]
        if c.lazy is None:
            for env in COMPACT_ENVS:
                combos += compact_combos(c, env)
        lb, ub = lazy_bounds(c)
        combos += [([max(z, 1) for z in lb], c.domE), ([max(z, 1) for z in ub], c.domE)]
        for z, e in combos:
            for r in c.rows:
                if not r.is_padding():
                    yield c.name, r, X.counter(r, z, us, c.P), e
