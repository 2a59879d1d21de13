"""An exact model of the last step of the search: which domain rows are reported, and which row of a target ItsPosition ends up with.

Written from the reference's behaviour alone -- ItsPosition._score / parse / get_position (itsxpress/SeqSample.py:400-498) and hmmsearch's
reporting rule for domains (a domain of a reported target is listed iff its conditional E-value P-value x domZ is at most domE) -- in
plain Python: no oracle, no mirror class, none of the engine's ranking keys.  Everything here is exact:

  reporting   exp(lnP) x Z <= domE with `decimal` at 60 digits, Z the counter of the row's (sample, profile);
  score       ItsPosition compares float(column 14), i.e. what %.1f printed: Decimal(float32 score) quantised to one place, half-even
              (the binary value is exact in Decimal, so this is what a correctly rounding printf prints); -0.0 == 0.0;
  argmax      rows are walked in table order (profile index, then target, then domain index); per target and side the FIRST row with a
              strictly greater printed score stays; the left prefix is tested first;
  positions   start = left.to_pos, stop = right.from_pos - 1, tlen as the table's column 3; None -> -1; KeyError -> in_ddict 0.

On top of that, the engine's two thinned row modes are stated in the same terms: the kept set of a compacted segment (rows that can
still end up as an argmax whatever domZ in [1, zmax] and domE >= dome_min turn out to be), and the lazy stage's three-valued verdict,
the undecided rows that matter, and the winners table.

A row is a Row below; a table is a list of them in any physical order.
"""
import decimal
import functools
import math
import struct
from decimal import Decimal

CTX = decimal.Context(prec=60, rounding=decimal.ROUND_HALF_EVEN, Emin=-999999999, Emax=999999999)
REGIONS = {"ITS2": ("3_", "4_"), "ITS1": ("1_", "2_"), "ALL": ("1_", "4_")}


def f32(x):
    """the float32 nearest to x, as a Python float"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


class Row(object):
    __slots__ = ("rep", "prof", "tlen", "ienv", "jenv", "dom_idx", "ndom", "flags", "bitscore", "lnP", "seq_reported")

    def __init__(self, rep, prof, tlen, ienv, jenv, dom_idx=0, ndom=1, flags=0, bitscore=0.0, lnP=-50.0, seq_reported=1):
        self.rep, self.prof, self.tlen, self.ienv, self.jenv = int(rep), int(prof), int(tlen), int(ienv), int(jenv)
        self.dom_idx, self.ndom, self.flags = int(dom_idx), int(ndom), int(flags)
        self.bitscore, self.lnP, self.seq_reported = f32(bitscore), float(lnP), int(seq_reported)

    def is_padding(self):
        return self.dom_idx < 0

    def ident(self):
        return (self.prof, self.rep, self.dom_idx)

    def copy(self):
        return Row(self.rep, self.prof, self.tlen, self.ienv, self.jenv, self.dom_idx, self.ndom, self.flags, self.bitscore, self.lnP, self.seq_reported)

    def __repr__(self):
        return "Row(rep=%d prof=%d dom=%d %r lnP=%r seq=%d env=%d..%d flags=%d)" % (self.rep, self.prof, self.dom_idx, self.bitscore, self.lnP,
                                                                                   self.seq_reported, self.ienv, self.jenv, self.flags)


# ---------------------------------------------------------------- reporting
@functools.lru_cache(maxsize=None)
def pvalue(lnP):
    return CTX.exp(Decimal(lnP))


def evalue_ratio(lnP, Z, domE):
    """exp(lnP) x Z / domE, exactly enough to tell its distance from 1 (None where Z is 0: the product is 0)"""
    if Z == 0:
        return None
    return CTX.divide(CTX.multiply(pvalue(lnP), Decimal(Z)), Decimal(domE))


def reported(row, Z, domE):
    """hmmsearch lists a domain iff its target is reported and P-value x domZ <= domE"""
    if row.is_padding() or not row.seq_reported:
        return False
    return CTX.multiply(pvalue(row.lnP), Decimal(Z)) <= Decimal(domE)


def counter(row, domz, usample, P):
    if usample is None:
        return domz[row.prof]
    return domz[usample[row.rep] * P + row.prof]


def reported_flags(rows, domz, domE, usample=None, P=None):
    """per row 0 / 1 (padding rows: None)"""
    return [None if r.is_padding() else int(reported(r, counter(r, domz, usample, P), domE)) for r in rows]


def lazy_verdict(row, lb, ub, domE):
    """1 reported under the upper bound (so under every count), 2 reported under the lower bound only, 0 never.  The row's own target is
    reported, so the count is at least 1 whatever the bounds say."""
    if reported(row, max(ub, 1), domE):
        return 1
    if reported(row, max(lb, 1), domE):
        return 2
    return 0


def lazy_verdicts(rows, lb, ub, domE, usample=None, P=None):
    return [None if r.is_padding() else lazy_verdict(r, counter(r, lb, usample, P), counter(r, ub, usample, P), domE) for r in rows]


# ---------------------------------------------------------------- printed score
def printed(bitscore):
    """the text %.1f prints for a float32 score"""
    q = Decimal(f32(bitscore)).quantize(Decimal("0.1"), rounding=decimal.ROUND_HALF_EVEN)
    return format(q, "f")


def tenths(bitscore):
    """the printed score in tenths, as an integer (-0.0 is 0)"""
    return int(Decimal(printed(bitscore)) * 10)


# ---------------------------------------------------------------- the table and ItsPosition
def table_order(rows, keep=None):
    """indices of the rows hmmsearch would list, in --domtblout order: profile (file order), then target, then domain; a row evaluated
    twice stays twice, next to itself"""
    idx = [i for i, r in enumerate(rows) if not r.is_padding() and (keep is None or keep[i])]
    return sorted(idx, key=lambda i: rows[i].ident())


def parse_domtbl(text):
    """the fields ItsPosition.parse reads from each line that is no comment"""
    out = []
    for line in text.split("\n"):
        if not line or line.startswith("#"):
            continue
        ll = line.split()
        out.append(dict(target=ll[0], tlen=int(ll[2]), profile=ll[3], score=float(ll[13]), from_pos=int(ll[19]), to_pos=int(ll[20])))
    return out


def lines_of_rows(rows, flags, names, target_name=lambda u: u):
    """the same fields for the reported rows of a table, as its domtbl.txt would hold them"""
    return [dict(target=target_name(rows[i].rep), tlen=rows[i].tlen, profile=names[rows[i].prof], score=float(printed(rows[i].bitscore)),
                 from_pos=rows[i].ienv, to_pos=rows[i].jenv, row=i) for i in table_order(rows, [bool(f) for f in flags])]


def walk(lines, left, right):
    """ItsPosition.parse + _score over parsed lines.  Returns (ddict, winners): ddict as the reference builds it, winners[(target, side)]
    = index into `lines` of the row that side ended up with."""
    dd, win = {}, {}
    for k, ln in enumerate(lines):
        t = ln["target"]
        if t not in dd:
            dd[t] = {}
        if ln["profile"].startswith(left):
            side = "left"
        elif ln["profile"].startswith(right):
            side = "right"
        else:
            continue
        if side in dd[t]:
            if ln["score"] > dd[t][side]["score"]:
                dd[t][side] = dict(score=ln["score"], to_pos=ln["to_pos"], from_pos=ln["from_pos"])
                win[(t, side)] = k
        else:
            dd[t][side] = dict(score=ln["score"], to_pos=ln["to_pos"], from_pos=ln["from_pos"])
            dd[t]["tlen"] = ln["tlen"]
            win[(t, side)] = k
    return dd, win


def get_position(dd, target):
    """ItsPosition.get_position: (start, stop, tlen) with None, or KeyError"""
    e = dd[target]
    start = int(e["left"]["to_pos"]) if "left" in e else None
    stop = int(e["right"]["from_pos"]) - 1 if "right" in e else None
    tlen = int(e["tlen"]) if "tlen" in e else None
    return (start, stop, tlen)


def coords4(dd, target):
    """the engine's row for a target: (start, stop, tlen, in_ddict), None -> -1, KeyError -> (-1, -1, -1, 0)"""
    try:
        p = get_position(dd, target)
    except KeyError:
        return (-1, -1, -1, 0)
    return tuple(-1 if v is None else v for v in p) + (1,)


class Result(object):
    """what the coordinates calls must return for a finalized table"""
    pass


def positions(rows, flags, names, left, right, U, uniq_of=None):
    """rep rows [U][4], read rows [n][4] (None without uniq_of), the four parity-risk counters, the ddict and the winning rows"""
    lines = lines_of_rows(rows, flags, names)
    dd, win = walk(lines, left, right)
    res = Result()
    res.ddict, res.lines = dd, lines
    res.winners = {k: lines[v]["row"] for k, v in win.items()}
    res.rep = [coords4(dd, u) for u in range(U)]
    res.read = None if uniq_of is None else [res.rep[u] if u >= 0 else (-1, -1, -1, 0) for u in uniq_of]
    # parity-risk counters: representatives whose winning left / right row came out of a clustered region (flags bit 0), and
    # representatives with a reported row of either side whose pair hit the region cap (bit 1); then the same over their reads
    multi = set(t for (t, _), i in res.winners.items() if rows[i].flags & 1)
    cap = set(ln["target"] for ln in lines if (ln["profile"].startswith(left) or ln["profile"].startswith(right)) and rows[ln["row"]].flags & 2)
    reads = [] if uniq_of is None else list(uniq_of)
    res.counters = dict(n_uniq_multi_winner=len(multi), n_reads_multi_winner=sum(1 for u in reads if u in multi),
                        n_uniq_region_cap=len(cap), n_reads_region_cap=sum(1 for u in reads if u in cap))
    return res


# ---------------------------------------------------------------- compaction
def cls_of(name):
    """the compaction's classes: 2-character name prefixes"""
    return name[:2]


def order_key(row):
    """a > b  <=>  among two reported rows of one target and side the walk ends up with a: the greater printed score, else the earlier
    profile, else the earlier domain"""
    return (tenths(row.bitscore), -row.prof, -row.dom_idx)


def certain_lnp(zmax, dome_min):
    return math.log(dome_min / zmax) - 1e-6


def compact_kept(segments, names, zmax=1e9, dome_min=1e-2):
    """per segment the indices (into the segment) of the rows a compacted search keeps, in row order.  A row is CERTAIN when its target
    is reported and lnP <= log(dome_min / zmax) - 1e-6; per (target, class) nothing below the best certain row seen so far (this segment
    and the ones before it) can end up as the argmax.  Kept: the best certain row itself, every uncertain row above it, and every row
    of a pair at the region cap (flags bit 1) of a reported target."""
    lim = certain_lnp(zmax, dome_min)
    best = {}
    out = []
    for seg in segments:
        for r in seg:
            if r.is_padding() or not r.seq_reported or not (r.lnP <= lim):
                continue
            g = (r.rep, cls_of(names[r.prof]))
            if g not in best or order_key(r) > best[g]:
                best[g] = order_key(r)
        keep = []
        for i, r in enumerate(seg):
            if r.is_padding() or not r.seq_reported:
                continue
            b = best.get((r.rep, cls_of(names[r.prof])))
            k = order_key(r)
            if ((k == b) if r.lnP <= lim else (b is None or k > b)) or (r.flags & 2):
                keep.append(i)
        out.append(keep)
    return out


def winners_table(rows, flags, names):
    """the kept-rows table of a thinned search: per target and 2-character prefix the reported row a walk in table order ends up with
    (the first with a strictly greater printed score); indices into rows, in table order, a row evaluated twice named once"""
    best = {}
    for i in table_order(rows, [bool(f) for f in flags]):
        g = (rows[i].rep, cls_of(names[rows[i].prof]))
        if g not in best or tenths(rows[i].bitscore) > tenths(rows[best[g]].bitscore):
            best[g] = i
    return sorted(best.values(), key=lambda i: rows[i].ident())


# ---------------------------------------------------------------- lazy
class Lazy(object):
    pass


def lazy_model(rows, names, lb, ub, domE, usample=None, P=None):
    """verdicts; the undecided rows that matter (count, profile flags, representative flags); the winners table (indices into rows, table
    order, a row evaluated twice named once) -- served only when nothing is pending"""
    res = Lazy()
    res.verdict = lazy_verdicts(rows, lb, ub, domE, usample, P)
    sure, has = {}, set()
    for r, v in zip(rows, res.verdict):
        if v == 1:
            has.add(r.rep)
            g = (r.rep, cls_of(names[r.prof]))
            if g not in sure or order_key(r) > sure[g]:
                sure[g] = order_key(r)
    res.pending_rows = []
    for i, (r, v) in enumerate(zip(rows, res.verdict)):
        if v != 2:
            continue
        b = sure.get((r.rep, cls_of(names[r.prof])))
        # it could take the place of its group's sure row, or give a target without any sure row its first row
        if r.rep not in has or b is None or order_key(r) > b:
            res.pending_rows.append(i)
    res.pending = len(res.pending_rows)
    res.prof_flags = sorted(set(rows[i].prof for i in res.pending_rows))
    res.uniq_flags = sorted(set(rows[i].rep for i in res.pending_rows))
    res.winners = winners_table(rows, [v == 1 for v in res.verdict], names)
    res.sure_flags = [None if v is None else int(v == 1) for v in res.verdict]
    return res
