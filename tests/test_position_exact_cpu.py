"""The exact model of domain reporting and ItsPosition's argmax (tests/position_exact.py) against the reference's recorded behaviour, and
the catalogue of tests/position_cases.py against the model -- everything that needs no GPU: the 36 golden cases, the domtbl formatter's
%.1f against the model's tenths, invariance under the rows' physical order, and the margin that keeps det_exp's last bit out of every
threshold the GPU tests compare."""
import json
import os
import random
import re
from decimal import Decimal

import numpy as np
import pytest

import position_cases as PC
import position_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PC.catalogue()


def _positions(case, region, flags=None):
    rs = PC.reads(case.reads)
    rows = case.rows
    if flags is None:
        flags = X.reported_flags(rows, case.domz, case.domE, case.usample(), case.P)
    left, right = X.REGIONS[region]
    return X.positions(rows, flags, case.names, left, right, rs.U, rs.uniq_of)


def test_model_reproduces_the_golden_cases(gold):
    """the model's own parser and walk over the recorded domtbl text: every ddict and every position the reference class gave"""
    cases = json.load(open(os.path.join(gold, "itsposition_cases.json")))
    assert len(cases) == 36
    for c in cases:
        left, right = X.REGIONS[c["region"]]
        dd, _ = X.walk(X.parse_domtbl(c["domtbl"]), left, right)
        assert dd == c["ddict"]
        for sq, exp in c["positions"].items():
            if exp == "KeyError":
                with pytest.raises(KeyError):
                    X.get_position(dd, sq)
            else:
                assert list(X.get_position(dd, sq)) == exp


def test_printed_score_is_what_printf_prints():
    rng = random.Random(5)
    xs = [34.25, 34.15, 34.75, 34.85, -0.04, 0.04, 0.05, -0.05, 0.25, 0.35, -12.34, 1999.96, -199.96, 0.0, -0.0]
    xs += [rng.randint(-20000, 200000) / 100.0 for _ in range(3000)] + [rng.uniform(-200, 2000) for _ in range(3000)]
    for x in xs:
        assert X.printed(x) == "%.1f" % X.f32(x), x
    assert X.printed(34.25) == "34.2" and X.printed(34.15) == "34.2" and X.printed(34.75) == "34.8" and X.printed(34.85) == "34.8"
    assert X.printed(-0.04) == "-0.0" and X.tenths(-0.04) == 0 == X.tenths(0.04) and float(X.printed(-0.04)) == float(X.printed(0.04))


@pytest.mark.parametrize("case", [c for c in CASES if c.expect], ids=lambda c: c.name)
def test_model_gives_the_recorded_or_hand_worked_positions(case):
    """golden tables turned into rows (shuffled): the file's own positions; the hand-made edge tables: the positions worked out by hand
    from the reference's code"""
    for region, exp in case.expect.items():
        res = _positions(case, region)
        for rep, want in exp.items():
            assert res.rep[rep] == want, (region, rep)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_formatter_text_parses_to_the_models_dictionary(case, tmp_path):
    """rows -> itsx_write_domtbl_arrays -> text -> the model's parser and the mirror class: the model's ddict.  Holds the formatter's
    %.1f to the model's tenths, and the model's table order to the file's."""
    from itsxpress_amd import ItsPosition, _lib
    L = _lib.lib()
    rs = PC.reads(case.reads)
    rows = case.rows
    if case.lazy:
        flags = X.lazy_model(rows, case.names, case.lazy["lb"], case.lazy["ub"], case.domE).sure_flags
    else:
        flags = X.reported_flags(rows, case.domz, case.domE, case.usample(), case.P)
    arr = PC.to_array(rows, flags)
    tn = ["t%d" % u for u in range(rs.U)]
    blob = lambda xs: ("".join(xs).encode(), np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64))
    pn, po = blob(case.names)
    tb, to = blob(tn)
    M = np.full(case.P, 45, np.int32)
    tau = np.full(case.P, -3.5, np.float32)
    lam = np.full(case.P, 0.7, np.float32)
    domz = np.array(case.domz[:case.P], np.int64)
    path = tmp_path / "domtbl.txt"
    rc = L.itsx_write_domtbl_arrays(os.fsencode(path), arr.ctypes.data, len(arr), rs.U, domz.ctypes.data, case.P, pn, po.ctypes.data,
                                    M.ctypes.data, tau.ctypes.data, lam.ctypes.data, tb, to.ctypes.data)
    assert rc == 0, L.itsx_writers_last_error()
    text = path.read_text()
    lines = X.parse_domtbl(text)
    want = X.lines_of_rows(rows, flags, case.names, target_name=lambda u: "t%d" % u)
    if case.lazy:           # a row evaluated twice is written twice by this writer; the parser's dictionary does not change
        assert len(lines) == len(want)
    for a, b in zip(lines, want):
        assert all(a[k] == b[k] for k in a), (a, b)
    assert len(lines) == len(want)
    for region, (left, right) in X.REGIONS.items():
        dd, _ = X.walk(lines, left, right)
        assert dd == X.walk(want, left, right)[0]
        assert ItsPosition(str(path), region).ddict == dd
        res = _positions(case, region, flags)
        for u in range(rs.U):
            assert res.rep[u] == X.coords4(dd, "t%d" % u)


@pytest.mark.parametrize("case", [c for c in CASES if not c.name.startswith("golden")], ids=lambda c: c.name)
def test_winners_do_not_depend_on_the_physical_order(case):
    rng = random.Random(hash(case.name) & 0xFFFF)
    rows = case.rows
    sh = [r.copy() for r in rows]
    rng.shuffle(sh)
    us = case.usample()
    for region, (left, right) in X.REGIONS.items():
        rs = PC.reads(case.reads)
        a = X.positions(rows, X.reported_flags(rows, case.domz, case.domE, us, case.P), case.names, left, right, rs.U, rs.uniq_of)
        b = X.positions(sh, X.reported_flags(sh, case.domz, case.domE, us, case.P), case.names, left, right, rs.U, rs.uniq_of)
        assert a.rep == b.rep and a.read == b.read and a.counters == b.counters and a.ddict == b.ddict
        assert {k: rows[i].ident() for k, i in a.winners.items()} == {k: sh[i].ident() for k, i in b.winners.items()}


def test_layouts_of_one_table_agree():
    """/order, /reversed, /shuffled and /split of a table hold the same rows: the same results"""
    groups = {}
    for c in CASES:
        if "/" in c.name:
            groups.setdefault(c.name.split("/")[0], []).append(c)
    assert len(groups) >= 5
    for name, cs in groups.items():
        assert len(cs) == 4
        ref = [_positions(cs[0], r).rep for r in cs[0].regions]
        for c in cs[1:]:
            assert sorted(r.ident() for r in c.rows if not r.is_padding()) == sorted(r.ident() for r in cs[0].rows)
            assert [_positions(c, r).rep for r in c.regions] == ref, c.name


def test_no_threshold_lies_within_det_exps_last_bit():
    """exp(lnP) x Z against domE is decided in double precision on the device, with an exp that is good to a bit or so: the catalogue
    holds no comparison nearer than 2^-40 (relative) to equality other than the exact ones, lnP = 0 with Z = domE."""
    margin = Decimal(2) ** -40
    n = exact = 0
    nearest = None
    for name, r, Z, domE in PC.threshold_checks():
        n += 1
        ratio = X.evalue_ratio(r.lnP, Z, domE)
        if ratio is None:
            continue
        d = abs(ratio - 1)
        if r.lnP == 0.0 and d == 0:
            exact += 1
            continue
        assert d > margin, (name, r, Z, domE)
        nearest = d if nearest is None else min(nearest, d)
    assert n > 50000 and exact >= 4
    assert nearest < Decimal("2e-9")            # the 1e-9 pairs are there


def test_catalogue_reads_and_shapes():
    rs = PC.reads("one")
    assert 30 <= rs.U <= 60 and min(len(s) for s in rs.seqs) == 20 and max(len(s) for s in rs.seqs) == 400
    assert rs.uniq_of.count(-1) == 3 and len(rs.seqs) - rs.uniq_of.count(-1) - rs.U == 6
    two = PC.reads("two")
    assert two.U == 2 * rs.U and two.S == 2
    sizes = sorted(len(c.rows) for c in CASES)
    assert {1, 255, 256, 257} <= set(sizes) and sizes[-1] > 3000
    assert any(not seg for c in CASES for seg in c.segments)
    assert sum(1 for c in CASES if c.name.startswith("golden")) == 36


def test_compaction_model_on_the_hand_made_table():
    case = [c for c in CASES if c.name == "compaction"][0]
    n = case.names
    for env, gone_extra in ((PC.COMPACT_ENVS[0], 0), (PC.COMPACT_ENVS[1], 0)):
        zmax, dmin = PC.compact_assumptions(env)
        kept = X.compact_kept(case.segments, n, zmax, dmin)
        rows = [case.segments[s][i] for s in range(len(case.segments)) for i in kept[s]]
        assert all(not r.is_padding() and r.seq_reported for r in rows)
        # what is kept decides exactly what the whole table decides, for every counter and domE inside the assumptions
        rs = PC.reads(case.reads)
        for z, e in PC.compact_combos(case, env):
            for region, (left, right) in X.REGIONS.items():
                a = X.positions(case.rows, X.reported_flags(case.rows, z, e), n, left, right, rs.U, rs.uniq_of)
                b = X.positions(rows, X.reported_flags(rows, z, e), n, left, right, rs.U, rs.uniq_of)
                assert a.rep == b.rep and a.read == b.read and a.counters == b.counters
    # by hand, default assumptions (certain: lnP -50): per representative 0 / 1 of the first segment the certain left row, the row above
    # it, the certain right row, the equal-but-earlier right row and the region-cap row stay; the later equal, the lower and the
    # unreported target's row go
    kept = X.compact_kept(case.segments, n)
    for u in (0, 1):
        got = sorted((case.segments[0][i].prof, case.segments[0][i].dom_idx) for i in kept[0] if case.segments[0][i].rep == u)
        l0, l2, r0, r1 = PC._prof(n, "3_", 0), PC._prof(n, "3_", 2), PC._prof(n, "4_", 0), PC._prof(n, "4_", 1)
        assert got == sorted([(l0, 0), (l2, 0), (r1, 0), (r0, 0), (r1, 1)])


def test_lazy_model_on_the_hand_made_table():
    case = [c for c in CASES if c.name == "lazy_pending"][0]
    n = case.names
    lz = X.lazy_model(case.rows, n, case.lazy["lb"], case.lazy["ub"], case.domE)
    assert sorted(set(v for v in lz.verdict if v is not None)) == [0, 1, 2]
    l0, l1, r0, r1 = PC._prof(n, "3_", 0), PC._prof(n, "3_", 1), PC._prof(n, "4_", 0), PC._prof(n, "4_", 1)
    assert lz.pending == 6 and lz.uniq_flags == [0, 3, 4, 5, 11] and lz.prof_flags == sorted([l0, l1, r0, r1])
    quiet = [c for c in CASES if c.name == "lazy_quiet"][0]
    lq = X.lazy_model(quiet.rows, n, quiet.lazy["lb"], quiet.lazy["ub"], quiet.domE)
    assert lq.pending == 0 and 2 in lq.verdict
    assert len(lq.winners) == len(set(quiet.rows[i].ident() for i in lq.winners)) == 6          # two of representative 9, two of 10, one each of 1 and 2


def test_debug_entry_is_declared_and_exported():
    from itsxpress_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "itsx_hip.h")).read()
    for name in ("itsx_debug_set_domains", "itsx_debug_get_rows"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert "#define ITSX_ABI_VERSION 6" in hdr and _lib.lib().itsx_abi_version() == 6
