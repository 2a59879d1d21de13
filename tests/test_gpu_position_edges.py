"""The last step of the search on the device -- the domain threshold (k_finalize, k_finalize_lazy), ItsPosition's argmax (k_positions,
k_position_coords, k_rep_coords, k_read_coords), the parity-risk counters (k_position_flags, k_count_flags), the compaction
(k_compact_*), the lazy verdicts (k_lazy_sure, k_lazy_pending) and the host's winners filter -- against the exact model of
tests/position_exact.py, on the hand-made tables of tests/position_cases.py put into a context with itsx_debug_set_domains.  Every
comparison is exact.  `pytest -m gpu`."""
import numpy as np
import pytest

import position_cases as PC
import position_exact as X

pytestmark = pytest.mark.gpu

CASES = PC.catalogue()
FIELDS = ("rep", "prof", "tlen", "ienv", "jenv", "dom_idx", "ndom", "flags", "bitscore", "lnP", "seq_reported")
COUNTERS = ("n_uniq_multi_winner", "n_reads_multi_winner", "n_uniq_region_cap", "n_reads_region_cap")


@pytest.fixture(scope="module")
def eng():
    from itsxpress_amd import Engine
    e = Engine(0)
    e._position_key = None
    yield e
    e.close()


def _prepare(eng, case):
    """profiles, reads and the dereplication of the case's read set (kept while consecutive cases share them)"""
    key = (case.reads, case.hmm)
    rs = PC.reads(case.reads)
    if eng._position_key != key:
        eng._position_key = None
        eng.set_rows_mode(None)
        assert eng.load_profiles(text=PC.hmm_text(case.hmm)) == case.P and eng.profile_names() == case.names
        eng.set_reads(rs.seqs)
        if rs.S > 1:
            eng.set_samples(rs.sample_of, rs.S)
        assert eng.derep(True, PC.MINLEN) == rs.U
        rep_of, strand, uniq_of = eng.get_derep()
        assert uniq_of.tolist() == rs.uniq_of and strand[-6:].tolist() == [1, -1, 1, -1, -1, 1]      # (the members: plus and minus strand)
        seed, _ = eng.get_uniques()
        assert seed.tolist() == rs.seed_read
        eng._position_key = key
    return rs


def _inject(eng, case, mode):
    eng.debug_set_domains(PC.to_array(case.rows), [len(s) for s in case.segments], mode)


def _same_rows(got, rows, idx, fields=FIELDS):
    assert len(got) == len(idx)
    want = PC.to_array([rows[i] for i in idx])
    for f in fields:
        assert np.array_equal(got[f], want[f]), f


def _check_coords(eng, rs, case, res, region, counters=True):
    left, right = X.REGIONS[region]
    rep = np.array(res.rep, np.int32).reshape(rs.U, 4)
    read = np.array(res.read, np.int32).reshape(len(rs.seqs), 4)
    got = np.stack(eng.rep_coords(left, right), axis=1)
    assert np.array_equal(got, rep), (case.name, region, np.nonzero((got != rep).any(axis=1))[0][:8])
    st = eng.stats()
    if counters:
        assert {k: st[k] for k in COUNTERS} == res.counters, (case.name, region)
    assert np.array_equal(np.stack(eng.trim_coords(left, right), axis=1), read), (case.name, region)
    assert np.array_equal(eng.rep_coords_device(left, right).cpu().numpy(), rep)
    assert np.array_equal(eng.trim_coords_device(left, right).cpu().numpy(), read)
    if counters:
        st = eng.stats()
        assert {k: st[k] for k in COUNTERS} == res.counters
    if case.expect and region in case.expect:           # recorded from the reference class, or worked out by hand from its code
        for u, want in case.expect[region].items():
            assert tuple(got[u]) == want, (case.name, region, u)
    # reads that were too short have no row; a member has its representative's
    for i, u in enumerate(rs.uniq_of):
        assert res.read[i] == ((-1, -1, -1, 0) if u < 0 else res.rep[u])


# ---------------------------------------------------------------- full mode
@pytest.mark.parametrize("case", PC.full_cases(), ids=lambda c: c.name)
def test_full_table_is_decided_as_the_model_decides_it(eng, case):
    rs = _prepare(eng, case)
    rows = case.rows
    _inject(eng, case, "full")
    assert int(eng.L.itsx_domz_count(eng.h)) == case.P * rs.S and not eng.get_domz().any()
    eng.set_domz(case.domz)
    eng.finalize(case.domE)
    flags = X.reported_flags(rows, case.domz, case.domE, case.usample(), case.P)
    raw = eng.debug_get_rows()                              # as injected, padding included, only dom_reported written
    _same_rows(raw, rows, list(range(len(rows))))
    assert raw["dom_reported"].tolist() == [0 if f is None else f for f in flags]
    order = X.table_order(rows)
    tab = eng.domains()                                     # --domtblout order, padding gone
    _same_rows(tab, rows, order)
    assert tab["dom_reported"].tolist() == [flags[i] for i in order]
    st = eng.stats()
    assert st["n_domains"] == len(order) and st["n_rows_resident"] == len(rows) and st["lazy"] == 0
    for region in case.regions:
        left, right = X.REGIONS[region]
        _check_coords(eng, rs, case, X.positions(rows, flags, case.names, left, right, rs.U, rs.uniq_of), region)


def test_full_table_written_as_domtbl_parses_to_the_models_dictionary(eng, tmp_path):
    case = [c for c in CASES if c.name == "ties/split"][0]
    rs = _prepare(eng, case)
    _inject(eng, case, "full")
    eng.set_domz(case.domz)
    eng.finalize(case.domE)
    p = tmp_path / "domtbl.txt"
    eng.write_domtbl(str(p))
    flags = X.reported_flags(case.rows, case.domz, case.domE)
    names = ["r%09d" % r for r in rs.seed_read]
    for region, (left, right) in X.REGIONS.items():
        dd, _ = X.walk(X.parse_domtbl(p.read_text()), left, right)
        assert dd == X.walk(X.lines_of_rows(case.rows, flags, case.names, target_name=lambda u: names[u]), left, right)[0] and len(dd) == 32


def test_injection_validates_its_rows(eng):
    from itsxpress_amd import EngineError
    case = [c for c in CASES if c.name == "sides/order"][0]
    rs = _prepare(eng, case)
    _inject(eng, case, "full")
    eng.set_domz(case.domz)
    eng.finalize(case.domE)
    before = eng.domains()
    good = PC.to_array(case.rows)
    for field, value in (("rep", rs.U), ("rep", -1), ("prof", case.P), ("prof", -1)):
        bad = good.copy()
        bad[field][3] = value
        with pytest.raises(EngineError) as e:
            eng.debug_set_domains(bad, None, "full")
        assert e.value.code == -1
    for seg, mode in (([len(good) - 1], 0), ([len(good), -0 - 1], 0), (None, 3), (None, -1)):
        with pytest.raises(EngineError) as e:
            eng.debug_set_domains(good, seg, mode)
        assert e.value.code == -1
    after = eng.domains()                                   # a refused table changes nothing
    assert before.tobytes() == after.tobytes()
    eng.debug_set_domains(good[:0], [], "full")             # no rows, no segments
    eng.finalize(10.0)
    assert len(eng.domains()) == 0 and not np.stack(eng.rep_coords("3_", "4_"), axis=1)[:, 3].any()


# ---------------------------------------------------------------- compact mode
@pytest.mark.parametrize("env", PC.COMPACT_ENVS, ids=["default", "tightened"])
@pytest.mark.parametrize("case", PC.full_cases(), ids=lambda c: c.name)
def test_compacted_table_keeps_the_models_rows_and_decides_alike(eng, case, env, monkeypatch, tmp_path):
    from itsxpress_amd import EngineError
    rs = _prepare(eng, case)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    zmax, dmin = PC.compact_assumptions(env)
    try:
        _inject(eng, case, "compact")
        kept = X.compact_kept(case.segments, case.names, zmax, dmin)
        krows = [case.segments[s][i] for s in range(len(case.segments)) for i in kept[s]]
        _same_rows(eng.debug_get_rows(), krows, list(range(len(krows))))
        assert eng.stats()["n_rows_resident"] == len(krows)
        rows = case.rows
        us = case.usample()
        for z, e in PC.compact_combos(case, env):
            eng.set_domz(z)
            eng.finalize(e)
            flags = X.reported_flags(rows, z, e, us, case.P)
            for region in case.regions:
                left, right = X.REGIONS[region]
                # the model on the WHOLE table: what full mode gives for these counters
                _check_coords(eng, rs, Unrecorded(case), X.positions(rows, flags, case.names, left, right, rs.U, rs.uniq_of), region)
            with pytest.raises(EngineError):
                eng.domains()                                   # thinned: refused unless the kept rows are asked for
            eng.set_kept_rows(True)
            win = X.winners_table(rows, flags, case.names)
            _same_rows(eng.domains(), rows, win)
            p = tmp_path / "domtbl.txt"
            eng.write_domtbl(str(p))
            names = ["r%09d" % r for r in rs.seed_read]
            for region in case.regions:
                left, right = X.REGIONS[region]
                assert X.walk(X.parse_domtbl(p.read_text()), left, right)[0] == X.walk(X.lines_of_rows(rows, flags, case.names, target_name=lambda u: names[u]), left, right)[0]
            eng.set_kept_rows(False)
        if case.compact_refused is not None and case.compact_refused["env"] == env:
            eng.set_domz(case.domz)
            with pytest.raises(EngineError) as err:
                eng.finalize(case.domE)
            assert err.value.code == -5
    finally:
        eng.set_kept_rows(False)


class Unrecorded(object):
    """a case without its recorded positions (they belong to its own counters and domE)"""

    def __init__(self, case):
        self.name, self.expect = case.name, None


# ---------------------------------------------------------------- lazy mode
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_lazy_table_verdicts_pending_rows_and_winners(eng, case):
    from itsxpress_amd import EngineError
    rs = _prepare(eng, case)
    rows = case.rows
    lb, ub = PC.lazy_bounds(case)
    try:
        _inject(eng, case, "lazy")
        assert int(eng.L.itsx_domz_count(eng.h)) == 2 * case.P * rs.S and not eng.get_domz().any()
        eng.set_domz(list(lb) + list(ub))
        if case.compact_refused is not None and not case.compact_refused["env"]:
            with pytest.raises(EngineError) as err:             # a lazy table is a thinned one: the same assumptions hold for it
                eng.finalize(case.domE)
            assert err.value.code == -5
            return
        eng.finalize(case.domE)
        lz = X.lazy_model(rows, case.names, lb, ub, case.domE, case.usample(), case.P)
        raw = eng.debug_get_rows()
        _same_rows(raw, rows, list(range(len(rows))))
        assert raw["dom_reported"].tolist() == [0 if v is None else v for v in lz.verdict]
        st = eng.stats()
        assert st["lazy"] == 1 and st["n_lazy_reruns"] == 0 and st["n_lazy_topup"] == 0 and st["n_lazy_completed"] == 0
        assert eng.lazy_pending() == lz.pending == st["n_lazy_pending"]
        assert np.nonzero(eng.lazy_pending_profiles())[0].tolist() == lz.prof_flags
        assert np.nonzero(eng.lazy_pending_uniques())[0].tolist() == lz.uniq_flags
        with pytest.raises(EngineError):                        # there are no pairs to evaluate behind a table that was handed in
            eng.lazy_complete(np.ones(case.P, np.int32))
        eng.set_kept_rows(True)
        if lz.pending:
            with pytest.raises(EngineError):
                eng.rep_coords("3_", "4_")
            with pytest.raises(EngineError):
                eng.domains()
            eng.set_partial_coords(True)
        else:
            _same_rows(eng.domains(), rows, lz.winners)
            assert (eng.domains()["dom_reported"] == 1).all()
        for region in case.regions:
            left, right = X.REGIONS[region]
            res = X.positions(rows, lz.sure_flags, case.names, left, right, rs.U, rs.uniq_of)
            same_as_full = all(v in (0, 1, None) for v in lz.verdict) and min(lb) >= 1 and list(lb) == list(case.domz)
            _check_coords(eng, rs, case if same_as_full else Unrecorded(case), res, region)
    finally:
        eng.set_partial_coords(False)
        eng.set_kept_rows(False)


def test_lazy_table_without_counters_is_refused(eng):
    from itsxpress_amd import EngineError
    case = [c for c in CASES if c.name == "lazy_pending"][0]
    _prepare(eng, case)
    _inject(eng, case, "lazy")
    with pytest.raises(EngineError) as e:
        eng.finalize(case.domE)
    assert e.value.code == -1 and "itsx_set_domz" in e.value.message
    st = eng.stats()
    assert st["n_lazy_topup"] == 0 and st["n_lazy_completed"] == 0 and st["n_lazy_reruns"] == 0
    assert (eng.debug_get_rows()["dom_reported"] == 0).all()           # nothing was decided
    with pytest.raises(EngineError):
        eng.rep_coords("3_", "4_")
    eng.set_domz(case.lazy["lb"] + case.lazy["ub"])
    eng.finalize(case.domE)
    assert eng.lazy_pending() == 6


# ---------------------------------------------------------------- end to end
def _rows_of(tab):
    return [X.Row(int(r["rep"]), int(r["prof"]), int(r["tlen"]), int(r["ienv"]), int(r["jenv"]), int(r["dom_idx"]), int(r["ndom"]), int(r["flags"]),
                  float(r["bitscore"]), float(r["lnP"]), int(r["seq_reported"])) for r in tab]


def test_real_search_with_duplicated_profiles_in_every_rows_mode(eng, fixture_reads, mini_hmm_text, tmp_path):
    """one left and one right profile again under a later name: every row of theirs ties exactly with its twin, and the earlier profile
    must keep the place.  Full, compact and lazy searches and the winners table against the model applied to the full table."""
    import synth
    names, seqs = fixture_reads
    blob, offs = synth.make_reads(mini_hmm_text, 80, seed=5)     # the fixture's reads hit no left profile of this set: 80 reads made from it
    syn = synth.to_strings(blob, offs)
    names, seqs = names + ["syn%03d" % i for i in range(len(syn))], seqs + syn
    blocks = PC._blocks(mini_hmm_text)
    pn = PC._names(mini_hmm_text)
    i3, i4 = PC._prof(pn, "3_", 1), PC._prof(pn, "4_", 2)         # the profiles that win most places on these reads
    twin = lambda b, nm: b.replace("NAME  " + nm, "NAME  " + nm[:2] + "zz_twin_of_" + nm[2:], 1)
    hmm = mini_hmm_text + twin(blocks[i3], pn[i3]) + twin(blocks[i4], pn[i4])
    eng._position_key = None
    try:
        eng.set_rows_mode("full")
        assert eng.load_profiles(text=hmm) == len(pn) + 2
        pnames = eng.profile_names()
        eng.set_reads(seqs, names)
        U = eng.derep()
        _, _, uniq_of = eng.get_derep()
        eng.search()
        z = eng.get_domz().tolist()
        eng.finalize()
        tab = eng.domains()
        rows = _rows_of(tab)
        flags = X.reported_flags(rows, z, 10.0)
        assert tab["dom_reported"].tolist() == flags and sum(flags) > 200
        twin_of = {i3: len(pn), i4: len(pn) + 1}
        at = {r.ident(): r for r in rows}
        tied = lambda r: r.prof in twin_of and (twin_of[r.prof], r.rep, r.dom_idx) in at and X.tenths(at[(twin_of[r.prof], r.rep, r.dom_idx)].bitscore) == X.tenths(r.bitscore)
        assert sum(1 for r in rows if tied(r)) > 40                # the twins' rows tie with the originals'
        model = {}
        for region, (left, right) in X.REGIONS.items():
            res = model[region] = X.positions(rows, flags, pnames, left, right, U, uniq_of.tolist())
            assert region == "ITS1" or sum(1 for r in res.rep if r[0] >= 0 or r[1] >= 0) > 50
        # ... and winners among them on both sides: places that only the tie's direction gives to the earlier profile
        for side in ("left", "right"):
            assert sum(1 for (_, sd), i in model["ITS2"].winners.items() if sd == side and tied(rows[i])) >= 10
        p = tmp_path / "domtbl.txt"
        eng.write_domtbl(str(p))
        seed, _ = eng.get_uniques()
        text = p.read_text()

        def check(counters):
            for region, (left, right) in X.REGIONS.items():
                res = model[region]
                assert np.array_equal(np.stack(eng.rep_coords(left, right), axis=1), np.array(res.rep, np.int32))
                if counters:
                    st = eng.stats()
                    assert {k: st[k] for k in COUNTERS} == res.counters
                assert np.array_equal(np.stack(eng.trim_coords(left, right), axis=1), np.array(res.read, np.int32))

        check(True)
        for region, (left, right) in X.REGIONS.items():            # the written table, parsed by the model
            dd, _ = X.walk(X.parse_domtbl(text), left, right)
            for u in range(U):
                assert X.coords4(dd, names[int(seed[u])]) == model[region].rep[u]
        for mode in ("compact", "lazy"):
            eng.set_rows_mode(mode)
            eng.search()
            eng.finalize()
            assert eng.lazy_pending() == 0
            check(mode == "compact")
            eng.set_kept_rows(True)                                  # the winners table of the thinned search
            _same_rows(eng.domains(), rows, X.winners_table(rows, flags, pnames), [f for f in FIELDS if f != "flags"])
            eng.set_kept_rows(False)
    finally:
        eng.set_kept_rows(False)
        eng.set_rows_mode(None)
