"""The lazy domain stage's bound on the device (csrc/k_lazy.hip: k_fwd_bound, k_bwd_bound and the join, k_lazy_bound)
against the float64 model, pair by pair (Engine.debug_lazy_pairs), on every case of tests/lazy_bound_cases.py and in five schedules
of pass A:

  a. pass A's score of every real pair within generic_check.tol(L, M) of hmm_generic.forward_nats_batch -- the rounding budget
     lazy_c's margin assumes; -inf where float64 says -inf; no NaN, no +inf;
  b. b10 = lazy_bound_cases.b10_model of the returned fb, nullsc and lazy_c, for every pair;
  c. lazy_c >= C(L) + the margin DESIGN.md 4b states, in float64, for every L that occurs;
  d. every domain row of the FULL table of the same input (ensemble envelopes and the overflow path's included) prints "%.1f"
     tenths that do not exceed its pair's b10, and its pair is on the lazy list;
  e. per (representative, two-character class) the pair of the full table's winning row under ItsPosition's rule, and every pair
     whose reported row ties its "%.1f", went through the domain stage (done = 1).
`pytest -m gpu`."""
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import generic_check as GC
import hmm_generic as G
import lazy_bound_cases as LB
from itsxpress_amd._lib import EngineError

pytestmark = pytest.mark.gpu

SWITCHES = ("ITSX_SHARE", "ITSX_SHARE_MIN", "ITSX_SHARE_TWO", "ITSX_BOUND_FOLD", "ITSX_SHARE_B", "ITSX_SHARE_GB", "ITSX_SHARE_CHECK",
            "ITSX_CHUNK_UNIQUES", "ITSX_LAZY_CHECK_BOUND", "ITSX_LAZY_EXACT_BOUND", "ITSX_KEEP_TRACE", "ITSX_ROWS", "ITSX_COMPACT_ROWS")
SCHEDULES = {"default": {},
             "no_sharing": {"ITSX_SHARE": 0},
             "one_sided": {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_TWO": 0},
             "two_sided": {"ITSX_SHARE_MIN": 0},
             "plain": {"ITSX_BOUND_FOLD": 0}}


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(GC.pool_size()) as ex:
        yield ex


_CASE = {}       # per case: the catalogue entry, the full table and the float64 Forward scores, made once and left unchanged


def _search(engine, c, mode, env, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    engine.set_rows_mode(mode)
    try:
        engine.load_profiles(text=c.hmm)          # (ITSX_BOUND_FOLD is read when the profiles are installed)
        engine.set_reads(c.seqs)
        engine.derep(minseqlength=1)
        engine.search(F1=c.F, F2=c.F, F3=c.F)
    finally:
        engine.set_rows_mode(None)


def _case(name, engine, monkeypatch, t, mini, allt, fx):
    if name in _CASE:
        return _CASE[name]
    c = LB.case(name, t, mini, allt, fx)
    d = dict(c=c, hm=G.parse_hmms(c.hmm))
    # the full table of the same input: every row of every pair, reported or not
    _search(engine, c, "full", {}, monkeypatch)
    engine.finalize()
    d["seed"] = engine.get_uniques()[0].copy()
    d["useqs"] = [c.seqs[int(i)] for i in d["seed"]]
    d["rows"] = engine.domains().copy()
    st = engine.stats()
    d["full_stats"] = st
    d["prof_names"] = engine.profile_names()
    assert [h["M"] for h in d["hm"]] == [engine.profile_tables(i)["M"] for i in range(engine.n_profiles)]
    assert st["n_past_msv"] > 0 and len(d["rows"]) > 0, "%s: the case does not reach the domain stage (%d pairs past MSV, %d rows)" % (
        name, st["n_past_msv"], len(d["rows"]))
    d["fwd"] = {}
    _CASE[name] = d
    return d


def _taken(name, sched, st, sw):
    """the schedule the switches ask for is the one that ran"""
    assert st["lazy"] == 1 and st["n_lazy_reruns"] == 0
    waves = name.startswith("waves_")
    if sched == "default":
        assert not any(k in sw for k in SWITCHES)
        if waves:
            assert st["share_B"] == 32 and st["two_sided"] == 1
    elif sched == "no_sharing":
        assert st["share_B"] == 0 and st["share_chains"] == 0 and st["two_sided"] == 0 and st["n_joined"] == 0 and st["bwd_rows"] == 0
        assert st["bound_rows"] == st["bound_rows_full"]
    elif sched == "one_sided":
        assert st["two_sided"] == 0 and st["n_joined"] == 0 and st["bwd_rows"] == 0 and st["n_bwd_launches"] == 0
        if waves:
            assert st["share_B"] == 32 and st["share_chains"] > 0 and st["bound_rows"] < st["bound_rows_full"]
    elif sched == "two_sided":
        if waves:
            assert st["share_B"] == 32 and st["share_chains"] > 0 and st["two_sided"] == 1 and st["n_joined"] > 0 and st["bwd_rows"] > 0
    else:
        assert sw.get("ITSX_BOUND_FOLD") == "0" and st["two_sided"] == 0 and st["n_joined"] == 0      # (two-sided sharing needs the folded table)
        if waves:
            assert st["share_B"] == 32 and st["share_chains"] > 0


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", list(LB.CASES))
def test_pass_a_bound_against_float64(name, sched, engine, pool, monkeypatch, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads):
    d = _case(name, engine, monkeypatch, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1])
    c, hm, useqs = d["c"], d["hm"], d["useqs"]
    _search(engine, c, "lazy", SCHEDULES[sched], monkeypatch)
    st, sw = engine.stats(), engine.switches()
    _taken(name, sched, st, sw)
    assert np.array_equal(engine.get_uniques()[0], d["seed"])
    recs, bias = engine.debug_lazy_pairs()
    recs = recs.copy()
    assert st["n_past_msv"] == d["full_stats"]["n_past_msv"]
    if name.startswith("waves_"):
        n = int(name.split("_")[1])
        per_prof = np.bincount(recs["prof"][(recs["prof"] >= 0) & (recs["xj"] >= 0)], minlength=len(hm))
        assert per_prof.max() == n and len({len(s) for s in useqs}) == len(LB.WAVE_LENGTHS)       # (the ragged last wave: n % 64 != 0 but at 64)
    pad = recs["prof"] < 0
    helper = ~pad & (recs["xj"] < 0)
    real = ~pad & ~helper
    assert real.sum() == st["n_past_msv"] > 0
    assert (recs["b10"][pad] == 0).all() and (recs["rep"][pad] == -1).all()
    assert (recs["b10"][helper] == 0).all() and (recs["done"][helper] == 1).all()                    # never selected
    R = recs[real]
    assert ((R["rep"] >= 0) & (R["rep"] < len(useqs))).all() and (R["prof"] < len(hm)).all()
    assert (R["L"] == np.array([len(useqs[int(r)]) for r in R["rep"]])).all()
    keys = [(int(r), int(p)) for r, p in zip(R["rep"], R["prof"])]
    assert len(set(keys)) == len(keys)
    # ---- a. pass A against the model (float64 once per case)
    missing = [k for k in keys if k not in d["fwd"]]
    if missing:
        assert not d["fwd"], "%s / %s: other pairs past the MSV filter than in the first schedule: %s" % (name, sched, missing[:5])
        d["fwd"].update(LB.forward_float64(hm, useqs, missing, pool))
    assert set(keys) == set(d["fwd"])
    fb = R["fb"]
    assert int(np.isnan(fb).sum()) == 0 and int((fb == np.inf).sum()) == 0
    bad, worst = [], 0.0
    for r, k in zip(R, keys):
        want, L, M = d["fwd"][k], int(r["L"]), hm[k[1]]["M"]
        if want < G.NEG / 2:
            if r["fb"] != -np.inf:
                bad.append("%s: float64 Forward is -inf, pass A says %r" % (k, float(r["fb"])))
            continue
        dev = abs(float(r["fb"]) - want) / GC.tol(L, M)
        worst = max(worst, dev)
        if not dev <= 1.0:
            bad.append("unique %d profile %d (L %d, M %d): pass A %.6f, float64 %.6f, tol %.2g" % (k[0], k[1], L, M, float(r["fb"]), want, GC.tol(L, M)))
    assert not bad, "\n".join(bad[:20])
    # ---- b. b10 is k_lazy_bound's arithmetic on the returned numbers
    assert bias == 1 << 23
    want10 = LB.b10_model(R["fb"], R["nullsc"], R["lazy_c"], bias)
    assert np.array_equal(R["b10"], want10), [(k, int(a), int(b)) for k, a, b in zip(keys, R["b10"], want10) if a != b][:10]
    # ---- c. lazy_c (and the null model's score beside it) for every length that occurs
    for L in sorted(set(int(x) for x in R["L"])):
        r = R[R["L"] == L][0]
        assert (R["lazy_c"][R["L"] == L] == r["lazy_c"]).all() and (R["nullsc"][R["L"] == L] == r["nullsc"]).all()
        assert float(r["lazy_c"]) >= LB.c_of_n(L) + LB.margin_bits(L), (L, float(r["lazy_c"]), LB.c_of_n(L), LB.margin_bits(L))
        assert float(r["lazy_c"]) <= LB.c_of_n(L) + LB.margin_bits(L) + 1e-6                          # ... and no slacker than one float32 step
        assert abs(float(r["nullsc"]) - LB.nullsc(L)) <= 1e-6 * max(1.0, abs(LB.nullsc(L)))
    # ---- d. the full table's rows obey the bound, on the engine's own numbers
    b10_of = dict(zip(keys, (int(x) for x in R["b10"])))
    rows = d["rows"]
    n_ens, tight = 0, 1 << 30
    for row in rows:
        k = (int(row["rep"]), int(row["prof"]))
        assert k in b10_of, "a full-table row of unique %d profile %d, but no such pair on the lazy list" % k
        n_ens += int(row["flags"]) & 1
        t10 = LB.printed_tenths(row["bitscore"]) + bias
        tight = min(tight, b10_of[k] - t10)
        assert t10 <= b10_of[k], "unique %d profile %d envelope %d-%d (flags %d): prints %.1f, bound %.1f" % (
            k[0], k[1], row["ienv"], row["jenv"], row["flags"], row["bitscore"], (b10_of[k] - bias) / 10.0)
    if name == "tandem":
        assert n_ens > 0 and d["full_stats"]["n_multidomain"] > 0 and d["full_stats"]["n_mr_overflow"] > 0
    # ---- e. the selection closes: the winner's pair and every pair that ties it are evaluated
    done0 = dict(zip(keys, (int(x) for x in R["done"])))
    engine.finalize()
    try:
        recs1, _ = engine.debug_lazy_pairs()
        R1 = recs1[(recs1["prof"] >= 0) & (recs1["xj"] >= 0)]
        assert np.array_equal(R1["rep"], R["rep"]) and np.array_equal(R1["prof"], R["prof"]) and np.array_equal(R1["b10"], R["b10"])
        assert (R1["done"] >= R["done"]).all()
        done = dict(zip(keys, (int(x) for x in R1["done"])))
    except EngineError:
        # finalize counted a profile in full (itsx_lazy_complete): the list is gone, every pair of that profile was evaluated, and
        # the rounds of the search itself must have held the winners already
        assert engine.stats()["n_lazy_completed_profiles"] > 0
        done = done0
    assert engine.stats()["n_lazy_reruns"] == 0
    groups = {}
    for row in rows:
        if row["dom_reported"] == 1:
            g = (int(row["rep"]), d["prof_names"][int(row["prof"])][:2])
            groups.setdefault(g, []).append((LB.printed_tenths(row["bitscore"]), int(row["prof"])))
    n_win = 0
    for (u, cls), lst in groups.items():
        top = max(t for t, _ in lst)
        for t, p in lst:
            if t == top:
                n_win += 1
                assert done[(u, p)] == 1, "unique %d class %s: the pair of profile %d holds a winning / tying row (%.1f) and was not evaluated" % (u, cls, p, t / 10.0)
                assert done0[(u, p)] == 1, "unique %d class %s profile %d: evaluated by finalize only, not by the search's two rounds" % (u, cls, p)
    print("[%s / %s] pairs=%d (helpers %d) rows=%d (ensemble %d) winners+ties=%d shortest L=%d lengths=%d worst pass A dev/tol=%.3f joined=%d chains=%d tightest row %d tenths below its bound" % (
        name, sched, len(R), int(helper.sum()), len(rows), n_ens, n_win, int(R["L"].min()), len(set(R["L"].tolist())), worst, st["n_joined"], st["share_chains"], tight))
