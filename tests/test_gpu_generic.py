"""The engine against the independent float64 statement (tests/hmm_generic.py) on every case of tests/edge_cases.py: the full
table's traces and domain rows checked directly (not through the oracle), and the production default (lazy + shared + two-sided,
no trace) checked against ItsPosition fed a float64 domain table.  `pytest -m gpu`."""
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import edge_cases
import generic_check as GC
import hmm_generic as G
import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(GC.pool_size()) as ex:
        yield ex


def _run(engine, hmm, seqs):
    engine.load_profiles(text=hmm)
    engine.set_reads(seqs)
    engine.derep()
    engine.search()
    engine.finalize()
    return engine.get_uniques()[0].copy()


@pytest.mark.parametrize("name", list(edge_cases.CASES))
def test_engine_agrees_with_float64(name, engine, pool, monkeypatch, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads):
    hmm, seqs, edge = edge_cases.case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1])
    hm = G.parse_hmms(hmm)
    # full table, every trace kept
    monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
    engine.set_rows_mode("full")
    try:
        seed = _run(engine, hmm, seqs)
        tr, dom = engine.pairtraces(), engine.domains()
    finally:
        engine.set_rows_mode(None)
    assert [h["M"] for h in hm] == [engine.profile_tables(i)["M"] for i in range(engine.n_profiles)]
    useqs = [seqs[int(i)] for i in seed]
    n_multi = engine.stats()["n_multidomain"]
    # the ensemble stage's float64 model replays the paths the CPU oracle sampled for the same pairs (tests/ensemble_exact.py)
    ens = GC.ensemble_models(orc.HmmSet(text=hmm), hm, useqs, tr, "rep", pool)
    rep, rows = GC.check(name, hm, useqs, tr, dom, "rep", pool, sample=None if edge else 40, seed=7, ens=ens)
    assert rep.unstated == 0
    if name == "multidomain":
        assert n_multi > 0 and "ens_domcorrection" in rep.worst                       # the case reaches the ensemble stage
    # the production default: no hooks, no trace
    monkeypatch.delenv("ITSX_KEEP_TRACE")
    seed2 = _run(engine, hmm, seqs)
    assert np.array_equal(seed, seed2)
    names = ["u%d" % i for i in range(len(useqs))]
    prof_names = engine.profile_names()
    n_sides = 0
    for left, right in (("3_", "4_"), ("1_", "2_")):
        want, shaky = GC.winners(rows, names, prof_names, left, right)
        st, sp, tl, ind = engine.rep_coords(left, right)
        for u, w in want.items():
            n_sides += 1
            got = (int(st[u]), int(sp[u]), int(tl[u]))
            assert ind[u]
            if got != w:
                if u in shaky:
                    rep.near.append(("winner", "unique %d %s%s" % (u, left, right), 0.0))
                else:
                    rep.fail.append("%s: unique %d (%s, %s): production default %s, float64 ItsPosition %s" % (name, u, left, right, got, w))
    assert n_sides > 0
    print(rep.finish())
