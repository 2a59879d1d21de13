"""The engine's multidomain ensemble stage (k_ensemble.hip) against the independent float64 model of tests/ensemble_exact.py, on the
inputs of tests/test_ensemble_exact_cpu.py: every `flags & 1` row of engine.domains() must have the model's envelope coordinates
exactly and the model's domcorrection within tol(Ld, M), in every layout the kernel gives a batch (one, two, up to seven and 64
regions per wave) and on the overflow path (k_mr_trace<true>).

The model replays the paths the CPU oracle sampled (the device kernel exports none); the engine is tied to it through its envelopes
and corrections here, and through its bitwise equality with the oracle in tests/test_gpu_parity.py and tests/test_gpu_caps.py.  The
device's clustering cannot be fed hand-made tuples without a hook in the product, so the clustering's decision edges are checked on
the oracle's function alone (tests/test_ensemble_exact_cpu.py::test_clustering_of_hand_made_tuples).  `pytest -m gpu`."""
from concurrent.futures import ProcessPoolExecutor

import pytest

import ensemble_exact as EX
import generic_check as GC
import orc

pytestmark = pytest.mark.gpu

COMPANIONS = 24                    # reads without a multidomain region that travel with the others: each run is a few dozen reads


@pytest.fixture(scope="module")
def models(t_hmm_text, mini_hmm_text):
    """{input: (profile text, reads, {(read, profile): [model region, ...]})}: the model's answer, computed once, the regions fanned
    out over the pool; of an input's reads only those with a multidomain region and a few companions are kept"""
    out, full = {}, {}
    orc.mr_fail_counts(True)
    with ProcessPoolExecutor(GC.pool_size()) as pool:
        for name, hmm, seqs in EX.inputs(t_hmm_text, mini_hmm_text):
            res, hs, hm, md = EX.oracle_and_model(hmm, seqs, pool)
            rolls, exc, msg = EX.verdict([r for lst in md.values() for _, r in lst])
            assert msg is None, msg
            full[name] = (seqs, hm, md)
            _, rep_of, _ = orc.derep(*orc.digitize(seqs))             # a duplicate (either strand) is searched once: its first copy
            first = [s for s in range(len(seqs)) if rep_of[s] == s]
            hit = {s for (s, p), lst in md.items() if lst} & set(first)
            keep = sorted(hit | set([s for s in first if s not in hit][:COMPANIONS]))
            new = {s: n for n, s in enumerate(keep)}
            out[name] = (hmm, [seqs[s] for s in keep], {(new[s], p): [r for _, r in lst] for (s, p), lst in md.items() if s in new})
    assert orc.mr_fail_counts(True) == [0] * 8
    EX.assert_inputs_hold_their_edges(full)
    return out


def _search(engine, hmm, seqs):
    engine.set_rows_mode("full")
    try:
        engine.load_profiles(text=hmm)
        engine.set_reads(seqs)
        engine.derep()
        engine.search()
        engine.finalize()
        return [int(i) for i in engine.get_uniques()[0]], engine.domains(), engine.stats()
    finally:
        engine.set_rows_mode(None)


@pytest.mark.parametrize("layout", ["one_per_wave", "two_per_wave", "seven_per_wave", "sixty_four_per_wave"])
@pytest.mark.parametrize("name", ["adversarial", "parity", "node_edges", "degenerate"])
def test_engine_envelopes_and_corrections_are_the_models(engine, models, monkeypatch, name, layout):
    hmm, seqs, md = models[name]
    assert len(seqs) <= 3 * COMPANIONS
    nreg = sum(len(lst) for lst in md.values())
    if layout != "one_per_wave":
        monkeypatch.setenv("ITSX_MR_ONE_MAX", "0")
        # lanes per wave = regions / ITSX_MR_WAVES, 2 at the least; 0 = waves of 64 lanes
        monkeypatch.setenv("ITSX_MR_WAVES", {"two_per_wave": "4096", "seven_per_wave": str(max(1, -(-nreg // 7))), "sixty_four_per_wave": "0"}[layout])
    monkeypatch.setenv("ITSX_KEEP_TRACE", "1")
    seed, dom, st = _search(engine, hmm, seqs)
    assert sorted(seed) == list(range(len(seqs)))
    assert st["n_multidomain"] == st["n_mr_clustered"] == nreg and st["n_mr_failed"] == 0
    if name == "adversarial":
        assert st["n_mr_overflow"] >= 1                              # the reads leave the fast kernel's bookkeeping: k_mr_trace<true> runs
    got, worst = {}, 0.0
    for d in dom[(dom["flags"] & 1) == 1]:
        s, p, i, j = seed[int(d["rep"])], int(d["prof"]), int(d["ienv"]), int(d["jenv"])
        got.setdefault((s, p), []).append((i, j))
        r = next((r for r in md.get((s, p), []) if r["ireg"] <= i and j <= r["jreg"]), None)
        assert r is not None and (i, j) in r["envs"], (name, layout, s, p, i, j, [r["envs"] for r in md.get((s, p), [])])
        want = float(r["n2sc"][i - r["ireg"]:j - r["ireg"] + 1].sum())
        lim = GC.tol(j - i + 1, r["M"])
        dev = abs(float(d["domcorrection"]) - want)
        worst = max(worst, dev / lim)
        assert dev <= lim, (name, layout, s, p, i, j, float(d["domcorrection"]), want, lim)
    want = {k: [e for r in lst for e in r["envs"]] for k, lst in md.items() if any(r["envs"] for r in lst)}
    assert got == want
    print("[%s %s] regions=%d envelopes=%d overflow=%d worst domcorrection dev/tol %.3f"
          % (name, layout, nreg, sum(len(v) for v in got.values()), st["n_mr_overflow"], worst))
