"""The top-up round of itsx_search_finalize counts reported targets only (engine.hip: lazy_topup, domain_pipeline's count-only mode).
Its pairs are unevaluated after round 2, so no row of theirs can win or tie ItsPosition's argmax: the round is there for the lower bounds
on domZ.  It keeps no rows, and a pair with a multidomain region is deferred -- left unevaluated, on the upper bound's side -- instead of
taking an ensemble invocation; only when a row is still undecided without the deferred pairs do they go through the ordinary pipeline
in a second sub-round.  Coordinates must be the full table's in every arm.  `pytest -m gpu`."""
import numpy as np
import pytest

import orc
import synth
from test_gpu_compact import _same
from test_gpu_lazy import _coords
from test_gpu_parity import _its2_subset

pytestmark = pytest.mark.gpu

_CACHE = {}


def _damaged(mini_hmm_text, n=3000, seed=75):
    """tests/test_gpu_lazy.py::test_top_up_round_settles_rows_from_below's reads: 60 % of them heavily damaged; and which are intact"""
    rng = np.random.default_rng(37)
    blob, offs = synth.make_reads(mini_hmm_text, n, seed=seed, fixed_len=0, len_range=(200, 520))
    seqs, intact = [], []
    for s in synth.to_strings(blob, offs):
        if rng.random() < 0.6:
            s = list(s)
            for q in rng.choice(len(s), int(len(s) * rng.uniform(0.3, 0.42)), replace=False):
                s[q] = str(rng.choice(list("ACGT")))
            s = "".join(s)
        else:
            intact.append(s)
        seqs.append(s)
    return seqs, intact


def _inputs(mini_hmm_text, t_hmm_text, doubled):
    """the reads (with `doubled`: 150 intact reads concatenated with themselves, the flank motifs twice), the profiles, and the full
    table's coordinates -- computed once per input and shared"""
    return _CACHE.setdefault(("in", doubled), _make_inputs(mini_hmm_text, t_hmm_text, doubled))


def _make_inputs(mini_hmm_text, t_hmm_text, doubled):
    seqs, intact = _damaged(mini_hmm_text)
    if doubled:
        seqs = seqs + [s + s for s in intact[:150]]
    return seqs, mini_hmm_text + _its2_subset(t_hmm_text, 25, 25)


def _full(engine, key, hmm, seqs):
    if ("full", key) not in _CACHE:
        _CACHE[("full", key)] = _coords(engine, hmm, seqs, "full")[0]
    return _CACHE[("full", key)]


def _lazy(engine, hmm, seqs, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return _coords(engine, hmm, seqs, "lazy")
    finally:
        for k in env:
            monkeypatch.delenv(k)
        engine.set_rows_mode(None)


def _default(engine, key, hmm, seqs, monkeypatch):
    """the lazy search with every switch of the top-up round at its default: coordinates and counters, once per input"""
    if ("lazy", key) not in _CACHE:
        _CACHE[("lazy", key)] = _lazy(engine, hmm, seqs, monkeypatch)
    return _CACHE[("lazy", key)]


def test_count_only_round_equals_the_full_table_and_the_whole_pipeline_round(engine, mini_hmm_text, t_hmm_text, monkeypatch):
    seqs, hmm = _inputs(mini_hmm_text, t_hmm_text, False)
    monkeypatch.setenv("ITSX_LAZY_ZUB_SCALE", "500000")      # (upper bounds as of a data set that much larger: weak rows stay undecided at first)
    ref = _full(engine, False, hmm, seqs)
    got, st = _default(engine, False, hmm, seqs, monkeypatch)
    print("count-only:", {k: st[k] for k in ("n_lazy_pending", "n_lazy_topup", "n_lazy_reruns", "n_lazy_completed", "n_topup_deferred", "n_topup_ensemble", "n_rows_resident")})
    assert st["lazy"] == 1 and st["n_lazy_pending"] > 0 and st["n_lazy_topup"] > 0 and st["n_lazy_reruns"] == 0
    assert _same(ref, got)
    old, st0 = _lazy(engine, hmm, seqs, monkeypatch, ITSX_TOPUP_COUNT_ONLY=0)
    print("whole pipeline:", {k: st0[k] for k in ("n_lazy_pending", "n_lazy_topup", "n_lazy_reruns", "n_lazy_completed", "n_topup_deferred", "n_topup_ensemble", "n_rows_resident")})
    assert st0["n_lazy_pending"] > 0 and st0["n_lazy_topup"] > 0 and st0["n_lazy_reruns"] == 0
    assert st0["n_topup_deferred"] == 0 and st0["n_topup_ensemble"] == 0
    assert _same(ref, old) and _same(old, got)
    # the count-only round leaves no rows behind, and what it defers it does not count as evaluated
    assert st["n_rows_resident"] <= st0["n_rows_resident"]
    assert st["n_lazy_topup"] == st0["n_lazy_topup"] - (0 if st["n_topup_ensemble"] else st["n_topup_deferred"])


def _oracle_multidomain_losers(hmm, seqs):
    """pairs of the CPU oracle's full table that hold a multidomain region's envelope and whose best row prints below their
    (target, 2-character prefix) group's best: pairs that cannot be winners"""
    codes, o = orc.digitize(seqs)
    _, orep, _ = orc.derep(codes, o)
    seeds = [i for i in range(len(seqs)) if orep[i] == i]
    c2, o2 = orc.digitize([seqs[i] for i in seeds])
    hs = orc.HmmSet(text=hmm)
    d = orc.SearchResult(hs, c2, o2, threads=8, keep_trace=0).domains
    d = d[d["dom_idx"] >= 0]
    names = [b.split("NAME  ")[1].split()[0] for b in hmm.split("//\n") if "NAME  " in b]
    cls = np.array([int(n[0]) for n in names])[d["prof"]]
    tenths = np.rint(d["bitscore"].astype(np.float64) * 10).astype(np.int64)
    group = d["seq"] * 8 + cls
    best = {}
    for g, t in zip(group.tolist(), tenths.tolist()):
        best[g] = max(best.get(g, -10 ** 9), t)
    pair_best = {}
    for s, p, t in zip(d["seq"].tolist(), d["prof"].tolist(), tenths.tolist()):
        pair_best[(s, p)] = max(pair_best.get((s, p), -10 ** 9), t)
    multi = d[(d["flags"] & 1) != 0]
    return sum(1 for s, p, c in set(zip(multi["seq"].tolist(), multi["prof"].tolist(), cls[(d["flags"] & 1) != 0].tolist()))
               if pair_best[(s, p)] < best[s * 8 + c])


def test_pairs_with_multidomain_regions_are_deferred_and_not_needed(engine, mini_hmm_text, t_hmm_text, monkeypatch):
    seqs, hmm = _inputs(mini_hmm_text, t_hmm_text, True)
    assert _oracle_multidomain_losers(hmm, seqs) > 0          # the full table has multidomain regions among pairs that cannot win
    monkeypatch.setenv("ITSX_LAZY_ZUB_SCALE", "500000")
    ref = _full(engine, True, hmm, seqs)
    got, st = _default(engine, True, hmm, seqs, monkeypatch)
    print("doubled:", {k: st[k] for k in ("n_lazy_pending", "n_lazy_topup", "n_lazy_completed", "n_topup_deferred", "n_topup_ensemble", "n_mr_clustered")})
    assert st["n_lazy_pending"] > 0 and st["n_lazy_topup"] > 0 and st["n_lazy_reruns"] == 0
    assert st["n_topup_deferred"] > 0 and st["n_topup_ensemble"] == 0
    assert _same(ref, got)


def test_second_sub_round_takes_the_deferred_pairs_through_the_ensemble_stage(engine, mini_hmm_text, t_hmm_text, monkeypatch):
    """ITSX_TOPUP_FORCE_SECOND (a test hook): as if the count-only sub-round had left rows of its profiles undecided"""
    seqs, hmm = _inputs(mini_hmm_text, t_hmm_text, True)
    monkeypatch.setenv("ITSX_LAZY_ZUB_SCALE", "500000")
    ref = _full(engine, True, hmm, seqs)
    _, st0 = _default(engine, True, hmm, seqs, monkeypatch)
    got, st = _lazy(engine, hmm, seqs, monkeypatch, ITSX_TOPUP_FORCE_SECOND=1)
    print("forced:", {k: st[k] for k in ("n_lazy_pending", "n_lazy_topup", "n_lazy_completed", "n_topup_deferred", "n_topup_ensemble", "n_mr_clustered")})
    assert st["n_topup_deferred"] > 0 and st["n_topup_ensemble"] == 1 and st["n_lazy_reruns"] == 0
    assert st["n_lazy_topup"] == st0["n_lazy_topup"] + st["n_topup_deferred"]      # the deferred pairs count once they are evaluated
    assert st["n_mr_clustered"] > st0["n_mr_clustered"]                            # ... by the ensemble stage
    assert _same(ref, got)
    # without the gate the hook is ignored, and reported as ignored
    monkeypatch.setenv("ITSX_TEST_HOOKS", "0")
    try:
        _, st1 = _lazy(engine, hmm, seqs, monkeypatch, ITSX_TOPUP_FORCE_SECOND=1)
        sw = engine.switches()
    finally:
        monkeypatch.setenv("ITSX_TEST_HOOKS", "1")
    assert st1["n_topup_ensemble"] == 0 and "ignored" in sw["ITSX_TOPUP_FORCE_SECOND"]


def test_a_nearly_needed_profile_takes_what_its_row_needs(engine, mini_hmm_text, t_hmm_text, monkeypatch):
    """ITSX_LAZY_TOPUP_ALL=2: a profile whose row needs more than two thirds of its unevaluated pairs (here profiles 4 and 35: 615 of 876)
    takes those, best bound first, instead of all of them; its remaining pairs would follow in a count-only sub-round of their own only if
    the row were still undecided.  It is not: fewer pairs evaluated than under the default rule, nothing counted in full, same coordinates."""
    seqs, hmm = _inputs(mini_hmm_text, t_hmm_text, False)
    monkeypatch.setenv("ITSX_LAZY_ZUB_SCALE", "500000")
    ref = _full(engine, False, hmm, seqs)
    _, st0 = _default(engine, False, hmm, seqs, monkeypatch)
    got, st = _lazy(engine, hmm, seqs, monkeypatch, ITSX_LAZY_TOPUP_ALL=2)
    print("by need:", {k: st[k] for k in ("n_lazy_pending", "n_lazy_topup", "n_lazy_completed", "n_topup_deferred", "n_topup_ensemble")}, "default:", st0["n_lazy_topup"], st0["n_topup_deferred"])
    assert st["n_lazy_pending"] > 0 and st["n_lazy_reruns"] == 0 and st["n_lazy_completed"] == 0 and st0["n_lazy_completed"] == 0
    assert 0 < st["n_lazy_topup"] + st["n_topup_deferred"] < st0["n_lazy_topup"] + st0["n_topup_deferred"]
    assert _same(ref, got)
