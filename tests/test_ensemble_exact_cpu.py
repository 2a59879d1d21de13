"""The CPU oracle's multidomain ensemble stage (oracle/orc_search.c: region_trace_ensemble) against the independent float64 model
of tests/ensemble_exact.py: every random choice of every sampled path replayed, the per-residue null2 scores, every envelope's
domcorrection, the envelopes themselves, and the clustering alone on hand-made tuples at its decision edges.  No GPU needed."""
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import ensemble_exact as EX
import generic_check as GC
import orc


@pytest.fixture(scope="module")
def models(t_hmm_text, mini_hmm_text):
    """{input: (reads, parsed profiles, model dict, oracle search)}, computed once"""
    out = {}
    orc.mr_fail_counts(True)
    with ProcessPoolExecutor(GC.pool_size()) as pool:
        for name, hmm, seqs in EX.inputs(t_hmm_text, mini_hmm_text):
            res, hs, hm, md = EX.oracle_and_model(hmm, seqs, pool)
            out[name] = (seqs, hm, md, res)
    assert orc.mr_fail_counts(True) == [0] * 8                       # every region could be sampled
    return out


def _regions(models, name):
    return [(s, p, reg, r) for (s, p), lst in models[name][2].items() for reg, r in lst]


NAMES = ["adversarial", "parity", "node_edges", "degenerate"]


def test_inputs_hold_their_edges(models):
    """at least 25 multidomain regions, one with 5 envelopes or more, one from residue 1, one to residue L, one with a degenerate
    residue, M = 46, 45 and 11 or 25; and the search itself sends every one of them to the stage"""
    EX.assert_inputs_hold_their_edges({n: v[:3] for n, v in models.items()})
    for name, (seqs, hm, md, res) in models.items():
        assert res.counts["multidomain"] == sum(len(l) for l in md.values()) > 0, name
    assert list(models) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_every_sampled_step_is_the_float64_models_choice(models, name):
    """no contradiction: the generator's start state, every step's bookkeeping (state, k, i, draws) and the branch every roll
    selects; at most 1 roll in 1000 excused by the band"""
    rs = [r for _, _, _, r in _regions(models, name)]
    rolls, exc, msg = EX.verdict(rs)
    print("[%s] regions=%d rolls=%d excused=%d" % (name, len(rs), rolls, len(exc)))
    assert rolls > 0 and msg is None, msg


@pytest.mark.parametrize("name", NAMES)
def test_null2_by_trace_and_domcorrection(models, name):
    """per residue n2sc within tol(Lr, M) nats of the model's; every ensemble envelope's domcorrection within tol(Ld, M) of the
    model's sum over the envelope"""
    seqs, hm, md, res = models[name]
    worst_n, worst_d, nrow = 0.0, 0.0, 0
    for s, p, reg, r in _regions(models, name):
        lim = GC.tol(r["jreg"] - r["ireg"] + 1, r["M"])
        dev = float(np.abs(reg["n2sc"].astype(np.float64) - r["n2sc"]).max())
        worst_n = max(worst_n, dev / lim)
        assert dev <= lim, (name, s, p, r["ireg"], r["jreg"], dev, lim)
    for d in res.domains[(res.domains["flags"] & 1) == 1]:
        s, p, i, j = int(d["seq"]), int(d["prof"]), int(d["ienv"]), int(d["jenv"])
        r = next(r for _, r in md[(s, p)] if r["ireg"] <= i and j <= r["jreg"])
        want = float(r["n2sc"][i - r["ireg"]:j - r["ireg"] + 1].sum())
        lim = GC.tol(j - i + 1, r["M"])
        dev = abs(float(d["domcorrection"]) - want)
        worst_d = max(worst_d, dev / lim)
        nrow += 1
        assert dev <= lim, (name, s, p, i, j, float(d["domcorrection"]), want, lim)
    print("[%s] worst dev/tol: n2sc %.3f domcorrection %.3f (%d envelopes)" % (name, worst_n, worst_d, nrow))
    assert nrow > 0


@pytest.mark.parametrize("name", NAMES)
def test_envelopes_equal_the_models(models, name):
    """the model's clustering of the tuples IT derives from the replayed paths == the oracle's envelopes, exactly; and the search's
    flagged rows are those envelopes"""
    seqs, hm, md, res = models[name]
    for s, p, reg, r in _regions(models, name):
        assert r["envs"] == reg["envs"], (name, s, p, r["ireg"], r["jreg"], r["envs"], reg["envs"])
    rows = {}
    for d in res.domains[(res.domains["flags"] & 1) == 1]:
        rows.setdefault((int(d["seq"]), int(d["prof"])), []).append((int(d["ienv"]), int(d["jenv"])))
    want = {k: [e for _, r in lst for e in r["envs"]] for k, lst in md.items() if any(r["envs"] for _, r in lst)}
    assert rows == want


# ---------------------------------------------------------------------------------------------------------------- clustering alone
def _paths(n, tuples, first=0):
    """n paths (traces first .. first+n-1) that each hold the given (i, j, k, m) domains, listed last-first"""
    return [(first + t,) + tuple(x) for t in range(n) for x in tuples]


def _bridge():
    """51 paths of one single-linkage chain in which the leftmost start seen twice (50) lies right of the rightmost end seen twice
    (40): best_i > best_j, and best_k > best_m"""
    tup = [(20 - a, 40, 11 - a, 31) for a in range(3)]
    tup += [(20 + 3 * a, 40 + 3 * a, 11 + 3 * a, 31 + 3 * a) for a in range(1, 10)]
    tup += [(50, 70 + 3 * a, 41, 61 + 3 * a) for a in range(39)]
    return [(t,) + x for t, x in enumerate(tup)]


def _tie():
    """101 paths (thr = 3) whose starts nobody reaches three times: 10 once, 11 and 12 twice (the tie; the first maximum wins),
    13 .. 108 once; every end at 300"""
    starts = [10, 11, 11, 12, 12] + list(range(13, 109))
    return [(t, i, 300, 1, 40) for t, i in enumerate(starts)]


A = (10, 100, 1, 40)
CLUSTER_CASES = {
    # sequence overlap of the smaller: 4/5 links, 79/99 does not
    "seq_4_of_5": _paths(60, [(1, 5, 1, 40)]) + _paths(60, [(2, 10, 1, 40)], 60),
    "seq_79_of_99": _paths(60, [(1, 99, 1, 40)]) + _paths(60, [(21, 150, 1, 40)], 60),
    # model overlap, counted without its "+ 1": 4/5 and 80/99 link, 79/99 does not (two clusters then; equally probable and 82/101
    # of the sequence shared, so the earlier one goes)
    "model_4_of_5": _paths(60, [(10, 110, 1, 5)]) + _paths(60, [(10, 110, 1, 9)], 60),
    "model_80_of_99": _paths(60, [(10, 110, 1, 99)]) + _paths(60, [(28, 160, 19, 150)], 60),
    "model_79_of_99": _paths(60, [(10, 110, 1, 99)]) + _paths(60, [(29, 160, 20, 150)], 60),
    # diagonals within 4 at one end, the other end far
    "diag_start_4": _paths(60, [A]) + _paths(60, [(14, 100, 1, 20)], 60),
    "diag_start_5": _paths(60, [A]) + _paths(60, [(15, 100, 1, 20)], 60),
    "diag_end_4": _paths(60, [A]) + _paths(60, [(30, 104, 1, 40)], 60),
    "diag_end_5": _paths(60, [A]) + _paths(60, [(30, 105, 1, 40)], 60),
    # a cluster in 49, 50, 51 of the 200 paths
    "in_49_paths": _paths(49, [A]), "in_50_paths": _paths(50, [A]), "in_51_paths": _paths(51, [A]),
    # an end point nobody reaches thr times, a tie in the histogram
    "tie": _tie(),
    # two clusters (unlinked on the model side) that dominate each other with equal probability: the earlier one goes
    "equal_dominance": _paths(60, [A]) + _paths(60, [(12, 100, 30, 45)], 60),
    # three clusters, the third clear of the first; the middle one more probable than the first; two domains per path
    "three_clusters": _paths(60, [(150, 240, 1, 40), A]) + _paths(70, [(15, 100, 30, 45)], 60),
    # the scan of a cluster's later neighbours stops where the overlap is exactly 0
    "overlap_zero": _paths(60, [(101, 150, 1, 40), A]) + _paths(70, [(120, 150, 30, 45)], 60),
    # a dominated cluster still dominates: only the most probable of three survives
    "chain_of_dominance": _paths(50, [(10, 100, 1, 10)]) + _paths(60, [(12, 102, 15, 25)], 50) + _paths(70, [(14, 104, 30, 40)], 110),
    "best_i_past_best_j": _bridge(),
    "empty": [],
}
# ceilf(ninc * 0.02f): an outlying start seen c times counts from thr on
for _n in (50, 51, 100, 101, 150):
    for _c in (1, 2, 3):
        CLUSTER_CASES["ceilf_%d_%d" % (_n, _c)] = _paths(_c, [(8, 100, 1, 40)]) + _paths(_n - _c, [A], _c)

# what each edge must do in the model (so that a case cannot drift off its edge unnoticed)
EXPECT = {"seq_4_of_5": [(1, 10)], "seq_79_of_99": [(1, 99), (21, 150)], "model_4_of_5": [(10, 110)], "model_80_of_99": [(10, 160)],
          "model_79_of_99": [(29, 160)], "diag_start_4": [(10, 100)], "diag_start_5": [(15, 100)], "diag_end_4": [(10, 104)],
          "in_49_paths": [], "in_50_paths": [(10, 100)], "in_51_paths": [(10, 100)], "tie": [(11, 300)],
          "equal_dominance": [(12, 100)], "three_clusters": [(15, 100), (150, 240)], "chain_of_dominance": [(14, 104)],
          "best_i_past_best_j": [], "empty": [],
          "ceilf_50_1": [(8, 100)], "ceilf_51_1": [(10, 100)], "ceilf_51_2": [(8, 100)], "ceilf_100_1": [(10, 100)],
          "ceilf_100_2": [(8, 100)], "ceilf_101_2": [(10, 100)], "ceilf_101_3": [(8, 100)], "ceilf_150_2": [(10, 100)],
          "ceilf_150_3": [(8, 100)]}


@pytest.mark.parametrize("case", list(CLUSTER_CASES))
def test_clustering_of_hand_made_tuples(case):
    """orc_spensemble_cluster (the function region_trace_ensemble calls) == the model's clustering, exactly, at every float32
    comparison's edge and every rule of the published procedure"""
    tuples = CLUSTER_CASES[case]
    want = EX.cluster(tuples)
    if case in EXPECT:
        assert want == EXPECT[case], (case, want)
    assert orc.spensemble_cluster(tuples) == want, case
