"""The float64 model of the optimal-accuracy alignment (tests/oa_exact.py) on its own: brute force over every path of tiny
problems, its invariants on the inputs of the GPU test, and the skip cap of tests/test_gpu_align.py's coordinate check."""
import math

import numpy as np
import pytest

import edge_cases as EC
import hmm_generic as G
import oa_cases as OC
import oa_exact as OA
import synth


def test_brute_force(mini_hmm_text, t_hmm_text):
    rng = np.random.default_rng(71)
    hm = G.parse_hmms(mini_hmm_text)[:4] + G.parse_hmms(EC._without_match_to_delete(EC._its2(t_hmm_text, 1, 1), 2))[:2]
    n = 0
    for h in hm:
        for M in (1, 2, 3):
            hc = OA.cut(h, M)
            for Ld in (1, 2, 3, 4):
                for _ in range(3):
                    L = Ld + int(rng.integers(0, 4))
                    seq = EC._rnd(rng, L, "ACGTN" if n % 5 == 0 else "ACGT")
                    ienv = int(rng.integers(1, L - Ld + 2))
                    m = OA.align(hc, seq, ienv, ienv + Ld - 1)
                    best, coords = OA.brute_force(m["P"])
                    assert abs(best - m["oasc"]) <= 1e-12, (h["name"], M, seq, ienv, best, m["oasc"])
                    mine = (m["hmm_from"], m["hmm_to"], m["ali_from"] - ienv + 1, m["ali_to"] - ienv + 1)
                    assert mine in coords, (h["name"], M, seq, ienv, mine, coords)
                    n += 1
    assert n >= 200


def _invariants(m, ienv, jenv):
    assert 1 <= m["hmm_from"] <= m["hmm_to"] <= m["M"]
    assert ienv <= m["ali_from"] <= m["ali_to"] <= jenv
    assert 0.0 < m["acc"] <= 1.0 + 1e-12
    c = m["constrained"](m["hmm_from"], m["hmm_to"], m["ali_from"], m["ali_to"])
    assert abs(c - m["oasc"]) <= 1e-12 * max(1.0, m["oasc"]), (c, m["oasc"])


def test_consensus_aligns_end_to_end(mini_hmm_text):
    rng = np.random.default_rng(72)
    for h, c in zip(G.parse_hmms(mini_hmm_text), synth.consensus_motifs(mini_hmm_text, "")):
        if not c or len(c) != h["M"]:
            continue
        m = OA.align(h, c, 1, len(c))
        _invariants(m, 1, len(c))
        assert (m["hmm_from"], m["hmm_to"], m["ali_from"], m["ali_to"]) == (1, h["M"], 1, len(c)), h["name"]
        a, b = int(rng.integers(5, 20)), int(rng.integers(5, 20))
        s = EC._rnd(rng, 30) + EC._rnd(rng, a) + c + EC._rnd(rng, b) + EC._rnd(rng, 30)
        ienv, jenv = 31, 30 + a + len(c) + b
        m = OA.align(h, s, ienv, jenv)
        _invariants(m, ienv, jenv)
        assert m["hmm_to"] - m["hmm_from"] >= h["M"] // 2


def _uses_md(m, node):
    """does the model's traceback leave match state `node` for the delete state after it?  (re-walked from the matrices)"""
    P = m["P"]
    AM, AI, AD, AN, AB = OA._fill(P)
    al = P.allowed
    i, k, st = m["ali_to"] - m["ienv"] + 1, m["hmm_to"], "M"
    while True:
        if st == "M":
            c = OA._m_cands(P, AM, AI, AD, AB, i, k)
            w = c.index(max(c))
            if w == 3:
                return False
            i, k, st = i - 1, k - 1, "MID"[w]
        elif st == "I":
            c = [AM[i - 1][k] if al[k][OA.MI] else OA.NINF, AI[i - 1][k] if al[k][OA.II] else OA.NINF]
            i, st = i - 1, "MI"[c.index(max(c))]
        else:
            c = [AM[i][k - 1] if al[k - 1][OA.MD] else OA.NINF, AD[i][k - 1] if al[k - 1][OA.DD] else OA.NINF]
            w = c.index(max(c))
            if w == 0 and k - 1 == node:
                return True
            k, st = k - 1, "MD"[w]


def test_zero_transition_is_never_used(t_hmm_text):
    sub = EC._its2(t_hmm_text, 2, 2)
    closed = G.parse_hmms(EC._without_match_to_delete(sub, 17))
    barely = G.parse_hmms(EC._without_match_to_delete(sub, 17, "30.00000"))
    plain = G.parse_hmms(sub)
    cons = synth.consensus_motifs(sub, "")
    used_plain = 0
    for hc, hb, hp, c in zip(closed, barely, plain, cons):
        assert hc["t"][17][OA.MD] == 0.0 and hb["t"][17][OA.MD] > 0.0
        # the consensus without node 18's residue: the best path deletes node 18, out of match state 17 where it may
        s = "ACGTACGTAC" + c[:17] + c[18:] + "TTGACCATGA"
        for h in (hc, hb, hp):
            m = OA.align(h, s, 11, 10 + len(c) - 1)
            m["ienv"] = 11
            _invariants(m, 11, 10 + len(c) - 1)
            P = m["P"]
            assert P.allowed[17][OA.MD] == (h is not hc)
            u = _uses_md(m, 17)
            if h is hc:
                assert not u
            elif h is hp:
                used_plain += u
    assert used_plain > 0          # the deletion does go through M17 -> D18 where the profile allows it


@pytest.mark.parametrize("name", OC.NAMES)
def test_invariants_and_skip_cap(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads):
    hmm, seqs, kw = OC.inputs(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1])
    rows = OC.oracle_rows(hmm, seqs, kw)
    assert rows
    if name.startswith("lanes"):
        assert len(rows) == int(name[5:])
    ms = OC.models(hmm, seqs, rows)
    hm = G.parse_hmms(hmm)
    skipped = 0
    for (p, s, ienv, jenv), m in zip(rows, ms):
        assert 1 <= m["hmm_from"] <= m["hmm_to"] <= hm[p]["M"]
        assert ienv <= m["ali_from"] <= m["ali_to"] <= jenv
        assert 0.0 < m["acc"] <= 1.0 + 1e-12
        assert abs(m["own"] - m["oasc"]) <= 1e-12 * max(1.0, m["oasc"])                # constrained(own coordinates) == oasc
        skipped += not m["margin"] > 2.0 * OA.eps(m["Ld"], m["M"], m["oasc"])
    print("[%s] rows=%d skipped=%d" % (name, len(rows), skipped))
    assert skipped <= OC.SKIP_CAP * len(rows), (skipped, len(rows))
