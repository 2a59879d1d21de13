"""The CPU oracle against the independent float64 statement (tests/hmm_generic.py) on every case of tests/edge_cases.py, and the
statement's fast forms against its node-by-node definition.  No GPU needed."""
import math
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import edge_cases
import generic_check as GC
import hmm_generic as G
import orc


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(GC.pool_size()) as ex:
        yield ex


def test_fast_forms_equal_the_definition(mini_hmm_text, t_hmm_text):
    """forward (multihit; unihit at another target length), MSV, bias filter, region decoding and domain scores of the vectorised
    forms == the node-by-node definition to 1e-9 nats: 56 random (profile, read) pairs over M = 11, 25, 45, 46, a '*' and a 1e-13
    M -> D, every IUPAC symbol, reads shorter than the model"""
    rng = np.random.default_rng(5)
    mini = edge_cases._blocks(mini_hmm_text)
    b45 = next(b for b in mini if "LENG  45" in b)
    sub = edge_cases._its2(t_hmm_text, 1, 1)
    text = "".join(b for b in mini if "LENG  11" in b or "LENG  25" in b) + b45 + edge_cases._stretch(b45, 46) \
        + edge_cases._without_match_to_delete(sub, 17) + edge_cases._without_match_to_delete(sub, 17, "30.00000")
    hm = G.parse_hmms(text)
    assert sorted({h["M"] for h in hm}) == [11, 25, 45, 46] and any(h["M"] > 17 and h["t"][17][2] == 0.0 for h in hm) \
        and any(h["M"] > 17 and abs(h["t"][17][2] - math.exp(-30.0)) < 1e-20 for h in hm)
    cons = [c for c in __import__("synth").consensus_motifs(text, "")]
    soup = "ACGTURYKMSWBDHVNacgtn"
    n = 0
    for j in range(56):
        h = hm[j % len(hm)]
        c = cons[j % len(cons)]
        kind = j % 4
        if kind == 0:
            s = "".join(rng.choice(list("ACGT"), int(rng.integers(5, h["M"]))))          # shorter than the model
        elif kind == 1:
            s = "".join(rng.choice(list(soup), int(rng.integers(30, 90))))              # every IUPAC symbol, any case
        else:
            s = "".join(rng.choice(list("ACGT"), int(rng.integers(10, 50)))) + c + "".join(rng.choice(list("ACGTN"), int(rng.integers(5, 40))))
        seqs = [s, s[: max(1, len(s) // 2)]]
        fb = G.forward_nats_batch(h, seqs)
        ub = G.forward_nats_batch(h, seqs, L_model=3 * len(s), unihit=True)
        mb = G.msv_nats_batch(h, seqs)
        bb = G.bias_filter_nats_batch(h, seqs)
        for k, q in enumerate(seqs):
            assert abs(fb[k] - G.forward_nats(h, q)) < 1e-9
            assert abs(ub[k] - G.forward_nats(h, q, L_model=3 * len(s), unihit=True)) < 1e-9
            assert abs(mb[k] - G.msv_nats(h, q)) < 1e-9
            assert abs(bb[k] - G.bias_filter_nats(h, q)) < 1e-9
        regs, info = G.decode_regions_fast(h, s, tol=2e-3)
        assert regs == G.decode_regions(h, s) and abs(info["total"] - fb[0]) < 1e-9
        for i1, i2 in regs + [(1, len(s)), (max(1, len(s) // 3), len(s))]:
            a, b = G.domain_bits_fast(h, s, i1, i2), G.domain_bits(h, s, i1, i2)
            assert np.allclose(a, b, rtol=0, atol=1e-9), (a, b)
            n += 1
    assert n >= 100


@pytest.mark.parametrize("name", list(edge_cases.CASES))
def test_oracle_agrees_with_float64(name, pool, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads):
    hmm, seqs, edge = edge_cases.case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1], scale=0.5)
    hs = orc.HmmSet(text=hmm)
    hm = G.parse_hmms(hmm)
    assert [h["M"] for h in hm] == list(hs.M)
    codes, o = orc.digitize(seqs)
    res = orc.SearchResult(hs, codes, o, keep_trace=2, threads=8)
    assert len(res.trace) == hs.n * len(seqs)
    ens = GC.ensemble_models(hs, hm, seqs, res.trace, "seq", pool)
    rep, rows = GC.check(name, hm, seqs, res.trace, res.domains, "seq", pool, sample=None if edge else 40, seed=7, ens=ens)
    assert rep.unstated == 0
    if name == "multidomain":
        assert res.counts["multidomain"] > 0 and "ens_domcorrection" in rep.worst      # the case reaches the ensemble stage
    # the oracle's per-read winners == ItsPosition fed a float64 domain table
    names = ["r%d" % i for i in range(len(seqs))]
    for left, right in (("3_", "4_"), ("1_", "2_")):
        want, shaky = GC.winners(rows, names, hs.names, left, right)
        st, sp, tl, ind = res.positions(left, right)
        for s, w in want.items():
            got = (int(st[s]), int(sp[s]), int(tl[s]))
            if got != w:
                if s in shaky:
                    rep.near.append(("winner", "read %d %s%s" % (s, left, right), 0.0))
                else:
                    rep.fail.append("%s: read %d (%s, %s): oracle %s, float64 ItsPosition %s" % (name, s, left, right, got, w))
    print(rep.finish())
