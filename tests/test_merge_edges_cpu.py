"""The paired-end merge oracle (oracle/orc_merge.c) held to the independent high-precision model and its catalogue of decision
edges (tests/merge_exact.py): reason, merged bases and qualities, shift and mismatches equal, the score within the model's bound
of the exact score.  The oracle's and the engine's host tables are held to the model's over all 94 x 94 entries."""
import numpy as np
import pytest

import merge_exact as mx
import orc

GROUP_NAMES = [g for g, _ in mx.GROUPS]


def check_against_model(case, res, got):
    """got = (reason, seq, qual, score, shift[, diffs]) of the oracle or the engine for `case`; res = the model's Result"""
    assert got[0] == res.reason, (case.name, got[0], res.reason)
    assert got[4] == res.shift, (case.name, got[4], res.shift)
    if len(got) > 5:
        assert got[5] == res.diffs, (case.name, got[5], res.diffs)
    if res.reason == "ok":
        assert (got[1], got[2]) == (res.seq, res.qual), case.name
        assert got[1] == got[1].upper()
    err, bound = abs(mx.F(float(got[3])) - res.score), mx.score_bound(res)
    assert err <= bound, (case.name, float(got[3]), float(res.score), float(err), float(bound))


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_oracle_equals_the_model_on_the_catalogue(group):
    cases = [(c, r) for c, r in mx.catalogue() if c.group == group]
    assert cases
    for c, res in cases:
        check_against_model(c, res, orc.merge_pair_ex(c.f, c.fq, c.r, c.rq, **c.kw))
        # the binding every other test uses gives the same answer
        assert orc.merge_pair(c.f, c.fq, c.r, c.rq, **c.kw) == orc.merge_pair_ex(c.f, c.fq, c.r, c.rq, **c.kw)[:5]


def test_oracle_equals_the_model_on_the_sweep():
    sw = mx.sweep()
    assert len(sw) == 300
    thin = [c.name for c, r in sw if mx.thin(r)]
    assert len(thin) <= 0.01 * len(sw), thin                    # a condition on the seed, not a measurement
    for c, res in sw:
        if c.name not in thin:
            check_against_model(c, res, orc.merge_pair_ex(c.f, c.fq, c.r, c.rq, **c.kw))
    # the sweep does reach the decisions: every reason but `empty` and `minovlen` occurs
    assert {r.reason for _, r in sw} >= {"ok", "nokmers", "repeat", "minscore", "maxdiffs", "staggered", "maxee"}


def test_the_catalogues_own_conditions():
    cat = mx.catalogue()
    assert {c.group for c, _ in cat} == set(GROUP_NAMES)
    for c, res in cat:
        assert not mx.thin(res), c.name
    by = {c.name: (c, r) for c, r in cat}
    # exact ties: every candidate scores 0.0, the largest shift is reported; candidates in different lanes and in the same lane
    for name in ("ties_period7_other_lanes", "ties_period64_same_lane", "ties_period8_both"):
        c, res = by[name]
        assert len(res.candidates) >= 3 and all(x.score == 0 for x in res.candidates)
        assert res.score == 0 and res.shift == max(x.shift for x in res.candidates)
        idx = [len(c.f) - 1 - x.shift for x in res.candidates]
        lanes = [i % 64 for i in idx]
        if "other" in name or "both" in name:
            assert len(set(lanes)) > 1
        if "same" in name:
            assert len(set(lanes)) == 1
        if "both" in name:
            assert any(j - i == 64 for i in idx for j in idx)
    # lane striping: the reported diagonal sits where the name says
    for c, res in cat:
        if c.group == "lanes":
            ndiag, idx = int(c.name.split("_")[1]), int(c.name.split("idx")[1])
            assert len(c.f) + len(c.r) - 1 == ndiag and len(c.f) - 1 - res.shift == idx, c.name
    assert {int(c.name.split("_")[1]) for c, _ in cat if c.group == "lanes"} >= {63, 64, 65, 128, 129}
    # the straddles stand where they should
    for name, lo, hi in (("score_below_16", 15.95, 16), ("score_above_16", 16, 16.05)):
        assert lo < by[name][1].score < hi
    for name, lo, hi in (("second_below_16", 15.95, 16), ("second_above_16", 16, 16.05)):
        assert lo < sorted(x.score for x in by[name][1].candidates)[-2] < hi
    assert by["drop_above_16"][1].candidates[0].dropped and by["drop_above_16"][1].candidates[0].raw > 16
    assert not by["drop_below_16"][1].candidates[0].dropped
    assert by["diffs_40_of_40"][1].diffs == 40 and by["diffs_41_of_40"][1].diffs == 41
    for m in (2.0, 0.5):
        assert m - 0.001 < by["maxee_%s_under" % m][1].ee < m < by["maxee_%s_over" % m][1].ee < m + 0.001
    assert by["overlap_8"][1].score < 16 < by["overlap_9"][1].score
    # every pair of quality bytes stands in an overlap of the posterior cases, agreeing; disagreeing where a merged read can show it
    same, diff = set(), set()
    for c, res in cat:
        if c.name.startswith("posterior_") and c.name[10:].isdigit():
            rc, rcq = mx.revcomp(c.r), c.rq[::-1]
            for p in range(len(c.f)):
                (same if c.f[p] == rc[p] else diff).add((ord(c.fq[p]), ord(rcq[p])))
    R = range(33, 127)
    assert same == {(a, b) for a in R for b in R}
    assert diff == {(a, b) for a in R for b in R if float(mx.mism_term(a, b)) > -15.9} and len(diff) > 4000
    assert all((a, a) in diff for a in range(33, 70))           # equal qualities on a disagreement: the reverse read's base
    assert max(len(c.f) + len(c.r) for c, _ in cat) <= 12000
    for name, f, fq, r, rq in mx.format_cases():
        with pytest.raises(mx.FormatError):
            mx.merge(f, fq, r, rq)
    assert len(mx.short_cases()) >= 40


def test_lower_case_is_read_as_upper_case():
    for c, res in mx.catalogue():
        if c.group == "lower":
            up = orc.merge_pair(c.f.upper(), c.fq, c.r.upper(), c.rq)
            assert orc.merge_pair(c.f, c.fq, c.r, c.rq) == up and up[0] == "ok" and up[1] == res.seq


def _ulps(got, exact):
    return float(abs(mx.F(float(got)) - exact) / mx.F(float(np.spacing(abs(float(exact))))))


def test_tables_equal_the_models():
    import ctypes as C
    from itsxpress_amd import _lib
    T = mx.tables()
    eng = [np.zeros(128), np.zeros((128, 128)), np.zeros((128, 128)), np.zeros((128, 128), np.uint8), np.zeros((128, 128), np.uint8)]
    assert _lib.lib().itsx_merge_tables(*[C.c_void_p(x.ctypes.data) for x in eng]) == 0
    near_half = []
    for who, (q2p, match, mism, qsame, qdiff) in (("oracle", orc.merge_tables()), ("engine", eng)):
        for a in range(94):
            for b in range(94):
                for name, tab, ex in (("match", match, T["match"]), ("mismatch", mism, T["mism"])):
                    got, exact = tab[a + 33][b + 33], ex[a][b]
                    if a < 2 or b < 2:                          # an error of 3/4 on either side: both probabilities are exactly 1/4
                        assert abs(exact) < 1e-60 and got == 0.0, (who, name, a, b, got)
                    else:
                        assert _ulps(got, exact) <= 4, (who, name, a, b, got, float(exact))
                for name, tab, ex, half in (("qsame", qsame, T["qsame"], T["same_half"]), ("qdiff", qdiff, T["qdiff"], T["diff_half"])):
                    if half[a][b] < 1e-9:
                        near_half.append((name, a, b))
                        continue
                    assert tab[a + 33][b + 33] == ex[a][b], (who, name, a, b)
    assert near_half == []                                      # no posterior stands within 1e-9 of a rounding boundary
