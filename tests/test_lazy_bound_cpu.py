"""The lazy domain stage's bound (csrc/k_lazy.hip) in float64, no GPU: the inequality itself, with no margin, on
every case of tests/lazy_bound_cases.py against the independent model of tests/hmm_generic.py, and k_lazy_bound's conversion of a
bound to biased %.1f tenths, restated in numpy (lazy_bound_cases.b10_model) and held to what Python's "%.1f" prints."""
import math
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import generic_check as GC
import hmm_generic as G
import lazy_bound_cases as LB

BIAS = 1 << 23                                  # LAZY_TENTHS_BIAS (csrc/k_api.h): the GPU test reads the engine's own


@pytest.fixture(scope="module")
def pool():
    with ProcessPoolExecutor(GC.pool_size()) as ex:
        yield ex


_SLACK = {}


@pytest.mark.parametrize("name", list(LB.CASES))
def test_every_envelope_obeys_the_bound_in_float64(name, pool, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads):
    """bits <= (fwdsc - nullsc) / ln 2 + C(n) for the whole-target envelope and every envelope the float64 region scan finds.  The
    catalogue's own cases check every (read, profile); the cases of tests/edge_cases.py, mostly random sequence, check the pairs
    whose float64 MSV score is within the byte filter's quantisation of passing (only pairs past that filter have a bound).
    Float64 rounding (far below 1e-9 bits) is the only allowance.  Prints the smallest slack."""
    c = LB.case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_reads[1])
    hm = G.parse_hmms(c.hmm)
    seqs = LB._uniq(c.seqs)
    tasks = []
    for p, h in enumerate(hm):
        if name in LB.OWN:
            keep = range(len(seqs))
        else:
            msv = G.msv_nats_batch(h, seqs)
            thr = GC.msv_threshold_bits(h) * LB.LN2
            keep = [i for i, s in enumerate(seqs) if msv[i] - GC.nullsc(len(s)) >= thr - GC.msv_limit(len(s), h["M"])]
        tasks += [((i, p), h, seqs[i]) for i in keep]
    assert tasks, "no pair of the case reaches the filter"
    tasks.sort(key=lambda t: -len(t[2]))
    worst, n_env, bad = (math.inf, None), 0, []
    for (i, p), rows in pool.map(LB.inequality_task, tasks, chunksize=1 if len(tasks) < 64 else 4):
        for ienv, jenv, bits, bound, slack in rows:
            n_env += 1
            what = "read %d (L %d) profile %d envelope %d-%d: bits %.6f bound %.6f" % (i, len(seqs[i]), p, ienv, jenv, bits, bound)
            if slack < worst[0]:
                worst = (slack, what)
            if not slack >= -1e-9:
                bad.append(what)
    assert n_env > 0
    print("[%s] pairs=%d envelopes=%d smallest slack %.4f bits at %s" % (name, len(tasks), n_env, worst[0], worst[1]))
    _SLACK[name] = worst
    assert not bad, "\n".join(bad[:20])


def test_smallest_slack_overall():
    """a finding, not a threshold: DESIGN.md 4b quotes it"""
    if not _SLACK:
        pytest.skip("runs after the cases")
    name = min(_SLACK, key=lambda k: _SLACK[k][0])
    print("smallest slack overall: %.4f bits, case %s, %s" % (_SLACK[name][0], name, _SLACK[name][1]))


def test_margin_and_c_of_n():
    """C(n) rises from 1.075 bits at n = 1 to 1 + (1 - 2 ln 1.5) / ln 2 = 1.273; the margin is 0.02 bits up to ~38 000 residues"""
    assert abs(LB.c_of_n(1) - (1.0 + (2.0 * math.log(8.0 / 9.0) + math.log(4.0 / 3.0)) / LB.LN2)) < 1e-15
    assert 1.07 < LB.c_of_n(1) < LB.c_of_n(11) < LB.c_of_n(440) < LB.c_of_n(65535) < 1.0 + (1.0 - 2.0 * math.log(1.5)) / LB.LN2 < 1.274
    assert LB.margin_bits(600) == 0.02 and LB.margin_bits(38000) == 0.02 and 0.0338 < LB.margin_bits(65535) < 0.0339


def _f32_at_or_below(x):
    f = np.float32(x)
    return f if float(f) <= x else np.nextafter(f, np.float32(-np.inf))


def test_b10_model_on_half_tenths():
    """hand-made bounds on a half tenth and one ulp to either side: half UP, the clamps at 1 and 2^24 - 1, NaN, +inf, -inf.  The
    bound is given through lazy_c with fb = nullsc = 0 (fb ln 2 has no exact float32), and once through fb - nullsc = 0."""
    z = np.float32(0.0)

    def one(c, fb=z):
        return int(LB.b10_model([fb], [z], [np.float32(c)], BIAS)[0])
    # the float32 values whose product with 10.0 is exactly m + 0.5 in float64
    for bits, want in ((0.25, 3), (0.75, 8), (1.25, 13), (3.75, 38), (-0.25, -2), (-1.75, -17), (-0.75, -7), (1024.25, 10243)):
        c = np.float32(bits)
        assert float(c) * 10.0 == want - 0.5
        assert one(c) == want + BIAS                                        # the half goes UP (rint would give the even neighbour)
        assert one(np.nextafter(c, np.float32(np.inf))) == want + BIAS
        assert one(np.nextafter(c, np.float32(-np.inf))) == want - 1 + BIAS
    assert int(LB.b10_model([np.float32(-7.5)], [np.float32(-7.5)], [np.float32(0.25)], BIAS)[0]) == 3 + BIAS
    # a decimal half tenth that float32 cannot hold: the float32 value decides
    for k in (-40.5, 0.5, 2.5, 12.5, 100.5):
        c = np.float32(k / 10.0)
        assert one(c) == math.floor(float(c) * 10.0 + 0.5) + BIAS
    # the clamps, at their edges (all exact in float32): 10 bits + 0.5 + bias = 3, 1, -2 -> 1; 2^24 - 3, 2^24 -> 2^24 - 1
    assert one(-838860.5) == 3 and one(-838860.75) == 1 and one(-838861.0) == 1 and one(-1e6) == 1 and one(-3e38) == 1
    assert one(838860.5) == LB.TENTHS_MAX - 2 and one(838860.75) == LB.TENTHS_MAX and one(1e6) == LB.TENTHS_MAX and one(3e38) == LB.TENTHS_MAX
    # no usable bound: always evaluated; -inf: the smallest bound of a pair (0 is "no pair here")
    assert one(1.0, np.float32(np.nan)) == LB.TENTHS_MAX and one(1.0, np.float32(np.inf)) == LB.TENTHS_MAX
    assert one(1.0, np.float32(-np.inf)) == 1
    assert one(0.0, np.float32(3.4e38)) == LB.TENTHS_MAX and one(0.0, np.float32(-3.4e38)) == 1


def test_b10_is_never_below_what_percent_1f_prints():
    """for any float32 score at or below the bound (in bits), the tenths "%.1f" prints + the bias <= b10: on the half tenths and
    their neighbours, and on a seeded sweep of bounds with the float32 values just below them"""
    rng = np.random.default_rng(6110)
    bounds = [m / 10.0 + 0.05 for m in range(-300, 3000, 7)] + [0.25, 0.75, -0.25, 1.25, 2.35, 2.45, 10.05, 99.95, 100.05]
    bounds += list(rng.uniform(-60.0, 400.0, 4000))
    bounds += [float(np.float32(b)) for b in bounds[:200]]
    z = np.float32(0.0)
    n = 0
    for b in bounds:
        c = np.float32(b)                                                   # the bound the kernel sees is made of float32 parts
        b10 = int(LB.b10_model([z], [z], [c], BIAS)[0])
        x = _f32_at_or_below(float(c))
        for _ in range(4):                                                  # the largest float32 scores not above the bound
            assert float(x) <= float(c)
            assert LB.printed_tenths(x) + BIAS <= b10, (b, float(x), "%.1f" % float(x), b10 - BIAS)
            n += 1
            x = np.nextafter(x, np.float32(-np.inf))
        for d in (0.04, 0.05, 0.06, 0.1, 0.15, 1.0):                        # and scores a tenth or so lower
            x = np.float32(float(c) - d)
            if float(x) <= float(c):
                assert LB.printed_tenths(x) + BIAS <= b10
    # bounds made the kernel's way, from a float32 score, nullsc and lazy_c: the float64 sum is not a float32
    for L in (1, 11, 46, 440, 20000, 65535):
        nsc, lc = np.float32(LB.nullsc(L)), np.float32(LB.c_of_n(L) + LB.margin_bits(L))
        for fb in rng.uniform(-40.0, 90.0, 300).astype(np.float32):
            bits = (float(fb) - float(nsc)) / 0.69314718055994529 + float(lc)
            b10 = int(LB.b10_model([fb], [nsc], [lc], BIAS)[0])
            x = _f32_at_or_below(bits)
            for _ in range(3):
                assert float(x) <= bits and LB.printed_tenths(x) + BIAS <= b10, (L, float(fb), float(x), b10 - BIAS)
                n += 1
                x = np.nextafter(x, np.float32(-np.inf))
    assert n > 10000
    assert LB.printed_tenths(np.float32(-0.04)) == 0 and LB.printed_tenths(np.float32(-0.06)) == -1 and LB.printed_tenths(np.float32(12.25)) == 122
