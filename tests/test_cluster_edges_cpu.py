"""CPU tests for the clustering edges (tests/cluster_edges.py): the exact numpy model (tests/align_exact.py) is held to py_align, and
the oracle's packed alignment and its clustering walk are held to the model on every case of the catalogue, the 50 000-base
pairs included.  Every comparison is exact equality."""
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import align_exact
import cluster_edges as CE
import orc
from test_cluster_cpu import py_align

_EXP = {}


@pytest.fixture(scope="module")
def expectations():
    """{key: (order, rep_of, strand, pct_id)} and {(query strand, target): (score, matches, columns)} by the model, computed once"""
    if not _EXP:
        with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            _EXP["cases"], _EXP["pairs"] = CE.expected_all(CE.keys(), pool)
    return _EXP["cases"], _EXP["pairs"]


def _edited(rng, a, alphabet, n_edits):
    b = list(a)
    for _ in range(n_edits):
        k = int(rng.integers(0, len(b)))
        op = rng.random()
        if op < 0.3 and len(b) > 2:
            del b[k]
        elif op < 0.6:
            b.insert(k, str(rng.choice(alphabet)))
        else:
            b[k] = str(rng.choice(alphabet))
    return "".join(b)


def test_model_equals_the_tuple_dp():
    rng = np.random.default_rng(5)
    pairs = []
    for k in range(260):
        alphabet = list("ACGT") if k % 3 else list("ACGTUNRYMKSWHBVD")
        a = "".join(rng.choice(alphabet, int(rng.integers(1, 55 if k % 2 else 61))))
        if k % 2:
            pairs.append((a, _edited(rng, a, alphabet, int(rng.integers(0, 7)))))
        else:
            pairs.append((a, "".join(rng.choice(alphabet, int(rng.integers(1, 61))))))
    u = "".join(rng.choice(list("ACGT"), 40))
    # constructed: repeats whose gap can sit anywhere, gaps at the very ends, one symbol, reads contained in one another
    pairs += [("CA" * 12, "CA" * 10), ("A" * 20, "A" * 13), ("ACG" * 9, "ACG" * 4 + "ATG" + "ACG" * 4), ("AAAAACCCCC", "AAAACCCCCC"), ("A", "A"), ("A", "C"), ("A", "N"),
              ("A", u), (u, u[5:]), (u, u[:-5]), (u, u[7:29]), (u, u[1:]), (u, u[:1] + u[2:]), (u, u[:-2] + u[-1:]), (u, u[:20] + u[29:]), (u, "N" * 40),
              (u, u[:10] + "N" * 6 + u[20:]), (u.replace("T", "U"), u), ("ACGT" * 6, "CGTA" * 6), (u[:20] + "RYMK" + u[24:], u), ("G" * 12, "G" * 5 + "T" + "G" * 7),
              (u + "ACGTACGT", "TTGACA" + u), ("N" * 9, "ACGTACGTA"), ("RRRRYYYY", "AGAGCTCT"), ("RRRRYYYY", "CTCTAGAG"), ("W" * 8, "S" * 8),
              (u[:30], u[10:]), (u, u[:12] + "G" + u[12:]), (u, u[:12] + "GATTACA" + u[12:]), (u[:8], u), (u[-8:], u), (u[16:24], u)]
    pairs += [(a, b[::-1]) for a, b in pairs[260:275]]
    assert len(pairs) >= 300 and all(len(a) <= 60 and len(b) <= 60 for a, b in pairs)
    for a, b in pairs:
        want = py_align(a, b)
        assert py_align(b, a) == want, (a, b)               # the definition is symmetric
        for q, t in ((a, b), (b, a)):
            assert align_exact.dp(q, t) == want, (q, t)
            assert align_exact.align(q, t) == want, (q, t)


def test_oracle_alignment_equals_the_model(expectations):
    """the packed int64 cell (score << 40, matches << 20, -columns) against three separate integers, on every pair the walks align"""
    _, pairs = expectations
    assert len(pairs) > 400 and max(max(len(q), len(t)) for q, t in pairs) == 50000
    for (q, t), want in pairs.items():
        if orc.align_identity(q, t) != want:
            where = [(k[1], CE.get(k).name) for k in CE.keys() if t in CE.get(k).reads and (q in CE.get(k).reads or CE.rc(q) in CE.get(k).reads)]
            assert orc.align_identity(q, t) == want, (where, len(q), len(t))


def _check(key, exp):
    case = CE.get(key)
    order, rep_of, strand, pct = exp
    codes, off = orc.digitize(case.reads)
    o = orc.cluster(codes, off, case.names, case.cid)
    what = "%s %s" % (key[1], case.name)
    assert o["order"].tolist() == order, what
    assert o["rep_of"].tolist() == rep_of, what
    assert o["strand"].tolist() == strand, what
    assert o["pct_id"].tolist() == pct, what
    # where the construction fixes the last read's fate, the model must say the same
    last = len(case.reads) - 1
    if case.joins == "dropped":
        assert rep_of[last] == -1, what
    elif case.joins is not None:
        assert (rep_of[last] not in (last, -1)) == case.joins, (what, rep_of, pct)


@pytest.mark.parametrize("group", list(CE.PAIRS))
def test_oracle_clusters_every_pair_like_the_model(group, expectations):
    cases, _ = expectations
    ks = [k for k in cases if k[0] == "pair" and k[1] == group]
    assert len(ks) == len(CE.PAIRS[group]())
    for k in ks:
        _check(k, cases[k])


@pytest.mark.parametrize("walk", list(CE.WALKS))
def test_oracle_walks_like_the_model(walk, expectations):
    cases, _ = expectations
    _check(("walk", walk, 0), cases[("walk", walk, 0)])


def test_the_cases_are_the_edges_they_are_named_for(expectations):
    cases, _ = expectations
    rep = lambda kind, name, k=0: cases[(kind, name, k)][1]
    pct = lambda kind, name, k=0: cases[(kind, name, k)][3]
    name_of = lambda g: [c.name for c in CE.PAIRS[g]()]
    # 11 shared words: no candidate although the alignment would pass; 12: a hit
    assert rep("walk", "words_11") == [0, 1] and rep("walk", "words_12") == [0, 0] and pct("walk", "words_12")[1] == 99.5
    assert rep("walk", "few_words") == [0, 0] and rep("walk", "no_words") == [0, 1, 2, 3, 4]
    # 31 rejections and the acceptor is still tried; 32 and the walk has ended
    assert rep("walk", "acceptor_rank_32") == list(range(32)) + [31] and rep("walk", "acceptor_rank_33") == list(range(34))
    assert rep("walk", "tie_length") == [0, 1, 1, 1] and rep("walk", "tie_position") == [0, 1, 0, 0]
    assert rep("walk", "plus_beside_minus") == [0, 1, 0] and cases[("walk", "plus_beside_minus", 0)][2] == [1, 1, 1]
    assert rep("walk", "minus_beats_plus") == [0, 1, 1] and cases[("walk", "minus_beats_plus", 0)][2] == [1, 1, -1]
    # exactly representable identities at the threshold are accepted
    th = name_of("threshold")
    for tag, want in (("id0.99_L100_K_subs", 99.0), ("id0.995_L200_K_subs", 99.5), ("id0.97_L100_K_subs", 97.0)):
        assert pct("pair", "threshold", th.index(tag))[1] == want
    lim = name_of("limits")
    assert rep("pair", "limits", lim.index("t50001_dropped_q300")) == [-1, 1] and rep("pair", "limits", lim.index("t50000_q300")) == [0, 0]
    # a short read inside a long centroid is a 100 % hit
    con = name_of("contained")
    assert all(pct("pair", "contained", k)[1] == 100.0 for k, n in enumerate(con) if "_exact_" in n) and sum("_exact_" in n for n in con) == 9
