"""tests/cigar_exact.py -- the model the engine's uc.txt alignments (itsx_align_clusters, csrc/k_cigar.hip) are held to -- against
tests/align_exact.py: the path its rule picks scores the optimal (score, matches, counted columns) for every (query strand, target)
pair the clustering model aligns on the threshold / ties / rows5 groups and the walks of tests/cluster_edges.py; its grammar; and the
C ABI's new entries (header, bindings, version)."""
import os
import re
from concurrent.futures import ProcessPoolExecutor

import pytest

import cigar_exact as X
import cluster_edges as CE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("threshold", "ties", "rows5")


def _path_of(pair):
    q, t = pair
    c = X.traceback(q, t)
    return c, X.rescore(q, t, c)


@pytest.fixture(scope="module")
def aligned_pairs():
    """{(query strand, target): align_exact's triple} of every alignment the clustering model makes on the groups and the walks"""
    keys = [k for k in CE.keys() if k[1] in GROUPS or k[0] == "walk"]
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        _, pairs = CE.expected_all(keys, pool)
        todo = sorted(pairs)
        paths = dict(zip(todo, pool.map(_path_of, todo, chunksize=4)))
    return pairs, paths


def test_the_rule_s_path_is_optimal(aligned_pairs):
    pairs, paths = aligned_pairs
    assert len(pairs) > 400
    kinds = set()
    for (q, t), want in pairs.items():
        cigar, got = paths[(q, t)]
        assert got == tuple(want), (cigar, got, want, len(q), len(t))
        X.parse(cigar)
        kinds |= set(re.sub("[0-9]", "", cigar))
    assert kinds == set("MID=")


def test_terminal_by_position_not_by_rank():
    """an I run at query position 0 followed directly by a D run: the first is terminal, the second interior"""
    q, t = "ACGTACGT", "TTACGTACGT"
    assert X.rescore(q, t, "2I8M") == (16 - 4, 8, 8)
    assert X.rescore("GG" + q, "TT" + q, "2I2D8M") == (16 - 4 - 24, 8, 10)
    assert X.rescore("GG" + q, "TT" + q, "2D2I8M") == (16 - 4 - 24, 8, 10)       # the D run lies at centroid position 0
    assert X.rescore(q + "GG", q + "TT", "8M2D2I") == (16 - 24 - 4, 8, 10)       # D at centroid position 8 of 10: interior; I at query position 10: terminal
    assert X.rescore(q, q, "=") == (16, 8, 8) == X.rescore(q, q, "8M")
    assert X.rescore("ACGN", "ACGR", "4M") == (6, 4, 4) and X.rescore("ACGY", "ACGR", "4M") == (6, 3, 4)
    for bad in ("7M", "9M", "8M2I", "2D8M"):
        with pytest.raises(ValueError):
            X.rescore(q, q, bad)
    with pytest.raises(ValueError):
        X.rescore(q, t, "=")


def test_grammar():
    for bad in ("0M", "1M", "3M2M", "=5M", "", "5M=", "M3", "03M", "3X", "3m", "*", "2M 2I"):
        with pytest.raises(ValueError):
            X.parse(bad)
    assert X.parse("=") == [("=", 0)]
    assert X.parse("M") == [("M", 1)] and X.parse("12MI3DM") == [("M", 12), ("I", 1), ("D", 3), ("M", 1)]
    assert X.parse("2I2D") == [("I", 2), ("D", 2)]


def test_traceback_spells_the_rule():
    """small cases whose optimal paths tie: diagonal first, then the gap in the query, then the gap in the centroid; gaps extend"""
    f = "ACGTTGCAAGCTTACG" * 3
    # a deletion inside a homopolymer: every placement of the gap scores the same; walking back the diagonal is taken while it can
    assert X.traceback(f + "AAAA" + f, f + "AAAAA" + f) == "48MI52M"
    assert X.traceback(f + "AAAAA" + f, f + "AAAA" + f) == "48MD52M"
    assert X.traceback(f, f.lower().replace("t", "u")) == "="
    assert X.traceback(f[5:], f) == "5I43M" and X.traceback(f, f[:-7]) == "41M7D"


def test_abi_declares_the_new_entries():
    from itsxpress_amd import _lib
    header = open(os.path.join(ROOT, "include", "itsx_hip.h")).read()
    assert re.search(r"int itsx_align_clusters\(itsx_ctx \*ctx, int64_t \*n_aligned, float \*ms_kernels\);", header)
    assert re.search(r"int itsx_get_cluster_cigars\(const itsx_ctx \*ctx, int64_t \*offs[^,]*, char \*text\);", header)
    assert {"itsx_align_clusters", "itsx_get_cluster_cigars"} <= set(_lib.EXPORTS)
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6
    L = _lib.lib()
    assert L.itsx_abi_version() == 6
    for name in ("itsx_align_clusters", "itsx_get_cluster_cigars"):
        assert getattr(L, name).argtypes is not None
