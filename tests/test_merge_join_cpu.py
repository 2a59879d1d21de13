"""Joining the read pairs that do not overlap (Engine.merge_join; include/itsx_hip.h: itsx_set_merge_join), the part that
needs no GPU: the ABI names, the plain-Python model (tests/join_exact.py) against hand-written literals, the reference's paired
arithmetic on joined reads, and what the CPU oracle finds on the paired fixture cut to 150 bases a mate -- the counts the
engine tests (tests/test_gpu_merge_join.py) then aim at."""
import collections
import os
import re

import numpy as np
import pytest

import join_cases
import join_exact as J
import orc
from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_set_merge_join", "itsx_merge_join_info", "itsx_merge_buffers_join"]


def test_abi_names_the_new_symbols_and_keeps_its_version():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert len(L.itsx_set_merge_join.argtypes) == 2 and len(L.itsx_merge_join_info.argtypes) == 4
    assert len(L.itsx_merge_buffers_join.argtypes) == len(L.itsx_merge_buffers.argtypes) + 1
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6 and L.itsx_abi_version() == 6      # additive
    m = re.search(r"int\s+itsx_merge_buffers_join\s*\(([^)]*)\)", header)
    assert m and m.group(1).split(",")[-1].strip() == "int8_t *joined"
    assert "PARITY UNPINNED" in header[header.index("joining the pairs that do not overlap"):header.index("int itsx_set_merge_join")]


def test_the_python_layers_name_the_setting():
    from itsxpress_amd import Engine
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.multi import MultiEngine
    from itsxpress_amd.stream import StreamEngine
    for cls in (Engine, SampleBatch, MultiEngine, StreamEngine):
        assert isinstance(getattr(cls, "merge_join"), property), cls
    assert callable(Engine.merge_join_info)
    import inspect
    assert inspect.signature(Engine.merge_pairs).parameters["join"].default is False
    from itsxpress_amd.SeqSample import SeqSamplePairedNotInterleaved
    assert list(inspect.signature(SeqSamplePairedNotInterleaved._merge_reads).parameters) == ["self", "threads", "stagger"]


def test_model_against_literals():
    assert J.upper("acgtnurykmswbdhv-*Az") == "ACGTNURYKMSWBDHV-*AZ"
    assert J.revcomp_as_merged("ACGT") == "ACGT" and J.revcomp_as_merged("AACG") == "CGTT"
    assert J.revcomp_as_merged("acgu") == "ACGT"                       # U complements to A
    assert J.revcomp_as_merged("ArCnGU-T") == "ANACNGNT"               # outside ACGTU: N
    assert J.join_pair("ACg", "!5~", "TTGn", "ABCD") == ("ACG" + "NNNNNNNN" + "NCAA", "!5~" + "IIIIIIII" + "DCBA")
    assert J.join_pair("A", "I", "c", "#") == ("ANNNNNNNNG", "IIIIIIIII#")
    assert J.joined_len("ACG", "TTGN") == 3 + 8 + 4 == len(J.join_pair("ACG", "III", "TTGN", "IIII")[0])
    assert [J.is_joined(k) for k in range(9)] == [False, True, False, True, False, True, False, False, False]
    assert [J.is_joined(n) for n in orc.MERGE_REASONS] == [False, True, False, True, False, True, False, False, False]
    assert J.read_of_pair(0, ("AC", "II"), "A", "I", "C", "I") == ("AC", "II")
    assert J.read_of_pair(3, None, "A", "I", "C", "I") == ("ANNNNNNNNG", "IIIIIIIIII")
    for k in (2, 4, 6, 7, 8):
        assert J.read_of_pair(k, None, "A", "I", "C", "I") is None
    assert J.fastq_text([("x", "AC", "I!"), ("y/1", "G", "~")]) == "@x\nAC\n+\nI!\n@y/1\nG\n+\n~\n"
    # R1 = ACGTAC, R2 as in its file = TTGCAT (revcomp ATGCAA): tlen 20; start 2 inside R1, stop 17 inside the R2 part
    (a, aq), (b, bq) = J.paired_slices("ACGTAC", "abcdef", "TTGCAT", "uvwxyz", 2, 17, 20)
    assert (a, aq, b, bq) == ("GTAC", "cdef", "CAT", "xyz")
    o1, o2 = J.trimmed_pair_files([("@p/1 c", "ACGTAC", "abcdef", "@p/2", "TTGCAT", "uvwxyz")] * 4, [(2, 17, 20), None, (-1, 17, 20), (9, 9, 20)])
    assert o1 == "@p/1 c\nGTAC\n+\ncdef\n" and o2 == "@p/2\nCAT\n+\nxyz\n"


def test_paired_arithmetic_cuts_each_mate_of_a_joined_read_at_its_own_anchor():
    """Dedup._get_paired_seq_generator: R1[start:stop], R2[tlen - stop : tlen - start].  On a joined read tlen = L1 + 8 + L2; with
    start inside R1 and stop inside the R2 part those are R1[start:] and R2[tlen - stop:], and R2's slice is the part of the joined
    read from the pad to `stop`, read back on R2's strand."""
    rng = np.random.default_rng(150)
    for _ in range(2000):
        L1, L2 = int(rng.integers(1, 320)), int(rng.integers(1, 320))
        s1 = "".join("ACGT"[k] for k in rng.integers(0, 4, L1))
        s2 = "".join("ACGT"[k] for k in rng.integers(0, 4, L2))
        q1 = "".join(chr(k) for k in rng.integers(33, 127, L1))
        q2 = "".join(chr(k) for k in rng.integers(33, 127, L2))
        bases, quals = J.join_pair(s1, q1, s2, q2)
        tlen = L1 + J.PAD + L2
        assert len(bases) == len(quals) == tlen
        start = int(rng.integers(0, L1 + 1))
        stop = int(rng.integers(L1 + J.PAD, tlen + 1))
        (a, aq), (b, bq) = J.paired_slices(s1, q1, s2, q2, start, stop, tlen)
        assert a == s1[start:] and aq == q1[start:]
        assert b == s2[tlen - stop:] and bq == q2[tlen - stop:]
        assert J.revcomp_as_merged(b) == bases[L1 + J.PAD:stop] and bq[::-1] == quals[L1 + J.PAD:stop]
        assert a == bases[start:L1]


@pytest.fixture(scope="module")
def its2_hmms(t_hmm_text):
    from bench import its2_profiles
    return orc.HmmSet(text=its2_profiles(t_hmm_text))


def _oracle_reads(pairs):
    """the oracle's verdict and the model's read for every pair: (counts by verdict, [(verdict, L1, bases)] of the reads in pair order)"""
    counts, reads = collections.Counter(), []
    for t1, s1, q1, t2, s2, q2 in pairs:
        o = orc.merge_pair(J.upper(s1), q1, J.upper(s2), q2)
        counts[o[0]] += 1
        rec = J.read_of_pair(o[0], (o[1], o[2]), s1, q1, s2, q2)
        if rec is not None:
            reads.append((o[0], len(s1), rec[0]))
    return counts, reads


def _coords(hs, reads):
    codes, offs = orc.digitize([r[2] for r in reads])
    res = orc.SearchResult(hs, codes, offs, T=10.0, F1=1e-6, F2=1e-6, F3=1e-6, threads=min(8, os.cpu_count() or 1))
    return res.positions("3_", "4_")[:2]


def test_oracle_on_the_fixture_with_every_pair_cut_to_150(its2_hmms):
    pairs = join_cases.all_cut()
    counts, reads = _oracle_reads(pairs)
    assert len(pairs) == 250 and dict(counts) == {"nokmers": 163, "minscore": 87}      # nothing merges, everything is joined
    assert len(reads) == 250 and all(L1 == 150 and len(b) == 308 for _, L1, b in reads)
    start, stop = _coords(its2_hmms, reads)
    ok = (start >= 0) & (stop >= 0) & (start < stop) & (start < 150) & (stop > 158)
    assert int(ok.sum()) == 244
    assert int(((start >= 0) & (stop >= 0) & (start < stop)).sum()) == 244                 # (none lies on one side of the pad)


def test_oracle_on_the_fixture_with_the_odd_pairs_cut_to_150(its2_hmms):
    pairs = join_cases.odd_cut()
    counts, reads = _oracle_reads(pairs)
    assert dict(counts) == {"ok": 121, "nokmers": 82, "minscore": 44, "maxee": 3}
    assert len(reads) == 247 and sum(v != "ok" for v, _, _ in reads) == 126
    start, stop = _coords(its2_hmms, reads)
    both = (start >= 0) & (stop >= 0)
    joined = np.array([v != "ok" for v, _, _ in reads])
    L1 = np.array([l for _, l, _ in reads])
    assert int((both & joined).sum()) == 121 and int((both & ~joined).sum()) == 121 == int((~joined).sum())
    assert bool(np.all((start < L1)[both & joined] & (stop > L1 + J.PAD)[both & joined]))   # every one of them spans the pad
    assert bool(np.all((start < stop)[both]))
