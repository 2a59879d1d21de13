"""CPU tests of the orientation oracle (oracle/orc_cluster.c: orc_orient, orc_orient_db_add) at its decision
edges: the C restatement is held to tests/orient_exact.py, an independent statement of the procedure on Python strings and sets.
Every case of the catalogue first shows its property on the MODEL's output (so a case that no longer hits its target fails), then
the oracle must equal the model on strand and both counts, with the DUST masking on and off.  Everything is an integer: exact."""
import numpy as np
import pytest

import orc
import orient_exact as M

ALL = M.CASE_NAMES + ("sweep",)
OFF_ONLY = ("distinct_words", "distinct_words_tandem")        # counted once only where DUST does not take the repeat away
ON_ONLY = ("distinct_words_masked",)


def _oracle(case):
    s, f, v = orc.orient(case.db, case.reads)
    return [(int(a), int(b), int(c)) for a, b, c in zip(s, f, v)]


def _same(got, exp, case):
    bad = [(i, case.reads[i][:60], g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert len(got) == len(exp) and not bad, (case.name, len(bad), bad[:5])


@pytest.mark.parametrize("name", ALL)
def test_case_shows_its_property_on_the_model(name):
    M.case(name).check(*M.outputs(name))


@pytest.mark.parametrize("name", [n for n in ALL if n not in OFF_ONLY])
def test_oracle_equals_the_model(name, monkeypatch):
    monkeypatch.delenv("ORC_QMASK", raising=False)
    case = M.case(name)
    assert True in case.modes
    case.check(*M.outputs(name))
    _same(_oracle(case), M.outputs(name)[0], case)


@pytest.mark.parametrize("name", [n for n in ALL if n not in ON_ONLY])
def test_oracle_equals_the_model_without_masking(name, monkeypatch):
    """ORC_QMASK=none against dust=False; the database bitmap is built under the same setting"""
    case = M.case(name)
    assert False in case.modes
    case.check(*M.outputs(name))
    monkeypatch.setenv("ORC_QMASK", "none")
    _same(_oracle(case), M.outputs(name)[1], case)


def test_catalogue_size():
    n_reads = sum(len(M.case(n).reads) for n in M.CASE_NAMES)
    assert len(M.CASE_NAMES) == 13 and n_reads > 2000 and len(M.sweep().reads) == M.SWEEP_READS
    assert len(M.case("rule_grid").reads) == M.GRID * M.GRID == 441
    for n in ALL:                                               # every case is compared under every setting it names
        assert M.case(n).modes == ((False,) if n in OFF_ONLY else (True,) if n in ON_ONLY else (True, False)), n


def test_reads_of_no_and_one_base_and_no_reads(monkeypatch):
    monkeypatch.delenv("ORC_QMASK", raising=False)
    p = M.pools()
    reads = ["", "A", p.word, "", "n", p.word[:11], ""]
    exp = M.orient(p.db, reads)
    assert exp == [(0, 0, 0), (0, 0, 0), (1, 1, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    s, f, v = orc.orient(p.db, reads)
    assert [(int(a), int(b), int(c)) for a, b, c in zip(s, f, v)] == exp
    assert M.orient(p.db, []) == []
    s, f, v = orc.orient(p.db, [])
    assert len(s) == len(f) == len(v) == 0
    # an empty database decides nothing; empty database sequences add nothing
    assert M.orient([], [p.word]) == M.orient(["", "A"], [p.word]) == [(0, 0, 0)]
    assert [int(x[0]) for x in orc.orient(["", "A"], [p.word])] == [0, 0, 0]


def test_the_hash_helper():
    otab, oltab, olb = M.table_sizes()
    assert M.word_value("CAAAAAAAAAAA") == 1 and M.word_value("AAAAAAAAAAAT") == 3 << 22 and M.word_value("T" * 12) == (1 << 24) - 1
    assert M.home_slot("CAAAAAAAAAAA", 1 << 14) == 2654435761 >> 18 and M.home_slot("A" * 12, oltab) == 0
    p = M.pools()
    for w in p.S + p.L + p.F:
        assert M.value_word(M.word_value(w)) == w
    assert {M.home_slot(w, otab) for w in p.S} == {otab - 2, otab - 1}
    assert {M.home_slot(w, oltab) for w in p.L} <= set(range(oltab - 4, oltab)) and len({M.home_slot(w, oltab) for w in p.L}) >= 2
    assert olb >= 1


def test_parse_fasta_is_pinned():
    P = M.parse_fasta
    assert P(b"") == [] and P(b"\n\n") == []
    assert P(b">a\nACGT\n") == [("a", "ACGT")]
    assert P(b">a\nACGT") == [("a", "ACGT")]                                        # no final newline
    assert P(b">a desc\r\nAC\r\nGT\r\n>b\r\n\r\nTT\r\n") == [("a desc", "ACGT"), ("b", "TT")]    # CRLF, folded, a blank line
    assert P(b">a\nAC\n\n\nGT\n") == [("a", "ACGT")]                                # blank lines do not break a sequence
    assert P(b">a >b\nAC\n>c ACGT\n>d\n") == [("a >b", "AC"), ("c ACGT", ""), ("d", "")]    # '>' and bases in a header; empty records
    assert P(b">a\nacgu\nRYKMSWBDHVNXx\n") == [("a", "acguRYKMSWBDHVNXx")]          # case kept, the whole alphabet
    assert P(b">a\nAC-GT.A C\tG*1>T\n") == [("a", "ACNGTNANCNGNNNT")]               # everything else reads as N
    assert P(b">\nAC\n") == [("", "AC")]
    # and what the model makes of it: a word across a line break is a word, one across a gap is not
    w = "ACGTTGCAAGCT"
    assert M.db_words([s for _, s in P(b">x\n" + w[:5].encode() + b"\r\n" + w[5:].encode() + b"\n")], False) == {w}
    assert M.db_words([s for _, s in P(b">x\n" + w[:5].encode() + b"-" + w[5:].encode() + b"\n")], False) == set()
