"""Exact dereplication at its packing edges, without a GPU: the oracle (oracle/orc_derep.c) against the plain text model of
tests/derep_exact.py on every case of the catalogue, the catalogue's own floors, and the owner's step of the cross-shard
dereplication (multi.owner_verdicts and its native twin) on tuples made from text."""
import hashlib

import numpy as np
import pytest

import derep_exact as dx


@pytest.mark.parametrize("name", sorted(dx.GROUPS))
def test_oracle_equals_the_text_model(name):
    """(building the group runs every builder's premise assertions)"""
    import orc
    for case in dx.group(name):
        nu, rep_of, strand, _, _, _ = dx.expected(case)
        if case.sample is None:
            blocks = [np.arange(len(case.seqs))]
        else:                                                # the oracle knows one sample: one call per sample (they are contiguous)
            blocks = [np.nonzero(case.sample == s)[0] for s in np.unique(case.sample)]
        got_nu = 0
        for idx in blocks:
            codes, offs = orc.digitize([case.seqs[i] for i in idx])
            nc, orep, ostrand = orc.derep(codes, offs, case.strand_both, case.minlen)
            base = int(idx[0]) if len(idx) else 0
            assert len(idx) == 0 or np.array_equal(idx, np.arange(base, base + len(idx)))
            got_nu += nc
            assert np.array_equal(np.where(orep >= 0, orep + base, -1), rep_of[idx]), (name, case.name)
            assert np.array_equal(ostrand, strand[idx]), (name, case.name)
        assert got_nu == nu, (name, case.name)


def test_every_group_meets_its_floor():
    """a case list that degenerates (no reverse-complement joins, no seeds) would pass everything: hold it to a floor"""
    for name in ("word_edges", "exceptions"):
        minus = seeds = 0
        for case in dx.group(name):
            if case.strand_both:
                nu, _, strand, _, _, _ = dx.expected(case)
                minus += int((strand == -1).sum())
                seeds += nu
        assert minus >= 100 and seeds >= 100, (name, minus, seeds)
    for name in dx.GROUPS:
        cases = dx.group(name)
        assert len(cases) >= 1 and len({c.name for c in cases}) == len(cases)
        assert name == "table_edges" or all(len(c.seqs) > 0 for c in cases)
    assert any(dx.n_minus(c) > 0 for c in dx.group("xxh_shapes"))
    assert sum(dx.n_minus(c) for c in dx.group("first_occurrence")) > 5000
    assert {len(c.seqs) for c in dx.group("table_edges")} == {0, 1, 504, 505}
    assert sorted(max(len(s) for s in c.seqs) for c in dx.group("length_order"))[-3:] == [8191, 8192, 65535]


def test_model_normalises_and_complements():
    assert dx.norm("acgun") == "ACGTN" and dx.rc("ACGTRYMKSWHBVDN") == "NHBVDWSMKRYACGT"
    for c in "ACGTRYMKSWHBVDN":
        assert dx.rc(dx.rc(c)) == c
    nu, rep, strand, uq, seed, ab = dx.derep(["ACGG", "ccgu", "AC", "ACGG", "CCGT"], True, 3)
    assert nu == 1 and list(rep) == [0, 0, -1, 0, 0] and list(strand) == [1, -1, 0, 1, -1] and list(uq) == [0, 0, -1, 0, 0]
    assert list(seed) == [0] and list(ab) == [4]
    nu, rep, strand, _, seed, ab = dx.derep(["ACGG", "ccgu", "AC", "ACGG", "CCGT"], False, 1)
    assert nu == 3 and list(rep) == [0, 1, 2, 0, 1] and list(ab) == [2, 2, 1]
    nu, rep, _, _, _, _ = dx.derep(["ACGG", "ACGG", "CCGT"], True, 1, sample=[0, 1, 1])
    assert nu == 2 and list(rep) == [0, 1, 1]


def text_tuples(shards, strand_both=True, minlen=1):
    """(recv [m, 5], src [m], per row the global index the model gives its sequence, per row the holders in the representative's
    orientation) of the shards' uniques: keys from BLAKE2b of the canonical text, the flag from the text comparison"""
    (_, grep, _, _, _, _), per = dx.global_derep(shards, strand_both, minlen)
    rows, src, want, texts = [], [], [], []
    base = 0
    for r, (sh, (nu, _, _, _, seed, _)) in enumerate(zip(shards, per)):
        for u, s in enumerate(seed):
            t = dx.norm(sh[s])
            canon = dx.canonical(t) if strand_both else t
            d = hashlib.blake2b(canon.encode(), digest_size=16).digest()
            k0, k1 = (int.from_bytes(d[i:i + 8], "little", signed=True) for i in (0, 8))
            flag = 1 if (not strand_both or t <= dx.rc(t)) else 0
            rows.append((k0, k1, base + int(s), flag, u))
            src.append(r)
            want.append(int(grep[base + int(s)]))
            texts.append(t)
        base += len(sh)
    return np.array(rows, np.int64).reshape(-1, 5), np.array(src, np.int64), np.array(want, np.int64), texts


@pytest.mark.parametrize("strand_both", [True, False])
@pytest.mark.parametrize("n_shards", [2, 3])
def test_owner_step_on_tuples_made_from_text(n_shards, strand_both):
    from itsxpress_amd import multi
    shards = dx.cross_shards(n_shards)
    recv, src, want, texts = text_tuples(shards, strand_both)
    whole = [s for sh in shards for s in sh]
    out = multi.owner_verdicts(recv, src)
    assert np.array_equal(out, multi.owner_verdicts_native(recv, src))
    assert np.array_equal(out[:, 0], want)                                      # the model's global first index
    flag_of = {int(g): int(f) for g, f in zip(recv[:, 2], recv[:, 3])}
    n_three = n_single = n_pal = 0
    for i in range(len(recv)):
        g = int(out[i, 0])
        assert out[i, 1] == flag_of[g]                                          # the representative row's flag
        same = np.nonzero(want == g)[0]
        holders = {(int(src[j]), int(recv[j, 4])) for j in same if recv[j, 3] == flag_of[g]}
        assert (int(out[i, 2]), int(out[i, 3])) in holders
        assert {tuple(out[j]) for j in same} == {tuple(out[i])}
        # the representative's text is this row's, or its reverse complement exactly where the flags differ
        t, rep = texts[i], dx.norm(whole[g])
        assert rep == (t if recv[i, 3] == out[i, 1] else dx.rc(t))
        n_three += len(same) == 3 and len({int(src[j]) for j in same}) == 3
        n_single += len(same) >= 2 and len(holders) == 1
        n_pal += len(same) >= 2 and dx.rc(t) == t
    if strand_both:
        assert n_single > 0 and n_pal > 0 and (n_shards < 3 or n_three > 0)
    else:
        assert (recv[:, 3] == 1).all()
