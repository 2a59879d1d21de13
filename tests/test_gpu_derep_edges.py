"""Stage A on the device (csrc/k_derep.hip, itsx_derep / build_unique_lists in engine.hip) against the plain text model of
tests/derep_exact.py, at the edges of the packed form: zero padding, the exception list, the reverse complement's word boundaries,
every shape of the key hash, palindromes, first occurrences, minseqlength, the table's size, per-sample seeds, the length-ordered
unique list, and the 128-bit keys by which the uniques of several shards meet.  Every comparison is equality.

Group sizes of the run on an MI355X (summed over a group's cases; the device's figures, equal to the model's):
  group             cases   reads  uniques  minus-strand joins
  word_edges           25     828      448                 274
  exceptions           24    3563     2033                1530
  xxh_shapes            2     264      165                  33
  palindromes           2      40       19                   2
  first_occurrence      2   40000      120               10088
  minlen                5      65       12                   8
  table_edges           4    1010     1010                   0
  samples               2    1680     1559                  59
  length_order         10   35789    33688                2101
  two shards (both strands / plus only)   182 reads, 91 / 135 global uniques, 48 / 0 minus-strand joins
The whole file takes under three seconds.

Mutations of csrc/k_derep.hip tried on scratch builds, and the first cases that caught each: one nibble of comp_code's table (R kept as
R): exceptions L15 and xxh_shapes; rc_word's tail mask dropped: word_edges L1, exceptions L15 and seven more tests; RcKey's
exception list not reversed: exceptions L15 and xxh_shapes; the length word taken out of the key together with same_forward's
length comparison: word_edges L1 and minlen (same_forward only ever sees two reads whose 64-bit keys are equal, and the key holds
the length, so its length comparison alone decides nothing short of a 64-bit collision).
"""
import numpy as np
import pytest

import derep_exact as dx

pytestmark = pytest.mark.gpu


def _run(engine, case, names=None):
    engine.set_reads(case.seqs, names)
    if case.sample is not None:
        engine.set_samples(case.sample, int(case.sample.max()) + 1)
    return engine.derep(strand_both=case.strand_both, minseqlength=case.minlen)


def _check(engine, group, case, got_nu):
    nu, rep_of, strand, uniq_of, seed_read, abundance = dx.expected(case)
    tag = (group, case.name)
    assert got_nu == nu, tag
    g_rep, g_strand, g_uniq = engine.get_derep()
    for what, got, want in (("rep_of", g_rep, rep_of), ("strand", g_strand, strand), ("uniq_of", g_uniq, uniq_of)):
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (tag, what, "read %d" % bad[0], case.seqs[bad[0]][:80], int(got[bad[0]]), int(want[bad[0]]), "%d reads differ" % len(bad))
    g_seed, g_ab = engine.get_uniques()
    assert np.array_equal(g_seed, seed_read), tag
    assert np.array_equal(g_ab, abundance), tag
    st = engine.stats()
    assert st["n_unique"] == nu and st["n_dropped_short"] == int((rep_of < 0).sum()), tag
    assert st["hash_reseeds"] == 0, tag


@pytest.mark.parametrize("group", ["xxh_shapes", "palindromes", "first_occurrence", "minlen", "table_edges"])
def test_derep_equals_the_text_model(engine, group):
    for case in dx.group(group):
        _check(engine, group, case, _run(engine, case))


def _fasta(path):
    names, seqs = [], []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].strip())
                seqs.append("")
            else:
                seqs[-1] += line.strip()
    return names, seqs


@pytest.mark.parametrize("group", ["word_edges", "exceptions"])
def test_derep_and_its_files_equal_the_text_model(engine, group, tmp_path):
    from itsxpress_amd.SeqSample import Dedup
    for k, case in enumerate(dx.group(group)):
        names = ["r%d" % i for i in range(len(case.seqs))]
        _check(engine, group, case, _run(engine, case, names))
        nu, rep_of, strand, _, seed_read, abundance = dx.expected(case)
        uc, rep = str(tmp_path / ("uc%d.txt" % k)), str(tmp_path / ("rep%d.fa" % k))
        engine.write_uc(uc)
        engine.write_rep_fasta(rep)
        # uc.txt through the mirror's parser: read -> representative
        dd = Dedup(uc_file=uc, rep_file=rep, seq_file=None)
        assert dd.matchdict == {names[i]: names[rep_of[i]] for i in range(len(names)) if rep_of[i] >= 0}, (group, case.name)
        with open(uc) as f:
            hits = {ll[8]: ll[4] for ll in (line.split("\t") for line in f) if ll[0] == "H"}
        assert hits == {names[i]: "-" if strand[i] < 0 else "+" for i in range(len(names)) if rep_of[i] >= 0 and rep_of[i] != i}, (group, case.name)
        # rep.fa: one record per unique of the model, the seed's own text.  The file lists them as vsearch --fastx_uniques does (by
        # falling abundance, then by label), so it is taken back to seed order by its labels; the order itself is the model's too
        fnames, fseqs = _fasta(rep)
        by_seed = sorted(zip(fnames, fseqs), key=lambda x: int(x[0][1:]))
        assert [n for n, _ in by_seed] == [names[s] for s in seed_read], (group, case.name)
        assert [dx.norm(s) for _, s in by_seed] == [dx.norm(case.seqs[s]) for s in seed_read], (group, case.name)
        order = sorted(range(nu), key=lambda u: (-int(abundance[u]), names[seed_read[u]].encode()))
        assert fnames == [names[seed_read[u]] for u in order], (group, case.name)


def test_samples_stay_apart(engine):
    for case in dx.group("samples"):
        got = _run(engine, case)
        d, h = engine.debug_read_samples()
        assert np.array_equal(d, case.sample) and np.array_equal(h, case.sample)
        _check(engine, "samples", case, got)
        rep_of = engine.get_derep()[0]
        assert (case.sample[rep_of] == case.sample).all()
    engine.set_samples(None, 1)


def test_length_ordered_unique_list(engine):
    """the list the HMM stages walk, read from the device: a permutation of the uniques whose lengths never decrease (the order inside
    one length is free), and after set_active_uniques the kept subsequence of it"""
    for case in dx.group("length_order"):
        got = _run(engine, case)
        _check(engine, "length_order", case, got)
        nu, _, _, _, seed_read, _ = dx.expected(case)
        ulen = np.array([len(case.seqs[s]) for s in seed_read], np.int64)
        lst = engine.debug_sorted_uniques()
        assert lst.shape[0] == nu and np.array_equal(np.sort(lst), np.arange(nu)), case.name
        assert (np.diff(ulen[lst]) >= 0).all(), case.name
        active = np.arange(nu) % 2 == 0
        engine.set_active_uniques(active)
        assert np.array_equal(engine.debug_sorted_uniques(), lst[active[lst]]), case.name


# ---------------------------------------------------------------- cross-shard keys
@pytest.fixture(scope="module")
def second_engine():
    from itsxpress_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("strand_both", [True, False])
def test_shards_meet_by_their_keys(engine, second_engine, strand_both):
    """two contexts as two shards, through the product's own steps (multi._h_derep, owner_verdicts, _h_verdict, _h_derep_arrays):
    equal 128-bit keys exactly for equal sequences (up to the reverse complement under --strand both), flags that tell the
    orientations apart, and per read the representative and strand of ONE dereplication of the whole input"""
    from itsxpress_amd import multi
    shards = dx.cross_shards(2)
    engines = [engine, second_engine]
    whole, per = dx.global_derep(shards, strand_both, 1)
    states, tups, base = [], [], 0
    for r, (e, sh) in enumerate(zip(engines, shards)):
        e.set_reads(sh, ["s%d_%d" % (r, i) for i in range(len(sh))])
        st = {"base": base, "rank": r, "world": 2}
        tup = multi._h_derep(e, st, strand_both, 1)
        assert tup.shape == (per[r][0], 4) and np.array_equal(tup[:, 2], per[r][4] + base)
        states.append(st)
        tups.append(tup)
        base += len(sh)
    # keys and flags against the text
    texts = [dx.norm(sh[s]) for sh, p in zip(shards, per) for s in p[4]]
    canon = [dx.canonical(t) if strand_both else t for t in texts]
    keys = [(int(k0), int(k1)) for t in tups for k0, k1 in t[:, :2]]
    flags = [int(f) for t in tups for f in t[:, 3]]
    by_key, by_text = {}, {}
    for i, (k, c) in enumerate(zip(keys, canon)):
        by_key.setdefault(k, []).append(i)
        by_text.setdefault(c, []).append(i)
    assert sorted(by_key.values()) == sorted(by_text.values())
    assert max(len(v) for v in by_text.values()) >= 2
    for rows in by_text.values():
        for i in rows:
            if not strand_both or dx.rc(texts[i]) == texts[i]:
                assert flags[i] == 1
            for j in rows:
                if strand_both and dx.rc(texts[i]) != texts[i]:
                    assert (flags[i] == flags[j]) == (texts[i] == texts[j])
    # the owner's step and the composition
    recv = np.concatenate([np.concatenate([t, np.arange(t.shape[0], dtype=np.int64)[:, None]], axis=1) for t in tups])
    src = np.concatenate([np.full(t.shape[0], r, np.int64) for r, t in enumerate(tups)])
    verdict = multi.owner_verdicts(recv, src)
    assert np.array_equal(verdict, multi.owner_verdicts_native(recv, src))
    cut = np.cumsum([0] + [t.shape[0] for t in tups])
    rep_of, strand = [], []
    scored = 0
    for r, (e, st) in enumerate(zip(engines, states)):
        v = verdict[cut[r]:cut[r + 1]]
        scored += multi._h_verdict(e, st, v)
        out = multi._h_derep_arrays(e, st, False, False)
        uq = out["uniq_of"].astype(np.int64)
        assert np.array_equal(uq, per[r][3]) and np.array_equal(out["seed_gidx_local"], per[r][4] + st["base"])
        rep_of.append(np.where(uq >= 0, v[np.maximum(uq, 0), 0], -1))
        strand.append(out["strand"])
    assert scored == whole[0]                                          # every sequence is scored once
    assert np.array_equal(np.concatenate(rep_of), whole[1])
    assert np.array_equal(np.concatenate(strand), whole[2])
    assert strand_both == bool((whole[2] == -1).any())
