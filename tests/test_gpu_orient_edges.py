"""GPU tests of read orientation at its decision edges and at the edges only the engine has: k_orient,
k_orient_long and the database loader itsx_orient_load_db (with the host DUST statement dust_host) are held to tests/orient_exact.py,
an independent statement of the procedure on Python strings and sets -- not to the oracle, which tests/test_orient_edges_cpu.py holds
to the same model.  Every comparison is between integers and exact.  The module works in a context of its own, so the session's
shared engine never holds one of these databases."""
import gzip

import numpy as np
import pytest

import orient_exact as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from itsxpress_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _load_db(eng, tmp_path, db, tag="db"):
    path = tmp_path / (tag + ".fasta")
    with open(path, "w") as f:
        for i, s in enumerate(db):
            f.write(">s%d\n%s\n" % (i, s))
    assert eng.orient_load_db(str(path)) == len(db)


def _orient(eng, reads):
    eng.set_reads(reads)
    s, f, v = eng.orient()
    return [(int(a), int(b), int(c)) for a, b, c in zip(s, f, v)]


def _same(got, exp, name, reads):
    bad = [(i, len(reads[i]), reads[i][:50], g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert len(got) == len(exp) and not bad, (name, len(bad), bad[:5])


def _run(eng, tmp_path, names, dust):
    """the named cases against the model under one masking setting (the caller has set ITSX_QMASK to match): cases that share a
    database go through one call, so that k_orient and k_orient_long run side by side"""
    groups = {}
    for n in names:
        case = M.case(n)
        case.check(*M.outputs(n))                     # the case hits its target, on the model's output
        groups.setdefault(tuple(case.db), []).append(case)
    for g, (db, cases) in enumerate(groups.items()):
        _load_db(eng, tmp_path, db, "db%d" % g)
        reads = [r for c in cases for r in c.reads]
        got = _orient(eng, reads)
        at = 0
        for c in cases:
            exp = M.outputs(c.name)[0 if dust else 1]
            _same(got[at:at + len(c.reads)], exp, c.name, c.reads)
            at += len(c.reads)


GROUPS = {"rules": ("rule_grid", "distinct_words_masked", "palindromes", "both_strands", "positions", "spoilers"),
          "tables": ("positions_long", "short_table", "long_table"),
          "case_and_u": ("case_and_u",), "dust": ("dust",), "sweep": ("sweep",)}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_catalogue_and_sweep_equal_the_model(eng, tmp_path, monkeypatch, group):
    monkeypatch.delenv("ITSX_QMASK", raising=False)
    assert {n for g in GROUPS.values() for n in g} == {n for n in M.CASE_NAMES + ("sweep",) if True in M.case(n).modes}
    _run(eng, tmp_path, GROUPS[group], True)


def test_masking_off_equals_the_model(eng, tmp_path, monkeypatch):
    """ITSX_QMASK=none, the database reloaded under the setting, against dust=False: every case that is compared without masking
    (the rule grid, the spoilers and the sweep among them, and the repeats that DUST would take away)"""
    monkeypatch.setenv("ITSX_QMASK", "none")
    names = [n for n in M.CASE_NAMES + ("sweep",) if False in M.case(n).modes]
    assert {"rule_grid", "spoilers", "sweep", "distinct_words", "distinct_words_tandem"} <= set(names)
    _run(eng, tmp_path, names, False)


def test_more_long_reads_than_blocks(eng, tmp_path, monkeypatch):
    """130 long reads in one call: every block of k_orient_long takes a second read (and some a third) from the work list, into a
    table that the read before must have left empty -- the read whose words sit in the table's last slots several times, and
    after each copy, in the same block, a read that shares words with it"""
    monkeypatch.delenv("ITSX_QMASK", raising=False)
    p = M.pools()
    t, s1, s2, short = M.long_table_reads()
    plain = M.case("positions_long").reads
    n = 2 * p.olblocks + 2
    reads, kinds = [], []
    for i in range(n):
        k = (i + i // p.olblocks) % 4                 # the read a block takes next is the next kind: t -> s1 -> s2 -> plain -> t
        reads.append((t, s1, s2, plain[i % 5])[k])
        kinds.append(k)
    assert n >= 130 and all(12012 <= len(r) <= 13000 for r in reads) and len(set(reads)) <= 8
    for i in range(n - p.olblocks):
        assert kinds[i + p.olblocks] == (kinds[i] + 1) % 4
    assert kinds.count(0) >= 30
    reads += short                                    # and k_orient beside it
    exp = M.orient(p.db, reads)
    assert exp[0] == (1, 32, 0) and exp[1] == (1, 16, 0) and exp[2] == (1, 16, 0) and exp[3] == (1, 1, 0)
    _load_db(eng, tmp_path, p.db)
    got = _orient(eng, reads)
    _same(got, exp, "long reads", reads)
    s, f, v = eng.orient()                            # once more in the same context: the tables were left empty
    _same([(int(a), int(b), int(c)) for a, b, c in zip(s, f, v)], exp, "long reads, second call", reads)


def test_more_reads_than_blocks(eng, tmp_path, monkeypatch):
    """65 536 + 300 short reads: the first 300 blocks of k_orient take a second read, one that shares words with their first"""
    monkeypatch.delenv("ITSX_QMASK", raising=False)
    p = M.pools()
    pos = list(dict.fromkeys(r for r in M.case("positions").reads if 12 <= len(r) <= 40 and p.word in r))
    cells = [(1, 0), (2, 0), (1, 1), (0, 1), (0, 2), (1, 1)]
    assert len(pos) > 200
    pool = []
    for k in range(len(pos)):
        pool += [pos[k], M.grid_read(*cells[k % 6])]
    nblocks = 65536
    reads = [pool[i % len(pool)] for i in range(nblocks)]
    for j in range(300):                              # the partner: other flanks around the same word / the next cell of the cycle
        k = (j % len(pool)) // 2
        reads.append(pos[(k + 7) % len(pos)] if j % 2 == 0 else M.grid_read(*cells[(k + 1) % 6]))
    assert all(12 <= len(r) <= 40 for r in reads)
    for j in range(0, 300, 7):
        a, b = M.words(reads[j]), M.words(reads[nblocks + j])
        assert reads[j] != reads[nblocks + j] and (a & b) & p.either, j
    exp = M.orient(p.db, reads)
    assert sum(1 for t in exp[nblocks:] if t[1] + t[2] > 0) == 300 and {t[0] for t in exp[nblocks:]} == {1, 0, -1}
    _load_db(eng, tmp_path, p.db)
    _same(_orient(eng, reads), exp, "short reads", reads)


# ------------------------------------------------------------------------------------------------------------ the database loader
def _loader_files():
    rng = np.random.default_rng(77)
    rnd = lambda n: "".join(rng.choice(list("ACGT"), n))
    fold = lambda s, w, nl="\n": nl.join(s[i:i + w] for i in range(0, len(s), w)) + nl
    a, b, c, d = rnd(60), rnd(45), rnd(40), rnd(36)
    files = {
        "folded": ">a\n" + fold(a, 7) + ">b\n" + fold(b, 11) + ">c\n" + fold(c, 12),
        "crlf": ">a x\r\n" + fold(a, 7, "\r\n") + ">b\r\n" + fold(b, 45, "\r\n"),
        "no_final_newline": ">a\n" + a + "\n>b\n" + b,
        "blank_lines": "\n\n>a\n" + a[:20] + "\n\n\n" + a[20:] + "\n\n>b\n\n" + b + "\n\n\n",
        "lower_and_u": ">a\n" + a.lower() + "\n>b\n" + b.replace("T", "U") + "\n>c\n" + c.lower().replace("t", "u") + "\n",
        "iupac": ">a\n" + a[:20] + "R" + a[21:40] + "n" + a[41:] + "\n>b\n" + b[:13] + "X" + b[14:30] + "Y" + b[31:] + "\n>c\n" + c[:12] + "N" + c[13:]
                 + "\n",
        "other_characters": ">a\n" + a[:14] + "-" + a[14:28] + "." + a[28:42] + " " + a[42:] + "\n>b\n" + b[:15] + "*" + b[15:30] + "1" + b[30:]
                            + "\n>c\n" + c[:20] + "\t" + c[20:] + "\n",
        "tiny_records": ">e0\n>e11\n" + a[:11] + "\n>e12\n" + b[:12] + "\n>e0b\n\n>e13\n" + c[:13] + "\n>last\n",
        "headers": ">a >b\n" + a + "\n>h " + b + "\n" + c + "\n>" + d + "\n>k\n" + d[:18] + ">" + d[18:] + "\n",
    }
    return {k: v.encode() for k, v in files.items()}


def _candidates(data, seqs):
    """every 12-mer a reading of the file could find: of each record as parsed, and of the whole text -- headers included -- with
    everything but A C G T U deleted (words across records, across removed characters, out of headers); both strands"""
    text = "".join(ch for ch in data.decode("latin-1") if ch.upper() in "ACGTU")
    cand = set(M.words(text, False))
    for s in seqs:
        cand |= M.words(s, False)
        cand |= M.words("".join(ch for ch in s if ch.upper() in "ACGTU"), False)
    return sorted(cand | {M.rc(w) for w in cand})


def _check_loader(eng, path, data, name):
    recs = M.parse_fasta(data)
    seqs = [s for _, s in recs]
    probes = _candidates(data, seqs)
    exp = M.orient(seqs, probes)
    n_in = sum(1 for t in exp if t[1] > 0)
    assert n_in >= 3 and len(probes) - n_in >= 3, (name, n_in, len(probes))        # words to find and words to miss
    assert eng.orient_load_db(str(path)) == len(recs), name
    _same(_orient(eng, probes), exp, name, probes)
    return exp


_LOADER_EDGES = ("folded", "crlf", "no_final_newline", "blank_lines", "lower_and_u", "iupac", "other_characters", "tiny_records", "headers")


@pytest.mark.parametrize("edge", _LOADER_EDGES)
def test_database_loader_reads_fasta_as_the_model(eng, tmp_path, monkeypatch, edge):
    monkeypatch.delenv("ITSX_QMASK", raising=False)
    files = _loader_files()
    assert set(files) == set(_LOADER_EDGES)
    data = files[edge]
    recs = M.parse_fasta(data)
    # each file is the edge it names, on the model's reading
    n = {"folded": 3, "crlf": 2, "no_final_newline": 2, "blank_lines": 2, "lower_and_u": 3, "iupac": 3, "other_characters": 3, "tiny_records": 6,
         "headers": 4}[edge]
    assert len(recs) == n, recs
    if edge == "folded":
        assert all(len(line) < M.W for line in data.split(b"\n")[1:3]) and len(M.db_words([s for _, s in recs])) > 100
    if edge == "tiny_records":
        assert [len(s) for _, s in recs] == [0, 11, 12, 0, 13, 0]
    if edge == "headers":
        assert recs[0][0] == "a >b" and len(recs[1][0]) == 47 and len(recs[2][0]) == 36 and recs[2][1] == "" and "N" in recs[3][1]
    path = tmp_path / (edge + ".fasta")
    path.write_bytes(data)
    exp = _check_loader(eng, path, data, edge)
    # the same file gzipped reads the same
    gz = tmp_path / (edge + ".fasta.gz")
    with gzip.open(gz, "wb") as f:
        f.write(data)
    assert _check_loader(eng, gz, data, edge + " (gzip)") == exp


def test_a_second_database_replaces_the_first(eng, tmp_path, monkeypatch):
    monkeypatch.delenv("ITSX_QMASK", raising=False)
    rng = np.random.default_rng(78)
    one, two = ("".join(rng.choice(list("ACGT"), 80)) for _ in range(2))
    probes = [one[:12], one[30:50], M.rc(one[10:40]), two[:12], two[30:50], M.rc(two[10:40]), one[:40] + two[:40]]
    _load_db(eng, tmp_path, [one], "one")
    first = _orient(eng, probes)
    _load_db(eng, tmp_path, [two], "two")
    second = _orient(eng, probes)
    assert first == M.orient([one], probes) == [(1, 1, 0), (1, 9, 0), (-1, 0, 19), (0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 29, 0)]
    assert second == M.orient([two], probes) == [(0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 0), (1, 9, 0), (-1, 0, 19), (1, 29, 0)]


# ------------------------------------------------------------------------------------------------------------ orient_apply
def test_orient_apply_keeps_the_reads_the_model_keeps(eng, tmp_path, monkeypatch):
    """the rule grid as two samples: the read set orient_apply leaves holds, per sample, exactly the reads the model keeps, the
    reverse ones reverse-complemented"""
    monkeypatch.delenv("ITSX_QMASK", raising=False)
    p = M.pools()
    case = M.case("rule_grid")
    exp = M.outputs("rule_grid")[0]
    case.check(*M.outputs("rule_grid"))
    samples = [list(range(0, len(case.reads), 2)), list(range(1, len(case.reads), 2))]
    paths = []
    for s, idx in enumerate(samples):
        paths.append(str(tmp_path / ("grid_%d.fq" % s)))
        with open(paths[-1], "w") as f:
            for i in idx:
                r = case.reads[i]
                f.write("@g%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    _load_db(eng, tmp_path, p.db)
    assert list(eng.load_reads_files(paths)) == [len(x) for x in samples]
    strand, cf, cr, kept = eng.orient_apply()
    order = samples[0] + samples[1]                   # the batch's reads: sample after sample
    _same([(int(a), int(b), int(c)) for a, b, c in zip(strand, cf, cr)], [exp[i] for i in order], "rule_grid through orient_apply",
          [case.reads[i] for i in order])
    keep = [[i for i in idx if exp[i][0] != 0] for idx in samples]
    assert [int(k) for k in kept] == [len(k) for k in keep] and min(len(k) for k in keep) > 50
    assert eng.read_names() == ["g%d" % i for k in keep for i in k]
    assert eng.debug_read_samples()[0].tolist() == [s for s, k in enumerate(keep) for _ in k]
    oriented = [case.reads[i] if exp[i][0] > 0 else M.revcomp_read(case.reads[i]) for k in keep for i in k]
    assert min(sum(1 for i in k if exp[i][0] < 0) for k in keep) > 20 and min(sum(1 for i in k if exp[i][0] > 0) for k in keep) > 20
    got = [tuple(x.copy() for x in eng.debug_packed_read(j)) for j in range(eng.n_reads)]
    eng.set_reads(oriented)
    for j, g in enumerate(got):
        e = eng.debug_packed_read(j)
        assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), (j, oriented[j][:40])
