"""What a context holds is one stage ladder (csrc/engine.hip: itsx_ctx::Stage, fall_to, StageTxn): reads, grouped, searched, final.

1. The ladder walk.  At each of four points (after set_reads, derep, search, finalize), in the "full" and the "lazy" rows mode, a fixed
   list of readers is called and each one's outcome recorded: "ok", or the code of its EngineError.  A reader that changes the state
   (search, finalize, align_domains + alignments, cluster + align_clusters + get_cluster_cigars) starts from the point rebuilt.  Then,
   from a finalized state that has a clustering, its alignments and the domain alignments, each of set_reads, set_samples, derep,
   cluster, load_profiles, set_active_uniques, search and finalize(domE=1e-3) is applied -- once each on its own ("each"), once one
   after the other ("chain") -- and the readers that change nothing are called after every one of them; search, finalize and
   align_domains are left out there because they are steps of the chain themselves (align_domains has trim_coords' guard).  The chain
   ends finalized and must give a fresh engine's coordinates.
   tests/golden/stage_ladder.json holds the outcomes recorded on the commit before the ladder (ed2f793, `python tests/test_gpu_stage_ladder.py
   out.json` writes them): successful call sequences answer exactly as they did.
2. A failed load.  set_reads that fails (a symbol outside the alphabet: -3; a read of 65 536 bases: -5) leaves no read set: whatever
   was grouped, searched or finalized before is gone, and trim_coords, rep_coords, get_derep, domains and write_domtbl answer -1
   instead of serving the old results for the new read count.  The failed sets are smaller than the set before them.
3. The same through the batch path (load_reads_files with keep_records).  The records go with the read set, before and after the
   ladder, so write_trimmed_samples by prefixes answers -1 with its message about itsx_keep_records, which it tests first; the guard
   "prefixes given before itsx_search_finalize" of the writers' shared helper is seen through trimmed_table, which needs no records."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_ladder.json")
MODES = ("full", "lazy")
POINTS = ("reads", "grouped", "searched", "final")
L, R = "3_", "4_"


def _outcome(fn):
    from itsxpress_amd import EngineError
    try:
        fn()
        return "ok"
    except EngineError as e:
        return int(e.code)


def _clustered_cigars(e):
    e.cluster(0.97)
    e.align_clusters()
    e.get_cluster_cigars()


def _quiet(e, tmp):
    """the readers that change nothing"""
    return [("get_derep", e.get_derep), ("get_uniques", e.get_uniques), ("write_uc", lambda: e.write_uc(os.path.join(tmp, "uc.txt"))),
            ("get_domz", e.get_domz), ("domains", e.domains), ("pairtraces", e.pairtraces), ("alignments", e.alignments),
            ("trim_coords", lambda: e.trim_coords(L, R)), ("rep_coords", lambda: e.rep_coords(L, R)),
            ("write_domtbl", lambda: e.write_domtbl(os.path.join(tmp, "domtbl.txt"))),
            ("trimmed_table", lambda: e.trimmed_table(region_prefixes=(L, R))), ("get_cluster_cigars", e.get_cluster_cigars)]


def _reach(e, seqs, point):
    e.set_reads(seqs)
    if point != "reads":
        e.derep()
    if point in ("searched", "final"):
        e.search()
    if point == "final":
        e.finalize()


def _base(e, seqs):
    """finalized, over a clustering with its alignments, the domain rows aligned where the rows mode keeps them"""
    e.set_reads(seqs)
    e.cluster(0.97)
    e.align_clusters()
    e.search()
    e.finalize()
    _outcome(e.align_domains)


def _steps(e, seqs, hmm):
    return [("set_reads", lambda: e.set_reads(seqs)), ("set_samples", lambda: e.set_samples(None, 1)), ("derep", e.derep),
            ("cluster", lambda: e.cluster(0.97)), ("load_profiles", lambda: e.load_profiles(text=hmm)),
            ("set_active_uniques", lambda: e.set_active_uniques(np.ones(e.n_unique, np.uint8))), ("search", e.search),
            ("finalize", lambda: e.finalize(domE=1e-3))]


def walk(e, hmm, seqs, mode, tmp):
    """the outcomes of one rows mode; leaves the engine finalized at the end of the chain"""
    out = {"walk": {}, "each": {}, "chain": {}}
    e.set_rows_mode(mode)
    e.load_profiles(text=hmm)
    for point in POINTS:
        _reach(e, seqs, point)
        row = {name: _outcome(fn) for name, fn in _quiet(e, tmp) if name not in ("alignments", "get_cluster_cigars")}
        for name, fn in (("search", e.search), ("finalize", e.finalize), ("align_domains", None), ("get_cluster_cigars", lambda: _clustered_cigars(e))):
            _reach(e, seqs, point)
            if fn is None:
                row["align_domains"] = _outcome(e.align_domains)
                row["alignments"] = _outcome(e.alignments)
            else:
                row[name] = _outcome(fn)
        out["walk"][point] = row
    for k, (name, _) in enumerate(_steps(e, seqs, hmm)):
        _base(e, seqs)
        out["each"][name] = {"the step": _outcome(_steps(e, seqs, hmm)[k][1])}
        out["each"][name].update({r: _outcome(fn) for r, fn in _quiet(e, tmp)})
    _base(e, seqs)
    for name, step in _steps(e, seqs, hmm):
        out["chain"][name] = {"the step": _outcome(step)}
        out["chain"][name].update({r: _outcome(fn) for r, fn in _quiet(e, tmp)})
    return out


def _coords(e):
    """trim_coords + rep_coords, or the code they are refused with"""
    from itsxpress_amd import EngineError
    try:
        return [a.copy() for a in e.trim_coords(L, R) + e.rep_coords(L, R)]
    except EngineError as x:
        return int(x.code)


def _reset(e):
    e.set_rows_mode(None)
    e.keep_records(False)


@pytest.fixture(scope="module")
def inputs(mini_hmm_text, fixture_reads):
    return mini_hmm_text, fixture_reads[1][:60]


@pytest.fixture(scope="module")
def fresh(inputs):
    """an engine of its own and its coordinates: {(mode, grouping, domE): trim_coords + rep_coords}, computed once"""
    from itsxpress_amd import Engine
    hmm, seqs = inputs
    e = Engine(0)
    res = {}
    try:
        for mode, group, domE in (("full", "derep", 10.0), ("full", "cluster", 1e-3), ("lazy", "cluster", 1e-3)):
            e.set_rows_mode(mode)
            e.load_profiles(text=hmm)
            e.set_reads(seqs)
            e.derep() if group == "derep" else e.cluster(0.97)
            e.search()
            _outcome(lambda: e.finalize(domE=domE))
            res[(mode, group, domE)] = _coords(e)
    finally:
        e.close()
    return res


def _same(a, b):
    if isinstance(a, int) or isinstance(b, int):
        return a == b
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", MODES)
def test_ladder_walk(engine, inputs, fresh, tmp_path, mode):
    hmm, seqs = inputs
    with open(GOLDEN) as f:
        exp = json.load(f)[mode]
    try:
        got = walk(engine, hmm, seqs, mode, str(tmp_path))
        coords = _coords(engine)
    finally:
        _reset(engine)
    for part in ("walk", "each", "chain"):
        assert set(got[part]) == set(exp[part])
        for key in exp[part]:
            if exp[part][key].get("the step", "ok") == "ok":
                assert got[part][key] == exp[part][key], (part, key)
                continue
            # a step that FAILED (lazy rows are kept for domE >= 0.01: finalize(domE=1e-3) is refused with -5): the same refusal, and
            # no finalized results behind it -- ed2f793 went on serving the finalize before it
            assert got[part][key]["the step"] == exp[part][key]["the step"], (part, key)
            assert all(got[part][key][r] == -1 for r in ("trim_coords", "rep_coords", "trimmed_table", "alignments")), (part, key)
    # the table is not a row of refusals: the finalized point answers more readers than the point after set_reads
    n_ok = [sum(v == "ok" for v in got["walk"][p].values()) for p in POINTS]
    assert n_ok[0] < n_ok[-1]
    assert _same(coords, fresh[(mode, "cluster", 1e-3)])
    assert coords == -1 if mode == "lazy" else int((coords[1] >= 0).sum()) > 10          # (the 4_ profiles' side: the reads hold no 3_ hit)


BAD = {"symbol": (["ACGTACGTACGTACGTACGTACGTACGTACGTACGT", "ACGTACGTJACGTACGTACGTACGTACGTACGTACGT", "TTGACGTACGTACGTACGTACGTACGTACGTACGTAA"], -3),
       "long": (["A" * 65536], -5)}


def _finalized(e, hmm, seqs):
    e.set_rows_mode("full")
    e.load_profiles(text=hmm)
    e.set_reads(seqs)
    e.derep()
    e.search()
    e.finalize()


@pytest.mark.parametrize("kind", sorted(BAD))
def test_failed_load_leaves_no_results(engine, inputs, fresh, tmp_path, kind):
    """ed2f793 fails this test at its first reader: after either failed load get_derep answers "ok" (have_derep, have_search and
    have_final were cleared on success only), with the context's read count already the failed set's"""
    from itsxpress_amd import EngineError
    hmm, seqs = inputs
    reads, code = BAD[kind]
    assert len(reads) < len(seqs) and (kind == "long" or max(map(len, reads)) <= max(map(len, seqs)))
    try:
        _finalized(engine, hmm, seqs)
        assert _same(_coords(engine), fresh[("full", "derep", 10.0)]) and int((fresh[("full", "derep", 10.0)][1] >= 0).sum()) > 10
        with pytest.raises(EngineError) as x:
            engine.set_reads(reads)
        assert x.value.code == code
        for name, fn in _quiet(engine, str(tmp_path)):
            if name in ("trim_coords", "rep_coords", "get_derep", "domains", "write_domtbl"):
                got = _outcome(fn)
                print("after the failed load (%s): %s -> %s" % (kind, name, got))
                assert got == -1, name
        engine.set_reads(seqs)
        engine.derep()
        engine.search()
        engine.finalize()
        assert _same(_coords(engine), fresh[("full", "derep", 10.0)])
    finally:
        _reset(engine)


def test_failed_load_after_a_batch_with_records(engine, inputs, fixture_reads, tmp_path):
    from itsxpress_amd import EngineError
    hmm, seqs = inputs
    files = []
    for k in range(2):
        files.append(str(tmp_path / ("s%d.fq" % k)))
        with open(files[-1], "w") as f:
            for n, s in list(zip(fixture_reads[0], seqs))[30 * k:30 * k + 30]:
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    outs = [str(tmp_path / ("t%d.fq" % k)) for k in range(2)]
    try:
        engine.set_rows_mode("full")
        engine.load_profiles(text=hmm)
        engine.keep_records(True)
        assert list(engine.load_reads_files(files)) == [30, 30]
        engine.derep()
        engine.search()
        engine.finalize()
        assert len(engine.write_trimmed_samples(outs, region_prefixes=(L, R))) == 2           # finalized, with records: both answer
        engine.trimmed_table(region_prefixes=(L, R))
        with pytest.raises(EngineError) as x:
            engine.set_reads(BAD["symbol"][0])
        assert x.value.code == -3
        with pytest.raises(EngineError, match="itsx_keep_records") as x:           # the records went with the read set
            engine.write_trimmed_samples(outs, region_prefixes=(L, R))
        assert x.value.code == -1
        with pytest.raises(EngineError, match="itsx_trimmed_table: prefixes given before itsx_search_finalize") as x:
            engine.trimmed_table(region_prefixes=(L, R))
        assert x.value.code == -1
    finally:
        _reset(engine)


if __name__ == "__main__":      # record the outcomes of the library in the tree: python tests/test_gpu_stage_ladder.py out.json
    import gzip
    import tempfile
    os.environ.setdefault("ITSX_TEST_HOOKS", "1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from itsxpress_amd import Engine
    with gzip.open(os.path.join(root, "tests", "golden", "fixture_reads.fa.gz"), "rt") as f:
        seqs_ = [ln.strip() for ln in f if ln[0] != ">"][:60]
    with open(os.path.join(root, "tests", "golden", "mini.hmm")) as f:
        hmm_ = f.read()
    eng = Engine(0)
    with tempfile.TemporaryDirectory() as tmp_:
        table = {m: walk(eng, hmm_, seqs_, m, tmp_) for m in MODES}
    eng.close()
    with open(sys.argv[1], "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
