"""GPU tests for the length and threshold edges of greedy clustering (tests/cluster_edges.py): the HIP engine against the exact
alignment model (tests/align_exact.py) through py_cluster -- not only against the oracle, which shares the engine's packed cell.
Bar: order, cluster map, strands, the bit patterns of the identities and the centroid count are equal, for every group as one
batch, sample by sample, for every tuning switch and with a helper context.  No tolerance, no case excused.  `pytest -m gpu`."""
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import cluster_edges as CE

pytestmark = pytest.mark.gpu

_EXP = {}


@pytest.fixture(scope="module")
def expectations():
    if not _EXP:
        with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            _EXP["cases"], _ = CE.expected_all(CE.keys(), pool)
    return _EXP["cases"]


@pytest.fixture(scope="module")
def helper():
    from itsxpress_amd import Engine
    h = Engine(0)
    yield h
    h.close()


def _want(exps):
    """the expectations of some samples in batch coordinates: (n_unique, rep_of, strand, pct, order)"""
    nu, reps, strs, pcts, ords, first = 0, [], [], [], [], 0
    for order, rep_of, strand, pct in exps:
        rep_of = np.asarray(rep_of, np.int64)
        nu += int((rep_of == np.arange(len(rep_of))).sum())
        reps.append(np.where(rep_of >= 0, rep_of + first, -1))
        strs.append(np.asarray(strand, np.int8))
        pcts.append(np.asarray(pct, np.float64))
        ords.append(np.asarray(order, np.int64) + first)
        first += len(rep_of)
    return nu, np.concatenate(reps), np.concatenate(strs), np.concatenate(pcts), np.concatenate(ords)


def _same(engine, nu, want, what):
    rep_of, strand, _ = engine.get_derep()
    pct, order = engine.get_cluster()
    assert np.array_equal(order, want[4]), ("order", what)
    assert np.array_equal(rep_of, want[1]), ("rep_of", what, np.flatnonzero(np.asarray(rep_of) != want[1])[:8])
    assert np.array_equal(strand, want[2]), ("strand", what)
    bad = np.flatnonzero(pct.view(np.uint64) != want[3].view(np.uint64))
    assert bad.size == 0, ("pct_id", what, bad[:8], pct[bad[:8]], want[3][bad[:8]])
    assert nu == want[0] and engine.stats()["n_unique"] == want[0], ("centroids", what)


def _solo(engine, case, exp, helpers=None):
    engine.set_reads(case.reads, case.names)
    nu = engine.cluster(case.cid, helpers=helpers) if helpers else engine.cluster(case.cid)
    _same(engine, nu, _want([exp]), case.name)
    return engine.stats()


def _batches(engine, group, cases):
    """the group's samples as one cluster_samples call per identity threshold; the counters of the calls added up"""
    all_cases = CE.PAIRS[group]()
    tot = dict(cl_certified=0, cl_alignments=0)
    for cid in sorted({c.cid for c in all_cases}):
        ks = [k for k, c in enumerate(all_cases) if c.cid == cid]
        reads = [r for k in ks for r in all_cases[k].reads]
        names = ["%s" % n for k in ks for n in all_cases[k].names]
        engine.set_reads(reads, names)
        engine.set_samples(np.repeat(np.arange(len(ks), dtype=np.int32), [len(all_cases[k].reads) for k in ks]), len(ks))
        nu = engine.cluster_samples(cid)
        want = _want([cases[("pair", group, k)] for k in ks])
        rep_of = engine.get_derep()[0]
        bad = np.flatnonzero(np.asarray(rep_of) != want[1])
        lens = np.cumsum([len(all_cases[k].reads) for k in ks])
        named = [all_cases[ks[int(np.searchsorted(lens, b, side="right"))]].name for b in bad[:8]]
        _same(engine, nu, want, (group, cid, named))
        st = engine.stats()
        for f in tot:
            tot[f] += st[f]
    return tot


@pytest.mark.parametrize("group", list(CE.PAIRS))
def test_every_group_as_one_batch(engine, group, expectations):
    _batches(engine, group, expectations)


@pytest.mark.parametrize("group", ["rows5", "rows8", "rows10", "multipass", "limits"])
def test_sample_by_sample(engine, group, expectations):
    """a sample clustered alone: ITS longest read selects the rows per lane, the passes and the LDS sizes"""
    for k, case in enumerate(CE.PAIRS[group]()):
        _solo(engine, case, expectations[("pair", group, k)])


@pytest.mark.parametrize("window", ["1", "4096"])
@pytest.mark.parametrize("walk", list(CE.WALKS))
def test_walks(engine, walk, window, expectations, monkeypatch):
    monkeypatch.setenv("ITSX_CL_WINDOW", window)
    _solo(engine, CE.WALKS[walk](), expectations[("walk", walk, 0)])


@pytest.mark.parametrize("env", [("ITSX_CL_NOPRECHECK", "1"), ("ITSX_CL_NOSCORE", "1"), ("ITSX_CL_ROWS", "5"), ("ITSX_CL_ROWS", "8"), ("ITSX_CL_ROWS", "10")],
                         ids=lambda e: "%s=%s" % e)
@pytest.mark.parametrize("group", ["threshold", "ties", "unlike_targets", "contained"])
def test_switches_change_nothing(engine, group, env, expectations, monkeypatch):
    monkeypatch.setenv(*env)
    _batches(engine, group, expectations)


@pytest.mark.parametrize("group", ["contained", "multipass"])
def test_with_a_helper_context(engine, helper, group, expectations):
    for k, case in enumerate(CE.PAIRS[group]()):
        _solo(engine, case, expectations[("pair", group, k)], helpers=[helper])


def test_the_named_paths_ran(engine, expectations, monkeypatch):
    # the certificate proves rejections at K + 1 edits without the dynamic program
    st = _batches(engine, "threshold", expectations)
    assert st["cl_certified"] > 0
    monkeypatch.setenv("ITSX_CL_NOPRECHECK", "1")
    st0 = _batches(engine, "threshold", expectations)
    assert st0["cl_certified"] == 0 and st0["cl_alignments"] > st["cl_alignments"]
    monkeypatch.delenv("ITSX_CL_NOPRECHECK")
    # the score pass takes the weakly seeded candidates of unlike length; without it they are aligned in full
    st = _batches(engine, "unlike_targets", expectations)
    monkeypatch.setenv("ITSX_CL_NOSCORE", "1")
    st1 = _batches(engine, "unlike_targets", expectations)
    assert st1["cl_alignments"] > st["cl_alignments"]
