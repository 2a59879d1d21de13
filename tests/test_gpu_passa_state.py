"""Pass A's two-array row state on the GPU (csrc/k_lazy.hip): k_fwd_bound carries (S, I+) and k_bwd_bound its dual (W, G); a saved
state is 25 float4.  Whatever the schedule -- block size, one- or two-sided, plain or folded recurrences, profiles in ranges, three
batches or four, rescales on many rows -- the shared scores are bitwise the unshared kernel's, a joined score is the walked one
within 2e-3 nats, the bound is HMMER's own Forward within 1e-3 nats, and every coordinate is the unshared search's and the full
table's.  The profiles include a 46-node model: the last pair's second node is live.  `pytest -m gpu`."""
import functools

import numpy as np
import pytest

import edge_cases
import synth
from test_gpu_compact import _same
from test_gpu_parity import _its2_subset
from test_gpu_share import _bench_reads, _edge_reads, _run

pytestmark = pytest.mark.gpu

CHECK = {"ITSX_SHARE_CHECK": 1, "ITSX_LAZY_CHECK_BOUND": 1, "ITSX_SHARE_MIN": 0}
_cache = {}


def _hmm(t_hmm_text):
    """six profiles of each side and a seventh stretched to 46 nodes"""
    blocks = [b + "//\n" for b in t_hmm_text.split("//\n") if "NAME  " in b]
    b46 = [b for b in blocks if b.split("NAME  ")[1].startswith("3_")][6]
    return _its2_subset(t_hmm_text, 6, 6) + edge_cases._stretch(b46, 46)


def _family(engine, t_hmm_text, monkeypatch):
    """~3 000 family reads and their coordinates without sharing, in the lazy and in the full rows mode (computed once)"""
    if "family" not in _cache:
        hmm = _hmm(t_hmm_text)
        seqs = _bench_reads(t_hmm_text, 3000, seed=9)
        lazy, st0 = _run(engine, hmm, seqs, "lazy", {"ITSX_SHARE": 0}, monkeypatch)
        full, _ = _run(engine, hmm, seqs, "full", {"ITSX_SHARE": 0}, monkeypatch)
        assert st0["share_B"] == 0
        _cache["family"] = (hmm, seqs, lazy, full)
    return _cache["family"]


def _check(st, got, lazy, full, tag):
    print(tag, {k: st[k] for k in ("share_B", "share_batches", "share_mismatch", "join_maxdiff", "lazy_bound_maxdiff", "two_sided", "n_joined")})
    assert st["share_mismatch"] == 0, tag
    assert st["join_maxdiff"] < 2e-3, tag
    assert st["lazy_bound_maxdiff"] < 1e-3, tag
    assert _same(lazy, got) and _same(full, got), tag


@pytest.mark.parametrize("B", [16, 32])
def test_default_schedule(engine, t_hmm_text, monkeypatch, B):
    hmm, seqs, lazy, full = _family(engine, t_hmm_text, monkeypatch)
    got, st = _run(engine, hmm, seqs, "lazy", {**CHECK, "ITSX_SHARE_B": B}, monkeypatch)
    assert st["share_B"] == B and st["share_chains"] > 0 and st["two_sided"] == 1 and st["n_joined"] > 0
    _check(st, got, lazy, full, "B=%d" % B)


def test_rescales_on_many_rows(engine, t_hmm_text, monkeypatch):
    """1e4 instead of 1e20: a domain rescales its rows several times, inside blocks and at their boundaries"""
    hmm, seqs, lazy, full = _family(engine, t_hmm_text, monkeypatch)
    monkeypatch.setenv("ITSX_BOUND_RESCALE_EXP", "4")
    got, st = _run(engine, hmm, seqs, "lazy", dict(CHECK), monkeypatch)
    assert st["share_B"] == 32 and st["n_joined"] > 0
    _check(st, got, lazy, full, "rescale")


@pytest.mark.parametrize("env", [{"ITSX_SHARE_TWO": 0}, {"ITSX_BOUND_FOLD": 0}, {"ITSX_SHARE_GB": 0.0005}], ids=["one_sided", "plain", "ranges"])
def test_schedule_arms(engine, t_hmm_text, monkeypatch, env):
    hmm, seqs, lazy, full = _family(engine, t_hmm_text, monkeypatch)
    for k, v in env.items():
        if k == "ITSX_BOUND_FOLD":
            monkeypatch.setenv(k, str(v))          # (not one of the switches _run resets)
    got, st = _run(engine, hmm, seqs, "lazy", {**CHECK, **env}, monkeypatch)
    assert st["share_B"] == 32 and st["share_chains"] > 0
    if "ITSX_SHARE_GB" in env:
        assert st["share_batches"] > 1 and st["two_sided"] == 1
    else:
        assert st["two_sided"] == 0               # (the plain recurrences share one-sidedly by the engine's own rule)
    _check(st, got, lazy, full, str(env))


def test_budget_divisor(engine, t_hmm_text, monkeypatch):
    hmm, seqs, lazy, full = _family(engine, t_hmm_text, monkeypatch)
    nb = []
    for div in ("3.8", "2.8"):
        monkeypatch.setenv("ITSX_SHARE_DIV", div)
        got, st = _run(engine, hmm, seqs, "lazy", dict(CHECK), monkeypatch)
        _check(st, got, lazy, full, "div=" + div)
        nb.append(st["share_batches"])
    assert nb[0] > nb[1], nb


def test_edge_reads(engine, t_hmm_text, monkeypatch):
    """reads shorter than, as long as and just past one and two blocks, and one family of ~2.3 kb, at F1 = F2 = F3 = 0.5 so that the
    short ones reach pass A"""
    rng = np.random.default_rng(91)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    lm = synth.consensus_motifs(t_hmm_text, "3_")[0]
    rm = synth.consensus_motifs(t_hmm_text, "4_")[0]
    seqs = _edge_reads(rng, lm, rm)
    for L in (15, 16, 17, 31, 32, 33, 64, 65):
        base = np.frombuffer(((lm + rm) * 2)[:L].encode(), np.uint8).copy()
        fam = [base]
        for pos in sorted({0, 1, L // 2, 14, 15, 16, 31, 32, L - 1} & set(range(L))):
            v = base.copy(); v[pos] = acgt[(np.searchsorted(acgt, v[pos]) + 1) % 4]; fam.append(v)
            x = base.copy(); x[pos] = ord("N"); fam.append(x)
        seqs += [bytes(s).decode() for s in fam]
    base = acgt[rng.integers(0, 4, 2300)].copy()
    for a in range(200, 1900, 700):
        base[a:a + 45] = np.frombuffer(lm.encode(), np.uint8)
        base[a + 250:a + 295] = np.frombuffer(rm.encode(), np.uint8)
    for j in range(30):
        v = base.copy()
        for pos in rng.integers(0, 2300, 3):
            v[pos] = acgt[(np.searchsorted(acgt, v[pos]) + 1 + rng.integers(0, 3)) % 4]
        seqs.append(bytes(v).decode())
    hmm = _hmm(t_hmm_text)
    monkeypatch.setattr(engine, "search", functools.partial(engine.search, F1=0.5, F2=0.5, F3=0.5))
    lazy, _ = _run(engine, hmm, seqs, "lazy", {"ITSX_SHARE": 0}, monkeypatch)
    full, _ = _run(engine, hmm, seqs, "full", {"ITSX_SHARE": 0}, monkeypatch)
    for B in (16, 32):
        got, st = _run(engine, hmm, seqs, "lazy", {**CHECK, "ITSX_SHARE_B": B}, monkeypatch)
        assert st["share_B"] == B and st["share_chains"] > 50
        _check(st, got, lazy, full, "edges B=%d" % B)
