"""The MSV filter's floored row (csrc/k_msv.hip: two packed instructions per register instead of three) where the naive version of it
is wrong: chains that start below bm0 - tec (reads that begin with N), lanes whose xB rises at different rows of a ragged wave,
overflow, narrow and full-width models, and saved / restored / joined states of the shared schedules.  hmmsearch's first filter
(p7_MSVFilter; reference call site itsxpress/SeqSample.py:191-209) is integer arithmetic: the bar is equality with the CPU oracle on
EVERY (representative, profile) pair -- a search with F1 = 1.0 keeps every pair on the trace with its xJ byte.  `pytest -m gpu`."""
import numpy as np
import pytest

import orc
import synth
from edge_cases import _stretch
from test_gpu_parity import _its2_subset
from test_gpu_share import _run

pytestmark = pytest.mark.gpu

_ENV = ("ITSX_SHARE", "ITSX_SHARE_B", "ITSX_SHARE_GB", "ITSX_SHARE_MIN", "ITSX_SHARE_CHECK", "ITSX_CHUNK_UNIQUES", "ITSX_SHARE_TWO",
        "ITSX_MSV_FLOOR")
ACGT = np.frombuffer(b"ACGT", np.uint8)
# the unshared kernel, and the shared one whatever the shared fraction
BOTH = ({"ITSX_SHARE": 0}, {"ITSX_SHARE_MIN": 0})


def _search(engine, hmm, seqs, monkeypatch, env=None, **flags):
    """(pair traces, stats, per-representative coordinates) of one search in full rows mode"""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    engine.set_rows_mode("full")
    try:
        engine.load_profiles(text=hmm)
        engine.set_reads(seqs)
        engine.derep()
        engine.search(**flags)
        engine.finalize()
        return engine.pairtraces(), engine.stats(), np.stack(engine.rep_coords("3_", "4_"))
    finally:
        engine.set_rows_mode(None)


def _oracle(engine, hmm, seqs, **flags):
    seed, _ = engine.get_uniques()
    useqs = [seqs[int(i)] for i in seed]
    codes, o = orc.digitize(useqs)
    return orc.SearchResult(orc.HmmSet(text=hmm), codes, o, threads=8, keep_trace=1, **flags), useqs


def _every_pair_equal(tr, st, res):
    ot = res.trace
    assert len(ot) == res.nseq * res.hs.n                                 # F1 = 1.0: every pair is on the trace
    assert len(tr) == len(ot), (len(tr), len(ot))
    assert np.array_equal(tr["rep"], ot["seq"]) and np.array_equal(tr["prof"], ot["prof"])
    bad = np.flatnonzero(tr["msv_xj"] != ot["msv_xj"])
    assert len(bad) == 0, [(int(ot["seq"][i]), int(ot["prof"][i]), int(tr["msv_xj"][i]), int(ot["msv_xj"][i])) for i in bad[:8]]
    assert np.array_equal(tr["msv_xj"], ot["msv_xj"])
    assert st["n_past_msv"] == res.counts["past_msv"]


def msv_rows(hs, i, seq):
    """the filter's plain recurrence on the oracle's own tables (rbv: biased costs by residue code and node): xJ, xB after every row and
    bm0.  For the checks that a case is what it is meant to be -- the comparison itself is against the oracle's search."""
    p = hs.msvparams(i)
    cost = hs.rbv(i).astype(np.int64)
    codes, _ = orc.digitize([seq])
    tjbm = int(orc.lib().orc_tjb_b(len(seq))) + p["tbm"]
    bm0 = max(p["base"] - tjbm, 0)
    c = np.zeros(hs.M[i] + 1, np.int64)
    xJ, xB, out = 0, bm0, []
    for x in codes[:len(seq)]:
        c[1:] = np.maximum(c[:-1], xB) + p["bias"] - cost[x, 1:]
        c[0] = 0
        xJ = max(xJ, max(int(c[1:].max()), 0) - p["tec"])
        xB = max(max(xJ, p["base"]) - tjbm, 0)
        out.append((xJ, xB))
    return out, bm0


def n_first_rows_below_the_floor(hs, useqs):
    """(read, profile) pairs whose first row's emissions are all negative while the floor bm0 is above tec: xJ stays below bm0 - tec"""
    first = orc.digitize([s[:1] for s in useqs])[0]
    n = 0
    for i in range(hs.n):
        p = hs.msvparams(i)
        cost = hs.rbv(i)
        for s, x in zip(useqs, first):
            bm0 = max(p["base"] - int(orc.lib().orc_tjb_b(len(s))) - p["tbm"], 0)
            n += bool((cost[x, 1:] > p["bias"]).all() and bm0 > p["tec"])
    return n


def _amplicons(t_hmm_text, n, seed, **kw):
    blob, offs = synth.make_reads(t_hmm_text, n, config=3, seed=synth.SEED + seed, fixed_len=0, frac_templates=1.0, rc_rate=0.0, **kw)
    return synth.to_strings(blob, offs)


# --------------------------------------------------------------------------------------------
def startup_reads(t_hmm_text):
    """about 64 reads: amplicons behind k leading N / R / Y, a read of N only, a fully degenerate read"""
    amps = sorted(set(_amplicons(t_hmm_text, 40, 31, len_range=(300, 330), n_rate=0.0)))[:3]      # (reads repeat their templates)
    assert len(amps) == 3
    seqs = []
    for k in (0, 1, 2, 15, 16, 17, 33):
        for a in amps:
            seqs += ["N" * k + a, "R" * k + a, "Y" * k + a] if k else [a]
    rng = np.random.default_rng(32)
    seqs += ["N" * 64, "".join(rng.choice(list("RYKMSWBDHVN"), 150))]
    return seqs


@pytest.mark.parametrize("profiles", ["mini", "its2"])
def test_chains_that_start_below_the_floor(engine, t_hmm_text, mini_hmm_text, monkeypatch, profiles):
    """the start-up rule: a first row whose emissions are all negative leaves xJ below bm0 - tec, where a floored row's xE = xB would
    lift it; the wave runs the plain row until its last working lane is past that"""
    hmm = mini_hmm_text if profiles == "mini" else _its2_subset(t_hmm_text, 10, 10)          # M = 25 and 11 are in the mini set
    seqs = startup_reads(t_hmm_text)
    assert 50 <= len(seqs) <= 80
    res = None
    for env in BOTH:
        tr, st, _ = _search(engine, hmm, seqs, monkeypatch, env, F1=1.0)
        if res is None:
            res, useqs = _oracle(engine, hmm, seqs, F1=1.0)
            assert n_first_rows_below_the_floor(res.hs, useqs) >= res.hs.n               # the case is not empty
        _every_pair_equal(tr, st, res)


# --------------------------------------------------------------------------------------------
def ragged_reads(t_hmm_text):
    """about 600 reads (three blocks of 256 lanes), lengths 20-620 next to each other in a wave, 2 % N, truncated reads, and reads that
    carry their 5' motif twice (s + s[:k]): lanes raise xB at different rows, and twice"""
    amps = _amplicons(t_hmm_text, 600, 33, len_range=(300, 420), n_rate=0.02)
    rng = np.random.default_rng(34)
    seqs = []
    for j, a in enumerate(amps):
        if j % 3 == 0:
            seqs.append(a[:int(rng.integers(20, len(a)))])                # truncated, down to 20 bases
        elif j % 3 == 1:
            seqs.append(a + a[:int(rng.integers(160, 621 - len(a)))])     # the 5' motif (at 60-155) a second time
        else:
            seqs.append(a)
    return seqs


@pytest.fixture(scope="module")
def ragged(t_hmm_text):
    return {"hmm": _its2_subset(t_hmm_text, 10, 10), "seqs": ragged_reads(t_hmm_text)}


def test_rising_xB_in_a_ragged_wave(engine, ragged, monkeypatch):
    hmm, seqs = ragged["hmm"], ragged["seqs"]
    L = np.array([len(s) for s in seqs])
    assert L.min() < 40 and L.max() > 600 and len(seqs) > 512
    res = None
    for env in BOTH:
        tr, st, _ = _search(engine, hmm, seqs, monkeypatch, env, F1=1.0)
        if res is None:
            res, _ = _oracle(engine, hmm, seqs, F1=1.0)
            assert (res.trace["msv_xj"] > 190).sum() > 300                # xB rose (xJ passed the base) in many pairs
        _every_pair_equal(tr, st, res)
    # counters and coordinates at the default flags
    res = None
    for env in BOTH:
        tr, st, co = _search(engine, hmm, seqs, monkeypatch, env)
        if res is None:
            res, _ = _oracle(engine, hmm, seqs)
        c = res.counts
        assert (st["n_past_msv"], st["n_past_bias"], st["n_past_fwd"]) == (c["past_msv"], c["past_bias"], c["past_fwd"]) and c["past_fwd"] > 100
        assert np.array_equal(co, np.stack(res.positions("3_", "4_")))


def test_plain_step_equals_the_floored_one(engine, ragged, monkeypatch):
    """ITSX_MSV_FLOOR=0 (the three-instruction row on every row) against the default, every pair of the ragged-wave input"""
    hmm, seqs = ragged["hmm"], ragged["seqs"]
    for env in BOTH:
        t0, s0, _ = _search(engine, hmm, seqs, monkeypatch, {**env, "ITSX_MSV_FLOOR": 0}, F1=1.0)
        assert engine.switches().get("ITSX_MSV_FLOOR") == "0"
        t1, s1, _ = _search(engine, hmm, seqs, monkeypatch, env, F1=1.0)
        assert "ITSX_MSV_FLOOR" not in engine.switches()
        assert len(t0) == len(t1) == s1["n_unique"] * s1["n_profiles"]
        assert np.array_equal(t0["rep"], t1["rep"]) and np.array_equal(t0["prof"], t1["prof"])
        assert np.array_equal(t0["msv_xj"], t1["msv_xj"]) and s0["n_past_msv"] == s1["n_past_msv"]


# --------------------------------------------------------------------------------------------
def overflow_reads(t_hmm_text):
    """reads that carry one profile's consensus two or three times back to back"""
    rng = np.random.default_rng(35)
    seqs = []
    for pre in ("3_", "4_"):
        for m in synth.consensus_motifs(t_hmm_text, pre)[:4]:
            for rep in (2, 3):
                fl = [bytes(ACGT[rng.integers(0, 4, int(n))]).decode() for n in rng.integers(10, 120, 2)]
                seqs.append(fl[0] + m * rep + fl[1])
    return seqs


def test_overflow(engine, t_hmm_text, monkeypatch):
    hmm = _its2_subset(t_hmm_text, 10, 10)
    seqs = overflow_reads(t_hmm_text)
    res = None
    for env in BOTH:
        tr, st, _ = _search(engine, hmm, seqs, monkeypatch, env, F1=1.0)
        if res is None:
            res, _ = _oracle(engine, hmm, seqs, F1=1.0)
            assert (res.trace["msv_xj"] == 255).any()
        _every_pair_equal(tr, st, res)


# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["mini", "46"])
def test_model_widths(engine, t_hmm_text, mini_hmm_text, monkeypatch, width):
    """11 and 25 nodes (padding cells sit on the floor) and 46 (no padding cell)"""
    hmm = mini_hmm_text
    if width == "46":
        blocks = [b + "//\n" for b in mini_hmm_text.split("//\n") if "NAME  " in b]
        hmm = _stretch(next(b for b in blocks if "LENG  45" in b), 46) + blocks[1]
        assert orc.HmmSet(text=hmm).M[0] == 46
    blob, offs = synth.make_reads(mini_hmm_text, 400, seed=3)
    seqs = synth.to_strings(blob, offs)
    res = None
    for env in BOTH:
        tr, st, _ = _search(engine, hmm, seqs, monkeypatch, env, F1=1.0)
        if res is None:
            res, _ = _oracle(engine, hmm, seqs, F1=1.0)
            assert (res.trace["msv_xj"] > 190).sum() > 50
            if width == "mini":
                assert sorted(res.hs.M)[:2] == [11, 25]
        _every_pair_equal(tr, st, res)


# --------------------------------------------------------------------------------------------
def _sub(v, pos):
    w = v.copy(); w[pos] = ACGT[(np.searchsorted(ACGT, w[pos]) + 1) % 4]
    return w


def sharing_families(t_hmm_text):
    """families for the prefix / suffix trees: a template plus variants with one substitution at rows 31 / 32 / 33 / 63 / 64 / 65 and in
    the last block; a family whose 5' hit ends before the first block boundary (the saved state has xB above bm0: `early`); a family
    whose template starts with N; recombinants without a row of their own.  Returns (reads, the early family's template)."""
    rng = np.random.default_rng(36)
    lm = synth.consensus_motifs(t_hmm_text, "3_")[0]
    rm = synth.consensus_motifs(t_hmm_text, "4_")[0]
    out, early = [], None
    for fam, L in enumerate((300, 320, 352, 417)):
        base = ACGT[rng.integers(0, 4, L)].copy()
        a = 2 if fam == 1 else 70                                          # fam 1: the 5' hit is over at row 47
        base[a:a + 45] = np.frombuffer(lm.encode(), np.uint8)
        base[L - 105:L - 60] = np.frombuffer(rm.encode(), np.uint8)
        if fam == 2:
            base[0] = ord("N")
        if fam == 1:
            early = bytes(base).decode()
        members = [base] + [_sub(base, p) for p in (31, 32, 33, 63, 64, 65, 100, 200, L - 20, L - 3, L - 1)]
        # recombinants: the prefix of one member with the suffix of another
        x, y = _sub(base, 40), _sub(base, L - 5)
        z = x.copy(); z[L - 5] = y[L - 5]
        members += [x, y, z]
        out += [bytes(m).decode() for m in members]
    order = rng.permutation(len(out))
    return [out[i] for i in order], early


def test_saved_restored_and_joined_states(engine, t_hmm_text, monkeypatch):
    hmm = _its2_subset(t_hmm_text, 6, 6)
    seqs, early = sharing_families(t_hmm_text)
    # the early family's state at every first block boundary has xB above bm0 for some profile: a child restores a risen floor
    hs = orc.HmmSet(text=hmm)
    for B in (16, 32, 64):
        risen = []
        for i in range(hs.n):
            rows, bm0 = msv_rows(hs, i, early)
            risen.append(rows[max(B, 48) - 1][1] > bm0)
        assert any(risen), B
    ref, _ = _run(engine, hmm, seqs, "lazy", {"ITSX_SHARE": 0}, monkeypatch)
    codes, o = orc.digitize(seqs)
    nc, orep, _ = orc.derep(codes, o)
    seeds = [i for i in range(len(seqs)) if orep[i] == i]
    c2, o2 = orc.digitize([seqs[i] for i in seeds])
    res = orc.SearchResult(hs, c2, o2, threads=8, keep_trace=0)
    uo = (np.cumsum(np.asarray(orep) == np.arange(len(seqs))) - 1)[np.maximum(orep, 0)]
    exp = np.stack([x[uo] for x in res.positions("3_", "4_")])
    assert np.array_equal(exp, np.stack(ref[0])) and (exp[0] >= 0).sum() > 40
    for B in (16, 32, 64):
        for two in ({}, {"ITSX_SHARE_TWO": 0}):
            got, st = _run(engine, hmm, seqs, "lazy", {"ITSX_SHARE_CHECK": 1, "ITSX_SHARE_MIN": 0, "ITSX_SHARE_B": B, **two}, monkeypatch)
            assert st["share_B"] == B and st["share_chains"] > 20 and st["two_sided"] == (0 if two else 1), (B, two)
            assert st["share_mismatch"] == 0, (B, two)
            assert all(np.array_equal(x, y) for x, y in zip(ref[0], got[0])), (B, two)
            assert np.array_equal(exp, np.stack(got[0])), (B, two)
