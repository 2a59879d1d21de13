"""Where the MSV filter keeps a lane's packed words (csrc/k_msv.hip), ITSX_MSV_WHOLE: 2 -- a wave of shared chains loads the WINDOW
of its rows once, the words from row0 >> 4 on, at most 16, indexed from the window's first word, and a wave whose window is longer
refills 16 words every 256 rows; 1, and the unshared kernel under 2 -- the whole read when the launch's longest fits 37 words; 0 -- 16
words at a time everywhere.  hmmsearch's first filter (p7_MSVFilter; reference call site itsxpress/SeqSample.py:191-209) is integer arithmetic
and the layout is none of its business: for every case and every layout arm, unshared, one-sided and two-sided, every
(representative, profile) cell equals the CPU oracle at F1 = 1.0 (a search that keeps every pair on the trace with its xJ byte) and
ITSX_SHARE_CHECK=1 -- the shared kernel's cells against the unshared kernel's, every one -- counts no difference.  A two-sided search is
a lazy one and keeps no trace: its cells are held to the unshared kernel's by that count, and those to the oracle by the unshared
search of the same arm.  The cases are the edges of the indexing.  `pytest -m gpu`."""
import numpy as np
import pytest

import orc
import synth
from edge_cases import _stretch
from test_gpu_msv_floor import ACGT, _every_pair_equal, _oracle, _search, _sub

pytestmark = pytest.mark.gpu

# the default, windows, the whole read, 16 words at a time
ARMS = ({}, {"ITSX_MSV_WHOLE": 2}, {"ITSX_MSV_WHOLE": 1}, {"ITSX_MSV_WHOLE": 0})
_OWN_ENV = ("ITSX_MSV_WHOLE", "ITSX_TEST_HOOKS", "ITSX_MSV_PB", "ITSX_PASSA_DBG")


@pytest.fixture(scope="module")
def hmm3(mini_hmm_text):
    """46 nodes (no padding cell), 45, and mini.hmm's 25- and 11-node profiles (padding cells on the floor)"""
    blocks = [b + "//\n" for b in mini_hmm_text.split("//\n") if "NAME  " in b]
    pick = lambda s: next(b for b in blocks if s in b)
    hmm = _stretch(pick("NAME  3_End_Tracheophyta_58S_end_eight_long"), 46) + pick("NAME  4_LSU_Tracheophyta_4_LSU_start_eight_long") + \
        pick("LENG  25") + pick("LENG  11")
    assert sorted(orc.HmmSet(text=hmm).M) == [11, 25, 45, 46]
    return hmm


@pytest.fixture(scope="module")
def motifs(mini_hmm_text):
    return [synth.consensus_motifs(mini_hmm_text, p)[0] for p in ("3_", "4_")] + synth.consensus_motifs(mini_hmm_text, "1_SSU_Chlorophyta")


def _template(rng, L, motifs):
    """random bases with the profiles' consensus strings where they fit: 3_ near the 5' end, 4_ near the 3' end, the short ones between;
    two fifths of a motif's bases redrawn, so that the hits are hits of every strength and few of them overflow"""
    base = ACGT[rng.integers(0, 4, L)].copy()
    for at, m in zip((L // 8, L - L // 8 - 45, L // 2, L // 2 + 30), motifs):
        if 0 <= at and at + len(m) <= L and L >= 100:
            v = np.frombuffer(m.encode(), np.uint8).copy()
            hit = rng.random(len(v)) < 0.4
            v[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
            base[at:at + len(m)] = v
    return base


def _with(v, subs=(), ns=()):
    w = v.copy()
    for p in subs:
        w = _sub(w, p)
    for p in ns:
        w[p] = ord("N")
    return w


def _strings(members, rng):
    seqs = sorted({bytes(m).decode() for m in members})
    return [seqs[i] for i in rng.permutation(len(seqs))]


def _set(monkeypatch, env):
    for k in _OWN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if k in _OWN_ENV:
            monkeypatch.setenv(k, str(v))


def _lazy_stats(engine, hmm, seqs, monkeypatch, env, **flags):
    """the statistics of one lazy (two-sided) search; the environment as _search sets it"""
    from test_gpu_msv_floor import _ENV
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    engine.set_rows_mode("lazy")
    try:
        engine.load_profiles(text=hmm)
        engine.set_reads(seqs)
        engine.derep()
        engine.search(**flags)
        engine.finalize()
        return engine.stats()
    finally:
        engine.set_rows_mode(None)


def _paths(engine, monkeypatch, capfd, hmm, seqs, env):
    """where the shared kernel's waves took their words from in a one-sided search, and the most ranges a batch took its profiles in:
    the diagnostic line of ITSX_TEST_HOOKS=1 ITSX_PASSA_DBG=64 (a counting instantiation of the same kernel source)"""
    import re
    env = {"ITSX_TEST_HOOKS": 1, "ITSX_PASSA_DBG": 64, "ITSX_SHARE_MIN": 0, "ITSX_SHARE_TWO": 0, **env}
    _set(monkeypatch, env)
    capfd.readouterr()
    _, st, _ = _search(engine, hmm, seqs, monkeypatch, env, F1=1.0)
    err = capfd.readouterr().err
    _set(monkeypatch, {})
    m = re.search(r"msv shared waves: whole read (\d+), window (\d+), 16 words at a time (\d+); profile ranges of a batch: at most (\d+)", err)
    assert m and st["share_chains"] > 0, err[-400:]
    return dict(zip(("whole", "window", "staged", "ranges"), map(int, m.groups())))


def _check(engine, monkeypatch, hmm, seqs, B=32, extra=None, want_join=True):
    """every arm x (unshared, one-sided, two-sided); returns the statistics of the default arm's one-sided and two-sided searches"""
    extra = extra or {}
    res, out = None, None
    for arm in ARMS:
        env = {**arm, **extra}
        _set(monkeypatch, env)
        tr, st, _ = _search(engine, hmm, seqs, monkeypatch, {"ITSX_SHARE": 0, **env}, F1=1.0)
        if res is None:
            res, _ = _oracle(engine, hmm, seqs, F1=1.0)                    # (one oracle run per case)
        assert st["share_B"] == 0, arm
        _every_pair_equal(tr, st, res)
        shared = {"ITSX_SHARE_MIN": 0, "ITSX_SHARE_CHECK": 1, "ITSX_SHARE_B": B, **env}
        _set(monkeypatch, env)
        tr, st1, _ = _search(engine, hmm, seqs, monkeypatch, {**shared, "ITSX_SHARE_TWO": 0}, F1=1.0)
        assert st1["share_B"] == B and st1["share_chains"] > 0 and st1["two_sided"] == 0, (arm, st1["share_B"], st1["share_chains"])
        assert st1["share_mismatch"] == 0, arm
        _every_pair_equal(tr, st1, res)
        _set(monkeypatch, env)
        st2 = _lazy_stats(engine, hmm, seqs, monkeypatch, shared, F1=1.0)
        assert st2["share_B"] == B and st2["two_sided"] == 1 and st2["share_chains"] > 0, (arm, st2["share_B"], st2["two_sided"])
        assert st2["share_mismatch"] == 0, arm
        assert st2["n_past_msv"] == res.counts["past_msv"] == res.nseq * res.hs.n
        if want_join:
            assert st2["n_joined"] > 0, arm
        if out is None:
            out = (st1, st2)
    _set(monkeypatch, {})
    return out


# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 32, 64])
def test_lengths_at_the_word_and_stage_edges(engine, hmm3, motifs, monkeypatch, B):
    """reads of 15 / 16 / 17 bases (one word, exactly one, one base into the second) and 255 / 256 / 257 / 272 (one stage of 16 words,
    one row into the second, one word into it): a template per length, variants that part from it at the first / a middle / the last
    base, an N there instead, and the same prefix one and two bases shorter"""
    rng = np.random.default_rng(801)
    members = []
    for L in (15, 16, 17, 255, 256, 257, 272):
        base = _template(rng, L, motifs)
        members.append(base)
        for p in sorted({0, 1, L // 2, 15 if L > 15 else L - 2, 16 if L > 16 else L - 3, L - 2, L - 1, min(L - 1, 255), min(L - 1, 256)}):
            members += [_with(base, [p]), _with(base, ns=[p])]
        members += [base[:L - 1], base[:L - 2]] if L > 20 else []
    seqs = _strings(members, rng)
    assert len(seqs) < 200
    _check(engine, monkeypatch, hmm3, seqs, B, want_join=B <= 32)


@pytest.mark.parametrize("longest", [592, 593])
def test_the_whole_read_switch(engine, hmm3, motifs, monkeypatch, longest):
    """the launch's longest read is 592 bases (37 words: the whole-read arm and the unshared kernel keep every word in LDS) or 593 (38:
    they stage 16 at a time): families at that length and at 300, variants that part in the first, a middle and the last word"""
    rng = np.random.default_rng(802 + longest)
    members = []
    for L in (300, longest):
        base = _template(rng, L, motifs)
        members.append(base)
        for p in (5, 40, 100, 250, 257, L - 20, L - 1):
            members += [_with(base, [p]), _with(base, [p], ns=[min(L - 1, p + 3)])]
        members.append(_with(base, ns=[L - 1]))
    seqs = _strings(members, rng)
    assert max(len(s) for s in seqs) == longest
    _check(engine, monkeypatch, hmm3, seqs, 32)


@pytest.mark.parametrize("B", [16, 32, 64])
def test_windows(engine, hmm3, motifs, monkeypatch, B):
    """chains that start at a row0 that is no multiple of 256 (variants that part at 70, 100, 200, 300, 400: row0 = 64 ... 384);
    windows that straddle row 256 (a 330-base variant from 200: words 12 .. 20); windows longer than 16 words, which fall back to
    16 words every 256 rows (a 580-base variant from 70: 32 words; every template: row0 = 0); an N on the first row of a window
    and on the row after a restore (where the variant parts, a multiple of 64, and one row later), on the last row before a refill
    and the first after it (255 / 256, 511 / 512) and on row 0; recombinants, which save a state and join at one boundary"""
    rng = np.random.default_rng(803)
    members = []
    for L in (330, 420, 580):
        base = _template(rng, L, motifs)
        members.append(base)
        for p in (70, 100, 200, 300, 400):
            if p < L - 1:
                members.append(_with(base, [p]))
        for p in (64, 128, 192, 256, 320, 384, 512):
            if p + 1 < L:
                members += [_with(base, ns=[p]), _with(base, [p], ns=[p + 1])]
        for p in (255, 256, 511, 512):
            if p < L:
                members += [_with(base, [70], ns=[p]), _with(base, ns=[p])]
        members.append(_with(base, ns=[0]))
        # x parts from the template in block 1 and ends like it: it joins after its first block.  z parts from x one block later: x saves
        # the state z starts from at the boundary at which it joins itself.  y, u: the same at the 3' end
        p1, p2 = B + B // 4, 2 * B + B // 8
        members += [_with(base, [p1]), _with(base, [p1, p2]), _with(base, [L - 5]), _with(base, [p1, L - 5]), _with(base, [p1, p2, L - 5])]
    seqs = _strings(members, rng)
    assert len(seqs) < 200
    st1, st2 = _check(engine, monkeypatch, hmm3, seqs, B)
    assert st1["share_nodes"] > 10 and st2["n_joined"] > 3 and st2["bwd_chains"] > 0


def test_the_waves_take_the_path_that_is_meant(engine, hmm3, motifs, monkeypatch, capfd):
    """under 2 the short windows are loaded once and the long ones (the templates, a 580-base variant from row 64) fall back to 16
    words at a time; under 1 every wave keeps whole reads (the longest has 37 words); under 0 every wave stages; a window of exactly 16
    words (rows 64 .. 320 of a 320-base read) is loaded once"""
    rng = np.random.default_rng(807)
    members = []
    # (a wave holds the chains of one depth whatever their lengths: each depth here has chains of one family only)
    base = _template(rng, 580, motifs)
    members += [base, _with(base, [70])]                       # from row 0: 37 words; from row 64: 33
    base = _template(rng, 330, motifs)
    members += [base, _with(base, [200]), _with(base, [300])]  # from row 0: 21 words; from row 192: 9; from row 288: 3
    seqs = _strings(members, rng)
    got = {w: _paths(engine, monkeypatch, capfd, hmm3, seqs, {"ITSX_MSV_WHOLE": w, "ITSX_SHARE_B": 32}) for w in (2, 1, 0)}
    assert got[2]["window"] > 0 and got[2]["staged"] > 0 and got[2]["whole"] == 0, got
    assert got[1]["whole"] > 0 and got[1]["window"] == 0 and got[1]["staged"] == 0, got
    assert got[0]["staged"] > 0 and got[0]["window"] == 0 and got[0]["whole"] == 0, got
    assert got[2]["window"] + got[2]["staged"] == got[1]["whole"] == got[0]["staged"], got
    # one family whose only shared chain walks rows 64 .. 320: words 4 .. 19, exactly 16
    base = _template(rng, 320, motifs)
    one = _paths(engine, monkeypatch, capfd, hmm3, _strings([base, _with(base, [70])], rng), {"ITSX_MSV_WHOLE": 2, "ITSX_SHARE_B": 64})
    assert one["window"] >= 1 and one["staged"] >= 1, one          # (the template itself, 20 words from row 0, stages)
    assert one["window"] + one["staged"] == 2, one


def test_one_valid_lane_and_a_nearly_empty_block(engine, hmm3, motifs, monkeypatch):
    """257 chains of one depth (variants of one template inside rows 64 .. 95: two blocks of lanes, the second with one valid lane) and
    a depth with one chain (the one variant that parts at 200)"""
    rng = np.random.default_rng(804)
    base = _template(rng, 300, motifs)
    members, seen = [base, _with(base, [200])], set()
    while len(seen) < 257:
        p, q = sorted(int(x) for x in rng.integers(64, 96, 2))
        r = int(rng.integers(0, 3))
        if p == q or (p, q, r) in seen:
            continue
        seen.add((p, q, r))
        v = _with(base, [p])
        v[q] = ACGT[(np.searchsorted(ACGT, v[q]) + 1 + r) % 4]
        members.append(v)
    seqs = _strings(members, rng)
    assert len(seqs) == 259
    st1, _ = _check(engine, monkeypatch, hmm3, seqs, 32)
    assert st1["share_chains"] >= 258


def test_a_ragged_wave(engine, hmm3, motifs, monkeypatch):
    """chains of one depth from 40 to 580 bases in one wave: most lanes end long before the wave's last row, and the wave's window
    (from row 32 to 580) is the longest lane's"""
    rng = np.random.default_rng(805)
    members = []
    for L in (40, 41, 100, 180, 257, 330, 580):
        base = _template(rng, L, motifs)
        members.append(base)
        for p in range(32, 40):
            members.append(_with(base, [p]))
    seqs = _strings(members, rng)
    _check(engine, monkeypatch, hmm3, seqs, 32, want_join=False)


@pytest.mark.parametrize("PB", [2, 3])
def test_profile_blocks_and_ranges(engine, hmm3, motifs, monkeypatch, capfd, PB):
    """blocks that take their lanes through PB profiles (test hook ITSX_MSV_PB; a job of this size gets 1): 4 profiles in blocks of 2
    (the last profile of the last block is the range's last) and of 3 (the last block is cut short); and with a slot budget that
    the one batch's states overfill, the profiles in several ranges, blocks cut at each range's end"""
    rng = np.random.default_rng(806)
    members = []
    for t in range(7):
        base = _template(rng, 580, motifs)
        members.append(base)
        for d in range(1, 35):
            members.append(_with(base, [16 * d + int(rng.integers(0, 16))]))
    seqs = _strings(members, rng)
    assert len(seqs) < 250
    hooks = {"ITSX_TEST_HOOKS": 1, "ITSX_MSV_PB": PB}
    _check(engine, monkeypatch, hmm3, seqs, 16, extra=hooks)
    st1, st2 = _check(engine, monkeypatch, hmm3, seqs, 16, extra={**hooks, "ITSX_SHARE_GB": 0.0002})
    # 0.0002 GB hold 214 748 / (256 B x 4 profiles) = 209 states of the filter (fewer of pass A's): a batch cannot be cut inside a
    # length, so this one, with more, takes its profiles in ranges
    assert st1["share_batches"] == 1 and st1["share_nodes"] > 209
    assert st2["share_batches"] == 1
    assert _paths(engine, monkeypatch, capfd, hmm3, seqs, {"ITSX_MSV_PB": PB, "ITSX_SHARE_B": 16, "ITSX_SHARE_GB": 0.0002})["ranges"] >= 2
