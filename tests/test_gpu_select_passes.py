"""The list-building passes between the DP kernels, each against a plain numpy statement of what it computes:

* the lazy stage's selection (k_lazy.hip: one bit per pair, a scan over the chunks of 64, one scatter) for round 0, round 1, the
  top-up round's marking and its key list;
* the envelope memoisation's table (k_derep.hip: k_region_keys with its wave-combined, pre-checked atomics, k_region_resolve);
* launch_exclusive_scan (k_util.hip).

Every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048                      # k_util.hip: elements one block of the scan takes


# ------------------------------------------------------------------------------------------------ scan
def _scan(engine, x, in_place):
    x = np.ascontiguousarray(x, np.int32)
    out = np.full(len(x), -7, np.int32)
    engine._chk(engine.L.itsx_debug_scan(engine.h, x.ctypes.data, len(x), out.ctypes.data, int(in_place)))
    return out


@pytest.mark.parametrize("in_place", [0, 1])
def test_exclusive_scan_sizes(engine, in_place):
    rng = np.random.default_rng(11)
    for n in (0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 1, SCAN_TILE * SCAN_TILE + 1):
        x = rng.integers(0, 65, n).astype(np.int32)
        exp = (np.cumsum(x, dtype=np.int64) - x).astype(np.int32)
        assert np.array_equal(_scan(engine, x, in_place), exp), n


# ------------------------------------------------------------------------------------------------ selection
class PairLists:
    """a pair list of seven profiles whose chunks span three tiles of the chunk scan plus one: [0] large and mixed, [1] no pairs, [2] / [3]
    exactly 64 / 65 pairs to select, [4] none, [5] all, [6] mixed; every segment ends in padding records (prof < 0, all 0xFF) unless its
    length is a multiple of 64, and some pairs are already done or ran for their row states only (xj < 0)"""
    P = 7
    NCLS = 6
    CLS = np.array([0, 1, 2, 3, 4, 5, 0], np.int8)

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        nch = 3 * SCAN_TILE + 1
        tot = [0, 0, 64 * 9 + 1, 64 * 7 + 63, 64 * 5, 64 * 3 + 17, 64 * 40 + 5]
        used = sum((t + 63) // 64 for t in tot)
        tot[0] = (nch - used) * 64 - 23
        self.total = np.array(tot, np.int64)
        self.seg = np.zeros(self.P + 1, np.int64)
        self.seg[1:] = np.cumsum((self.total + 63) // 64 * 64)
        self.NP = int(self.seg[-1])
        assert self.NP == nch * 64
        pr = np.full((self.NP, 4), -1, np.int32)
        for p in range(self.P):
            a, n = int(self.seg[p]), int(self.total[p])
            pr[a:a + n, 0] = np.arange(n)                          # useq: the position inside the segment
            pr[a:a + n, 1] = p
            pr[a:a + n, 2] = rng.integers(0, 256, n)
            pr[a:a + n, 3] = rng.integers(300, 580, n)
        self.pairs = pr
        self.real = pr[:, 1] >= 0
        self.U = int(self.total.max())
        self.done = np.zeros(self.NP, np.uint8)
        self.b10 = np.zeros(self.NP, np.uint32)

    def rows(self, p):
        return np.arange(int(self.seg[p]), int(self.seg[p] + self.total[p]))

    def pick(self, rng, p, k):
        return rng.choice(self.rows(p), k, replace=False)


def _flags(mode, pl, done, b10, group=None, sorted_uniq=None, slot=None, cutoff=None):
    useq, prof, xj = pl.pairs[:, 0].astype(np.int64), pl.pairs[:, 1].astype(np.int64), pl.pairs[:, 2]
    live = pl.real & (done == 0)
    ps, us = np.where(pl.real, prof, 0), np.where(pl.real, useq, 0)
    i = np.arange(pl.NP, dtype=np.uint64)
    if mode == 0:
        g = group[us * pl.NCLS + pl.CLS[ps]]
        return live & ((g & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF) - i)
    if mode == 1:
        bc = group[sorted_uniq[us].astype(np.int64) * pl.NCLS + pl.CLS[ps]]
        return live & ((bc == 0) | (b10.astype(np.uint64) >= (bc >> np.uint64(40))))
    sl = slot[ps]
    live = live & (xj >= 0) & (sl >= 0)
    if mode == 3:
        return live
    hi, lo = cutoff[2 * np.maximum(sl, 0)], cutoff[2 * np.maximum(sl, 0) + 1]
    return live & (((hi > 0) & (b10 >= hi)) | ((lo > 0) & (b10 <= lo)))


def _expected_list(pl, f):
    seg = np.zeros(pl.P + 1, np.int64)
    parts = []
    for p in range(pl.P):
        idx = np.flatnonzero(f[pl.seg[p]:pl.seg[p + 1]]) + pl.seg[p]
        pad = (-len(idx)) % 64
        seg[p + 1] = seg[p] + len(idx) + pad
        parts += [pl.pairs[idx], np.full((pad, 4), -1, np.int32)]
    return seg, np.concatenate(parts).reshape(-1, 4)


def _select(engine, mode, pl, done, b10, group=None, sorted_uniq=None, slot=None, cutoff=None, n_slots=0):
    done = done.copy()
    out_seg = np.full(pl.P + 1, -1, np.int64)
    out_pairs = np.full((pl.NP, 4), 12345, np.int32)
    keys, vals = np.zeros(pl.NP, np.uint64), np.zeros(pl.NP, np.int32)
    n = C.c_int64(-1)
    ptr = lambda a: a.ctypes.data if a is not None else None
    engine._chk(engine.L.itsx_debug_select(
        engine.h, mode, pl.pairs.ctypes.data, pl.NP, pl.seg.ctypes.data, pl.P, done.ctypes.data, b10.ctypes.data,
        pl.CLS.ctypes.data, pl.NCLS, ptr(group), 0 if group is None else len(group), ptr(sorted_uniq), 0 if sorted_uniq is None else len(sorted_uniq),
        ptr(slot), ptr(cutoff), n_slots, out_seg.ctypes.data, out_pairs.ctypes.data, pl.NP, keys.ctypes.data, vals.ctypes.data, C.byref(n)))
    return done, out_seg, out_pairs[:max(n.value, 0)], keys[:max(n.value, 0)], vals[:max(n.value, 0)], n.value


def _check_list(engine, mode, pl, done, b10, counts=None, **kw):
    f = _flags(mode, pl, done, b10, **{k: v for k, v in kw.items() if k != "n_slots"})
    if counts is not None:
        got_counts = [int(f[pl.seg[p]:pl.seg[p + 1]].sum()) for p in range(pl.P)]
        for p, c in counts.items():
            assert got_counts[p] == c, (p, got_counts)
    exp_seg, exp_pairs = _expected_list(pl, f)
    got_done, got_seg, got_pairs, _, _, n = _select(engine, mode, pl, done, b10, **kw)
    assert np.array_equal(got_seg, exp_seg)
    assert n == exp_seg[-1]
    assert np.array_equal(got_pairs, exp_pairs)
    assert np.array_equal(got_done, np.where(f, 1, done).astype(np.uint8))
    return f


@pytest.fixture(scope="module")
def lists():
    pl = PairLists(5)
    rng = np.random.default_rng(6)
    done = np.zeros(pl.NP, np.uint8)
    for p in (0, 6):
        done[pl.pick(rng, p, int(pl.total[p]) // 3)] = 1
    pl.done = done
    return pl


def test_select_round0(engine, lists):
    pl, rng = lists, np.random.default_rng(21)
    done = pl.done.copy()
    gtop = np.zeros(pl.U * pl.NCLS, np.uint64)
    win = lambda i: (np.uint64(1000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i.astype(np.uint64))
    # profiles 0 and 6 share class 0: a group's winner is a pair of either, or of neither; some winners are done already
    g0 = np.arange(pl.U)
    own = rng.integers(0, 3, pl.U)
    w = np.where((own == 1) & (g0 < pl.total[6]), pl.seg[6] + g0, pl.seg[0] + g0)
    gtop[g0 * pl.NCLS + 0] = np.where(own == 2, np.uint64(0), win(w))
    for p, k in ((2, 64), (3, 65), (4, 0), (5, int(pl.total[5]))):
        rows = pl.pick(rng, p, k)
        gtop[pl.pairs[rows, 0].astype(np.int64) * pl.NCLS + pl.CLS[p]] = win(rows)
    f = _check_list(engine, 0, pl, done, pl.b10, counts={1: 0, 2: 64, 3: 65, 4: 0, 5: int(pl.total[5])}, group=gtop)
    assert f[pl.seg[0]:pl.seg[1]].sum() > 1000 and f[pl.seg[6]:pl.seg[7]].sum() > 100
    r0 = pl.rows(0)
    done_winners = ((gtop[pl.pairs[r0, 0].astype(np.int64) * pl.NCLS] & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF) - r0.astype(np.uint64)) & (done[r0] == 1)
    assert done_winners.sum() > 1000 and not f[r0][done_winners].any()      # a winner that is done already is not selected again


def test_select_round1_with_ties(engine, lists):
    pl, rng = lists, np.random.default_rng(22)
    done = pl.done.copy()
    su = rng.permutation(pl.U).astype(np.int32)
    bestc = np.zeros(pl.U * pl.NCLS, np.uint64)
    b10 = np.zeros(pl.NP, np.uint32)
    b10[pl.real] = rng.integers(990, 1011, int(pl.real.sum()))
    key = lambda thr: (thr.astype(np.uint64) << np.uint64(40)) | np.uint64(0x12345)
    thr0 = rng.integers(990, 1011, pl.U)
    bestc[np.arange(pl.U) * pl.NCLS + 0] = np.where(rng.random(pl.U) < 0.2, np.uint64(0), key(thr0))      # 0: the group has no certain row
    for p, k in ((2, 64), (3, 65), (4, 0)):
        bestc[np.arange(pl.U) * pl.NCLS + pl.CLS[p]] = key(np.full(pl.U, 1000))
        b10[pl.rows(p)] = 999
        rows = pl.pick(rng, p, k)
        b10[rows[:k // 2]] = 1000                                  # ties with the threshold are selected
        b10[rows[k // 2:]] = 1001
    # (profile 5's groups keep bestc == 0: every pair of it is selected)
    f = _check_list(engine, 1, pl, done, b10, counts={1: 0, 2: 64, 3: 65, 4: 0, 5: int(pl.total[5])}, group=bestc, sorted_uniq=su)
    r0 = pl.rows(0)
    bc0 = bestc[su[pl.pairs[r0, 0]].astype(np.int64) * pl.NCLS]
    ties = (bc0 != 0) & (b10[r0] == (bc0 >> np.uint64(40))) & (done[r0] == 0)
    assert ties.sum() > 1000 and f[r0][ties].all()


def test_select_topup(engine, lists):
    pl, rng = lists, np.random.default_rng(23)
    done = pl.done.copy()
    b10 = np.zeros(pl.NP, np.uint32)
    b10[pl.real] = rng.integers(1, 5000, int(pl.real.sum()))
    pairs = pl.pairs.copy()
    helpers = pl.pick(rng, 0, 5000)
    pairs[helpers, 2] = -1                                         # ran for their row states only: never selected
    pl2 = PairLists.__new__(PairLists)
    pl2.__dict__.update(pl.__dict__)
    pl2.pairs = pairs
    slot = np.array([0, 1, 2, 3, -1, 4, 5], np.int32)              # profile 4 has no undecided rows
    for p, k in ((2, 64), (3, 65)):
        b10[pl.rows(p)] = 10
        b10[pl.pick(rng, p, k)] = 4000
    cut = np.array([4500, 0, 1, 0, 4000, 0, 4000, 0, 1, 0, 3000, 200], np.uint32)      # slot 4 (profile 5): all; slot 5 (profile 6): both ends
    f = _check_list(engine, 2, pl2, done, b10, counts={1: 0, 2: 64, 3: 65, 4: 0, 5: int(pl.total[5])}, slot=slot, cutoff=cut, n_slots=6)
    assert not f[helpers].any()
    # the key list of the same profiles: every unevaluated pair, in list order
    f3 = _flags(3, pl2, done, b10, slot=slot)
    _, _, _, keys, vals, n = _select(engine, 3, pl2, done, b10, slot=slot, n_slots=6)
    idx = np.flatnonzero(f3)
    assert n == len(idx) and np.array_equal(vals, idx.astype(np.int32))
    exp_keys = (slot[pairs[idx, 1]].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - b10[idx].astype(np.uint64))
    assert np.array_equal(keys, exp_keys)


def test_select_nothing_and_everything(engine, lists):
    pl = lists
    gtop = np.zeros(pl.U * pl.NCLS, np.uint64)
    _check_list(engine, 0, pl, pl.done.copy(), pl.b10, counts={p: 0 for p in range(pl.P)}, group=gtop)      # an empty list: nothing allocated
    bestc = np.zeros(pl.U * pl.NCLS, np.uint64)
    su = np.arange(pl.U, dtype=np.int32)
    done = np.zeros(pl.NP, np.uint8)
    _check_list(engine, 1, pl, done, pl.b10, counts={p: int(pl.total[p]) for p in range(pl.P)}, group=bestc, sorted_uniq=su)
    _check_list(engine, 1, pl, np.ones(pl.NP, np.uint8), pl.b10, counts={p: 0 for p in range(pl.P)}, group=bestc, sorted_uniq=su)


# ------------------------------------------------------------------------------------------------ region keys
def _regions(engine, reads, regions, pairs):
    engine.set_reads(reads)
    regions = np.ascontiguousarray(regions, np.int32).reshape(-1, 4)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 4)
    rep = np.full(len(regions), -9, np.int32)
    uq = np.full(len(regions), -9, np.int32)
    engine._chk(engine.L.itsx_debug_region_keys(engine.h, regions.ctypes.data, len(regions), pairs.ctypes.data, len(pairs), rep.ctypes.data, uq.ctypes.data))
    first, exp = {}, np.full(len(regions), -1, np.int32)
    for g, (pi, ienv, jenv, _) in enumerate(regions.tolist()):
        if pi < 0:
            continue
        useq, prof, _, L = pairs[pi].tolist()
        exp[g] = first.setdefault((prof, L, reads[useq][ienv - 1:jenv]), g)
    assert np.array_equal(rep, exp)
    assert np.array_equal(uq, (exp == np.arange(len(regions))).astype(np.int32))
    return exp


def _rnd(rng, k):
    return "".join(rng.choice(list("ACGT"), int(k)))


def test_region_keys_all_identical(engine):
    rng = np.random.default_rng(31)
    core = _rnd(rng, 150)
    reads = [_rnd(rng, i % 17) + core + _rnd(rng, 5) for i in range(40)]      # the same envelope at 17 different offsets
    pairs = [(r, 3, 0, 400) for r in range(40)]
    regions = [(g % 40, (g % 40) % 17 + 1, (g % 40) % 17 + 150, 0) for g in range(1000)]
    exp = _regions(engine, reads, regions, pairs)
    assert (exp == 0).all()


def test_region_keys_all_distinct_at_the_fullest_table(engine):
    """504 distinct regions: 2 n + 16 = 1024 slots exactly, the fullest table a search builds"""
    rng = np.random.default_rng(32)
    reads = [_rnd(rng, 200) for _ in range(504)]
    pairs = [(r, r % 5, 0, 350) for r in range(504)]
    regions = [(r, 1 + r % 30, 120 + r % 70, 0) for r in range(504)]
    exp = _regions(engine, reads, regions, pairs)
    assert np.array_equal(exp, np.arange(504))


def test_region_keys_near_duplicates_and_holes(engine):
    """regions that differ only in an exception symbol, in L or in the profile are distinct; pair < 0 records have no representative"""
    rng = np.random.default_rng(33)
    a, b = _rnd(rng, 60), _rnd(rng, 70)
    reads = [a + "N" + b, a + "R" + b, a + "N" + b, a + "A" + b, "GG" + a + "N" + b + "T", a + "Y" + b[:-1]]
    pairs = [(0, 2, 0, 400), (1, 2, 0, 400), (2, 2, 0, 400), (3, 2, 0, 400), (4, 2, 0, 400), (5, 2, 0, 400),
             (0, 3, 0, 400), (0, 2, 0, 401), (2, 3, 0, 400), (2, 2, 0, 401)]
    n = len(a) + 1 + len(b)
    base = [(0, 1, n), (1, 1, n), (2, 1, n), (3, 1, n), (4, 3, n + 2), (5, 1, n - 1), (6, 1, n), (7, 1, n), (8, 1, n), (9, 1, n),
            (0, 1, len(a)), (1, 1, len(a)), (0, len(a) + 2, n), (1, len(a) + 2, n)]      # (the last four leave the exception outside)
    regions = []
    for k in range(600):
        if k % 7 == 3:
            regions.append((-1, 0, 0, 0))
        else:
            p, i, j = base[int(rng.integers(0, len(base)))]
            regions.append((p, i, j, 0))
    exp = _regions(engine, reads, regions, pairs)
    assert len(set(exp[exp >= 0].tolist())) == 8      # the whole with N (reads 0, 2, 4), with R, A, Y, profile 3, L 401, and the two parts without the exception
