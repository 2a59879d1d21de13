"""The MSV filter's floored row (csrc/k_msv.hip) as a numpy statement, against the plain recurrence it replaces.

Plain row (HMMER's p7_MSVFilter in signed, unfloored cells):  c'[k] = max(c[k-1], xB) + e[k],  xE = max(0, max_k c'[k]),
xJ = max(xJ, xE - tec),  xB = max(xJ - tjbm, bm0).  Floored row: a register keeps c'' = max(c, xB) - xB - 32768, the row is one
saturating 16-bit add, xE = max_k c'' + xB + 32768, and the cells sink by delta when xB rises by delta.  The two must agree on xJ
and xB after EVERY row, for lanes of one wave that switch to the floored row together (the kernel's wave-uniform start-up test).
Without the start-up rule they do not: a first row whose emissions are all negative reads xE = xB instead of the true maximum."""
import numpy as np

W = 46                    # cells (the widest model)
WAVE = 64
NEG = -32768


def _reads(n, seed):
    """emission rows e[n, rows, W] (bias - cost, as the kernel's table holds them), lengths, and per-read bm0, tjbm, tec"""
    rng = np.random.default_rng(seed)
    Lmax = 120
    L = rng.integers(5, Lmax + 1, n)
    e = -rng.integers(1, 9, (n, Lmax, W)).astype(np.int32)                # mismatches
    M = rng.choice([11, 25, 45, 46], n)
    for i in range(n):
        e[i, :, M[i]:] = -250                                            # padding cells: cost 255
        for _ in range(rng.integers(0, 4)):                              # planted diagonals: a hit, weak or strong
            r0, k0, ln = rng.integers(0, L[i]), rng.integers(0, M[i]), rng.integers(3, 46)
            for j in range(ln):
                if r0 + j < L[i] and k0 + j < M[i] and rng.random() < 0.93:
                    e[i, r0 + j, k0 + j] = rng.integers(1, 8)
    kind = rng.integers(0, 8, n)
    for i in range(n):
        if kind[i] == 0:                                                 # an all-negative first row (a read that begins with N)
            e[i, 0, :] = np.minimum(e[i, 0, :], -1)
        elif kind[i] == 1:                                               # ... several of them
            k = rng.integers(2, 20); e[i, :k, :] = np.minimum(e[i, :k, :], -1)
        elif kind[i] == 2:                                               # all-negative rows in the middle of the read
            a = rng.integers(0, L[i]); e[i, a:a + rng.integers(1, 10), :] = -rng.integers(1, 9)
        elif kind[i] == 3:                                               # every row negative (a fully degenerate read)
            e[i] = np.minimum(e[i], -1)
    tec = rng.integers(1, 7, n)
    tjbm = rng.integers(25, 90, n)
    tjbm[rng.random(n) < 0.05] = rng.integers(190, 230)                  # bm0 = 0: a very long read
    bm0 = np.maximum(190 - tjbm, 0)
    return e, L, bm0.astype(np.int32), tjbm.astype(np.int32), tec.astype(np.int32)


def plain(e, L, bm0, tjbm, tec):
    n, R, _ = e.shape
    c = np.zeros((n, W), np.int32)
    xJ = np.zeros(n, np.int32); xB = bm0.copy(); xEmax = np.zeros(n, np.int32)
    hJ = np.zeros((R, n), np.int32); hB = np.zeros((R, n), np.int32)
    for r in range(R):
        act = r < L
        prev = np.concatenate([np.zeros((n, 1), np.int32), c[:, :-1]], axis=1)
        cn = np.maximum(prev, xB[:, None]) + e[:, r, :]
        xE = np.maximum(cn.max(axis=1), 0)
        nJ = np.maximum(xJ, xE - tec)
        nB = np.maximum(nJ - tjbm, bm0)
        c[act] = cn[act]; xJ = np.where(act, nJ, xJ); xB = np.where(act, nB, xB); xEmax = np.where(act, np.maximum(xEmax, xE), xEmax)
        hJ[r] = xJ; hB[r] = xB
    return hJ, hB, xEmax


def floored(e, L, bm0, tjbm, tec, startup=True):
    """the kernel's schedule: lanes in waves of 64; a wave runs the plain row while any working lane has xJ < bm0 - tec, converts
    its registers once and goes on with the floored row"""
    n, R, _ = e.shape
    c = np.zeros((n, W), np.int32)                                       # real cells in the plain phase, c'' in the floored one
    fl = np.zeros(n, bool)
    xJ = np.zeros(n, np.int32); xB = bm0.copy()
    hJ = np.zeros((R, n), np.int32); hB = np.zeros((R, n), np.int32)
    wave = np.arange(n) // WAVE
    nw = int(wave.max()) + 1
    for r in range(R):
        act = r < L
        below = act & (xJ + tec < bm0) if startup else np.zeros(n, bool)
        wbelow = np.bincount(wave, below, nw) > 0
        conv = ~fl & ~wbelow[wave]
        cc = np.maximum(c, xB[:, None]) - xB[:, None] - 32768             # max with xB, subtract xB + 32768
        c[conv] = cc[conv]; fl |= conv
        # the plain row
        prev = np.concatenate([np.zeros((n, 1), np.int32), c[:, :-1]], axis=1)
        cn = np.maximum(prev, xB[:, None]) + e[:, r, :]
        xE = np.maximum(cn.max(axis=1), 0)
        # the floored row: prev of cell 1 is the floor, the add saturates
        prevf = np.concatenate([np.full((n, 1), NEG, np.int32), c[:, :-1]], axis=1)
        cf = np.clip(prevf + e[:, r, :], NEG, 32767)
        xEf = cf.max(axis=1) + xB + 32768
        cn = np.where(fl[:, None], cf, cn)
        xE = np.where(fl, xEf, xE)
        nJ = np.maximum(xJ, xE - tec)
        nB = np.maximum(nJ - tjbm, bm0)
        delta = nB - xB
        assert (delta >= 0).all()
        cn = np.where(fl[:, None], np.clip(cn - delta[:, None], NEG, 32767), cn)     # xB rose: the cells sink by as much
        c[act] = cn[act]; xJ = np.where(act, nJ, xJ); xB = np.where(act, nB, xB)
        hJ[r] = xJ; hB[r] = xB
    return hJ, hB


def test_floored_recurrence_equals_the_plain_one_after_every_row():
    n = 4096
    e, L, bm0, tjbm, tec = _reads(n, 20240607)
    assert (e[:, 0, :].max(axis=1) < 0).sum() > 200                       # all-negative first rows
    assert ((e.max(axis=2) < 0) & (np.arange(e.shape[1])[None, :] < L[:, None])).sum() > 2000      # all-negative rows
    pJ, pB, xEmax = plain(e, L, bm0, tjbm, tec)
    assert (pB[-1] > bm0).sum() > 200                                    # xB rose in many reads
    assert (pJ[-1] + tec >= 250).sum() > 20                              # ... into the overflow range in some
    fJ, fB = floored(e, L, bm0, tjbm, tec)
    assert np.array_equal(pJ, fJ) and np.array_equal(pB, fB)
    # the overflow test without a running maximum of xE: max_i xE_i = xJ + tec whenever xJ > 0
    pos = pJ[-1] > 0
    assert pos.sum() > 1000 and np.array_equal(xEmax[pos], (pJ[-1] + tec)[pos])
    assert (xEmax[~pos] <= tec[~pos]).all()


def test_without_the_start_up_rule_the_floored_recurrence_differs():
    n = 4096
    e, L, bm0, tjbm, tec = _reads(n, 20240607)
    pJ, pB, _ = plain(e, L, bm0, tjbm, tec)
    fJ, fB = floored(e, L, bm0, tjbm, tec, startup=False)
    bad = (pJ != fJ).any(axis=0)
    assert bad.sum() >= 1
    # every such read starts below bm0 - tec with an all-negative first row: the case the rule is for
    assert ((bm0 - tec)[bad] > 0).all() and (e[bad, 0, :].max(axis=1) < 0).all()
