"""One catalogue of the length and threshold edges of greedy clustering (cluster_id < 1), shared by tests/test_cluster_edges_cpu.py
and tests/test_gpu_cluster_edges.py.  Every case is named and seeded: Case(name, reads, names, cid, joins).

PAIRS[group]() gives the samples of a group: label `a` is the target, `b` the query (`c` a second one); a group is clustered in
a call of its own, so that ITS longest read selects the engine's code path (rows per lane, multi-pass, LDS sizes).  `joins` says,
where the construction fixes it, whether the last read joins a cluster (True), founds one (False) or is dropped ("dropped");
None leaves the outcome to the model (tests/align_exact.py through py_cluster).
WALKS[name]() gives small samples whose candidate walk stands at an edge; the builders check that edge with py_words.
"""
from collections import namedtuple

import numpy as np

from test_cluster_cpu import py_dust, py_words

Case = namedtuple("Case", "name reads names cid joins")

_COMP = str.maketrans("ACGTUNRYMKSWHBVD", "TGCAANYRKMSWDVBH")
_NEXT = str.maketrans("ACGT", "CGTA")


def rc(s):
    return s[::-1].translate(_COMP)


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), int(n)))


def _sub(s, pos):
    """s with other bases at the positions pos (0-based)"""
    s = list(s)
    for p in pos:
        s[p] = s[p].translate(_NEXT)
    return "".join(s)


def _cut(s, pos, k=1):
    """s without the k bases at each of the positions pos"""
    for p in sorted(pos, reverse=True):
        s = s[:p] + s[p + k:]
    return s


def _spread(L, n, lo=12):
    """n positions inside (lo, L - lo), far enough apart for their 8-mers not to meet"""
    return [lo + (k + 1) * (L - 2 * lo) // (n + 1) for k in range(n)]


def _pair(name, a, b, cid, joins=None):
    return Case(name, [a, b], ["a", "b"], cid, joins)


# ---------------------------------------------------------------- pairs
def _row_group(seed, lengths, cid=0.97):
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        t = _rnd(rng, L)
        m = L // 2
        out += [_pair("L%d_q32_exact" % L, t, t[m:m + 32], cid, True),
                _pair("L%d_q33_one_sub" % L, t, _sub(t[m:m + 33], [16]), cid, False),
                _pair("L%d_q33_minus" % L, t, rc(t[3:36]), cid, True),
                _pair("L%d_qmax_edits" % L, t, _cut(_sub(t, _spread(L, 3)), [L // 3]) + "G", cid),
                _pair("L%d_qmax_minus" % L, t, rc(_sub(t, _spread(L, 2))), cid, True),
                _pair("L%d_qmax_end_gaps" % L, t, _cut(t, [1, L - 2]), cid),
                _pair("L%d_short_centroid" % L, t[7:7 + 40], _sub(t, [m + 60]), cid, True)]
        assert max(len(r) for c in out[-7:] for r in c.reads) == L
    return out


def rows5():
    return _row_group(101, [319])


def rows8():
    return _row_group(102, [320, 511])


def rows10():
    return _row_group(103, [512, 639])


def multipass():
    rng = np.random.default_rng(104)
    out, cid = [], 0.97
    for L in (640, 641, 1300, 2040, 2041, 5000):
        t = _rnd(rng, L)
        m = L // 2
        out += [_pair("L%d_q40" % L, t, t[m:m + 40], cid, True),
                _pair("L%d_q300_edits" % L, t, _cut(_sub(t[m - 100:m + 201], [50, 180]), [120]), cid),
                _pair("L%d_q120_minus" % L, t, rc(_sub(t[L - 120:], [60])), cid, True),
                _pair("L%d_q200_far" % L, t, _sub(t[10:210], _spread(200, 7)), cid, False)]
        if L <= 2100:
            out += [_pair("L%d_qmax_edits" % L, t, _cut(_sub(t, _spread(L, 5)), [L // 3, 2 * L // 3]) + "CA", cid),
                    _pair("L%d_qmax_minus" % L, t, rc(_sub(t, _spread(L, 3))), cid, True),
                    _pair("L%d_qmax_long_gap" % L, t, _cut(t, [m], 9), cid)]
        else:
            out += [_pair("L%d_q639" % L, t, _sub(t[1000:1639], _spread(639, 4)), cid, True),
                    _pair("L%d_q640" % L, t, _cut(t[2000:2641], [300]), cid),
                    _pair("L%d_short_centroid" % L, t[4000:4600], _sub(t, [4300]), cid, True)]
    return out


_LONG = {}


def _long(L):
    """ONE read per length: its DUST mask and its alignments are computed once per process"""
    if L not in _LONG:
        _LONG[L] = _rnd(np.random.default_rng(1000 + L), L)
    return _LONG[L]


def contained():
    out, cid = [], 0.97
    for L, qlens in ((2041, (100, 300, 600)), (20000, (100, 400, 600)), (50000, (150, 600, 350))):
        t = _long(L)
        for where, n in zip(("start", "middle", "end"), qlens):
            p = {"start": 0, "middle": L // 2 - 77, "end": L - n}[where]
            q = t[p:p + n]
            out.append(_pair("L%d_%s_exact_q%d" % (L, where, n), t, q, cid, True))
            if L < 50000 or where == "middle":
                out.append(_pair("L%d_%s_near_q%d" % (L, where, n), t, rc(_cut(_sub(q, [n // 3]), [2 * n // 3])), cid, True))
        out.append(_pair("L%d_long_query_short_centroid" % L, _sub(t[L // 3:L // 3 + 500], [250]), t, cid, True))
    return out


def limits():
    rng = np.random.default_rng(106)
    t = _rnd(rng, 200)
    t50, cid = _long(50000), 0.97
    return [_pair("q31_dropped", t, t[50:81], cid, "dropped"),
            _pair("q32_kept", t, t[50:82], cid, True),
            _pair("t50000_q300", t50, _sub(t50[31000:31300], [100]), cid, True),
            _pair("t50001_dropped_q300", t50 + "A", _sub(t50[31000:31300], [100]), cid, False)]


def budget(cid, L):
    """K: the most edits E for which 100.0 * (L - E) / L >= 100.0 * cid holds, by the definition's own expression"""
    K = 0
    while 100.0 * (L - (K + 1)) / L >= 100.0 * cid:
        K += 1
    return K


def threshold():
    out = []
    for ci, cid in enumerate((0.97, 0.99, 0.995)):
        for L in (100, 200, 400):
            rng = np.random.default_rng(107 + 10 * ci + L)
            t = _rnd(rng, L)
            K = budget(cid, L)
            tag = "id%g_L%d" % (cid, L)
            for E, joins in ((K, True), (K + 1, False)):
                if E == 0:
                    continue
                w = "K" if joins else "K+1"
                pos = _spread(L, E)
                subs = _sub(t, pos)
                out += [_pair("%s_%s_subs" % (tag, w), t, subs, cid, joins),
                        _pair("%s_%s_subs_minus" % (tag, w), t, rc(subs), cid, joins),
                        _pair("%s_%s_gaps_in_query" % (tag, w), t, _cut(t, pos), cid, joins),
                        _pair("%s_%s_gaps_in_target" % (tag, w), _cut(t, pos), t, cid, joins),
                        _pair("%s_%s_one_long_gap" % (tag, w), t, _cut(t, [L // 2], E), cid, joins)]
                for lo, hi in ((1, 0), (0, 50), (7, 23), (50, 1)):        # free overhangs of the query on either side
                    out.append(_pair("%s_%s_subs_overhang_%d_%d" % (tag, w, lo, hi), t, _rnd(rng, lo) + subs + _rnd(rng, hi), cid, joins))
                out.append(_pair("%s_%s_subs_target_overhang" % (tag, w), _rnd(rng, 9) + t + _rnd(rng, 31), subs, cid, joins))
                # the last edit at the first, second, last-but-one and last position: an interior gap there may turn terminal
                for p in (0, 1, L - 2, L - 1):
                    out += [_pair("%s_%s_sub_at_%d" % (tag, w, p + 1), t, _sub(t, pos[:-1] + [p]), cid),
                            _pair("%s_%s_gap_at_%d" % (tag, w, p + 1), t, _cut(_sub(t, pos[:-1]), [p]), cid)]
    return out


def ties():
    rng = np.random.default_rng(108)
    cid = 0.9
    f = lambda: _rnd(rng, 45)
    out = []
    for name, x, y in (("tandem_CA", "CA" * 15, "CA" * 13), ("homopolymer_A", "A" * 20, "A" * 17), ("tandem_ACG", "ACG" * 10, "ACG" * 4 + "ATG" + "ACG" * 4),
                       ("homopolymer_vs_sub", "G" * 12, "G" * 5 + "T" + "G" * 7), ("tandem_shift", "ACGT" * 8, "CGTA" * 8), ("gap_or_mismatch", "AAAAACCCCC", "AAAACCCCCC")):
        l, r = f(), f()
        out += [_pair(name, l + x + r, l + y + r, cid), _pair(name + "_swapped", l + y + r, l + x + r, cid),
                _pair(name + "_minus", l + x + r, rc(l + y + r), cid)]
    t = _rnd(rng, 160)
    out += [_pair("n_run", t, t[:60] + "N" * 12 + t[72:], cid, True), _pair("n_run_in_target", t[:60] + "N" * 12 + t[72:], t, cid, True),
            _pair("n_run_against_gap", t, t[:60] + "N" * 5 + t[72:], cid), _pair("u_for_t", t, t.replace("T", "U"), cid, True),
            _pair("u_for_t_minus", t.replace("T", "U"), rc(t), cid, True)]
    codes = "RYMKSWHBVDN"
    q = list(t)
    for k, c in enumerate(codes):                            # every code, at four positions each
        for j in range(4):
            p = 20 + 11 * k + 3 * j
            q[p] = c
    q = "".join(q)
    q2 = list(t)
    for k, c in enumerate(codes * 4):
        q2[24 + 3 * k] = c
    q2 = "".join(q2)
    out += [_pair("iupac_in_query", t, q, cid), _pair("iupac_in_target", q, t, cid), _pair("iupac_both", q, q2, cid), _pair("iupac_both_minus", q2, rc(q), cid)]
    return out


def unlike_targets():
    rng = np.random.default_rng(109)
    cid = 0.97
    out = []
    for k, Lq in enumerate((300, 639, 200)):
        a, b = _rnd(rng, 100), _rnd(rng, 2040)
        mid = _rnd(rng, Lq - 120)
        cases = {"both_reject": a[20:80] + mid + b[1000:1060],
                 "long_accepts": _sub(b[700:700 + Lq - 50], [40, Lq - 100]) + a[30:80],
                 "both_accept": a + _sub(b[300:300 + Lq - 100], _spread(Lq - 100, 2)),
                 "minus": rc(a[20:80] + mid + b[1000:1060])}
        for name, q in cases.items():
            out.append(Case("q%d_%s" % (Lq, name), [a, b, q], ["a", "b", "c"] if k != 1 else ["b", "a", "c"], cid, None))
            s = rc(q) if name == "minus" else q              # one strand of the query holds both targets as candidates
            assert len(py_words(s) & py_words(a)) >= 12 and len(py_words(s) & py_words(b)) >= 12
    # both candidates share one 19-base seed (12 words) with an otherwise unrelated query: no diagonal says anything about either,
    # so the optimal scores of the 100-base and the 2 040-base target are computed side by side
    for k in range(4):
        a, b = _rnd(rng, 100), _rnd(rng, 2040)
        q = _rnd(rng, 60) + a[40:59] + _rnd(rng, 50) + b[1500:1519] + _rnd(rng, 52)
        assert len(py_words(q) & py_words(a)) >= 12 and len(py_words(q) & py_words(b)) >= 12
        out.append(Case("q200_weak_seeds_%d" % k, [a, b, rc(q) if k % 2 else q], ["a", "b", "c"], 0.93, False))
    return out


PAIRS = dict(rows5=rows5, rows8=rows8, rows10=rows10, multipass=multipass, contained=contained, limits=limits, threshold=threshold,
             ties=ties, unlike_targets=unlike_targets)


# ---------------------------------------------------------------- walks
def _words(s):
    return py_words(s, py_dust(s))


def _holes(s, keep):
    """s with an N in every 8-mer except inside the runs keep = [(start, length)]"""
    out = list(s)
    for p in range(0, len(s), 7):
        if not any(a - 1 < p < a + n for a, n in keep):
            out[p] = "N"
    for a, n in keep:                                        # the run ends exactly where it should
        if a > 0:
            out[a - 1] = "N"
        if a + n < len(s):
            out[a + n] = "N"
    return "".join(out)


def _shared_words(tag, n_shared):
    rng = np.random.default_rng(201)
    t = _rnd(rng, 200)
    q = list(_holes(t, [(40, n_shared + 7), (120, 15)]))
    q[127] = q[127].translate(_NEXT)                         # eight words of the query's own, none of them the centroid's
    q = "".join(q)
    assert len(_words(q)) == n_shared + 8 and len(_words(q) & _words(t)) == n_shared
    return Case(tag, [t, q], ["a", "b"], 0.97, n_shared >= 12)


def words_11():
    return _shared_words("words_11", 11)


def words_12():
    return _shared_words("words_12", 12)


def few_words():
    rng = np.random.default_rng(202)
    t = _rnd(rng, 200)
    q = _holes(t, [(90, 13)])
    assert len(_words(q)) == 6 and _words(q) <= _words(t)    # fewer than 12 of its own: all six must be shared, and are
    return Case("few_words", [t, q], ["a", "b"], 0.97, True)


def no_words():
    rng = np.random.default_rng(203)
    t = _rnd(rng, 200)
    q = _holes(t, [])
    low = "CA" * 50
    assert not _words(q) and not _words(low) and not _words(rc(low)) and py_words(low)
    return Case("no_words", [t, q, low, low, q], ["a", "b", "c", "d", "e"], 0.97, False)


def _rank(n_reject):
    """n_reject centroids that share more words with the query than the acceptor does and miss 0.99; the acceptor ranks behind them"""
    rng = np.random.default_rng(204)
    x, y = _rnd(rng, 20), _rnd(rng, 6 * 33 + 2)
    q = x + y
    acc = y
    rej = [_sub(q, [20 + 6 * k + j for j in range(4)]) for k in range(n_reject)]
    reads = rej + [acc, q]
    names = ["r%02d" % k for k in range(n_reject)] + ["s", "t"]
    qw = _words(q)
    cands = sorted((-len(qw & _words(r)), len(r), pos) for pos, r in enumerate(reads[:-1]) if len(qw & _words(r)) >= 12)
    assert len(cands) == n_reject + 1 and cands[-1][2] == n_reject and cands.index(cands[-1]) == n_reject      # the acceptor: rank n_reject + 1
    return Case("acceptor_rank_%d" % (n_reject + 1), reads, names, 0.99, n_reject < 32)


def acceptor_rank_32():
    return _rank(31)


def acceptor_rank_33():
    return _rank(32)


def _tie(tag, la, lb):
    rng = np.random.default_rng(205)
    k = _rnd(rng, 100)
    ca = _rnd(rng, la) + k + _rnd(rng, la)
    cb = _rnd(rng, lb) + k + _rnd(rng, lb)
    assert len(_words(k) & _words(ca)) == len(_words(k) & _words(cb)) == len(_words(k)) >= 12
    return Case(tag, [ca, cb, k, rc(k)], ["a", "b", "c", "d"], 0.97, True)


def tie_length():
    return _tie("tie_length", 60, 40)                        # the later, shorter centroid is tried first


def tie_position():
    return _tie("tie_position", 40, 40)                      # same count, same length: the earlier centroid


def plus_beside_minus():
    rng = np.random.default_rng(206)
    q = _rnd(rng, 300)
    a = q[150:]
    b = rc(_sub(q, [200, 260]))
    assert len(_words(rc(q)) & _words(b)) > len(_words(q) & _words(a)) >= 12
    return Case("plus_beside_minus", [a, b, q], ["a", "b", "c"], 0.99, True)


def minus_beats_plus():
    rng = np.random.default_rng(207)
    q = _rnd(rng, 300)
    a = _sub(q[100:], [60, 140])                             # plus: 198 / 200
    b = rc(_sub(q, [200]))                                   # minus: 299 / 300 (and 197 / 200 against a: two centroids)
    assert len(_words(rc(q)) & _words(b)) >= 12 and len(_words(q) & _words(a)) >= 12
    return Case("minus_beats_plus", [a, b, q], ["a", "b", "c"], 0.99, True)


WALKS = dict(words_11=words_11, words_12=words_12, few_words=few_words, no_words=no_words, acceptor_rank_32=acceptor_rank_32,
             acceptor_rank_33=acceptor_rank_33, tie_length=tie_length, tie_position=tie_position, plus_beside_minus=plus_beside_minus,
             minus_beats_plus=minus_beats_plus)


# ---------------------------------------------------------------- expectations
_ALIGNED = {}


def model_align(q, t):
    """tests/align_exact.py, every pair once per process"""
    import align_exact
    if (q, t) not in _ALIGNED:
        _ALIGNED[(q, t)] = align_exact.align(q, t)
    return _ALIGNED[(q, t)]


def expected(case):
    """(order, rep_of, strand, pct_id) of a case by py_cluster on the exact model"""
    import functools

    import test_cluster_cpu as T
    if not hasattr(T.py_dust, "cache_info"):
        T.py_dust = functools.lru_cache(maxsize=None)(T.py_dust)        # a 50 000-base mask takes seconds: once per read and process
    rep_of, strand, pct, order = T.py_cluster(case.reads, case.names, case.cid, align=model_align)
    return order, rep_of, strand, pct


def get(key):
    kind, name, k = key
    return PAIRS[name]()[k] if kind == "pair" else WALKS[name]()


def keys():
    """(kind, group or walk, index) of every case"""
    return [("pair", g, k) for g in PAIRS for k in range(len(PAIRS[g]()))] + [("walk", w, 0) for w in WALKS]


def _expected_of(key):
    seen = set(_ALIGNED)
    e = expected(get(key))
    return key, e, {p: v for p, v in _ALIGNED.items() if p not in seen}


def expected_all(ks, pool=None):
    """{key: expectation} and {(query strand, target): model alignment} of the cases ks; through a process pool when one is given"""
    out, pairs = {}, {}
    for key, e, al in (pool.map(_expected_of, ks, chunksize=1) if pool is not None else map(_expected_of, ks)):
        out[key] = e
        pairs.update(al)
    return out, pairs
