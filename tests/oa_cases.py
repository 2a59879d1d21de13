"""The inputs of the optimal-accuracy tests (tests/test_oa_exact_cpu.py, tests/test_gpu_align.py): named cases of tests/edge_cases.py
and three of their own, each (profile text, reads, search settings), and the float64 side of a list of rows (tests/oa_exact.py) on
a pool of processes."""
import multiprocessing as mp

import numpy as np

import edge_cases as EC
import hmm_generic as G
import oa_exact as OA
import synth

EDGE = ("node_limits", "zero_transitions", "degenerate", "rescaling", "multidomain", "domz")
LANES = (1, 63, 64, 65)
NAMES = EDGE + ("short",) + tuple("lanes%d" % n for n in LANES)
LOW_T = dict(T=-1000.0, F1=1e-6, F2=1e-6, F3=1e-6)          # with finalize(domE=1e9): every domain of a pair past the filters is reported
SKIP_CAP = 0.10


def inputs(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs):
    """(profile text, reads, search settings)"""
    if name in EDGE:
        hmm, seqs, _ = EC.case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs)
        if name == "zero_transitions":                   # the two variants of two profiles of either side, and half the reads
            bl = EC._blocks(hmm)
            n = len(bl) // 2
            hmm = "".join(bl[i] for i in (0, 1, 4, 5, n, n + 1, n + 4, n + 5))
            seqs = seqs[:8]
        return hmm, seqs, dict(LOW_T)
    bl = EC._blocks(mini_hmm_text)
    if name == "short":
        # targets of 3-8 residues, every filter at 0.5: the shortest envelopes the search can report
        rng = np.random.default_rng(61)
        hmm = "".join(b for b in bl if "LENG  11" in b or "LENG  25" in b)
        cons = [c for c in synth.consensus_motifs(hmm, "") if c]
        seqs = []
        for n in range(3, 9):
            for c in cons:
                for _ in range(3):
                    a = int(rng.integers(0, len(c) - n + 1))
                    seqs.append(c[a:a + n])
            seqs.append(EC._rnd(rng, n))
        return hmm, sorted(set(seqs)), dict(T=-1000.0, F1=0.5, F2=0.5, F3=0.5)
    n = int(name[5:])
    # one profile, n distinct reads that each carry one copy of its consensus: n reported envelopes (lane masks, the second wave)
    hmm = next(b for b in bl if "LENG  45" in b)
    c = synth.consensus_motifs(hmm, "")[0]
    # (flanks of a fixed dinucleotide, told apart by their lengths: nothing in them that a second envelope could come from)
    seqs = ["AC" * (2 + k // 9) + c + "GT" * (2 + k % 9) for k in range(n)]
    assert len(set(seqs)) == n
    return hmm, seqs, dict(T=10.0, F1=1e-6, F2=1e-6, F3=1e-6)


_HM = None


def _init(hmm):
    global _HM
    _HM = G.parse_hmms(hmm)


def _one(args):
    prof, seq, ienv, jenv = args
    m = OA.align(_HM[prof], seq, ienv, jenv)
    out = {k: m[k] for k in ("hmm_from", "hmm_to", "ali_from", "ali_to", "oasc", "acc", "margin", "M", "Ld")}
    out["own"] = m["constrained"](m["hmm_from"], m["hmm_to"], m["ali_from"], m["ali_to"])
    return out


def _check(args):
    prof, seq, ienv, jenv, got, what = args
    m, dev, e, skipped, fails = OA.check_row(_HM[prof], seq, ienv, jenv, got, what)
    return dict(dev=dev, eps=e, skipped=skipped, fails=fails, model={k: m[k] for k in ("hmm_from", "hmm_to", "ali_from", "ali_to", "oasc", "acc", "margin", "M", "Ld")})


def _map(fn, hmm, tasks):
    if len(tasks) < 8:
        _init(hmm)
        return [fn(t) for t in tasks]
    import generic_check as GC
    with mp.get_context("fork").Pool(GC.pool_size(), initializer=_init, initargs=(hmm,)) as pool:
        return pool.map(fn, tasks, chunksize=max(1, len(tasks) // (4 * GC.pool_size())))


def models(hmm, seqs, rows):
    """rows: (prof, seq index, ienv, jenv) -> the model's results, in order"""
    return _map(_one, hmm, [(p, seqs[s], i, j) for p, s, i, j in rows])


def checks(hmm, seqs, rows):
    """rows: (prof, seq index, ienv, jenv, dict of the engine's five values) -> oa_exact.check_row's verdicts, in order"""
    return _map(_check, hmm, [(p, seqs[s], i, j, got, "profile %d read %d envelope %d..%d" % (p, s, i, j)) for p, s, i, j, got in rows])


def oracle_rows(hmm, seqs, kw):
    """the reported envelopes of the CPU oracle's search (the engine's rows are held to them elsewhere): (prof, seq, ienv, jenv)"""
    import orc
    hs = orc.HmmSet(text=hmm)
    codes, o = orc.digitize(seqs)
    res = orc.SearchResult(hs, codes, o, T=kw["T"], F1=kw["F1"], F2=kw["F2"], F3=kw["F3"], keep_trace=1, threads=8, domE=1e9)
    return [(int(d["prof"]), int(d["seq"]), int(d["ienv"]), int(d["jenv"])) for d in res.domains if d["dom_idx"] >= 0 and d["dom_reported"] == 1]
