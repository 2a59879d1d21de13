#!/usr/bin/env python
"""Denoising a batch's feature table of trimmed ITS2 into ZOTUs on the device (itsx_denoise_table).

    python scripts/denoise_run.py [SAMPLES [READS_PER_SAMPLE [PASSES]]]      (default 384 2000 3)

The workload is scripts/feature_table_run.py's (its generator and files): the batch is loaded, dereplicated, searched and its feature
table made once; then, after one warm-up, PASSES timed calls of Engine.denoise_table(alpha=2, minsize=8): the call's own ms_kernels
and its wall time (the arrays come back inside the call).

There is no earlier figure to beat.  The comparison arm is the model's own distance routine (tests/denoise_model.py, numpy on the
host) on a fixed random sample of 2 000 of the run's (feature, centroid) pairs that reach the distance kernel, scaled to all of them:
a stand-in for "the same pairs on the host", not usearch or vsearch.

Per level the pairs are counted again here from the totals, the lengths and the result's centroids with the kernel's two prunings
(they must sum to the call's own counters).  Prints one JSON line.
"""
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench import its2_profiles  # noqa: E402
from denoise_model import levenshtein  # noqa: E402
from feature_table_run import write_sample  # noqa: E402
from itsxpress_amd import Engine, SeqSampleNotPaired  # noqa: E402
from itsxpress_amd.SeqSample import _REGION_PREFIX  # noqa: E402
from itsxpress_amd.batch import SampleBatch  # noqa: E402


def dmax_of(aq, at, skew):
    """the cut-off of every (feature total, centroid total) pair, [len(aq), len(at)]"""
    k = np.zeros((len(aq), len(at)), np.int32)
    for s in skew:
        k += aq[:, None].astype(np.float64) <= s * at[None, :].astype(np.float64)
    return k


def levels_of(totals, skew):
    lv, f0, F = [], 0, len(totals)
    while f0 < F:
        lv.append(f0)
        if len(skew) == 0:
            break
        thr = skew[0] * float(totals[f0])
        f0 += int(np.searchsorted(-totals[f0:].astype(np.float64), -thr, side="left"))      # the first total <= thr
    return lv + [F]


def level_pairs(ft, t):
    """per level: features, centroids standing before it, pairs that reach the kernel, pairs out by the skew, by the length"""
    totals, lens, skew = ft.totals.astype(np.int64), ft.lengths.astype(np.int64), t.max_skew
    lv = levels_of(totals, skew)
    cent = t.zotu_feature.astype(np.int64)
    rows = []
    for l in range(len(lv) - 1):
        f0, f1 = lv[l], lv[l + 1]
        c = cent[cent < f0]
        uq, cq = np.unique(np.stack([totals[f0:f1], lens[f0:f1]], 1), axis=0, return_counts=True)
        reach = by_skew = by_len = 0
        if len(c):
            uc, cc = np.unique(np.stack([totals[c], lens[c]], 1), axis=0, return_counts=True)
            k = dmax_of(uq[:, 0], uc[:, 0], skew)
            near = np.abs(uq[:, 1][:, None] - uc[:, 1][None, :]) <= k
            w = cq[:, None] * cc[None, :]
            reach, by_skew, by_len = int(w[(k > 0) & near].sum()), int(w[k == 0].sum()), int(w[(k > 0) & ~near].sum())
        rows.append({"level": l, "first_total": int(totals[f0]), "features": f1 - f0, "centroids_before": int(len(c)), "pairs": reach,
                     "skipped_skew": by_skew, "skipped_length": by_len})
    return rows


def sample_pairs(ft, t, n, seed=7):
    """n of the run's pairs that reach the distance kernel, drawn with a fixed seed"""
    rng = np.random.default_rng(seed)
    totals, lens, skew = ft.totals.astype(np.int64), ft.lengths.astype(np.int64), t.max_skew
    lv = np.array(levels_of(totals, skew))
    cent = t.zotu_feature.astype(np.int64)
    out = []
    while len(out) < n and len(cent) and len(skew):
        q = rng.integers(0, len(totals), 4096)
        c = cent[rng.integers(0, len(cent), 4096)]
        f0 = lv[np.searchsorted(lv, q, side="right") - 1]
        k = np.zeros(4096, np.int32)
        for s in skew:
            k += totals[q].astype(np.float64) <= s * totals[c].astype(np.float64)
        ok = (c < f0) & (k > 0) & (np.abs(lens[q] - lens[c]) <= k)
        out += list(zip(q[ok].tolist(), c[ok].tolist()))
    return out[:n]


def main():
    argv = sys.argv[1:]
    S = int(argv[0]) if len(argv) > 0 else 384
    n = int(argv[1]) if len(argv) > 1 else 2000
    passes = int(argv[2]) if len(argv) > 2 else 3
    os.environ["ITSXPRESS_ARRAYS"] = "0"
    os.environ["ITSXPRESS_STREAM"] = "0"
    os.environ.pop("ITSXPRESS_GPUS", None)
    thmm = gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt").read()
    tmp = tempfile.mkdtemp(prefix="itsx_denoise_")
    try:
        files = [write_sample(tmp, s, n, thmm) for s in range(S)]
        hmm = os.path.join(tmp, "its2.hmm")
        with open(hmm, "w") as f:
            f.write(its2_profiles(thmm))
        eng = Engine(0)
        objs = [SeqSampleNotPaired(f, os.path.join(tmp, "work")) for f in files]
        b = SampleBatch(objs, engine=eng, keep_records=True)
        b.deduplicate(threads=1)
        b._search(hmmfile=hmm, threads=1)
        ft = eng.trimmed_table(region_prefixes=_REGION_PREFIX["ITS2"])
        eng.denoise_table(alpha=2.0, minsize=8)                 # warm-up: buffers at their working size
        wall, kern = [], []
        for _ in range(passes):
            t0 = time.perf_counter()
            t = eng.denoise_table(alpha=2.0, minsize=8)
            wall.append(time.perf_counter() - t0)
            kern.append(t.ms_kernels / 1e3)
        rows = level_pairs(ft, t)
        counted = (sum(r["pairs"] for r in rows), sum(r["skipped_skew"] for r in rows), sum(r["skipped_length"] for r in rows))
        same = counted == (t.n_pairs, t.n_skipped_skew, t.n_skipped_length) and len(rows) == t.n_levels
        # the comparison arm: the model's distance on 2 000 of the pairs
        pairs = sample_pairs(ft, t, 2000)
        seqs = ft.sequences
        t0 = time.perf_counter()
        dist = [levenshtein(seqs[q], seqs[c]) for q, c in pairs]
        host_s = time.perf_counter() - t0
        symbols = float(np.mean([len(seqs[c]) for _, c in pairs])) if pairs else 0.0

        def stat(v):
            return {"median_s": round(float(np.median(v)), 6), "spread_s": round(max(v) - min(v), 6), "all_s": [round(x, 6) for x in v]}
        k_med = float(np.median(kern))
        print(json.dumps({"denoise_table": True, "samples": S, "reads_per_sample": n, "passes": passes, "reads_counted": ft.n_counted,
                          "features": ft.n_features, "zotus": t.n_zotus, "entries": int(len(t.entry_count)), "dropped_reads": t.n_dropped_reads,
                          "max_skew": t.max_skew.tolist(), "levels": t.n_levels, "pairs": t.n_pairs, "skipped_skew": t.n_skipped_skew,
                          "skipped_length": t.n_skipped_length, "per_level": rows, "level_counts_agree": bool(same),
                          "device_ms_kernels": stat(kern), "device_wall": stat(wall),
                          "mean_target_symbols_of_sampled_pairs": round(symbols, 2),
                          "target_symbols_stepped": t.n_columns, "symbols_stepped_per_pair": round(t.n_columns / max(t.n_pairs, 1), 2),
                          "target_symbols_per_s_over_ms_kernels": round(t.n_columns / k_med, 1) if k_med > 0 else None,
                          "host_model_sample": {"pairs": len(pairs), "seconds": round(host_s, 4),
                                                "pairs_per_s": round(len(pairs) / host_s, 1) if host_s > 0 else None,
                                                "scaled_to_all_pairs_s": round(host_s / max(len(pairs), 1) * t.n_pairs, 2),
                                                "within_cut_off_fraction": round(float(np.mean([d <= len(t.max_skew) for d in dist])), 4) if dist else None}}))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
