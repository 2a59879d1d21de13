"""Greedy clustering (cluster_id < 1) of many small samples: the per-sample loop against one itsx_cluster_samples call.

S samples of n cfg4-shaped reads each (bench.py --workload cfg4's generator arguments: 2x250-merged reads of 300-480 bases,
one seed per sample) are clustered at --cluster-id in one process and one engine context, the two arms alternated:
  loop:  set_reads + cluster for every sample (what the QIIME 2 plugin does per sample);
  batch: set_reads of all samples + set_samples + cluster_samples.
Every repeat checks that rep_of, strand, pct_id and order are equal between the arms.  Prints one JSON line.

  python scripts/batch_cluster_bench.py --samples 384 --reads 2000 --repeats 3
"""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cfg4_samples(n_samples, n_reads, hmm_text=None):
    """[(reads, names)] per sample: bench.py's cfg4 generator arguments, seed SEED + 5 + 1000 s for sample s"""
    import synth
    if hmm_text is None:
        with gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt") as f:
            hmm_text = f.read()
    out = []
    for s in range(n_samples):
        blob, offs = synth.make_reads(hmm_text, n_reads, config=5, seed=synth.SEED + 5 + 1000 * s, left="1_", right="4_",
                                      fixed_len=0, len_range=(300, 480))
        reads = synth.to_strings(blob, offs)
        names = ["s%03d:%07d" % (s, (i * 7919) % 1000003) for i in range(len(reads))]
        out.append((reads, names))
    return out


def run_loop(eng, samples, cid):
    t, reps, strs, pcts, ords, first = 0.0, [], [], [], [], 0
    for reads, names in samples:
        t0 = time.perf_counter()
        eng.set_reads(reads, names)
        eng.cluster(cid)
        t += time.perf_counter() - t0
        rep_of, strand, _ = eng.get_derep()
        pct, order = eng.get_cluster()
        reps.append(np.where(rep_of >= 0, rep_of + first, -1)); strs.append(strand); pcts.append(pct); ords.append(order + first)
        first += len(reads)
    return t, (np.concatenate(reps), np.concatenate(strs), np.concatenate(pcts), np.concatenate(ords))


def run_batch(eng, samples, cid):
    reads = [r for s in samples for r in s[0]]
    names = [n for s in samples for n in s[1]]
    smp = np.repeat(np.arange(len(samples), dtype=np.int32), [len(s[0]) for s in samples])
    t0 = time.perf_counter()
    eng.set_reads(reads, names)
    eng.set_samples(smp, len(samples))
    eng.cluster_samples(cid)
    t = time.perf_counter() - t0
    rep_of, strand, _ = eng.get_derep()
    pct, order = eng.get_cluster()
    return t, (rep_of.copy(), strand.copy(), pct.copy(), order.copy())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--cluster-id", type=float, default=0.995)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from itsxpress_amd import Engine
    samples = cfg4_samples(args.samples, args.reads)
    eng = Engine(0)
    run_batch(eng, samples[:2], args.cluster_id)          # warm-up: module load, first allocations
    run_loop(eng, samples[:2], args.cluster_id)
    tl, tb, windows = [], [], 0
    for _ in range(max(3, args.repeats)):
        t, a = run_loop(eng, samples, args.cluster_id)
        tl.append(t)
        t, b = run_batch(eng, samples, args.cluster_id)
        tb.append(t)
        windows = int(eng.stats()["cl_windows"])
        names = ("rep_of", "strand", "pct_id", "order")
        for nm, x, y in zip(names, a, b):
            eq = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if nm == "pct_id" else np.array_equal(x, y)
            assert eq, "%s differs between the per-sample loop and the batch" % nm
    loop_s, batch_s = float(np.median(tl)), float(np.median(tb))
    print(json.dumps({"samples": args.samples, "reads_per_sample": args.reads, "cluster_id": args.cluster_id, "repeats": len(tl),
                      "loop_s": round(loop_s, 4), "batch_s": round(batch_s, 4), "speedup": round(loop_s / batch_s, 3),
                      "loop_all_s": [round(x, 4) for x in tl], "batch_all_s": [round(x, 4) for x in tb],
                      "batch_cl_windows": windows, "n_clusters": int(eng.n_unique), "arrays_equal": True}))
    eng.close()


if __name__ == "__main__":
    main()
