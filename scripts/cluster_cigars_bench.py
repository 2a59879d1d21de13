#!/usr/bin/env python3
"""What itsx_align_clusters costs beside the clustering it follows (profiles/cluster_cigars.md): bench.py --workload cfg4's reads
(2x250-merged, 300-480 bases, seed and generator as there), Engine.cluster(0.995) and then Engine.align_clusters(), each `--runs`
times in one process; one JSON line.  --no-align times the clustering alone (a tree that has no such call).
usage: cluster_cigars_bench.py [--reads 1000000] [--runs 3] [--no-align] [--root TREE]"""
import argparse
import gzip
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package and tests/ are used")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "tests"))
    import synth
    from itsxpress_amd import Engine
    with gzip.open(os.path.join(args.root, "tests", "golden", "T.hmm.gz"), "rt") as f:
        thmm = f.read()
    blob, offs = synth.make_reads(thmm, args.reads, config=5, seed=synth.SEED + 5, as_array=True, left="1_", right="4_", fixed_len=0, len_range=(300, 480))
    eng = Engine(0)
    out = {"reads": args.reads, "mean_len": float(offs[-1]) / args.reads, "cluster_ms": [], "cluster_kernel_ms": [], "align_wall_ms": [], "align_kernel_ms": [],
           "switches": {k: v for k, v in os.environ.items() if k.startswith("ITSX_")}}
    for _ in range(args.runs):
        eng.set_reads_buffer(blob, offs)
        t = time.perf_counter()
        nu = eng.cluster(0.995, strand_both=True)
        out["cluster_ms"].append((time.perf_counter() - t) * 1e3)
        out["cluster_kernel_ms"].append(eng.stats()["ms_cluster"])
    out["centroids"] = int(nu)
    if not args.no_align:
        for _ in range(args.runs):
            t = time.perf_counter()
            info = eng.align_clusters()
            out["align_wall_ms"].append((time.perf_counter() - t) * 1e3)
            out["align_kernel_ms"].append(info["ms_kernels"])
        out["members"] = info["n_aligned"]
        t = time.perf_counter()
        cig = eng.get_cluster_cigars()
        out["fetch_ms"] = (time.perf_counter() - t) * 1e3
        out["equal"] = sum(1 for c in cig if c == "=")
        out["text_bytes"] = sum(len(c) for c in cig)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
