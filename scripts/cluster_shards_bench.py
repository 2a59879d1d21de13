"""Greedy clustering (cluster_id < 1) of one sample with the centroid stream in shards (itsx_cluster_multi, DESIGN section 4a'').

cfg4-shaped reads (bench.py --workload cfg4's generator: 2x250-merged reads of 300-480 bases) are clustered at --cluster-id in one
process, arm after arm:
  1 context         Engine.cluster (itsx_cluster);
  K contexts, dev 0 a leader and K - 1 helpers on device 0 (shards share one GPU: the overhead of sharding);
  K devices         a leader on device 0 and one helper on each of devices 1 .. K - 1 (only when that many are visible).
Every arm's rep_of, strand, pct_id (bit patterns) and order are checked equal to the one-context arm.  The wall time is the cluster
call alone; windows come from itsx_stats; the bytes copied between contexts per window come from a second, untimed run of the
arm with ITSX_CL_DEBUG=1.  One JSON line per arm, then a summary line.

  python scripts/cluster_shards_bench.py --reads 1000000 3000000 --out profiles/cluster_shards.jsonl
"""
import argparse
import gzip
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cfg4_reads(n, hmm_text):
    import synth
    blob, offs = synth.make_reads(hmm_text, n, config=5, left="1_", right="4_", fixed_len=0, len_range=(300, 480))
    reads = synth.to_strings(blob, offs)
    return reads, ["r%09d" % i for i in range(len(reads))]


def cluster(eng, reads, names, cid, helpers):
    eng.set_reads(reads, names)
    t0 = time.perf_counter()
    nu = eng.cluster(cid, helpers=helpers or None)
    dt = time.perf_counter() - t0
    rep_of, strand, _ = eng.get_derep()
    pct, order = eng.get_cluster()
    return dt, (nu, rep_of.copy(), strand.copy(), pct.view(np.uint64).copy(), order.copy())


def copied_per_window(eng, reads, names, cid, helpers):
    """MB copied between contexts per window: the ITSX_CL_DEBUG summary line of an untimed run (the library writes to fd 2)"""
    os.environ["ITSX_CL_DEBUG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            eng.set_reads(reads, names)
            eng.cluster(cid, helpers=helpers)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["ITSX_CL_DEBUG"]
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"\[cluster\] (\d+) shards, columns per shard ([\d ]+), ([\d.]+) MB copied per window", text)
    return (float(m.group(3)), [int(x) for x in m.group(2).split()]) if m else (None, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[1_000_000, 3_000_000])
    ap.add_argument("--cluster-id", type=float, default=0.995)
    ap.add_argument("--same-device", type=int, nargs="+", default=[2, 4], help="contexts on device 0")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from itsxpress_amd import Engine
    import torch
    ndev = torch.cuda.device_count()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt") as f:
        hmm = f.read()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    eng = Engine(0)
    for n in args.reads:
        reads, names = cfg4_reads(n, hmm)
        t1, ref = cluster(eng, reads, names, args.cluster_id, None)
        windows = int(eng.stats()["cl_windows"])
        emit({"reads": n, "arm": "1 context", "contexts": 1, "devices": [0], "wall_s": round(t1, 3), "windows": windows,
              "n_unique": int(ref[0]), "mb_copied_per_window": 0.0})
        arms = [("%d contexts, device 0" % k, [0] * k) for k in args.same_device]
        arms += [("%d devices" % k, list(range(k))) for k in range(2, 9)]
        for name, devs in arms:
            if max(devs) >= ndev:
                emit({"reads": n, "arm": name, "contexts": len(devs), "devices": devs, "result": "not measured",
                      "why": "%d device(s) visible" % ndev})
                continue
            helpers = [Engine(d) for d in devs[1:]]
            try:
                t, got = cluster(eng, reads, names, args.cluster_id, helpers)
                equal = all(np.array_equal(a, b) for a, b in zip(got[1:], ref[1:])) and got[0] == ref[0]
                mb, cols = copied_per_window(eng, reads, names, args.cluster_id, helpers)
            finally:
                for h in helpers:
                    h.close()
            emit({"reads": n, "arm": name, "contexts": len(devs), "devices": devs, "wall_s": round(t, 3),
                  "windows": int(eng.stats()["cl_windows"]), "n_unique": int(got[0]), "equal_to_one_context": bool(equal),
                  "time_vs_one_context": round(t / t1, 3), "mb_copied_per_window": mb, "columns_per_shard": cols})
            if not equal:
                raise SystemExit("arm %r differs from the one-context clusters at %d reads" % (name, n))
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            for s in lines:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
