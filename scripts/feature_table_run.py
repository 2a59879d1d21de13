#!/usr/bin/env python
"""The feature table of a batch's trimmed ITS2 on the device against what a user does today.

    python scripts/feature_table_run.py [SAMPLES [READS_PER_SAMPLE [PASSES]]]      (default 384 2000 3)

The workload is scripts/batch_bench.py's: sample s is synth.make_reads(T.hmm, n, config=2, seed=synth.SEED + 100 + s), written here as
one FASTQ file per sample so that the batch keeps its records.  The batch is loaded, dereplicated and searched once; then PASSES timed
passes alternate two arms in this one process:

  device  Engine.trimmed_table(region_prefixes=ITS2) alone: the call's own ms_kernels and its wall time (the arrays and the sequences
          come back inside the call).
  host    SampleBatch.write_trimmed to plain files (cut from the records on the device, the fastest writer the batch has), then the base
          lines of every file counted with collections.Counter.  This is the repository's own stand-in for "write the files and
          dereplicate them", not vsearch.

Both arms' tables are compared once.  Prints one JSON line with the medians and the spreads (max - min).
"""
import gzip
import json
import os
import shutil
import sys
import tempfile
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from bench import its2_profiles  # noqa: E402
from itsxpress_amd import Engine, SeqSampleNotPaired  # noqa: E402
from itsxpress_amd.SeqSample import _REGION_PREFIX  # noqa: E402
from itsxpress_amd.batch import SampleBatch  # noqa: E402


def write_sample(d, s, n, thmm):
    """sample s of batch_bench.py's plain workload as a FASTQ file (fixed-length reads: the records are one numpy block)"""
    blob, offs = synth.make_reads(thmm, n, config=2, seed=synth.SEED + 100 + s, as_array=True)
    L = int(offs[1] - offs[0])
    assert (np.diff(offs) == L).all()
    head = b"@s%04d_000000000\n" % s
    rec = np.empty((n, len(head) + L + 3 + L + 1), np.uint8)
    rec[:, :len(head)] = np.frombuffer(head, np.uint8)
    for k in range(9):
        rec[:, 7 + k] = 48 + (np.arange(n) // 10 ** (8 - k)) % 10
    rec[:, len(head):len(head) + L] = np.asarray(blob, np.uint8).reshape(n, L)
    rec[:, len(head) + L:len(head) + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, len(head) + L + 3:-1] = ord("I")
    rec[:, -1] = 10
    path = os.path.join(d, "s%04d.fastq" % s)
    rec.tofile(path)
    return path


def main():
    argv = sys.argv[1:]
    S = int(argv[0]) if len(argv) > 0 else 384
    n = int(argv[1]) if len(argv) > 1 else 2000
    passes = int(argv[2]) if len(argv) > 2 else 3
    os.environ["ITSXPRESS_ARRAYS"] = "0"
    os.environ["ITSXPRESS_STREAM"] = "0"
    os.environ.pop("ITSXPRESS_GPUS", None)
    thmm = gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt").read()
    tmp = tempfile.mkdtemp(prefix="itsx_feature_table_")
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
        prefixes = _REGION_PREFIX["ITS2"]
        outs = [os.path.join(tmp, "trimmed_%04d.fq" % k) for k in range(S)]

        def device():
            t0 = time.perf_counter()
            t = eng.trimmed_table(region_prefixes=prefixes)
            return time.perf_counter() - t0, t

        def host():
            t0 = time.perf_counter()
            b.write_trimmed(outs, "ITS2")
            tw = time.perf_counter() - t0
            cells = Counter()
            for k, p in enumerate(outs):
                with open(p, "rb") as f:
                    for line in f.read().split(b"\n")[1::4]:
                        if line:
                            cells[(line, k)] += 1
            return time.perf_counter() - t0, tw, cells

        device()
        host()                                                  # warm-up: buffers at their working size, files' pages allocated once
        wall, kern, hwall, hwrite = [], [], [], []
        for _ in range(passes):                                 # the arms alternate
            dt, t = device()
            wall.append(dt)
            kern.append(t.ms_kernels / 1e3)
            ht, tw, cells = host()
            hwall.append(ht)
            hwrite.append(tw)
        dense = t.dense()
        seqs = t.sequences
        same = (len(cells) == len(t.entry_count) and
                all(cells[(seqs[f].encode(), int(s))] == int(c) for f in range(t.n_features)
                    for s, c in zip(t.entry_sample[t.row_off[f]:t.row_off[f + 1]], t.entry_count[t.row_off[f]:t.row_off[f + 1]])))

        def stat(v):
            return {"median_s": round(float(np.median(v)), 6), "spread_s": round(max(v) - min(v), 6), "all_s": [round(x, 6) for x in v]}
        print(json.dumps({"feature_table": True, "samples": S, "reads_per_sample": n, "passes": passes, "reads_counted": t.n_counted,
                          "features": t.n_features, "entries": int(len(t.entry_count)), "table_cells": int(dense.size),
                          "device_ms_kernels": stat(kern), "device_wall": stat(wall), "host_write_and_count": stat(hwall),
                          "host_write_trimmed_only": stat(hwrite), "identical_tables": bool(same)}))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
