"""Per-sample batching: S small samples through the path one by one (what the QIIME 2 plugin's loop does,
q2_itsxpress.py:273-333, here already on one shared context) against ONE batched pass (itsx_set_samples).
Checks that both give the same per-read coordinates.  Usage: python scripts/batch_bench.py [n_samples] [reads_per_sample]

--paired: the same comparison for PAIRED samples from their files, through the mirror classes: S samples of n 2x250 pairs one by one
(`SeqSamplePairedNotInterleaved._merge_reads` + `deduplicate` + `_search`, what q2_itsxpress.py:72-80 + 273-333 do per manifest
row) against `SampleBatch.merge_reads` + `deduplicate` + `_search`, in one process on one shared context; checks that every sample's
seq.fq (where written) / uc.txt / rep.fa / domtbl.txt are the same bytes.  ITSXPRESS_ARRAYS / ITSXPRESS_DOMTBL apply as usual.
Usage: python scripts/batch_bench.py --paired [n_samples] [pairs_per_sample]"""
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.environ.get("GRAFT_REPO_ROOT", "/root/repo")
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import synth  # noqa: E402
from bench import its2_profiles  # noqa: E402
from itsxpress_amd import Engine  # noqa: E402

PAIRED = "--paired" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--paired"]
S = int(argv[0]) if len(argv) > 0 else 96
n = int(argv[1]) if len(argv) > 1 else 10000
thmm = gzip.open(ROOT + "/tests/golden/T.hmm.gz", "rt").read()


def write_paired_sample(d, s, n_pairs):
    """one sample's R1 / R2 (plain FASTQ): amplicons of 300-480 bases from a library of ITS templates, sequenced as 2x250 with
    Illumina-like qualities and errors (scripts/paired_run.py's recipe)"""
    rng = np.random.default_rng(1000 + s)
    nt = max(1, n_pairs // 50)
    tb, to = synth.make_reads(thmm, nt, config=3, seed=synth.SEED + 300 + s, fixed_len=0, len_range=(300, 480), frac_templates=1.0,
                              sub_rate=0.0, n_rate=0.0, rc_rate=0.0)
    tb, tlen = np.frombuffer(tb, np.uint8), np.diff(to)
    tmat = np.full((nt, 480), ord("A"), np.uint8)
    for t in range(nt):
        tmat[t, :tlen[t]] = tb[to[t]:to[t + 1]]
    w = 1.0 / np.arange(1, nt + 1) ** 1.1
    ids = rng.choice(nt, size=n_pairs, p=w / w.sum())
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGTN", b"TGCAN"):
        comp[a] = b
    acgt = np.frombuffer(b"ACGT", np.uint8)
    qv, qp = np.array([2, 12, 22, 30, 37, 38], np.uint8), [.001, .009, .03, .08, .28, .6]
    sides = (tmat[ids, :250], comp[tmat[ids[:, None], tlen[ids][:, None] - 1 - np.arange(250)[None, :]]])
    paths = []
    for tag, reads in zip((b"1", b"2"), sides):
        q = rng.choice(qv, size=reads.shape, p=qp)
        err = rng.random(reads.shape) < 10.0 ** (-q.astype(np.float64) / 10.0)
        reads = reads.copy()
        reads[err] = acgt[rng.integers(0, 4, int(err.sum()))]
        head = b"@s%04d_0000000 " % s + tag + b":N:0:1\n"
        rec = np.empty((n_pairs, len(head) + 250 + 3 + 250 + 1), np.uint8)
        rec[:, :len(head)] = np.frombuffer(head, np.uint8)
        for k in range(7):
            rec[:, 7 + k] = 48 + (np.arange(n_pairs) // 10 ** (6 - k)) % 10
        rec[:, len(head):len(head) + 250] = reads
        rec[:, len(head) + 250:len(head) + 253] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, len(head) + 253:len(head) + 503] = q + 33
        rec[:, -1] = 10
        path = os.path.join(d, "s%04d_R%s.fastq" % (s, tag.decode()))
        with open(path, "wb") as f:
            f.write(rec.tobytes())
        paths.append(path)
    return paths


def paired_main():
    from itsxpress_amd import SeqSamplePairedNotInterleaved
    from itsxpress_amd.SeqSample import _fast_from_env
    from itsxpress_amd.batch import SampleBatch
    tmp = tempfile.mkdtemp(prefix="itsx_batch_bench_")
    try:
        files = [write_paired_sample(tmp, s, n) for s in range(S)]
        hmm = os.path.join(tmp, "its2.hmm")
        with open(hmm, "w") as f:
            f.write(its2_profiles(thmm))
        eng = Engine(0)
        kinds = ("uc_file", "rep_file", "dom_file") if _fast_from_env() else ("seq_file", "uc_file", "rep_file", "dom_file")

        def digest(objs):
            out = []
            for o in objs:
                h = hashlib.sha256()
                for k in kinds:
                    p = str(getattr(o, k))
                    h.update(open(p, "rb").read() if os.path.exists(p) else b"-")
                out.append(h.hexdigest())
            return out

        def one_by_one(fs, tag):
            objs = []
            for k, (r1, r2) in enumerate(fs):
                o = SeqSamplePairedNotInterleaved(r1, os.path.join(tmp, tag, "%04d" % k), r2)
                o._engine = eng
                o._merge_reads(threads=1, stagger=False)
                o.deduplicate(threads=1)
                o._search(hmmfile=hmm, threads=1)
                objs.append(o)
            return objs

        def batched(fs, tag):
            objs = [SeqSamplePairedNotInterleaved(r1, os.path.join(tmp, tag), r2) for r1, r2 in fs]
            b = SampleBatch(objs, engine=eng)
            b.merge_reads(threads=1, stagger=False)
            b.deduplicate(threads=1)
            b._search(hmmfile=hmm, threads=1)
            return objs, b

        from itsxpress_amd.trim import cache_clear
        one_by_one(files[:2], "warm1")         # warm-up on two samples: first-touch costs outside the timed legs
        batched(files[:2], "warm2")
        # each leg starts with an empty text cache: whichever runs second must not find the R1 / R2 texts the first one left there
        cache_clear()
        t0 = time.perf_counter()
        solo = one_by_one(files, "solo")
        t_one = time.perf_counter() - t0
        d_one = digest(solo) if not _fast_from_env() else None
        cache_clear()
        t0 = time.perf_counter()
        objs, b = batched(files, "batch")
        t_bat = time.perf_counter() - t0
        same = None if d_one is None else d_one == digest(objs)
        print(json.dumps({"paired": True, "samples": S, "pairs_per_sample": n, "merged_reads": int(b.counts.sum()),
                          "arrays_mode": _fast_from_env(), "domtbl": os.environ.get("ITSXPRESS_DOMTBL", "full"),
                          "one_by_one_s": round(t_one, 3), "batched_s": round(t_bat, 3), "one_by_one_over_batched": round(t_one / t_bat, 2),
                          "pairs_per_s_one_by_one": round(S * n / t_one), "pairs_per_s_batched": round(S * n / t_bat),
                          "identical_files": same}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if PAIRED:
    paired_main()
    sys.exit(0)
eng = Engine(0)
eng.load_profiles(text=its2_profiles(thmm))
parts = [synth.make_reads(thmm, n, config=2, seed=synth.SEED + 100 + s) for s in range(S)]


def one_by_one():
    out = []
    for blob, offs in parts:
        eng.set_reads_buffer(blob, offs)
        eng.derep()
        eng.search()
        eng.finalize()
        out.append([x.copy() for x in eng.trim_coords("3_", "4_")])
    return out


def batched():
    blob = b"".join(bytes(b) for b, _ in parts)
    offs = np.concatenate([[0]] + [o[1:] + k for (_, o), k in zip(parts, np.cumsum([0] + [int(o[-1]) for _, o in parts[:-1]]))]).astype(np.int64)
    smp = np.repeat(np.arange(S, dtype=np.int32), [len(o) - 1 for _, o in parts])
    eng.set_reads_buffer(blob, offs)
    eng.set_samples(smp, S)
    eng.derep()
    eng.search()
    eng.finalize()
    a = eng.trim_coords("3_", "4_")
    first = np.concatenate([[0], np.cumsum([len(o) - 1 for _, o in parts])])
    return [[x[first[i]:first[i + 1]] for x in a] for i in range(S)]


res = {}
for name, fn in (("one_by_one", one_by_one), ("batched", batched)):
    fn()                                   # warm-up: buffers grow to their working size
    t0 = time.perf_counter()
    out = fn()
    res[name] = time.perf_counter() - t0
    res[name + "_out"] = out
same = all(np.array_equal(a, b) for x, y in zip(res["one_by_one_out"], res["batched_out"]) for a, b in zip(x, y))
print(json.dumps({"samples": S, "reads_per_sample": n, "one_by_one_s": round(res["one_by_one"], 3), "batched_s": round(res["batched"], 3),
                  "reads_per_s_one_by_one": round(S * n / res["one_by_one"]), "reads_per_s_batched": round(S * n / res["batched"]),
                  "identical_coordinates": bool(same)}))
