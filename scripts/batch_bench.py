"""Per-sample batching: S small samples through the path one by one (what the QIIME 2 plugin's loop does,
q2_itsxpress.py:273-333, here already on one shared context) against ONE batched pass (itsx_set_samples).
Checks that both give the same per-read coordinates.  Usage: python scripts/batch_bench.py [n_samples] [reads_per_sample]

--paired: the same comparison for PAIRED samples from their files, through the mirror classes: S samples of n 2x250 pairs one by one
(`SeqSamplePairedNotInterleaved._merge_reads` + `deduplicate` + `_search`, what q2_itsxpress.py:72-80 + 273-333 do per manifest
row) against `SampleBatch.merge_reads` + `deduplicate` + `_search`, in one process on one shared context; checks that every sample's
seq.fq (where written) / uc.txt / rep.fa / domtbl.txt are the same bytes.  ITSXPRESS_ARRAYS / ITSXPRESS_DOMTBL apply as usual.
Usage: python scripts/batch_bench.py --paired [n_samples] [pairs_per_sample]

--orient: the same comparison for single-end CCS-style samples that are oriented first (the plugin with trim_ccs, q2_itsxpress.py:284-285):
S samples of n reads cut from the orientation database's sequences, some reverse-complemented, one by one
(`SeqSampleNotPaired.orient_reads` + `deduplicate` + `_search`) against `SampleBatch.orient_reads` + `deduplicate` + `_search`; checks
that every sample's oriented.fq / uc.txt / rep.fa / domtbl.txt are the same bytes.
Usage: python scripts/batch_bench.py --orient [n_samples] [reads_per_sample]

--trim: paired samples from raw files to each sample's trimmed merged reads, file to file: `merge_reads(write_seq_files=True)` +
`deduplicate` + `_search` + `write_trimmed` (every seq.fq written, then parsed again by the host writer) against
`SampleBatch(keep_records=True)` (the records stay on the device, one `itsx_write_trimmed_samples`).  Warm context, the two legs
alternating, medians and the spread of each; checks that every sample's output is the same bytes.
Usage: python scripts/batch_bench.py --trim [n_samples] [pairs_per_sample] [repeats]

--trim-paired: the plugin's main case, `trim_pair_output_unmerged`, on one warm context: a `SampleBatch(keep_records=True)` is merged,
dereplicated and searched, and its `write_paired_trimmed` -- the host loop: every sample's R1 / R2 read and parsed again by
`itsx_write_trimmed_paired` -- runs `repeats` times with the text cache as the merge left it and `repeats` times with it emptied first;
then the same for a `SampleBatch(keep_records="pairs")`, whose `write_paired_trimmed` is one `itsx_write_trimmed_paired_samples` from the
pair records on the device.  Medians, the plan's and the copy's device times, and a check that every sample's two files are the same bytes.
Usage: python scripts/batch_bench.py --trim-paired [n_samples] [pairs_per_sample] [repeats]

--pairs-flow: the flow `SampleBatch(keep_records="pairs")` exists for, from the compressed input files to the compressed output files on
one warm context -- `merge_reads` + `deduplicate` + `_search` + `write_trimmed` + `write_paired_trimmed` (gzipped) -- once per arm of
`--inflate host,device` x `--parse host,device` (SampleBatch.inflate / .parse; default: host alone), the arms alternated within every
repeat, the first repeat the warm-up.  The inputs are gzip files of the device deflate's members (`--plain-inputs`: plain text).
Per arm the stage times of every repeat, the parse and inflate counters, and a check that every arm wrote the same bytes.
Usage: python scripts/batch_bench.py --pairs-flow [n_samples] [pairs_per_sample] [repeats] [--inflate LIST] [--parse LIST] [--plain-inputs]

--share-samples: sample sharing (Engine.share_samples: each distinct representative of a batch scored once for all the samples it occurs
in) against the same batch without it, on one warm context in the full rows mode (--rows lazy / compact: in that rows mode, with
Engine.share_samples_lazy as the setting; a lazy search's counters are bounds, so its identity check covers the coordinates only), the
two arms alternated within every repeat, the first
repeat the warm-up: derep + search + finalize + coordinates of S samples of n single-end reads handed over as arrays.  --overlap F (0..1,
default 0.5) shapes the synthetic manifest: a share F of each sample's DISTINCT sequences is replaced by sequences drawn from a pool
common to all samples (as large as one sample's distinct set, so a pool sequence turns up in about F of the samples); the rest are the
sample's own.  The overlap is the generator's, not a real manifest's.  Per arm the wall times of every repeat, median and spread, the
search's share of it; for the sharing arm the classes, the uniques not scored, the rows copied and the device time of both steps; and a
check that both arms gave the same counters and coordinates.
Usage: python scripts/batch_bench.py --share-samples [n_samples] [reads_per_sample] [repeats] [--overlap F] [--rows full|lazy|compact]"""
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
ORIENT = "--orient" in sys.argv
TRIM = "--trim" in sys.argv
TRIM_PAIRED = "--trim-paired" in sys.argv
PAIRS_FLOW = "--pairs-flow" in sys.argv
PLAIN_INPUTS = "--plain-inputs" in sys.argv
SHARE_SAMPLES = "--share-samples" in sys.argv
argv = [a for a in sys.argv[1:] if a not in ("--paired", "--orient", "--trim", "--trim-paired", "--pairs-flow", "--plain-inputs", "--share-samples")]
ROWS = "full"
if "--rows" in argv:
    k = argv.index("--rows")
    ROWS = argv[k + 1]
    del argv[k:k + 2]
    if not SHARE_SAMPLES or ROWS not in ("full", "lazy", "compact"):
        sys.exit("--rows takes full, lazy or compact and goes with --share-samples")
OVERLAP = 0.5
if "--overlap" in argv:
    k = argv.index("--overlap")
    OVERLAP = float(argv[k + 1])
    del argv[k:k + 2]
    if not SHARE_SAMPLES or not 0.0 <= OVERLAP <= 1.0:
        sys.exit("--overlap takes a share between 0 and 1 and goes with --share-samples")
WHERE = {}
for opt in ("--inflate", "--parse"):           # where the batch's loaders inflate and parse: host, device or a comma-separated list (arms)
    if opt in argv:
        k = argv.index(opt)
        WHERE[opt[2:]] = argv[k + 1].split(",")
        del argv[k:k + 2]
if any(w not in ("host", "device") for l in WHERE.values() for w in l) or (WHERE and not PAIRS_FLOW):
    sys.exit("--inflate / --parse take host, device or a comma-separated list of them, and go with --pairs-flow")
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


def write_orient_sample(d, s, n_reads, db):
    """one sample's reads (plain FASTQ): stretches of 300-900 bases of the orientation database's sequences with 0.5 % substitutions,
    two of five reverse-complemented, every fifth read sequenced twice (something to dereplicate)"""
    rng = np.random.default_rng(2000 + s)
    comp = bytes.maketrans(b"ACGTURYMKSWHBVDN", b"TGCAAYRKMSWDVBHN")
    recs = []
    for i in range(n_reads):
        if i % 5 == 4 and recs:
            seq = recs[int(rng.integers(0, len(recs)))][1]
        else:
            src = db[int(rng.integers(0, len(db)))]
            L = min(len(src), int(rng.integers(300, 901)))
            a = int(rng.integers(0, len(src) - L + 1))
            seq = bytearray(src[a:a + L])
            for p in np.nonzero(rng.random(L) < 0.005)[0]:
                seq[p] = b"ACGT"[int(rng.integers(0, 4))]
            seq = bytes(seq)
            if i % 5 in (1, 3):
                seq = seq.translate(comp)[::-1]
        recs.append((b"s%04d_%07d" % (s, i), seq))
    path = os.path.join(d, "s%04d_ccs.fastq" % s)
    with open(path, "wb") as f:
        for name, seq in recs:
            f.write(b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    return path


def orient_main():
    import importlib
    import itsxpress_amd.definitions as definitions
    os.environ.setdefault("ITSXPRESS_DB_DIR", ROOT + "/tests/golden")      # where the orientation database lies unless the caller says otherwise
    importlib.reload(definitions)
    from itsxpress_amd import SeqSampleNotPaired
    from itsxpress_amd.SeqSample import _fast_from_env
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.definitions import ROOT_DIR
    from itsxpress_amd.trim import cache_clear
    db, cur = [], []
    for line in gzip.open(os.path.join(ROOT_DIR, "universal_orient_ref_clean.fasta.gz"), "rb"):
        if line.startswith(b">"):
            if cur:
                db.append(b"".join(cur))
            cur = []
        else:
            cur.append(line.strip().upper())
    if cur:
        db.append(b"".join(cur))
    tmp = tempfile.mkdtemp(prefix="itsx_batch_bench_")
    try:
        files = [write_orient_sample(tmp, s, n, db) for s in range(S)]
        hmm = os.path.join(tmp, "its2.hmm")
        with open(hmm, "w") as f:
            f.write(its2_profiles(thmm))
        eng = Engine(0)
        kinds = ("seq_file", "uc_file", "rep_file", "dom_file")

        def digest(objs):                      # per sample, one hash per file: a difference names its file
            return [[hashlib.sha256(open(str(getattr(o, k)), "rb").read() if os.path.exists(str(getattr(o, k))) else b"-").hexdigest() for k in kinds]
                    for o in objs]

        def one_by_one(fs, tag):
            objs = []
            for k, f in enumerate(fs):
                o = SeqSampleNotPaired(f, os.path.join(tmp, tag, "%04d" % k))
                o._engine = eng
                o.orient_reads(threads=1)
                o.deduplicate(threads=1)
                o._search(hmmfile=hmm, threads=1)
                objs.append(o)
            return objs

        def batched(fs, tag):
            objs = [SeqSampleNotPaired(f, os.path.join(tmp, tag)) for f in fs]
            b = SampleBatch(objs, engine=eng)
            b.orient_reads(threads=1)
            b.deduplicate(threads=1)
            b._search(hmmfile=hmm, threads=1)
            return objs, b

        one_by_one(files[:2], "warm1")         # warm-up on two samples: first-touch costs outside the timed legs
        eng.set_rows_mode(None)
        batched(files[:2], "warm2")
        cache_clear()                          # each leg starts with an empty text cache
        t0 = time.perf_counter()
        solo = one_by_one(files, "solo")
        t_one = time.perf_counter() - t0
        d_one = digest(solo) if not _fast_from_env() else None
        eng.set_rows_mode(None)
        cache_clear()
        t0 = time.perf_counter()
        objs, b = batched(files, "batch")
        t_bat = time.perf_counter() - t0
        d_bat = digest(objs) if d_one is not None else None
        same = None if d_one is None else d_one == d_bat
        if same is False:                      # which files of which samples differ
            bad = [(i, k) for i, (x, y) in enumerate(zip(d_one, d_bat)) for k, a, c in zip(kinds, x, y) if a != c]
            print("differing files (sample, kind), the first of %d: %s" % (len(bad), bad[:12]), file=sys.stderr)
        print(json.dumps({"orient": True, "samples": S, "reads_per_sample": n, "oriented_reads": int(b.counts.sum()),
                          "arrays_mode": _fast_from_env(), "domtbl": os.environ.get("ITSXPRESS_DOMTBL", "full"),
                          "one_by_one_s": round(t_one, 3), "batched_s": round(t_bat, 3), "one_by_one_over_batched": round(t_one / t_bat, 2),
                          "reads_per_s_one_by_one": round(S * n / t_one), "reads_per_s_batched": round(S * n / t_bat),
                          "identical_files": same}))
        return 1 if same is False else 0       # the files of the two legs must be the same bytes
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def trim_main():
    import torch
    from itsxpress_amd import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.trim import cache_clear
    os.environ["ITSXPRESS_ARRAYS"] = "0"
    repeats = int(argv[2]) if len(argv) > 2 else 5
    tmp = tempfile.mkdtemp(prefix="itsx_batch_bench_")
    try:
        files = [write_paired_sample(tmp, s, n) for s in range(S)]
        hmm = os.path.join(tmp, "its2.hmm")
        with open(hmm, "w") as f:
            f.write(its2_profiles(thmm))
        eng = Engine(0)

        def leg(fs, tag, keep):
            objs = [SeqSamplePairedNotInterleaved(r1, os.path.join(tmp, tag), r2) for r1, r2 in fs]
            b = SampleBatch(objs, engine=eng, keep_records=keep)
            if keep:
                b.merge_reads(threads=1, stagger=False)
            else:
                b.merge_reads(threads=1, stagger=False, write_seq_files=True)
            torch.cuda.synchronize()
            used = torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]
            b.deduplicate(threads=1)
            b._search(hmmfile=hmm, threads=1)
            outs = [os.path.join(tmp, tag, "trimmed_%04d.fq" % k) for k in range(len(objs))]
            t0 = time.perf_counter()
            ret = b.write_trimmed(outs, "ITS2")
            return outs, ret, time.perf_counter() - t0, used, int(b.counts.sum())

        leg(files[:2], "warm_files", False)    # warm-up on two samples: first-touch costs outside the timed legs
        leg(files[:2], "warm_kept", True)
        times = {False: [], True: []}
        wtimes = {False: [], True: []}
        used = {}
        digests = {}
        for r in range(repeats):               # the legs alternate; each starts with an empty text cache
            for keep in (False, True):
                cache_clear()
                tag = "%s_%d" % ("kept" if keep else "files", r)
                t0 = time.perf_counter()
                outs, ret, tw, mem, merged = leg(files, tag, keep)
                times[keep].append(time.perf_counter() - t0)
                wtimes[keep].append(tw)
                used[keep] = mem
                if r == 0:
                    digests[keep] = ([hashlib.sha256(open(p, "rb").read()).hexdigest() for p in outs], [tuple(x) for x in ret])
                    nbytes = sum(os.path.getsize(p) for p in outs)
                shutil.rmtree(os.path.join(tmp, tag), ignore_errors=True)
        same = digests[False] == digests[True]
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"trim": True, "samples": S, "pairs_per_sample": n, "merged_reads": merged, "repeats": repeats, "trimmed_bytes": nbytes,
                          "files_path_s": [round(x, 3) for x in times[False]], "records_path_s": [round(x, 3) for x in times[True]],
                          "files_path_median_s": round(med[False], 3), "records_path_median_s": round(med[True], 3),
                          "files_path_spread_s": round(max(times[False]) - min(times[False]), 3),
                          "write_trimmed_files_median_s": round(float(np.median(wtimes[False])), 3),
                          "write_trimmed_records_median_s": round(float(np.median(wtimes[True])), 3),
                          "device_bytes_after_merge_files": used[False], "device_bytes_after_merge_records": used[True],
                          "identical_outputs": same}))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def trim_paired_main():
    from itsxpress_amd import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.trim import cache_clear
    os.environ["ITSXPRESS_ARRAYS"] = "0"
    repeats = int(argv[2]) if len(argv) > 2 else 5
    tmp = tempfile.mkdtemp(prefix="itsx_batch_bench_")
    try:
        files = [write_paired_sample(tmp, s, n) for s in range(S)]
        hmm = os.path.join(tmp, "its2.hmm")
        with open(hmm, "w") as f:
            f.write(its2_profiles(thmm))
        eng = Engine(0)

        def searched(fs, tag, keep):
            objs = [SeqSamplePairedNotInterleaved(r1, os.path.join(tmp, tag), r2) for r1, r2 in fs]
            b = SampleBatch(objs, engine=eng, keep_records=keep)
            b.merge_reads(threads=1, stagger=False)
            b.deduplicate(threads=1)
            b._search(hmmfile=hmm, threads=1)
            return b

        def write(b, tag):
            d = os.path.join(tmp, tag)
            os.makedirs(d, exist_ok=True)
            o1 = [os.path.join(d, "t_%04d_R1.fq" % k) for k in range(len(b.samples))]
            o2 = [os.path.join(d, "t_%04d_R2.fq" % k) for k in range(len(b.samples))]
            t0 = time.perf_counter()
            ret = b.write_paired_trimmed(o1, o2, "ITS2")
            return o1 + o2, [int(x) for x in ret], time.perf_counter() - t0

        for keep in (True, "pairs"):           # warm-up on two samples: first-touch costs outside the timed calls
            write(searched(files[:2], "warm_%s" % keep, keep), "warm_out_%s" % keep)
        times = {"host": [], "host_cold_cache": [], "device": []}
        kernels = []
        digests = {}
        # a read set is one batch's at a time: first the batch that keeps no pair records (write_paired_trimmed is the host loop, with
        # the text cache as the merge left it and emptied first), then the batch that keeps them -- the same warm context and inputs
        for keep, legs in ((True, ("host", "host_cold_cache")), ("pairs", ("device",))):
            b = searched(files, "batch_%s" % keep, keep)
            for r in range(repeats):
                for leg in legs:
                    if leg == "host_cold_cache":
                        cache_clear()
                    tag = "%s_%d" % (leg, r)
                    outs, ret, dt = write(b, tag)
                    times[leg].append(dt)
                    if leg == "device":
                        st = eng.stats()
                        kernels.append((st["ms_trim_plan"], st["ms_trim_copy"]))
                    if r == 0:
                        digests[leg] = ([hashlib.sha256(open(p, "rb").read()).hexdigest() for p in outs], ret)
                        nbytes = sum(os.path.getsize(p) for p in outs)
                    shutil.rmtree(os.path.join(tmp, tag), ignore_errors=True)
        same = digests["host"] == digests["device"] == digests["host_cold_cache"]
        print(json.dumps({"trim_paired": True, "samples": S, "pairs_per_sample": n, "merged_reads": int(b.counts.sum()), "repeats": repeats,
                          "pairs_written": int(sum(digests["device"][1])), "trimmed_bytes": nbytes,
                          "host_s": [round(x, 3) for x in times["host"]], "host_cold_cache_s": [round(x, 3) for x in times["host_cold_cache"]],
                          "device_s": [round(x, 3) for x in times["device"]],
                          "host_median_s": round(float(np.median(times["host"])), 3),
                          "host_cold_cache_median_s": round(float(np.median(times["host_cold_cache"])), 3),
                          "device_median_s": round(float(np.median(times["device"])), 3),
                          "plan_kernels_median_ms": round(float(np.median([k[0] for k in kernels])), 3),
                          "copy_kernels_median_ms": round(float(np.median([k[1] for k in kernels])), 3),
                          "identical_outputs": same}))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def pairs_flow_main():
    from itsxpress_amd import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    from itsxpress_amd.trim import cache_clear
    os.environ["ITSXPRESS_ARRAYS"] = "0"
    repeats = int(argv[2]) if len(argv) > 2 else 4
    arms = [(i, p) for i in WHERE.get("inflate", ["host"]) for p in WHERE.get("parse", ["host"])]
    tmp = tempfile.mkdtemp(prefix="itsx_batch_bench_")
    try:
        eng = Engine(0)
        files = [write_paired_sample(tmp, s, n) for s in range(S)]
        if not PLAIN_INPUTS:
            for fs in files:
                for k, p in enumerate(fs):
                    with open(p, "rb") as f:
                        text = f.read()
                    with open(p + ".gz", "wb") as f:
                        f.write(eng.deflate_device(text, [0, len(text)])[0])
                    os.remove(p)
                    fs[k] = p + ".gz"
        hmm = os.path.join(tmp, "its2.hmm")
        with open(hmm, "w") as f:
            f.write(its2_profiles(thmm))
        counters = ("n_parse_device", "n_parse_declined", "n_inflate_device", "n_inflate_declined")

        def flow(fs, tag, arm):
            d = os.path.join(tmp, tag)
            os.makedirs(d, exist_ok=True)
            cache_clear()                      # every run reads and inflates its inputs itself
            st0 = eng.stats()
            t, t0 = {}, time.perf_counter()
            objs = [SeqSamplePairedNotInterleaved(r1, d, r2) for r1, r2 in fs]
            b = SampleBatch(objs, engine=eng, keep_records="pairs")
            b.inflate, b.parse = arm
            b.merge_reads(threads=1, stagger=False)
            t["merge"] = time.perf_counter() - t0
            moved = {k: int(eng.stats()[k] - st0[k]) for k in counters}
            t0 = time.perf_counter()
            b.deduplicate(threads=1)
            b._search(hmmfile=hmm, threads=1)
            t["derep+search"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            om = [os.path.join(d, "m_%04d.fq.gz" % k) for k in range(len(fs))]
            o1 = [os.path.join(d, "t_%04d_R1.fq.gz" % k) for k in range(len(fs))]
            o2 = [os.path.join(d, "t_%04d_R2.fq.gz" % k) for k in range(len(fs))]
            b.write_trimmed(om, "ITS2", gzipped=True)
            ret = b.write_paired_trimmed(o1, o2, "ITS2", gzipped=True)
            t["write"] = time.perf_counter() - t0
            st = eng.stats()
            digest = hashlib.sha256(b"".join(gzip.decompress(open(p, "rb").read()) for p in om + o1 + o2)).hexdigest()
            shutil.rmtree(d, ignore_errors=True)
            return dict({"s_" + k: round(v, 3) for k, v in t.items()}, s_total=round(sum(t.values()), 3), ms_parse=round(float(st["ms_parse"]), 2),
                        ms_trim_copy=round(float(st["ms_trim_copy"]), 2), **moved), digest, int(sum(ret)), int(b.counts.sum())
        for arm in arms:                       # warm-up on two samples: first-touch costs outside the timed runs
            flow(files[:2], "warm_%s_%s" % arm, arm)
        out = [dict(inflate=i, parse=p, runs=[]) for i, p in arms]
        digests = set()
        for r in range(repeats):
            for k, arm in enumerate(arms):
                res, digest, written, merged = flow(files, "run_%d_%d" % (r, k), arm)
                out[k]["runs"].append(res)
                digests.add((digest, written, merged))
                print("[batch_bench] repeat %d, inflate %s, parse %s: %.2f s (merge %.2f s, derep+search %.2f s, write %.2f s)" % (r, arm[0], arm[1], res["s_total"], res["s_merge"], res["s_derep+search"], res["s_write"]), file=sys.stderr, flush=True)
        for a in out:
            timed = a["runs"][1:] or a["runs"]
            a["merge_median_s"] = round(float(np.median([x["s_merge"] for x in timed])), 3)
            a["total_median_s"] = round(float(np.median([x["s_total"] for x in timed])), 3)
        print(json.dumps({"pairs_flow": True, "samples": S, "pairs_per_sample": n, "repeats": repeats, "inputs": "plain" if PLAIN_INPUTS else "device-deflated gzip",
                          "merged_reads": merged, "pairs_written": written, "arms": out, "identical_outputs": len(digests) == 1}))
        return 0 if len(digests) == 1 else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def overlap_manifest(n_samples, reads_per_sample, overlap):
    """S samples of n reads (strings): every sample is its own draw of the generator (Zipf over its templates, substitutions, a few
    reverse complements: duplicates inside the sample), then a share `overlap` of its distinct sequences is replaced, read for read, by
    distinct sequences of a pool common to all samples (drawn without replacement, so the sample's distinct count stays)"""
    def draw(seed):
        blob, offs = synth.make_reads(thmm, reads_per_sample, config=2, seed=seed)
        return synth.to_strings(blob, offs)
    pool = list(dict.fromkeys(draw(synth.SEED + 99)))
    out = []
    for s in range(n_samples):
        rng = np.random.default_rng(7000 + s)
        reads = draw(synth.SEED + 100 + s)
        distinct = list(dict.fromkeys(reads))
        k = min(int(round(overlap * len(distinct))), len(pool))
        swap = dict(zip((distinct[i] for i in rng.choice(len(distinct), k, replace=False)), (pool[j] for j in rng.choice(len(pool), k, replace=False))))
        out.append([swap.get(r, r) for r in reads])
    return out


def share_samples_main():
    repeats = int(argv[2]) if len(argv) > 2 else 4
    samples = overlap_manifest(S, n, OVERLAP)
    blob = "".join(r for x in samples for r in x).encode()
    offs = np.concatenate([[0], np.cumsum([len(r) for x in samples for r in x])]).astype(np.int64)
    smp = np.repeat(np.arange(S, dtype=np.int32), [len(x) for x in samples])
    eng = Engine(0)
    eng.load_profiles(text=its2_profiles(thmm))
    eng.set_rows_mode(ROWS)
    setting = "share_samples" if ROWS == "full" else "share_samples_lazy"      # each rows mode has its own setting

    def run(share):
        setattr(eng, setting, share)
        t0 = time.perf_counter()
        eng.set_reads_buffer(blob, offs)
        eng.set_samples(smp, S)
        nu = eng.derep()
        t1 = time.perf_counter()
        eng.search()
        t2 = time.perf_counter()
        domz = eng.get_domz().copy()
        eng.finalize()
        coords = [x.copy() for x in eng.trim_coords("3_", "4_")]
        t3 = time.perf_counter()
        info = eng.sample_sharing_info()
        st = eng.stats()
        return dict(s_total=round(t3 - t0, 4), s_search=round(t2 - t1, 4), s_finalize_coords=round(t3 - t2, 4), n_unique=int(nu), n_pairs=int(st["n_pairs"]),
                    ms_msv=round(float(st["ms_msv"]), 2), ms_filters=round(float(st["ms_filters"]), 2), ms_domains=round(float(st["ms_domains"]), 2),
                    **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in info.items()}), (domz, coords)

    arms = {False: [], True: []}
    results = {}
    try:
        for r in range(repeats + 1):           # repeat 0 is the warm-up: buffers grow to their working size
            for share in (False, True):
                res, payload = run(share)
                if r == 0:
                    results[share] = payload
                    continue
                arms[share].append(res)
                print("[batch_bench] repeat %d, %s %s: %.3f s (search %.3f s)" % (r, setting, share, res["s_total"], res["s_search"]), file=sys.stderr, flush=True)
    finally:
        setattr(eng, setting, False)
        eng.set_rows_mode(None)
    # (a lazy search's counters are bounds, and which pairs it evaluates may depend on the last bits of pass A's scores, hence on the
    # prefix tree of the uniques searched: both arms' bounds are valid, not necessarily equal -- the identity check is the coordinates')
    same = (ROWS == "lazy" or np.array_equal(results[False][0], results[True][0])) and all(np.array_equal(a, b) for a, b in zip(results[False][1], results[True][1]))
    out = {"share_samples": True, "samples": S, "reads_per_sample": n, "overlap": OVERLAP, "repeats": repeats, "rows_mode": ROWS, "setting": setting}
    for share, name in ((False, "off"), (True, "on")):
        for key in ("s_total", "s_search"):
            v = [x[key] for x in arms[share]]
            out["%s_%s" % (name, key)] = v
            out["%s_%s_median" % (name, key)] = round(float(np.median(v)), 4)
            out["%s_%s_spread" % (name, key)] = round(max(v) - min(v), 4)
        out["%s_last" % name] = arms[share][-1]
    out["off_over_on_total"] = round(out["off_s_total_median"] / out["on_s_total_median"], 3)
    out["off_over_on_search"] = round(out["off_s_search_median"] / out["on_s_search_median"], 3)
    out["identical_counters_and_coordinates" if ROWS != "lazy" else "identical_coordinates"] = bool(same)
    print(json.dumps(out))
    return 0 if same else 1


if SHARE_SAMPLES:
    if len(argv) < 1:
        S, n = 384, 2000
    sys.exit(share_samples_main())
if PAIRS_FLOW:
    if len(argv) < 1:
        S, n = 384, 2000
    sys.exit(pairs_flow_main())
if TRIM_PAIRED:
    if len(argv) < 1:
        S, n = 384, 2000
    sys.exit(trim_paired_main())
if TRIM:
    if len(argv) < 1:
        S, n = 384, 2000
    sys.exit(trim_main())
if PAIRED:
    paired_main()
    sys.exit(0)
if ORIENT:
    sys.exit(orient_main())
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
