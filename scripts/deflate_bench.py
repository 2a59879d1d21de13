#!/usr/bin/env python3
"""The batch writers' gzip output deflated on the host (the default) against deflated on the device (Engine.deflate = "device",
csrc/k_deflate.hip), in one process on one warm context, the two arms alternating after a warm-up of each.

Two workloads: (a) the batch shape of scripts/batch_bench.py --trim -- S paired samples of n 2x250 pairs from their files through
`SampleBatch(keep_records=True)`: merged, dereplicated, searched, then `write_trimmed(gzipped=True)` timed in both arms; (b) one
single-end sample of N cfg2 reads loaded with its records kept, dereplicated, searched, then `write_trimmed_samples(gzipped=True)`
timed in both arms.  Per arm: every run's seconds, the median and the spread; for the device arm the kernel's GB/s of text from device
events (itsx_stats.ms_deflate).  Every device file is inflated and compared with the host arm's text once.
Ratio: output bytes over text bytes of the first 64 MiB of workload (b)'s text, beside zlib levels 1 and 6 on the same text taken as
independent members per itsx_deflate_block_bytes() bytes.

Usage: python scripts/deflate_bench.py [--samples 384] [--pairs 2000] [--reads 10000000] [--repeats 5] [--out profiles/device_deflate.md]"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def say(*a):
    print(*a, flush=True)


def write_paired_sample(thmm, d, s, n_pairs):
    """one sample's R1 / R2 (plain FASTQ): amplicons of 300-480 bases from a library of ITS templates, sequenced as 2x250 with
    Illumina-like qualities and errors (scripts/batch_bench.py's samples)"""
    import synth
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


def text_digest(path):
    h = hashlib.sha256()
    with gzip.open(path, "rb") as f:
        for piece in iter(lambda: f.read(16 << 20), b""):
            h.update(piece)
    return h.digest()


def timed_arms(eng, write, repeats, text_bytes):
    """write(tag) writes the files and returns their paths; the arms alternate, each after one untimed run"""
    res = {"host": [], "device": []}
    kernel_ms, out_bytes, paths = [], {}, {}
    for r in range(-1, repeats):
        for arm in ("host", "device"):
            eng.deflate = arm
            try:
                t0 = time.perf_counter()
                p = write("%s_%d" % (arm, r))
                dt = time.perf_counter() - t0
            finally:
                eng.deflate = "host"
            if r < 0:
                paths[arm] = p
                out_bytes[arm] = sum(os.path.getsize(x) for x in p)
                continue
            res[arm].append(dt)
            if arm == "device":
                kernel_ms.append(eng.stats()["ms_deflate"])
            for x in p:
                os.remove(x)
    same = all(text_digest(a) == text_digest(b) for a, b in zip(paths["host"], paths["device"]))
    out = {"text_bytes": text_bytes, "same_text": same}
    for arm in res:
        v = res[arm]
        out[arm] = {"runs_s": [round(x, 3) for x in v], "median_s": round(float(np.median(v)), 3), "spread_s": round(max(v) - min(v), 3),
                    "out_bytes": out_bytes[arm], "ratio": round(out_bytes[arm] / max(1, text_bytes), 4)}
    km = float(np.median(kernel_ms))
    out["device"]["kernel_ms_median"] = round(km, 2)
    out["device"]["kernel_GBps_of_text"] = round(text_bytes / 1e9 / (km / 1e3), 2) if km > 0 else None
    out["device_faster_beyond_host_spread"] = bool(out["host"]["median_s"] - out["device"]["median_s"] > out["host"]["spread_s"])
    return out


def batch_workload(eng, tmp, thmm, S, n, repeats):
    from bench import its2_profiles
    from itsxpress_amd import SeqSamplePairedNotInterleaved
    from itsxpress_amd.batch import SampleBatch
    os.environ["ITSXPRESS_ARRAYS"] = "0"
    d = os.path.join(tmp, "batch")
    os.makedirs(d)
    files = [write_paired_sample(thmm, d, s, n) for s in range(S)]
    hmm = os.path.join(d, "its2.hmm")
    with open(hmm, "w") as f:
        f.write(its2_profiles(thmm))
    os.makedirs(os.path.join(d, "work"))
    objs = [SeqSamplePairedNotInterleaved(r1, os.path.join(d, "work"), r2) for r1, r2 in files]
    b = SampleBatch(objs, engine=eng, keep_records=True)
    b.merge_reads(threads=1, stagger=False)
    b.deduplicate(threads=1)
    b._search(hmmfile=hmm, threads=1)
    plain = [os.path.join(d, "plain_%04d.fq" % k) for k in range(S)]
    b.write_trimmed(plain, "ITS2")
    text_bytes = sum(os.path.getsize(p) for p in plain)
    for p in plain:
        os.remove(p)
    say("batch: %d samples, %d merged reads, %.1f MB of trimmed text" % (S, int(b.counts.sum()), text_bytes / 1e6))

    def write(tag):
        outs = [os.path.join(d, "%s_%04d.fq.gz" % (tag, k)) for k in range(S)]
        b.write_trimmed(outs, "ITS2", gzipped=True)
        return outs
    res = timed_arms(eng, write, repeats, text_bytes)
    res.update(samples=S, pairs_per_sample=n, merged_reads=int(b.counts.sum()))
    return res


def single_workload(eng, tmp, thmm, n, repeats):
    import synth
    from bench import its2_profiles
    d = os.path.join(tmp, "single")
    os.makedirs(d)
    blob, offs = synth.make_reads(thmm, n, config=2, seed=synth.SEED + 2)
    bases, offs = np.frombuffer(blob, np.uint8), np.asarray(offs, np.int64)
    lens = np.diff(offs)
    fq = os.path.join(d, "in.fastq")
    rng = np.random.default_rng(9)
    with open(fq, "wb") as f:                # Illumina-like qualities: high, decaying along the read (scripts/file_run.py's)
        qtab = np.stack([(np.clip(38 - (np.arange(600) // 25) - rng.integers(0, 6, 600), 2, 40) + 33).astype(np.uint8) for _ in range(64)])
        if lens.min() == lens.max():
            L, step = int(lens[0]), 1 << 20
            for lo in range(0, n, step):
                m = min(step, n - lo)
                head = np.frombuffer(b"@read0000000000 1:N:0:1\n", np.uint8)
                rec = np.empty((m, head.size + L + 3 + L + 1), np.uint8)
                rec[:, :head.size] = head
                idx = np.arange(lo, lo + m)
                for k in range(10):
                    rec[:, 5 + k] = 48 + (idx // 10 ** (9 - k)) % 10
                rec[:, head.size:head.size + L] = bases[offs[lo]:offs[lo + m]].reshape(m, L)
                rec[:, head.size + L:head.size + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
                rec[:, head.size + L + 3:head.size + 2 * L + 3] = qtab[idx & 63, :L]
                rec[:, -1] = 10
                f.write(rec.tobytes())
        else:
            for i in range(n):
                s = bases[offs[i]:offs[i + 1]]
                f.write(b"@read%d 1:N:0:1\n" % i + s.tobytes() + b"\n+\n" + qtab[i & 63, :len(s)].tobytes() + b"\n")
    say("single: %d reads written (%.2f GB)" % (n, os.path.getsize(fq) / 1e9))
    eng.load_profiles(text=its2_profiles(thmm))
    eng.keep_records(True)
    try:
        eng.load_reads_files([fq])
    finally:
        eng.keep_records(False)
    os.remove(fq)
    eng.derep()
    eng.search()
    eng.finalize()
    plain = os.path.join(d, "plain.fq")
    (nw, tot), = eng.write_trimmed_samples([plain], region_prefixes=("3_", "4_"))
    text_bytes = os.path.getsize(plain)
    with open(plain, "rb") as f:
        sample = f.read(64 << 20)
    os.remove(plain)
    say("single: %d of %d reads trimmed, %.2f GB of trimmed text" % (nw, n, text_bytes / 1e9))

    def write(tag):
        out = os.path.join(d, tag + ".fq.gz")
        eng.write_trimmed_samples([out], region_prefixes=("3_", "4_"), gzipped=True)
        return [out]
    res = timed_arms(eng, write, repeats, text_bytes)
    res.update(reads=n, reads_written=int(nw))
    # the ratio, on the same bytes for every coder
    B = int(eng.L.itsx_deflate_block_bytes())
    dev = sum(len(z) for z in eng.deflate_device(sample, [0, len(sample)]))
    ratio = {"sample_bytes": len(sample), "block_bytes": B, "device": round(dev / len(sample), 4)}
    for level in (1, 6):
        z = 0
        for o in range(0, len(sample), B):
            c = zlib.compressobj(level, zlib.DEFLATED, 31)
            z += len(c.compress(sample[o:o + B])) + len(c.flush())
        ratio["zlib_%d" % level] = round(z / len(sample), 4)
    res["ratio_members_per_block"] = ratio
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_deflate.md"))
    args = ap.parse_args()
    from itsxpress_amd import Engine
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt") as f:
        thmm = f.read()
    tmp = tempfile.mkdtemp(prefix="itsx_deflate_bench_")
    try:
        eng = Engine(0)
        res = {}
        if args.samples > 0:
            res["batch"] = batch_workload(eng, tmp, thmm, args.samples, args.pairs, args.repeats)
            say(json.dumps(res["batch"]))
        if args.reads > 0:
            res["single"] = single_workload(eng, tmp, thmm, args.reads, args.repeats)
            say(json.dumps(res["single"]))
        eng.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lines = ["# Device deflate against the host's, `write_trimmed(gzipped=True)`", "",
             "Command: `python scripts/deflate_bench.py --samples %d --pairs %d --reads %d --repeats %d`" % (args.samples, args.pairs, args.reads, args.repeats), "",
             "One process, one warm context, one MI355X and the host's I/O threads; the arms alternate after one untimed run of each.", "",
             "| workload | text | host median (runs; spread) | device median (runs; spread) | device kernel | out / text host | out / text device |",
             "|---|---|---|---|---|---|---|"]
    for name, r in res.items():
        h, dv = r["host"], r["device"]
        what = "%d samples x %d pairs (%d merged reads)" % (r["samples"], r["pairs_per_sample"], r["merged_reads"]) if name == "batch" \
            else "1 sample, %d cfg2 reads (%d written)" % (r["reads"], r["reads_written"])
        lines.append("| %s | %.1f MB | %.3f s (%s; %.3f) | %.3f s (%s; %.3f) | %.2f ms, %s GB/s of text | %.4f | %.4f |" % (
            what, r["text_bytes"] / 1e6, h["median_s"], " ".join("%.3f" % x for x in h["runs_s"]), h["spread_s"], dv["median_s"],
            " ".join("%.3f" % x for x in dv["runs_s"]), dv["spread_s"], dv["kernel_ms_median"], dv["kernel_GBps_of_text"], h["ratio"], dv["ratio"]))
    lines.append("")
    for name, r in res.items():
        lines.append("- %s: every device file inflates to the host arm's text: %s; device faster than the host arm by more than the host runs' spread: %s"
                     % (name, r["same_text"], r["device_faster_beyond_host_spread"]))
    if "single" in res:
        q = res["single"]["ratio_members_per_block"]
        lines += ["", "Ratio on the first %.0f MiB of the single sample's trimmed text, independent members per %d bytes: device %.4f, zlib level 1 %.4f, zlib level 6 %.4f."
                  % (q["sample_bytes"] / 2 ** 20, q["block_bytes"], q["device"], q["zlib_1"], q["zlib_6"])]
    lines += ["", "```json", json.dumps(res), "```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    say("\n".join(lines))
    return 0 if all(r["same_text"] for r in res.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
