#!/usr/bin/env python3
"""File to file on one GPU: a gzip FASTQ of N synthetic 300-bp reads in, a compressed FASTQ of the trimmed reads out
-- what a user of `itsxpress --fastq x.fq.gz --single_end --region ITS2 --outfile y.fq.gz` waits for, stage by stage
(load = inflate + parse + upload + device packing; write = slice + block-parallel deflate; the input's text is shared
between the two through the reader's cache, ITSX_TEXT_CACHE_GB=0 turns that off).
--flip F reverse-complements that share of the generated reads (qualities reversed); --stream --orient profiles orients them inside
the streamed run (StreamEngine.plan_orient), --stream --orient staged as a user had to before: a plain engine writes oriented.fq,
the streamed run reads that.
Prints one JSON line.  usage: file_run.py [--reads 1000000] [--out-kind gz|zst|plain] [--stream [--check]] [--flip 0.33 --orient profiles]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--out-kind", default="gz", choices=["gz", "zst", "plain"])
    ap.add_argument("--rows", default="lazy", choices=["lazy", "compact", "full"], help="the search's rows mode (lazy = what ITSXPRESS_ARRAYS=1 selects)")
    ap.add_argument("--shape", default="cfg1", choices=["cfg1", "cfg2"], help="cfg1: 300-base reads; cfg2: merged reads of 300-580 bases")
    ap.add_argument("--stream", action="store_true", help="file-order chunks scored while the file is inflated (itsxpress_amd/stream.py)")
    ap.add_argument("--chunk-mb", type=float, default=0.0, help="--stream: text per chunk (0: about a tenth of the file)")
    ap.add_argument("--stream-write", action="store_true", help="--stream: the writer inside the pipeline too (provisional thresholds per chunk)")
    ap.add_argument("--deflate", default="host", choices=["host", "device"], help="--stream --stream-write with gz output: where the writer's gzip members are made (StreamEngine.deflate)")
    ap.add_argument("--inflate", default="host", choices=["host", "device"], help="where the whole-file load inflates the input (Engine.inflate); not with --stream")
    ap.add_argument("--parse", default="host", choices=["host", "device"], help="where the whole-file load parses the FASTQ text (Engine.parse); not with --stream")
    ap.add_argument("--loads", type=int, default=1, help="whole-file load: this many timed loads, the text cache cleared before each (the stages' total counts the last)")
    ap.add_argument("--in-writer", default="host", choices=["host", "device"], help="who writes the generated in.fastq.gz: the host writer (members of 4 MiB of text) or the device deflate (of 65 535 bytes)")
    ap.add_argument("--flip", type=float, default=0.0, help="this share of the generated reads is reverse-complemented, qualities reversed")
    ap.add_argument("--orient", default="none", choices=["none", "profiles", "staged"],
                    help="--stream: orientation by the profiles -- profiles: inside the streamed run, chunk by chunk (plan_orient); staged: a plain engine "
                         "orients the whole file and writes oriented.fq first, the streamed run reads that")
    ap.add_argument("--check", action="store_true", help="--stream: compare the coordinates with one context on the whole file")
    ap.add_argument("--input-dir", default="", help="keep the generated in.fastq.gz here and use it again when it is there (several arms over one file)")
    args = ap.parse_args()
    if args.inflate == "device" and args.stream:
        ap.error("--inflate device is the whole-file loaders' mode: the streamed loaders inflate on the host (not with --stream)")
    if args.parse == "device" and args.stream:
        ap.error("--parse device is the whole-file loaders' mode: the streamed loaders parse on the host (not with --stream)")
    if args.orient != "none" and not args.stream:
        ap.error("--orient is the streamed run's: with --stream")
    if not 0.0 <= args.flip <= 1.0:
        ap.error("--flip is a share of the reads: 0 .. 1")
    import synth
    from bench import its2_profiles
    from itsxpress_amd import Engine, _lib
    from itsxpress_amd.trim import write_trimmed_fastq, read_text, cache_clear
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt") as f:
        thmm = f.read()
    if args.shape == "cfg2":
        blob, offs = synth.make_reads(thmm, args.reads, config=3, seed=synth.SEED + 3, fixed_len=0, len_range=(300, 580))
    else:
        blob, offs = synth.make_reads(thmm, args.reads, config=2, seed=synth.SEED + 2)
    n = args.reads
    rng = np.random.default_rng(9)
    tmp = tempfile.mkdtemp(prefix="itsx_file_run_")
    try:
        plain = os.path.join(tmp, "in.fastq")
        bases = np.frombuffer(blob, np.uint8)
        flipped = np.random.default_rng(11).random(n) < args.flip          # (the same reads whether the file is generated or found)
        comp = np.arange(256, dtype=np.uint8)
        comp[np.frombuffer(b"ACGTacgt", np.uint8)] = np.frombuffer(b"TGCAtgca", np.uint8)

        def read_in(i):
            """read i as the input file holds it"""
            s = bases[offs[i]:offs[i + 1]]
            return comp[s[::-1]] if flipped[i] else s

        tag = ("_flip%g" % args.flip if args.flip > 0 else "") + ("_dev" if args.in_writer == "device" else "")
        kept = os.path.join(args.input_dir, "in_%s_%d%s.fastq.gz" % (args.shape, n, tag)) if args.input_dir else ""
        if kept and os.path.exists(kept) and os.path.exists(kept + ".size"):
            fq = kept
            in_bytes, in_gz = int(open(kept + ".size").read()), os.path.getsize(fq)
        else:
            with open(plain, "wb") as f:                  # Illumina-like qualities: high, decaying along the read
                qtab = [(np.clip(38 - (np.arange(600) // 25) - rng.integers(0, 6, 600), 2, 40) + 33).astype(np.uint8).tobytes() for _ in range(64)]
                for i in range(n):
                    s = bases[offs[i]:offs[i + 1]]
                    q = qtab[i & 63][:len(s)]
                    if flipped[i]:
                        s, q = comp[s[::-1]], q[::-1]
                    f.write(b"@read%d 1:N:0:1\n" % i + s.tobytes() + b"\n+\n" + q + b"\n")
            fq = kept or os.path.join(tmp, "in.fastq.gz")
            if kept:
                os.makedirs(args.input_dir, exist_ok=True)
            if args.in_writer == "device":
                e0 = Engine(0)
                text = open(plain, "rb").read()
                with open(fq, "wb") as f:
                    f.write(e0.deflate_device(text, [0, len(text)])[0])
                del text
                e0.close()
            else:
                write_trimmed_fastq(plain, fq, np.zeros(n, np.int32), np.full(n, 1 << 30, np.int32), gzipped=True)
            in_bytes, in_gz = os.path.getsize(plain), os.path.getsize(fq)
            os.remove(plain)
            if kept:
                open(kept + ".size", "w").write(str(in_bytes))

        eng = Engine(0)
        eng.set_rows_mode(args.rows)
        eng.load_profiles(text=its2_profiles(thmm))
        # first-touch costs (context, code objects, allocator) outside the stages: one small pass of the whole path
        eng.set_reads([bases[offs[i]:offs[i + 1]].tobytes().decode() for i in range(2000)], ["w%d" % i for i in range(2000)])
        eng.derep()
        eng.search()
        eng.finalize()
        t = {}
        extra = {}
        if args.stream:
            # file-order chunks: chunk k is dereplicated and scored while chunk k + 1 is inflated and parsed (itsxpress_amd/stream.py)
            from itsxpress_amd.stream import StreamEngine
            strand = None
            if args.orient == "staged":
                # what a streamed run needed before plan_orient: the whole file oriented on a plain engine, oriented.fq written in full
                # size, and the streamed run inflating, parsing and loading that
                from itsxpress_amd.trim import write_oriented_fastq
                cache_clear()
                t0 = time.perf_counter()
                eng.load_reads_file(fq)
                strand, _, _ = eng.orient_profiles()
                extra["orient_ms"] = round(eng.last_orient_ms, 1)
                oriented = os.path.join(tmp, "oriented.fq")
                write_oriented_fastq(fq, oriented, np.where(strand == 0, 1, strand).astype(np.int8))
                t["orient (plain engine, oriented.fq written)"] = time.perf_counter() - t0
                extra["oriented_fq_MB"] = round(os.path.getsize(oriented) / 1e6, 1)
                fq_run = oriented
            else:
                fq_run = fq
            eng.close()
            cache_clear()
            t0 = time.perf_counter()
            se = StreamEngine(0, chunk_mb=args.chunk_mb or None)
            if args.orient == "profiles":
                se.plan_orient()
            se.set_rows_mode(args.rows)
            out = os.path.join(tmp, "trimmed.fastq" + {"gz": ".gz", "zst": ".zst", "plain": ""}[args.out_kind])
            if args.stream_write:
                se.deflate = args.deflate
                se.plan_output(out, "3_", "4_", gzipped=args.out_kind == "gz", zstd_file=args.out_kind == "zst")
            se.load_reads_file(fq_run)
            se.derep()
            se.load_profiles(text=its2_profiles(thmm))
            se.search()
            t["load+search (streamed)"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            se.finalize()
            t["finalize"] = time.perf_counter() - t0
            nu = se.n_unique
            if args.stream_write and not args.check:    # (the writer has had its rows chunk by chunk: nobody needs the per-read arrays)
                start = stop = None
            else:
                t0 = time.perf_counter()
                start, stop, tlen, ind = se.trim_coords("3_", "4_")
                t["coords"] = time.perf_counter() - t0
            if args.stream_write:
                t0 = time.perf_counter()
                sw = se.finish_output()
                t["write (the part left after the pipeline)"] = time.perf_counter() - t0
                extra_w = {"late_uniques": se._out.n_late_uniques}
                extra["deflate"] = se._out.plan["deflate"]
                extra["ms_deflate"] = round(se._out.ms_deflate, 1)          # (device: the deflate kernel's time over all units)
                extra["units_device"], extra["units_host_sliced"] = se._out.units_device, se._out.units_host      # (which path was timed)
            if args.orient == "profiles":
                strand = se.orient_strands()[0]
                extra["orient_ms"] = round(sum(st.get("orient_ms", 0.0) for _, st in se._engs), 1)      # (the chunks' kernels, summed)
            if strand is not None:
                extra["strands(-1, 0, +1)"] = [int((strand == v).sum()) for v in (-1, 0, 1)]
                extra["strand_is_the_flip"] = round(float(((strand == -1) == flipped)[strand != 0].mean()), 4) if (strand != 0).any() else None
            # every chunk dereplicates (and, oriented, scans) its own distinct texts: the chunks' counts against the file's
            extra["chunk_uniques"] = [int(e.n_unique) for e, _ in se._engs]
            extra = {**extra, "orient": args.orient, "flip": args.flip, "stream_chunks": se.world, "stream_timeline_s(chunk, text ready, loaded, searched)": se.timeline,
                     "chunk_load_s": [st.get("load_s") for _, st in se._engs], "finalize_s": getattr(se, "finalize_s", None)}
            if args.check:                              # the same file through one context: identical coordinates
                e1 = Engine(0)
                e1.set_rows_mode(args.rows)
                e1.load_profiles(text=its2_profiles(thmm))
                e1.load_reads_file(fq_run)
                if args.orient == "profiles":           # (the whole file oriented in one piece: the strands and coordinates the chunks must give)
                    extra["strands_equal_one_context"] = bool(np.array_equal(e1.orient_profiles_apply()[0], strand))
                    assert extra["strands_equal_one_context"]
                e1.derep(); e1.search(); e1.finalize()
                ref = e1.trim_coords("3_", "4_")
                extra["coordinates_equal_one_context"] = bool(all(np.array_equal(a, b) for a, b in zip((start, stop, tlen, ind), ref)))
                assert extra["coordinates_equal_one_context"]
                e1.close()
        else:
            eng.inflate = args.inflate
            eng.parse = args.parse
            loads, ms_parse = [], []
            for _ in range(max(1, args.loads)):
                cache_clear()
                t0 = time.perf_counter()
                eng.load_reads_file(fq)
                t["load"] = time.perf_counter() - t0
                loads.append(round(t["load"], 3))
                ms_parse.append(round(eng.stats()["ms_parse"], 1))
            st = eng.stats()
            extra = {**extra, "parse": args.parse, "load_s": loads, "ms_parse": ms_parse, "parse_texts_device": st["n_parse_device"], "parse_texts_declined": st["n_parse_declined"]}
            extra = {**extra, "inflate": args.inflate, "ms_inflate": round(st["ms_inflate"], 1), "inflate_members": st["n_inflate_members"],
                     "inflate_files_device": st["n_inflate_device"], "inflate_files_declined": st["n_inflate_declined"]}
            t0 = time.perf_counter()
            nu = eng.derep()
            eng.search()
            eng.finalize()
            start, stop, tlen, ind = eng.trim_coords("3_", "4_")
            t["path"] = time.perf_counter() - t0
        out = os.path.join(tmp, "trimmed.fastq" + {"gz": ".gz", "zst": ".zst", "plain": ""}[args.out_kind])
        if args.stream and args.stream_write:
            nw, tot = sw
            extra["representatives_that_waited_for_the_exact_thresholds"] = extra_w["late_uniques"]
            if args.check:                              # the one-go writer on the same coordinates: the same bytes
                ref_out = out + ".ref"
                assert write_trimmed_fastq(fq, ref_out, start, stop, gzipped=args.out_kind == "gz", zstd_file=args.out_kind == "zst",
                                           strand=strand) == (nw, tot)
                if args.deflate == "device":                # (other bytes, the same records)
                    extra["output_text_equal_one_go_writer"] = read_text(ref_out) == read_text(out)
                    assert extra["output_text_equal_one_go_writer"]
                else:
                    extra["output_bytes_equal_one_go_writer"] = open(ref_out, "rb").read() == open(out, "rb").read()
                    assert extra["output_bytes_equal_one_go_writer"]
        else:
            t0 = time.perf_counter()
            nw, tot = write_trimmed_fastq(fq, out, start, stop, gzipped=args.out_kind == "gz", zstd_file=args.out_kind == "zst",
                                          strand=strand if args.stream else None)
            t["write"] = time.perf_counter() - t0
        total = sum(t.values())
        # the output holds exactly the kept reads, sliced: check a sample against the coordinates
        if start is None:
            start, stop, _, _ = se.trim_coords("3_", "4_")          # (after the clock stopped: for the checks below)
        kept = np.flatnonzero((start >= 0) & (stop >= 0) & (start < stop))
        assert nw == len(kept)
        big = os.path.getsize(out) > (1 << 30) or tot > (1 << 30)      # (ctypes.string_at takes a C int: the whole text of a 10 M-read run does not fit)
        lines = [] if big else read_text(out).split(b"\n")
        assert big or len(lines) == 4 * nw + 1
        for k in (() if big else (0, nw // 2, nw - 1)):
            i = int(kept[k])
            assert lines[4 * k] == b"@read%d 1:N:0:1" % i
            s = read_in(i)
            if args.stream and strand is not None and strand[i] < 0:       # (an oriented run slices the read's reverse complement)
                s = comp[s[::-1]]
            assert lines[4 * k + 1] == s.tobytes()[start[i]:stop[i]]
        # the output's text: per written record its title line, "\n", bases, "\n+\n", qualities, "\n" = title + 5 + 2 x (bases kept), summed
        # (the titles are the b"@read%d 1:N:0:1" written above: the fixed part plus the digits of the read's number)
        digits = np.searchsorted(10 ** np.arange(1, 12), kept, side="right") + 1
        text_bytes = int(digits.sum()) + (len(b"@read 1:N:0:1") + 5) * int(nw) + 2 * int(tot)
        print(json.dumps({
            "reads": n, "shape": args.shape, "rows": args.rows, "unique": int(nu), "written": int(nw), "out_kind": args.out_kind,
            "input_MB": round(in_bytes / 1e6, 1), "input_gz_MB": round(in_gz / 1e6, 1), "output_MB": round(os.path.getsize(out) / 1e6, 1),
            "output_text_MB": round(text_bytes / 1e6, 1),
            "stages_s": {k: round(v, 3) for k, v in t.items()}, "s_total": round(total, 3), **extra,
            "reads_per_s_file_to_file": round(n / total), "io_threads": int(os.environ.get("ITSX_IO_THREADS", 0)) or min(os.cpu_count(), 32),
            "codecs": _lib.lib().itsx_io_codecs()}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
