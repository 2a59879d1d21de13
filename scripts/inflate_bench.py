#!/usr/bin/env python3
"""Reader timing: a gzip FASTQ of N synthetic 300-bp reads through itsx_io_read, serially (libdeflate / zlib) and with the
block-parallel inflater (pinflate.cpp), with and without huge pages.  usage: inflate_bench.py [reads]
--device [reads]: the device inflate (csrc/k_inflate.hip) against the host's on the same files -- N synthetic 300-bp reads written by the
host writer (members of 4 MiB of text) and by the device deflate (members of 65 535 bytes): the load's wall time with Engine.inflate =
"host" and "device", alternated, three timed runs each after one warm-up, and for the device the kernels' time (ms_inflate), GB/s of
text for the kernels alone and for the whole call with upload and fetch.  Prints one JSON line per file."""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time
sys.path.insert(0, %r)
from itsxpress_amd.trim import read_text
for i in range(3):
    t0 = time.perf_counter(); t = read_text(sys.argv[1]); print("%%.3f s  %%d bytes" %% (time.perf_counter() - t0, len(t)), flush=True)
''' % ROOT


def device_arm(n):
    import json
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    from itsxpress_amd import Engine
    from itsxpress_amd.trim import cache_clear, write_trimmed_fastq
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    tmpl = acgt[rng.integers(0, 4, (max(1, n // 50), 300))]
    H = 21                                                                    # "@read%09d 1:N:0\n", then bases "\n+\n" qualities "\n"
    rec = np.empty((n, H + 300 + 3 + 300 + 1), np.uint8)
    rec[:, :H] = np.frombuffer(b"".join(b"@read%09d 1:N:0\n" % i for i in range(n)), np.uint8).reshape(n, H)
    rec[:, H:H + 300] = tmpl[rng.integers(0, len(tmpl), n)]
    err = rng.random((n, 300)) < 0.003
    rec[:, H:H + 300][err] = acgt[rng.integers(0, 4, int(err.sum()))]
    rec[:, H + 300:H + 303] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, H + 303:H + 603] = (np.clip(38 - (np.arange(300) // 25)[None, :] - rng.integers(0, 6, (n, 300)), 2, 40) + 33).astype(np.uint8)
    rec[:, H + 603] = 10
    text = rec.tobytes()
    del rec
    tmp = tempfile.mkdtemp(prefix="itsx_inflate_")
    plain = os.path.join(tmp, "in.fastq")
    with open(plain, "wb") as f:
        f.write(text)
    eng = Engine(0)
    files = {}
    files["host writer (4 MiB members)"] = os.path.join(tmp, "host.fastq.gz")
    write_trimmed_fastq(plain, files["host writer (4 MiB members)"], np.zeros(n, np.int32), np.full(n, 1 << 30, np.int32), gzipped=True)
    files["device writer (65 535-byte members)"] = os.path.join(tmp, "device.fastq.gz")
    with open(files["device writer (65 535-byte members)"], "wb") as f:
        f.write(eng.deflate_device(text, [0, len(text)])[0])
    os.remove(plain)
    for name, path in files.items():
        gz = open(path, "rb").read()
        walls = {"host": [], "device": []}
        raw, ms, counts = [], [], None
        for run in range(4):                                                  # run 0: the warm-up
            for where in ("host", "device"):
                eng.inflate = where
                cache_clear()
                t0 = time.perf_counter()
                got = eng.load_reads_file(path)
                w = time.perf_counter() - t0
                assert got == n
                if run:
                    walls[where].append(round(w, 3))
            t0 = time.perf_counter()
            out = eng.inflate_device(gz)
            w = time.perf_counter() - t0
            assert len(out) == len(text) and (run or out == text)
            st = eng.stats()
            if run:
                raw.append(round(w, 3))
                ms.append(round(st["ms_inflate"], 1))
            counts = (st["n_inflate_members"], st["n_inflate_device"], st["n_inflate_declined"])
        k = sorted(ms)[1]
        print(json.dumps({"file": name, "reads": n, "text_MB": round(len(text) / 1e6, 1), "gz_MB": round(len(gz) / 1e6, 1), "members": counts[0],
                          "load_wall_s_host": walls["host"], "load_wall_s_device": walls["device"], "ms_inflate": ms,
                          "kernels_GBps_of_text": round(len(text) / k / 1e6, 2), "inflate_device_call_s(upload, kernels, fetch)": raw,
                          "call_GBps_of_text": round(len(text) / sorted(raw)[1] / 1e9, 2), "files_device": counts[1], "files_declined": counts[2]}), flush=True)
    eng.close()
    for p in files.values():
        os.remove(p)


def main():
    import numpy as np
    if len(sys.argv) > 1 and sys.argv[1] == "--device":
        return device_arm(int(sys.argv[2]) if len(sys.argv) > 2 else 10000000)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    tmpl = acgt[rng.integers(0, 4, (max(1, n // 50), 300))]
    reads = tmpl[rng.integers(0, len(tmpl), n)].copy()
    err = rng.random(reads.shape) < 0.003
    reads[err] = acgt[rng.integers(0, 4, int(err.sum()))]
    q = (np.clip(38 - (np.arange(300) // 25)[None, :] - rng.integers(0, 6, reads.shape), 2, 40) + 33).astype(np.uint8)
    tmp = tempfile.mkdtemp(prefix="itsx_inflate_")
    path = os.path.join(tmp, "in.fastq.gz")
    with gzip.open(path, "wb", compresslevel=6) as f:
        for i in range(n):
            f.write(b"@read%d 1:N:0:1\n" % i + reads[i].tobytes() + b"\n+\n" + q[i].tobytes() + b"\n")
    print("compressed MB", round(os.path.getsize(path) / 1e6, 1), flush=True)
    for name, env in (("serial", {"ITSX_PARALLEL_INFLATE": "0"}), ("parallel, 4-KB pages", {"ITSX_HUGEPAGES": "0"}), ("parallel, huge pages", {})):
        e = dict(os.environ, ITSX_TEXT_CACHE_GB="0", ITSX_TRACE_ALLOC="1", **env)
        out = subprocess.run([sys.executable, "-c", CHILD, path], env=e, capture_output=True, text=True)
        print("==", name)
        print(out.stdout.strip())
        print("\n".join(l for l in out.stderr.split("\n") if "parallel inflate" in l))
    os.remove(path)


if __name__ == "__main__":
    main()
