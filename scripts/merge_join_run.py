#!/usr/bin/env python3
"""What joining the pairs that do not overlap costs (Engine.merge_join, itsx_set_merge_join), on one GPU.

N synthetic ITS2 amplicons are sequenced as 2x250 with Illumina-like qualities and errors; half of the templates are 300-480 bases
long (their mates overlap and merge), half 520-700 (no overlap: dropped with the setting off, joined with it on).  One warm context
per arm, the arms alternated within every pass, the first pass the warm-up (it allocates) and --passes timed ones after it:

  off      this build, merge_join off (the kernel instantiated without the join: the parent commit's code)
  on       this build, merge_join on
  parent   --parent-lib: the parent commit's libitsx_hip.so, which knows no such setting

Every arm goes through the C ABI directly (one small binding for all of them: the parent's library lacks the new symbols), calls
itsx_merge_pairs_load on the same two plain FASTQ files and then dereplicates and searches the read set it got.  Reported per arm and
pass: ms_merge (the merge kernel's event time), the merge-and-load call's wall time with its pack step, the reads it left, and the
search's wall time on them.  Prints one JSON line.

usage: merge_join_run.py [--pairs 1000000] [--passes 3] [--parent-lib build/parent/libitsx_hip.so]"""
import argparse
import ctypes as C
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


def note(t0, what):
    print("[merge_join_run] %6.1f s  %s" % (time.perf_counter() - t0, what), file=sys.stderr, flush=True)


def make_files(n, tmp, t0):
    """R1.fastq / R2.fastq of n pairs (records of one fixed width, so the text is one array) and the ITS2 profiles' file"""
    import synth
    from bench import its2_profiles
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt") as f:
        thmm = f.read()
    rng = np.random.default_rng(23)
    nt = max(2, n // 50)
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGTN", b"TGCAN"):
        comp[a] = b
    tmat = np.full((nt, 700), ord("A"), np.uint8)
    tlen = np.zeros(nt, np.int64)
    for half, (k0, k1, rng_len) in enumerate(((0, nt // 2, (300, 480)), (nt // 2, nt, (520, 700)))):
        tb, to = synth.make_reads(thmm, k1 - k0, config=3, seed=synth.SEED + 11 + half, fixed_len=0, len_range=rng_len, frac_templates=1.0,
                                  sub_rate=0.0, n_rate=0.0, rc_rate=0.0)
        tb = np.frombuffer(tb, np.uint8)
        for t in range(k1 - k0):
            tmat[k0 + t, :to[t + 1] - to[t]] = tb[to[t]:to[t + 1]]
        tlen[k0:k1] = np.diff(to)
    # every second pair from the long half: the two halves alternate through the file
    ids = np.where(np.arange(n) % 2 == 0, rng.integers(0, nt // 2, n), rng.integers(nt // 2, nt, n))
    L = tlen[ids]
    fwd = tmat[ids, :250]
    rev = comp[tmat[ids[:, None], L[:, None] - 1 - np.arange(250)[None, :]]]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    qv = np.array([2, 12, 22, 30, 37, 38], np.uint8)
    qp = [.001, .009, .03, .08, .28, .6]
    paths = []
    for tag, reads in (("1", fwd), ("2", rev)):
        q = rng.choice(qv, size=reads.shape, p=qp)
        err = rng.random(reads.shape) < 10.0 ** (-q.astype(np.float64) / 10.0)
        reads = reads.copy()
        reads[err] = acgt[rng.integers(0, 4, int(err.sum()))]
        titles = np.frombuffer(b"".join(b"@P%08d %s\n" % (i, tag.encode()) for i in range(n)), np.uint8).reshape(n, 13)
        rec = np.empty((n, 13 + 250 + 3 + 250 + 1), np.uint8)
        rec[:, :13] = titles
        rec[:, 13:263] = reads
        rec[:, 263:266] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 266:516] = q + 33
        rec[:, 516] = 10
        p = os.path.join(tmp, "R%s.fastq" % tag)
        rec.tofile(p)
        paths.append(p)
        note(t0, "R%s written" % tag)
    hmm = os.path.join(tmp, "its2.hmm")
    with open(hmm, "w") as f:
        f.write(its2_profiles(thmm))
    return paths, hmm, int((L > 490).sum())


class Ctx:
    """one context of one build of the engine, through the few entry points this run needs"""

    def __init__(self, lib_path, hmm):
        from itsxpress_amd import _lib
        self.dtype = _lib.STATS_DTYPE_ALL
        L = self.L = C.CDLL(lib_path)
        vp, i32, i64, f64, cp = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_char_p
        for name, res, args in (("itsx_create", vp, [i32, i32]), ("itsx_destroy", None, [vp]), ("itsx_last_error", cp, [vp]),
                                ("itsx_load_profiles_file", i32, [vp, cp, vp]), ("itsx_merge_pairs_load", i32, [vp, cp, cp, i32, f64, i32, vp, vp]),
                                ("itsx_derep", i32, [vp, i32, i32, vp]), ("itsx_search", i32, [vp, f64, f64, f64, f64]),
                                ("itsx_search_finalize", i32, [vp, f64]), ("itsx_get_stats", i32, [vp, vp, i64]), ("itsx_io_cache_clear", None, [])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        self.has_join = hasattr(L, "itsx_set_merge_join")
        if self.has_join:
            L.itsx_set_merge_join.restype, L.itsx_set_merge_join.argtypes = i32, [vp, i32]
            L.itsx_merge_join_info.restype, L.itsx_merge_join_info.argtypes = i32, [vp, vp, i64, vp]
        self.h = L.itsx_create(0, 0)
        if not self.h:
            raise RuntimeError(L.itsx_last_error(None).decode())
        npf = C.c_int32(0)
        self.chk(L.itsx_load_profiles_file(self.h, os.fsencode(hmm), C.byref(npf)))

    def chk(self, rc):
        if rc != 0:
            raise RuntimeError("itsx_hip error %d: %s" % (rc, self.L.itsx_last_error(self.h).decode()))

    def stats(self):
        s = np.zeros(1, self.dtype)
        self.chk(self.L.itsx_get_stats(self.h, s.ctypes.data, s.itemsize))
        return s[0]

    def one_pass(self, paths, join):
        L = self.L
        if self.has_join:
            self.chk(L.itsx_set_merge_join(self.h, int(join)))
        L.itsx_io_cache_clear()                               # every arm reads and parses the two files itself
        n, m, u = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        t0 = time.perf_counter()
        self.chk(L.itsx_merge_pairs_load(self.h, os.fsencode(paths[0]), os.fsencode(paths[1]), 40, 2.0, 0, C.byref(n), C.byref(m)))
        t1 = time.perf_counter()
        st = self.stats()
        out = {"ms_merge_kernel": round(float(st["ms_merge"]), 3), "s_merge_and_load": round(t1 - t0, 3), "ms_pack": round(float(st["ms_pack"]), 1),
               "pairs": int(n.value), "merged": int(m.value), "reads": int(st["n_reads"])}
        if self.has_join:
            j = C.c_int64(0)
            self.chk(L.itsx_merge_join_info(self.h, None, n.value, C.byref(j)))
            out["joined"] = int(j.value)
        t2 = time.perf_counter()
        self.chk(L.itsx_derep(self.h, 1, 1, C.byref(u)))
        t3 = time.perf_counter()
        self.chk(L.itsx_search(self.h, 10.0, 1e-6, 1e-6, 1e-6))
        self.chk(L.itsx_search_finalize(self.h, 10.0))
        t4 = time.perf_counter()
        out.update({"uniques": int(u.value), "s_derep": round(t3 - t2, 3), "s_search": round(t4 - t3, 3)})
        return out

    def close(self):
        self.L.itsx_destroy(self.h)


def summary(runs, key):
    v = sorted(r[key] for r in runs)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": round(v[-1] - v[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=3, help="timed passes after the warm-up pass")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libitsx_hip.so: its merge is the third arm")
    args = ap.parse_args()
    from itsxpress_amd import _lib
    t0 = time.perf_counter()
    tmp = tempfile.mkdtemp(prefix="itsx_merge_join_run_")
    try:
        paths, hmm, n_long = make_files(args.pairs, tmp, t0)
        arms = [("off", _lib.LIB_PATH, False), ("on", _lib.LIB_PATH, True)]
        if args.parent_lib:
            arms.insert(0, ("parent", os.path.abspath(args.parent_lib), False))
        ctxs = {name: Ctx(path, hmm) for name, path, _ in arms}
        assert not args.parent_lib or not ctxs["parent"].has_join, "--parent-lib names a library that has the setting"
        runs = {name: [] for name, _, _ in arms}
        for p in range(args.passes + 1):
            for name, _, join in arms:
                r = ctxs[name].one_pass(paths, join)
                if p > 0:
                    runs[name].append(r)
                note(t0, "pass %d %s: %s" % (p, name, json.dumps(r)))
        for c in ctxs.values():
            c.close()
        keys = ("ms_merge_kernel", "s_merge_and_load", "s_search", "s_derep")
        res = {"pairs": args.pairs, "pairs_without_overlap": n_long, "passes": args.passes,
               "arms": {name: {"runs": runs[name], **{k: summary(runs[name], k) for k in keys}} for name in runs}}
        off, on = runs["off"][0], runs["on"][0]
        assert off["merged"] == on["merged"] and on["reads"] == on["merged"] + on["joined"] and off["reads"] == off["merged"]
        if args.parent_lib:
            assert runs["parent"][0]["merged"] == off["merged"] and runs["parent"][0]["reads"] == off["reads"]
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
