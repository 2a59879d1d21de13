#!/usr/bin/env python3
"""What orientation by the profiles costs, on configs[1]-shaped input (1 M synthetic reads of 300 bases, the stand-in taxon's ITS2
profiles: bench.py --workload cfg1).  One warm context, one warm-up pass and three timed passes per arm:

  profiles  Engine.orient_profiles_apply(): its ms_kernels (device time of both scans and the step's own kernels) and its wall time,
            then derep + search in the same context: stats()["ms_msv"], the cost of the search's one (shared) forward scan;
  kmer      Engine.orient_apply() with the universal database on the same reads: wall time.

Prints one JSON line; --out also writes it to a file.  Needs a GPU.

    python3 scripts/orient_profiles_run.py --out orient_profiles.json
"""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return dict(min=round(xs[0], 3), median=round(xs[len(xs) // 2], 3), max=round(xs[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    from bench import its2_profiles
    from itsxpress_amd import Engine
    gold = os.path.join(ROOT, "tests", "golden")
    with gzip.open(os.path.join(gold, "T.hmm.gz"), "rt") as f:
        thmm = f.read()
    blob, offs = synth.make_reads(thmm, args.reads, config=2, seed=synth.SEED + 2, as_array=True)
    eng = Engine(0)
    eng.set_rows_mode("lazy")
    nprof = eng.load_profiles(text=its2_profiles(thmm))
    eng.orient_load_db(os.path.join(gold, "universal_orient_ref_clean.fasta.gz"))
    ms_kernels, wall_profiles, ms_msv, wall_kmer, n_flipped, n_undecided, n_kept = [], [], [], [], 0, 0, 0
    for k in range(args.passes + 1):                         # pass 0 warms both arms up
        eng.set_reads_buffer(blob, offs)
        t0 = time.perf_counter()
        strand, _, _ = eng.orient_profiles_apply()           # (returns after the device has finished: the strands are on the host)
        t1 = time.perf_counter()
        nu = eng.derep()
        eng.search()
        st = eng.stats()
        eng.set_reads_buffer(blob, offs)
        t2 = time.perf_counter()
        _, _, _, kept = eng.orient_apply()
        t3 = time.perf_counter()
        if k:
            ms_kernels.append(eng.last_orient_ms); wall_profiles.append(1e3 * (t1 - t0)); ms_msv.append(st["ms_msv"]); wall_kmer.append(1e3 * (t3 - t2))
        n_flipped, n_undecided, n_kept = int((strand < 0).sum()), int((strand == 0).sum()), int(kept.sum())
    res = dict(metric="orientation by the profiles, configs[1] shape", reads=args.reads, profiles=nprof, n_unique=int(nu), passes=args.passes,
               ms_kernels_orient_profiles_apply=spread(ms_kernels), wall_ms_orient_profiles_apply=spread(wall_profiles),
               ms_msv_following_search=spread(ms_msv), wall_ms_kmer_orient_apply=spread(wall_kmer),
               ratio_kernels_to_one_shared_scan=round(spread(ms_kernels)["median"] / max(spread(ms_msv)["median"], 1e-9), 2),
               n_flipped=n_flipped, n_undecided=n_undecided, n_kept_by_kmer=n_kept)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
