#!/usr/bin/env python3
"""Records pass A's row counters (bound_rows, bound_rows_full, bwd_rows of Engine.stats()) of the build it runs on, for the fixed
inputs of tests/list_passes_inputs.py, into tests/golden/list_passes_stats.json (or the path given): the counters where they are a
function of the input (the unshared schedule; list_passes_inputs.STATS_RECORDED says why the others are not), the representatives and
the pairs past the filter in every schedule; every schedule's counters of this run go to stderr.  Run it on the build whose counters
are the reference -- the commit before the wave list stopped reading the pairs -- on a GPU:

    python3 scripts/make_list_passes_stats.py [out.json]

tests/test_gpu_list_passes.py holds every later build to these values."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.setdefault("ITSX_TEST_HOOKS", "1")

import list_passes_inputs as LP  # noqa: E402
from itsxpress_amd import Engine  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "list_passes_stats.json")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T.hmm.gz"), "rt") as f:
        t = f.read()
    eng = Engine(0)
    res = {}
    for name in LP.STATS_INPUTS:
        hmm, seqs = LP.stats_input(t, name)
        for sched in LP.STATS_SCHEDULES:
            LP.lazy_search(eng, hmm, seqs, LP.SCHEDULES[sched], os.environ.__setitem__, lambda k: os.environ.pop(k, None))
            st = eng.stats()
            res["%s/%s" % (name, sched)] = {k: int(st[k]) for k in LP.STATS_RECORDED[sched]}
            print("%s/%s" % (name, sched), {k: int(st[k]) for k in LP.STATS_KEYS}, file=sys.stderr)
    eng.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
