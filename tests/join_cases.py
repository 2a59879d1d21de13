"""Inputs shared by the merge-join tests (tests/test_merge_join_cpu.py, tests/test_gpu_merge_join*.py): the paired fixture with
mates cut to their first 150 bases, so that they no longer overlap.  Cut to 100 the anchors are gone, cut to 120 the 5' anchor
ends past R1; 150 keeps both anchors and removes every overlap."""
import gzip
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R1 = os.path.join(GOLD, "4774-1-MSITS3_R1.fastq.gz")
R2 = os.path.join(GOLD, "4774-1-MSITS3_R2.fastq.gz")
CUT = 150


def read_fastq(path):
    """[(whole title line with its '@', bases, qualities)]"""
    out = []
    with gzip.open(path, "rt") as f:
        while True:
            h = f.readline()
            if not h:
                break
            s = f.readline().rstrip("\n")
            f.readline()
            q = f.readline().rstrip("\n")
            out.append((h.rstrip("\n"), s, q))
    return out


def label(title):
    return title[1:].split()[0]


def fixture_pairs(cut=lambda i: False):
    """[(title1, s1, q1, title2, s2, q2)] of the fixture; pair i (0-based) has both mates cut to CUT bases where cut(i)"""
    out = []
    for i, ((t1, s1, q1), (t2, s2, q2)) in enumerate(zip(read_fastq(R1), read_fastq(R2))):
        if cut(i):
            s1, q1, s2, q2 = s1[:CUT], q1[:CUT], s2[:CUT], q2[:CUT]
        out.append((t1, s1, q1, t2, s2, q2))
    return out


def all_cut():
    return fixture_pairs(lambda i: True)


def odd_cut():
    """the mixed set: the odd-numbered pairs (0-based) cut, the even ones whole"""
    return fixture_pairs(lambda i: i % 2 == 1)


def write_pair_files(pairs, p1, p2, gz=False):
    t1 = "".join("%s\n%s\n+\n%s\n" % (a, b, c) for a, b, c, _, _, _ in pairs)
    t2 = "".join("%s\n%s\n+\n%s\n" % (d, e, f) for _, _, _, d, e, f in pairs)
    for p, t in ((p1, t1), (p2, t2)):
        if gz:
            with gzip.open(p, "wt") as f:
                f.write(t)
        else:
            with open(p, "w") as f:
                f.write(t)
    return p1, p2


# ---------------------------------------------------------------- synthetic pairs for the kernel's verdicts and edges
_COMP = str.maketrans("ACGTN", "TGCAN")
LENS = (1, 2, 3, 63, 64, 65, 250, 251)


def _rc(s):
    return s[::-1].translate(_COMP)


def synthetic_pairs(n=600, seed=8):
    """the recipe of tests/test_gpu_merge.py::test_merge_synthetic_pairs: overlapping mates of random fragments with quality-driven
    noise, every 17th a tandem repeat, every 11th staggered.  [(f, fq, r, rq)]"""
    import numpy as np
    rng = np.random.default_rng(seed)
    acgt = np.array(list("ACGT"))
    out = []
    for i in range(n):
        L = int(rng.integers(120, 520))
        frag = "".join(acgt[rng.integers(0, 4, L)])
        if i % 17 == 0:
            frag = ("ACGGTCATTG" * 60)[:L]
        fl, rl = int(rng.integers(80, 300)), int(rng.integers(80, 300))
        f = frag[:fl]
        r = _rc(frag[max(0, L - rl):])
        if i % 11 == 0:
            f = frag[L // 3:][:fl]

        def noisy(s, rate):
            s = list(s)
            q = []
            for k in range(len(s)):
                qq = int(rng.choice([2, 8, 14, 20, 30, 38, 40], p=[.02, .05, .08, .1, .15, .5, .1]))
                if rng.random() < 10 ** (-qq / 10.0) * rate:
                    s[k] = str(acgt[rng.integers(0, 4)])
                if rng.random() < 0.004:
                    s[k] = "N"
                    qq = 0
                q.append(chr(33 + qq))
            return "".join(s), "".join(q)
        f, q1 = noisy(f, 1.0)
        r, q2 = noisy(r, 1.5)
        out.append((f, q1, r, q2))
    return out


def _bases(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def _quals(rng, n, lo=33, hi=127):
    return "".join(chr(k) for k in rng.integers(lo, hi, n))


def unrelated_pairs(seed=81):
    """unrelated random mates, every combination of the lengths in LENS: whole waves, one lane more, one lane less"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return [(_bases(rng, fl), _quals(rng, fl), _bases(rng, rl), _quals(rng, rl)) for fl in LENS for rl in LENS]


def verdict_pairs(seed=82):
    """one pair built for each verdict the recipe above may miss: 4 (more than 40 mismatches on a diagonal that still scores: the
    mismatches sit where one mate has quality '#'), 5 (a clean overlap of 9 bases), 7 (a merged read whose tail is quality '+') and
    8 (an empty mate, on either side)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    frag = _bases(rng, 300)                                              # 4: overlap 250, 45 of its bases changed under a '#'
    f, fq = frag[:275], ["I"] * 275
    r_fwd, rq_fwd = list(frag[25:]), ["I"] * 275
    for k in range(45):
        p = 5 * k + 7
        r_fwd[p] = "ACGT"[("ACGT".index(r_fwd[p]) + 1) % 4]
        rq_fwd[p] = "#"
    out.append((f, "".join(fq), _rc("".join(r_fwd)), "".join(rq_fwd)[::-1]))
    frag = _bases(rng, 191)                                              # 5: mates of 100 bases that share 9
    out.append((frag[:100], "I" * 100, _rc(frag[91:]), "I" * 100))
    frag = _bases(rng, 260)                                              # 7: 60 bases of quality '+' ahead of a clean overlap
    out.append((frag[:200], "+" * 60 + "I" * 140, _rc(frag[100:]), "I" * 160))
    out.append(("", "", _bases(rng, 40), "I" * 40))                      # 8
    out.append((_bases(rng, 40), "I" * 40, "", ""))
    return out


def edge_pairs(seed=83):
    """unrelated mates whose R2 holds r, U, n and lower case at both ends, and qualities '!' and '~' at both ends of both mates"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for fl, rl in ((150, 150), (64, 65), (7, 9)):
        f, r = _bases(rng, fl), _bases(rng, rl)
        r = "rUn" + r[3:rl - 4].lower()[:2] + r[5:rl - 4] + "acnU" if rl > 12 else "rUa" + r[3:rl - 3] + "gnU"
        assert len(r) == rl
        fq = "!~" + _quals(rng, fl - 4) + "~!"
        rq = "~!" + _quals(rng, rl - 4) + "!~"
        out.append((f, fq, r, rq))
        out.append((f.lower() if fl < 100 else f[:3].lower() + f[3:], fq, r, rq))      # R1 in lower case too: read in upper case
    return out


def long_pair(total, seed):
    """two unrelated mates of `total` bases in all (the first one base longer when total is odd)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    fl = (total + 1) // 2
    rl = total - fl
    return (_bases(rng, fl), _quals(rng, fl, 35, 75), _bases(rng, rl), _quals(rng, rl, 35, 75))


def tiny_pairs(n, seed=84):
    """n pairs of 1-3 bases a mate"""
    import numpy as np
    rng = np.random.default_rng(seed)
    fl, rl = rng.integers(1, 4, n), rng.integers(1, 4, n)
    fb, rb = _bases(rng, int(fl.sum())), _bases(rng, int(rl.sum()))
    fqb, rqb = _quals(rng, int(fl.sum())), _quals(rng, int(rl.sum()))
    fo = [0] + [int(x) for x in fl.cumsum()]
    ro = [0] + [int(x) for x in rl.cumsum()]
    return [(fb[fo[i]:fo[i + 1]], fqb[fo[i]:fo[i + 1]], rb[ro[i]:ro[i + 1]], rqb[ro[i]:ro[i + 1]]) for i in range(n)]
