"""One catalogue of the search's edge shapes, shared by the float64 tests (tests/test_generic_cpu.py, tests/test_gpu_generic.py) and
the GPU tests that build the same profiles and reads.  Every case is named and seeded and gives (profile text, reads)."""
import numpy as np

import synth


def _stretch(block, M_new):
    """a profile of M_new nodes made from a 45-node HMMER3/f block: the last node is repeated (the repeats take an inner
    node's transitions, the final node keeps the terminal ones)"""
    lines = block.split("\n")
    i_leng = next(k for k, ln in enumerate(lines) if ln.startswith("LENG"))
    M = int(lines[i_leng].split()[1])
    lines[i_leng] = "LENG  %d" % M_new
    i_hmm = next(k for k, ln in enumerate(lines) if ln.startswith("HMM "))
    first = i_hmm + 5                         # HMM, header, COMPO, node-0 inserts, node-0 transitions
    node = lambda k: lines[first + 3 * (k - 1): first + 3 * k]
    inner_t = node(M - 1)[2]
    out = lines[:first + 3 * (M - 1)]
    last = node(M)
    for k in range(M, M_new + 1):
        m = last[0].split()
        m[0] = str(k)
        out += ["  " + "  ".join(m), last[1], inner_t if k < M_new else last[2]]
    out += lines[first + 3 * M:]
    return "\n".join(out).replace("NAME  ", "NAME  ", 1)


def _without_match_to_delete(hmm_text, node, value="*"):
    """the profiles of `hmm_text` with t(M_node -> D_node+1) = 0 ('*'; or exp(-value)) -- the delete path past that node lives on D -> D alone"""
    out, k = [], None
    for ln in hmm_text.split("\n"):
        f = ln.split()
        if ln.startswith("HMM "):
            k = 0
        elif k is not None and len(f) >= 5 and f[0].isdigit():
            k = int(f[0])
        elif k == node and len(f) == 7 and f[6] != "*" and not ln.lstrip().startswith("1.38629  1.38629"):
            f[2] = value
            ln = "          " + "  ".join("%7s" % x for x in f)
            k = None
        if ln.startswith("//"):
            k = None
        out.append(ln)
    return "\n".join(out)


def _ccs_reads(t_hmm_text, rng, lengths, per_family=6):
    """CCS-shaped targets (--trim-ccs inputs, itsxpress/SeqSample.py:48-91): kilobases of random sequence with full and PARTIAL copies of
    a left and a right motif in tandem, a few error variants of each"""
    acgt = np.frombuffer(b"ACGT", np.uint8)
    lm = [m for m in synth.consensus_motifs(t_hmm_text, "3_") if len(m) == 45]
    rm = [m for m in synth.consensus_motifs(t_hmm_text, "4_") if len(m) == 45]
    seqs = []
    for L in lengths:
        base = acgt[rng.integers(0, 4, L)].copy()
        a = int(rng.integers(50, 400))
        while a + 400 < L:
            l, r = lm[int(rng.integers(0, len(lm)))], rm[int(rng.integers(0, len(rm)))]
            cut = int(rng.integers(0, 25))                                 # a partial copy now and then
            base[a:a + 45 - cut] = np.frombuffer(l.encode(), np.uint8)[cut:]
            b = a + 45 + int(rng.integers(100, 260))
            base[b:b + 45] = np.frombuffer(r.encode(), np.uint8)
            a = b + 45 + int(rng.integers(200, 3000))
        for j in range(per_family):
            v = base.copy()
            for pos in rng.integers(0, L, 1 + j):
                v[pos] = acgt[(np.searchsorted(acgt, v[pos]) + 1 + rng.integers(0, 3)) % 4]
            if j == per_family - 1:
                v[int(rng.integers(0, L))] = ord("N")
            seqs.append(bytes(v).decode())
    return seqs


def _blocks(hmm_text):
    return [b + "//\n" for b in hmm_text.split("//\n") if "NAME  " in b]


def _name(block):
    return block.split("NAME  ")[1].split("\n")[0].strip()


def _its2(hmm_text, n3, n4):
    bl = _blocks(hmm_text)
    return "".join([b for b in bl if _name(b).startswith("3_")][:n3] + [b for b in bl if _name(b).startswith("4_")][:n4])


def _rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def _sprinkle(rng, s, rate, sym="N"):
    s = np.frombuffer(s.encode(), np.uint8).copy()
    s[rng.random(len(s)) < rate] = ord(sym)
    return bytes(s).decode()


# each builder: (t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs, scale) -> (profile text, reads, edge)
# scale < 1 draws fewer reads in the large (sampled) cases; edge = every pair is checked (no sampling)

def bench_its2(t, mini, allt, fx, scale):
    blob, offs = synth.make_reads(t, max(8, int(48 * scale)), config=2, seed=synth.SEED + 41, fixed_len=0, len_range=(300, 580),
                                  n_rate=0.01, frac_templates=1.0)
    return _its2(t, 12, 12), synth.to_strings(blob, offs), False


def all_taxa(t, mini, allt, fx, scale):
    bl = _blocks(allt)
    Ms = [int(b.split("LENG")[1].split()[0]) for b in bl]
    pick = set(range(0, len(bl), 41)) | {int(np.argmin(Ms)), int(np.argmax(Ms))}
    return "".join(bl[i] for i in sorted(pick)), list(fx[:max(6, int(24 * scale))]), False


def node_limits(t, mini, allt, fx, scale):
    rng = np.random.default_rng(46)
    bl = _blocks(mini)
    b45 = next(b for b in bl if "LENG  45" in b)
    small = [b for b in bl if "LENG  11" in b or "LENG  25" in b]
    hmm = _stretch(b45, 46) + "".join(small)
    cons = [c for c in synth.consensus_motifs(hmm, "") if c]
    seqs = []
    for n in (33, 44, 45, 46, 47, 60):
        seqs.append(_rnd(rng, n))
        c = cons[n % len(cons)]
        s = (c * (n // len(c) + 1))[:n] if len(c) < n else c[:n]
        seqs.append(s)
    seqs += [_rnd(rng, 80) + cons[0] + _rnd(rng, 120), _rnd(rng, 60) + cons[-1] + _rnd(rng, 40) + cons[-2] + _rnd(rng, 60)]
    return hmm, seqs, True


def zero_transitions(t, mini, allt, fx, scale):
    sub = _its2(t, 4, 4)
    hmm = _without_match_to_delete(sub, 17) + _without_match_to_delete(sub, 17, "30.00000")
    blob, offs = synth.make_reads(t, 16, config=3, seed=synth.SEED + 47, fixed_len=0, len_range=(200, 560), n_rate=0.003,
                                  frac_templates=1.0)
    return hmm, synth.to_strings(blob, offs), True


def degenerate(t, mini, allt, fx, scale):
    rng = np.random.default_rng(48)
    cons3, cons4 = synth.consensus_motifs(mini, "3_"), synth.consensus_motifs(mini, "4_")
    soup = "ACGTURYKMSWBDHVN"
    m = list(cons3[0])
    m[10:16] = "NNNNNN"
    seqs = [_rnd(rng, 90) + cons3[1] + _rnd(rng, 40, soup) + cons4[1] + _rnd(rng, 50),
            _rnd(rng, 300, soup),
            _sprinkle(rng, _rnd(rng, 120) + cons3[0] + _rnd(rng, 150) + cons4[0] + _rnd(rng, 60), 0.02),
            _rnd(rng, 70) + "".join(m) + _rnd(rng, 100) + cons4[2] + _rnd(rng, 30),
            "N" * 120, soup * 8 + cons3[2] + soup * 4]
    return mini, seqs, True


def rescaling(t, mini, allt, fx, scale):
    rng = np.random.default_rng(49)
    cons3, cons4 = synth.consensus_motifs(mini, "3_"), synth.consensus_motifs(mini, "4_")
    seqs = [cons3[0] * 7, cons4[1] * 7, (cons3[0] + _rnd(rng, 30) + cons4[0]) * 3,
            cons4[0][:20] + cons3[0] + cons4[0][20:], _rc(cons3[0]) + _rnd(rng, 80) + _rc(cons4[0])]
    return mini, seqs, True


def long(t, mini, allt, fx, scale):
    rng = np.random.default_rng(50)
    sub = _its2(t, 2, 2)
    lm = [m for m in synth.consensus_motifs(sub, "3_")]
    rm = [m for m in synth.consensus_motifs(sub, "4_")]
    seqs = _ccs_reads(t, rng, [2000, 7000, 20000], per_family=1)
    seqs.append(_rnd(rng, 65535 - 310 - len(lm[0]) - len(rm[0])) + lm[0] + _rnd(rng, 310) + rm[0])      # the engine's longest read
    return sub, seqs, True


def multidomain(t, mini, allt, fx, scale):
    rng = np.random.default_rng(51)
    cons3, cons4 = synth.consensus_motifs(mini, "3_"), synth.consensus_motifs(mini, "4_")
    seqs = []
    for j in range(8):
        k = 2 + j % 2
        parts = [_rnd(rng, int(rng.integers(20, 80)))]
        for _ in range(k):
            parts += [cons3[int(rng.integers(0, len(cons3)))], _rnd(rng, int(rng.integers(3, 40))), cons4[int(rng.integers(0, len(cons4)))],
                      _rnd(rng, int(rng.integers(3, 60)))]
        seqs.append(_sprinkle(rng, "".join(parts), 0.01, "A"))
    # the copies above lie far enough apart for a region each; TANDEM PARTIAL copies (concatemer-like, as the adversarial reads of
    # tests/test_gpu_caps.py) do form multidomain regions, which the traceback ensemble resolves
    for j in range(6):
        c = (cons3 if j % 2 == 0 else cons4)[int(rng.integers(0, 3))]
        parts = [_rnd(rng, int(rng.integers(0, 40)))]
        for _ in range(int(rng.integers(3, 7))):
            a = int(rng.integers(0, len(c) // 2))
            parts.append(c[a:int(rng.integers(a + len(c) // 3, len(c) + 1))])
        seqs.append("".join(parts) + _rnd(rng, int(rng.integers(0, 40))))
    return mini, seqs, True


def domz(t, mini, allt, fx, scale):
    """domZ decides: 8 reads carry a full copy of one motif and a weak partial copy (a domain whose P-value is near 1), 40 reads
    carry nothing.  With domZ = the 8 reported sequences the weak domains are reported (P * 8 <= 10); counted over all 48 reads
    they would not be."""
    rng = np.random.default_rng(52)
    bl = _blocks(mini)
    hmm = bl[0]
    c = synth.consensus_motifs(hmm, "")[0]
    seqs = []
    for j in range(8):
        part = list(c[int(rng.integers(0, 8)):][:14 + j])
        for p in rng.choice(len(part), 3, replace=False):
            part[p] = "ACGT"[int(rng.integers(0, 4))]
        seqs.append(_rnd(rng, 60) + c + _rnd(rng, 90) + "".join(part) + _rnd(rng, 70))
    seqs += [_rnd(rng, int(rng.integers(200, 400))) for _ in range(40)]
    return hmm, seqs, True


CASES = dict(bench_its2=bench_its2, all_taxa=all_taxa, node_limits=node_limits, zero_transitions=zero_transitions,
             degenerate=degenerate, rescaling=rescaling, long=long, multidomain=multidomain, domz=domz)


def case(name, t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs, scale=1.0):
    """(profile text, reads, edge) of the named case"""
    return CASES[name](t_hmm_text, mini_hmm_text, all_its2_hmm_text, fixture_seqs, scale)
