"""Orientation by the profiles (itsx_orient_profiles), the rule in plain Python.  TEST INFRASTRUCTURE ONLY.

For a text t: n_fwd(t) = the profiles whose MSV filter passes on t at F1, n_rev(t) = n_fwd(revcomp(t)); strand +1 if n_fwd > n_rev,
-1 if n_rev > n_fwd, 0 otherwise.  Reads take their strand from their text: the read set is dereplicated (strand both, per sample,
empty reads dropped), a read that is the reverse complement of its seed gets the seed's strand negated and its counts swapped, a
dropped read 0 / 0 / 0.  Applying reverse-complements the reads of strand -1 (qualities reversed) and keeps every other read as it is.

The pass counts come from outside: from the oracle's pair traces (`oracle_counts`: tests/orc.py, used as it is, on the texts and on
reverse complements built from Python strings) or from any other list of pair traces (`trace_counts`).  Nothing here is a tolerance.
"""
import numpy as np

_RC = str.maketrans("ACGTURYMKSWHBVDNacgturymkswhbvdn", "TGCAAYRKMSWDVBHNtgcaayrkmswdvbhn")
_CANON = str.maketrans("acgturymkswhbvdnU", "ACGTTRYMKSWHBVDNT")
IUPAC = "NRYKMBDHVSW"


def revcomp(s):
    """positions mirrored, every symbol complemented (IUPAC, case kept, U reads as T)"""
    return s[::-1].translate(_RC)


def canon(s):
    """what the engine packs: case folded, U as T"""
    return s.translate(_CANON)


def derep(texts, samples=None):
    """strand-both dereplication of full texts, inside each sample, empty reads dropped: (rep_of, strand) per read -- rep_of = the
    index of the cluster's first read (-1 dropped), strand = -1 where the read is that read's reverse complement"""
    n = len(texts)
    rep_of, strand = np.full(n, -1, np.int64), np.zeros(n, np.int8)
    seen = {}
    for r, t in enumerate(texts):
        if not t:
            continue
        smp = 0 if samples is None else int(samples[r])
        c = canon(t)
        if (smp, c) in seen:
            rep_of[r], strand[r] = seen[(smp, c)], 1
        elif (smp, revcomp(c)) in seen:
            rep_of[r], strand[r] = seen[(smp, revcomp(c))], -1
        else:
            seen[(smp, c)] = r
            rep_of[r], strand[r] = r, 1
    return rep_of, strand


def trace_counts(trace, n):
    """profiles that passed the MSV filter per sequence, from pair traces (the oracle's or the engine's: fields seq, pass_msv)"""
    tr = trace[trace["pass_msv"] != 0]
    seq = tr["seq" if "seq" in trace.dtype.names else "rep"]          # (the engine's traces name the representative)
    return np.bincount(seq.astype(np.int64), minlength=n).astype(np.int32)[:n] if n else np.zeros(0, np.int32)


def oracle_counts(hs, texts, F1=1e-6, threads=4):
    """(n_fwd, n_rev) of every text from the oracle's pair traces.  Empty texts get 0 / 0; equal texts are searched once.
    F2 = F3 = 1e-300 let nothing past the filters that follow: pass_msv does not depend on them, and the domain stage is not needed."""
    import orc

    def search(distinct):
        codes, offs = orc.digitize(distinct)
        res = orc.SearchResult(hs, codes, offs, F1=F1, F2=1e-300, F3=1e-300, keep_trace=1, threads=threads)
        return trace_counts(res.trace, len(distinct))
    return counts_by(texts, search)


def counts_by(texts, count_fn):
    """(n_fwd, n_rev) of every text, count_fn(list of distinct non-empty texts) -> passes per text being asked once, for the texts
    and their reverse complements as explicit strings"""
    distinct = sorted({canon(t) for t in texts if t} | {revcomp(canon(t)) for t in texts if t})
    cnt = dict(zip(distinct, count_fn(distinct))) if distinct else {}
    nf = np.array([cnt[canon(t)] if t else 0 for t in texts], np.int32)
    nr = np.array([cnt[revcomp(canon(t))] if t else 0 for t in texts], np.int32)
    return nf, nr


def verdict(nf, nr):
    return int(nf > nr) - int(nr > nf)


def model(nf, nr, rep_of, rstrand, texts=None, quals=None):
    """nf / nr: pass counts of every read's OWN text on its forward / reverse strand -- only the entries of the seeds (rep_of[r] == r)
    are read.  Returns dict(strand, count_fwd, count_rev[, texts][, quals]): per read, and the reads as the apply step leaves them."""
    n = len(rep_of)
    strand, cf, cr = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for r in range(n):
        s = int(rep_of[r])
        if s < 0:
            continue
        f, v = (int(nr[s]), int(nf[s])) if rstrand[r] < 0 else (int(nf[s]), int(nr[s]))
        strand[r], cf[r], cr[r] = verdict(f, v), f, v
    out = dict(strand=strand, count_fwd=cf, count_rev=cr)
    if texts is not None:
        out["texts"] = [revcomp(t) if strand[r] < 0 else t for r, t in enumerate(texts)]
    if quals is not None:
        out["quals"] = [q[::-1] if strand[r] < 0 else q for r, q in enumerate(quals)]
    return out


# ---------------------------------------------------------------------------------------------- the inputs of the issue's table
def synthetic_reads(mini_hmm_text, n=2000, seed=7):
    import synth
    blob, offs = synth.make_reads(mini_hmm_text, n, seed=seed)
    return synth.to_strings(blob, offs)


def random_reads(count=50, L=300, seed=101):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list("ACGT"), L)) for _ in range(count)]


def tie_reads(amplicons, count=20):
    """s + revcomp(s): the same text on both strands"""
    return [s + revcomp(s) for s in amplicons[:count]]


# ---------------------------------------------------------------------------------------------- the GPU catalogue against mini.hmm
def catalogue(mini_hmm_text):
    """(reads, samples, kinds): the catalogue of tests/test_gpu_orient_profiles.py.  kinds[r] is "decided" (a flipped or forward
    amplicon: the model's strand must be non-zero), "zero" (a tie, a random or a short read, the empty read: must be 0) or "free"."""
    synth_reads = synthetic_reads(mini_hmm_text)
    clean = [s for s in dict.fromkeys(synth_reads) if set(s) <= set("ACGT")]
    amp = clean[0]                                   # (whichever strand the generator gave it: the test asserts it is decided)
    reads, kinds = [], []

    def add(s, kind):
        reads.append(s); kinds.append(kind)

    for s in synth_reads:
        add(s, "free")
    import synth
    long_amp = next(s for s in synth.to_strings(*synth.make_reads(mini_hmm_text, 50, seed=9, fixed_len=320, rc_rate=0.0)) if set(s) <= set("ACGT"))
    for L in range(300, 316):                        # the word-tail offsets 0..15 of k_oa_words: the right flank (60 bases) cut back
        add(long_amp[:L], "decided"); add(revcomp(long_amp[:L]), "decided")
    flipped = revcomp(amp)
    Lf = len(flipped)
    # the generator puts the right anchor at 195..239 of a 300-base template: 215 of a forward read, 84 of a flipped one
    anchor_pos = (84, 215)
    for sym in IUPAC:
        for p in (0, Lf - 1, 15, 16, 17, Lf - 16, Lf - 17, Lf - 18) + anchor_pos:
            t = list(flipped); t[p] = sym
            add("".join(t), "decided")
    # amplicons no other read of the catalogue holds, so that each of these is scanned itself
    extra = [s for s in dict.fromkeys(synth.to_strings(*synth.make_reads(mini_hmm_text, 60, seed=11, rc_rate=0.0)))
             if set(s) <= set("ACGT") and s not in set(synth_reads)]
    e0, e1, e2, e3 = extra[2:6]
    add(revcomp(e0).lower(), "decided"); add(e1[:100] + e1[100:200].lower() + e1[200:], "decided")
    add(revcomp(e2).replace("T", "U"), "decided"); add(e3.replace("T", "u"), "decided")
    for s in tie_reads(clean[2:22]):
        add(s, "zero")
    for s in random_reads():
        add(s, "zero")
    pair =[extra[0], revcomp(extra[0]), revcomp(extra[1]), extra[1]]      # a text and its reverse complement, either one first
    for s in pair:
        add(s, "decided")
    add("", "zero")
    rng = np.random.default_rng(5)
    long_read = "".join(rng.choice(list("ACGT"), 9000)) + flipped + "".join(rng.choice(list("ACGT"), 20000 - 9000 - Lf))
    add(long_read, "decided")
    for L in (1, 15, 16, 17, 33):
        add(amp[:L], "zero")                         # (a flank's random bases on either strand: at least 60 before the first anchor)
    samples = [0] * len(reads)
    for s in pair:                                   # the same pair in a second sample
        add(s, "decided"); samples.append(1)
    return reads, np.array(samples, np.int32), kinds
