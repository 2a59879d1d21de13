"""Score classes of a sample batch as plain text (the model behind itsx_set_sample_sharing), shared by
tests/test_sample_sharing_cpu.py and tests/test_gpu_sample_sharing.py.

The QIIME 2 plugin runs one vsearch and one hmmsearch per manifest row (itsxpress/q2_itsxpress.py:273-333).  Per sample,
`vsearch --fastx_uniques --strand both` keeps the FIRST occurrence of a sequence as its representative, in that occurrence's own
orientation (tests/derep_exact.py states this and is reused here).  hmmsearch scores a target from its residues alone, so two
representatives get the same rows exactly when they are the same text in the same orientation: a CLASS is the set of uniques, over
all samples, with equal representative text; its HOLDER is the member with the smallest unique index.  A representative and its
reverse complement are different targets and lie in different classes.  Text is compared as the engine reads it (derep_exact.norm:
upper case, U == T); N, or any other IUPAC code, is a residue of its own.

The consequence the engine is held to: with the holder's results copied to every member, each member has the domain rows, the
dom_reported flags under its OWN sample's domZ, the coordinates and the domtbl.txt lines of a run that scored every unique --
`expected_from_unshared` states it on arrays.  The model shares nothing with csrc/k_derep.hip: no packing, no hash.
"""
import numpy as np

import derep_exact


def representatives(seqs, sample, strand_both=True, minlen=1):
    """-> (texts, usample): the normalised text of every unique's representative in unique order (= input order of the seeds), and
    the sample of each"""
    _, _, _, _, seed_read, _ = derep_exact.derep(seqs, strand_both, minlen, sample)
    texts = [derep_exact.norm(seqs[int(r)]) for r in seed_read]
    usample = np.array([0 if sample is None else int(sample[int(r)]) for r in seed_read], np.int64)
    return texts, usample


def classes(texts):
    """-> (class_of int64[U], holder int64[C], offsets int64[C + 1], members int64[U]): classes numbered by their holders in rising
    unique index, the members of each in rising unique index"""
    first = {}
    class_of = np.zeros(len(texts), np.int64)
    holder = []
    for u, t in enumerate(texts):
        if t not in first:
            first[t] = len(holder)
            holder.append(u)
        class_of[u] = first[t]
    members = np.argsort(class_of, kind="stable").astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(class_of, minlength=len(holder)))]).astype(np.int64)
    return class_of, np.array(holder, np.int64), offsets, members


def batch_classes(seqs, sample, strand_both=True, minlen=1):
    texts, usample = representatives(seqs, sample, strand_both, minlen)
    return classes(texts) + (usample,)


def same_partition(a, b):
    """two labelings of the same uniques name the same classes (none merged, none split)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape != b.shape:
        return False
    fa, fb = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fa.setdefault(x, y) != y or fb.setdefault(y, x) != x:
            return False
    return True


def expected_from_unshared(dom, domz, class_of, holder, usample, n_profiles):
    """What sharing must reproduce, stated from an UNSHARED run's row table `dom` (structured array with rep, prof, dom_idx,
    seq_reported, ...) and counters domz[S][P]:
      * the rows of member m are the rows of its class's holder with rep = m (every field but rep and dom_reported equal);
      * domz[s][p] = the members m of sample s whose holder has a row (prof p, dom_idx 0, seq_reported 1).
    Returns the list of violations (empty: the unshared run itself has the property the mode relies on)."""
    bad = []
    by_rep = {}
    for i, r in enumerate(dom["rep"].tolist()):
        by_rep.setdefault(r, []).append(i)
    fields = [f for f in dom.dtype.names if f not in ("rep", "dom_reported")]
    cnt = np.zeros_like(np.asarray(domz).reshape(-1, n_profiles))
    for m in range(len(class_of)):
        h = int(holder[int(class_of[m])])
        rows_h = dom[by_rep.get(h, [])]
        rows_m = dom[by_rep.get(m, [])]
        key = lambda a: np.lexsort((a["dom_idx"], a["prof"]))
        rows_h, rows_m = rows_h[key(rows_h)], rows_m[key(rows_m)]
        if len(rows_h) != len(rows_m) or any(rows_h[f].tobytes() != rows_m[f].tobytes() for f in fields):
            bad.append(("rows", m, h))
        first = rows_h[(rows_h["dom_idx"] == 0) & (rows_h["seq_reported"] == 1)]
        np.add.at(cnt[int(usample[m])], first["prof"], 1)
    if not np.array_equal(cnt, np.asarray(domz).reshape(-1, n_profiles)):
        bad.append(("domz",))
    return bad
