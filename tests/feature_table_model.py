"""The text model of the feature table of the trimmed regions (itsx_trimmed_table): plain strings and collections.Counter.

Read i is counted iff start[i] >= 0, stop[i] >= 0, start[i] < stop[i] and min(stop[i], len) - start[i] >= min_len; its sequence is
seq.upper().replace("U", "T")[start:min(stop, len)]; features are the distinct sequences, ordered by descending total count, ties by
the smaller index of the feature's first read."""
from collections import Counter


def feature_table(seqs, start, stop, samples=None, n_samples=1, min_len=1):
    """-> dict(sequences, totals, first_read, counts = [F][n_samples] lists, feature_of_read = per read, -1 not counted)"""
    cells, first, key_of = Counter(), {}, []
    for i, seq in enumerate(seqs):
        a, b = int(start[i]), int(stop[i])
        key = None
        if a >= 0 and b >= 0 and a < b and min(b, len(seq)) - a >= min_len:
            key = seq.upper().replace("U", "T")[a:min(b, len(seq))]
            cells[(key, 0 if samples is None else int(samples[i]))] += 1
            first.setdefault(key, i)
        key_of.append(key)
    totals = Counter()
    for (key, _), c in cells.items():
        totals[key] += c
    order = sorted(first, key=lambda k: (-totals[k], first[k]))
    rank = {k: f for f, k in enumerate(order)}
    return dict(sequences=order, totals=[totals[k] for k in order], first_read=[first[k] for k in order],
                counts=[[cells.get((k, s), 0) for s in range(n_samples)] for k in order],
                feature_of_read=[-1 if k is None else rank[k] for k in key_of])
