"""The denoising rule of itsx_denoise_table (include/itsx_hip.h) as a model: sequential, no levels, no pruning, a plain Levenshtein DP.
It shares no code with the package.  The DP runs one query against all the centroids at once, row by row with numpy."""
import numpy as np


def levenshtein_many(query, targets):
    """the Levenshtein distance (unit costs, global, symbols compared literally) of `query` to every string of `targets`"""
    if not targets:
        return []
    q = np.frombuffer(query.encode(), np.uint8)
    lens = np.array([len(t) for t in targets])
    width = int(lens.max())
    tt = np.zeros((len(targets), width), np.uint8)              # (0 matches no symbol; the cells past a target's end are never read)
    for k, t in enumerate(targets):
        tt[k, :len(t)] = np.frombuffer(t.encode(), np.uint8)
    # the plain recurrence D[i][j] = min(D[i-1][j] + 1, D[i-1][j-1] + (q[i] != t[j]), D[i][j-1] + 1), one row at a time, kept as
    # R[j] = D[i][j] - j: the third term becomes R[j-1], so a running minimum along the row serves it
    dt = np.int16 if len(q) + width < 30000 else np.int64
    row = np.zeros((len(targets), width + 1), dt)                # D[0][j] = j
    new = np.empty_like(row)
    for i in range(1, len(q) + 1):
        new[:, 0] = i
        np.add(row[:, :-1], (tt != q[i - 1]).view(np.int8) - 1, out=new[:, 1:], casting="unsafe")
        np.minimum(new[:, 1:], row[:, 1:] + 1, out=new[:, 1:])
        np.minimum.accumulate(new, axis=1, out=row)
    return [int(row[k, lens[k]]) + int(lens[k]) for k in range(len(targets))]


def levenshtein(a, b):
    return levenshtein_many(a, [b])[0]


def denoise(sequences, totals, counts, max_skew, minsize):
    """sequences / totals / counts (rows of per-sample counts) of a feature table in table order -> the denoised table"""
    D = len(max_skew)
    centroids, zotu_of, dist_of, dropped = [], [], [], 0
    for q, (s, a) in enumerate(zip(sequences, totals)):
        best = None
        for z, d in enumerate(levenshtein_many(s, [sequences[t] for t in centroids])):
            if 1 <= d <= D and float(a) <= float(max_skew[d - 1]) * float(totals[centroids[z]]) and (best is None or d < best[0]):
                best = (d, z)                                     # (centroids ascend: the first of a tie stays)
        if best is not None:
            zotu_of.append(best[1])
            dist_of.append(best[0])
        elif a >= minsize:
            zotu_of.append(len(centroids))
            dist_of.append(0)
            centroids.append(q)
        else:
            zotu_of.append(-1)
            dist_of.append(-1)
            dropped += int(a)
    n_samples = len(counts[0]) if len(counts) else 1
    rows = [[0] * n_samples for _ in centroids]
    for f, z in enumerate(zotu_of):
        if z >= 0:
            rows[z] = [x + int(y) for x, y in zip(rows[z], counts[f])]
    return {"zotu_feature": centroids, "zotu_total": [sum(r) for r in rows], "counts": rows, "zotu_of_feature": zotu_of,
            "dist_of_feature": dist_of, "n_dropped_reads": dropped}
