"""Denoising the feature table without a GPU: the model of the rule on a hand-written case, the level claim of the device's schedule
checked on the model, the skew table, the C ABI's declarations, and the denoised table's two files byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from denoise_model import denoise, levenshtein, levenshtein_many

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_denoise_table", "itsx_denoise_table_get", "itsx_denoise_table_features", "itsx_denoise_table_info", "itsx_trimmed_table_size"]


def test_levenshtein():
    assert levenshtein("KITTEN", "SITTING") == 3 and levenshtein("A", "A") == 0 and levenshtein("ACGT", "ANGT") == 1
    assert levenshtein_many("ACGT", ["ACGT", "A", "ACGTT", "TGCA", "CGT"]) == [0, 3, 1, 4, 1]
    assert levenshtein_many("ACGT", []) == []


def test_model_on_a_hand_written_case():
    A = "ACGTACGTACGTACGTACGT"
    B = "TTGGCCAATTGGCCAATTGG"
    seqs = [A,                                   # 0: a centroid
            B,                                   # 1: a centroid, far from A
            A[:9] + "G" + A[10:],                # 2: one edit from 0, but 17 * 8 > 128: a centroid
            A[:5] + "T" + A[6:],                 # 3: one edit from 0 and 16 * 8 == 128: taken at the edge
            B[:-1] + "A",                        # 4: one edit from 1, but 16 * 8 > 127 = 128 - 1: a centroid
            B[:-1] + "C",                        # 5: under minsize, one edit from 1 (taken) and from 4 (3 * 8 > 16)
            "GGGGGGGGGGGGGGGGGGGG",              # 6: under minsize, far from all: unassigned
            A[:9] + "T" + A[10:],                # 7: one edit from 0 and from 2, both take it: the tie goes to the earlier centroid
            A[:5] + "T" + A[6:12] + "T" + A[13:]]      # 8: one edit from 3, which was taken and is no centroid: two edits from 0
    totals = [128, 127, 17, 16, 16, 3, 3, 2, 2]
    counts = [[t - t // 2, t // 2] for t in totals]
    assert levenshtein(seqs[8], seqs[3]) == 1 and levenshtein(seqs[8], seqs[0]) == 2 and levenshtein(seqs[8], seqs[2]) == 3
    assert levenshtein(seqs[7], seqs[0]) == 1 and levenshtein(seqs[7], seqs[2]) == 1
    m = denoise(seqs, totals, counts, [2.0 ** -3, 2.0 ** -5], minsize=8)
    assert m["zotu_feature"] == [0, 1, 2, 4]
    assert m["zotu_of_feature"] == [0, 1, 2, 0, 3, 1, -1, 0, 0]
    assert m["dist_of_feature"] == [0, 0, 0, 1, 0, 1, -1, 1, 2]
    assert m["n_dropped_reads"] == 3 and m["zotu_total"] == [128 + 16 + 2 + 2, 127 + 3, 17, 16]
    assert m["counts"] == [[74, 74], [66, 64], [9, 8], [8, 8]]
    m2 = denoise(seqs, totals, counts, [2.0 ** -3, 2.0 ** -7], minsize=8)     # the second skew at 1 / 128: 2 > 1, 8 is not taken at d = 2
    assert m2["zotu_of_feature"] == [0, 1, 2, 0, 3, 1, -1, 0, -1] and m2["n_dropped_reads"] == 5
    none = denoise(seqs, totals, counts, [], minsize=3)          # D = 0: nothing is taken
    assert none["zotu_feature"] == [0, 1, 2, 3, 4, 5, 6] and none["n_dropped_reads"] == 4 and none["dist_of_feature"] == [0] * 7 + [-1, -1]


def _by_levels(seqs, totals, counts, max_skew, minsize):
    """the device's schedule on the model's distance: a level's features are decided against the centroids of the earlier levels only"""
    F, D = len(seqs), len(max_skew)
    cent, zotu_of, dist_of = [], [None] * F, [None] * F
    f0 = 0
    while f0 < F:
        f1 = f0 + 1
        while D > 0 and f1 < F and float(totals[f1]) > max_skew[0] * float(totals[f0]):
            f1 += 1
        if D == 0:
            f1 = F
        new = []
        for q in range(f0, f1):
            best = None
            for z, d in enumerate(levenshtein_many(seqs[q], [seqs[t] for t in cent])):
                if 1 <= d <= D and float(totals[q]) <= max_skew[d - 1] * float(totals[cent[z]]) and (best is None or (d, z) < best):
                    best = (d, z)
            if best:
                zotu_of[q], dist_of[q] = best[1], best[0]
            elif totals[q] >= minsize:
                zotu_of[q], dist_of[q] = len(cent) + len(new), 0
                new.append(q)
            else:
                zotu_of[q], dist_of[q] = -1, -1
        cent += new
        f0 = f1
    return cent, zotu_of, dist_of


def test_levels_give_the_sequential_result():
    rng = np.random.default_rng(21)
    for it in range(200):
        templates = ["".join(rng.choice(list("ACGT"), int(rng.integers(4, 9)))) for _ in range(3)]
        seqs = set()
        for _ in range(int(rng.integers(2, 25))):
            s = list(templates[int(rng.integers(0, 3))])
            for _e in range(int(rng.integers(0, 4))):
                op, p = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
                if op == 0:
                    s[p] = "ACGT"[int(rng.integers(0, 4))]
                elif op == 1:
                    s.insert(p, "ACGT"[int(rng.integers(0, 4))])
                elif len(s) > 1:
                    del s[p]
            seqs.add("".join(s))
        seqs = sorted(seqs)
        totals = sorted((int(x) for x in np.minimum(rng.geometric(0.02, len(seqs)), rng.geometric(0.3, len(seqs)) * 3)), reverse=True)
        counts = [[t] for t in totals]
        skews = [[0.5, 0.25, 0.125], [0.125, 0.03125], [0.9, 0.9, 0.5], [0.3], []][it % 5]
        minsize = (1, 2, 8)[it % 3]
        m = denoise(seqs, totals, counts, skews, minsize)
        cent, zotu_of, dist_of = _by_levels(seqs, totals, counts, skews, minsize)
        assert (cent, zotu_of, dist_of) == (m["zotu_feature"], m["zotu_of_feature"], m["dist_of_feature"]), it


def test_unoise_skews():
    from itsxpress_amd.engine import unoise_skews
    s = unoise_skews(2.0, None, None)
    assert s.dtype == np.float64 and s.tolist() == [2.0 ** -(2.0 * d + 1) for d in range(1, 32)]
    assert unoise_skews(2.0, None, 3).tolist() == [0.125, 0.03125, 0.0078125]
    assert unoise_skews(2.0, 128, None).tolist() == [2.0 ** -3, 2.0 ** -5, 2.0 ** -7]      # 128 / 128 == 1 still accepts one read
    assert unoise_skews(2.0, 127, None).tolist() == [2.0 ** -3, 2.0 ** -5]
    assert unoise_skews(2.0, 128, 2).tolist() == [2.0 ** -3, 2.0 ** -5]
    assert unoise_skews(2.0, 7, None).tolist() == [] and unoise_skews(2.0, 1000, 0).tolist() == []
    assert unoise_skews(0.5, None, 2).tolist() == [2.0 ** -1.5, 0.25]
    assert (np.diff(unoise_skews(3.5)) < 0).all() and len(unoise_skews(3.5)) == 31
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            unoise_skews(bad, 100, None)


def test_header_exports_and_makefile_name_the_calls():
    from itsxpress_amd import _lib
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS, name
    assert "#define ITSX_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header)
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "Makefile")) as f:
        assert "k_denoise.o" in f.read()


def test_denoised_files_byte_for_byte(tmp_path):
    """write_denoised_table's files from given arrays, through the host formatter, with no device: three ZOTUs over three samples whose
    centroids are features 0, 2 and 5 of some table; size= is the ZOTU's total"""
    from itsxpress_amd.batch import write_denoised_files
    fa, tsv = str(tmp_path / "z.fa"), str(tmp_path / "z.tsv")
    write_denoised_files(fa, tsv, 3, np.array([9, 4, 2]), np.array([0, 2, 5]), np.array([0, 2, 3, 5]), np.array([0, 2, 1, 0, 1]),
                         np.array([6, 3, 4, 1, 1]), ["GATTACA", "NRY", "T"], ["aa", "bb", "cc"], ["x.fq", "y.fq", "z.fq"])
    assert open(fa, "rb").read() == b">aa;size=9\nGATTACA\n>bb;size=4\nNRY\n>cc;size=2\nT\n"
    assert open(tsv, "rb").read() == b"#feature\tx.fq\ty.fq\tz.fq\naa\t6\t0\t3\nbb\t0\t4\t0\ncc\t1\t1\t0\n"
    write_denoised_files(None, tsv, 1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32),
                         np.zeros(0, np.int32), [], [], ["only"])
    assert open(tsv, "rb").read() == b"#feature\tonly\n"
    with pytest.raises(ValueError):
        write_denoised_files(fa, tsv, 2, np.array([1]), np.array([0]), np.array([0, 1]), np.array([0]), np.array([1]), ["A"], ["a"], ["one"])


def test_banded_distance_against_a_full_matrix(tmp_path):
    """csrc/k_dn_band.h is plain C++: the kernel's column step, cut-off and windowed match table against a full DP matrix on the host"""
    exe = str(tmp_path / "dn_band_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "itsxpress_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "csrc", "dn_band_check.cpp")], check=True)
    out = subprocess.run([exe, "60000"], check=True, capture_output=True, text=True).stdout
    assert re.fullmatch(r"ok \d{7,}\n", out), out
