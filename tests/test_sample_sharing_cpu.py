"""Sample sharing (itsx_set_sample_sharing) without a GPU: the interface in every layer, the switch, and the plain-text model of the
score classes (tests/sample_classes_exact.py) on hand-written samples with known answers.  The engine is held to the model in
tests/test_gpu_sample_sharing.py."""
import os
import re

import numpy as np
import pytest

import derep_exact
import sample_classes_exact as sce
from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("itsx_set_sample_sharing", "itsx_sample_sharing_info", "itsx_sample_sharing_times", "itsx_debug_sample_classes")


def test_abi_names_the_new_symbols():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6          # additive: no new version
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert re.search(r"int itsx_set_sample_sharing\(itsx_ctx \*ctx, int on\);", header)
    assert re.search(r"int itsx_sample_sharing_info\(const itsx_ctx \*ctx, int64_t \*n_classes, int64_t \*n_uniques_shared, int64_t \*n_rows_expanded\);", header)
    assert re.search(r"int itsx_debug_sample_classes\(itsx_ctx \*ctx, int32_t \*class_of, int64_t n\);", header)
    # every entry's comment names the loop of the reference it stands for
    for name in NEW:
        at = header.index("int %s(" % name)
        comment = header[header.rindex("/*", 0, at):at]
        assert "q2_itsxpress.py:273-333" in comment, name


def test_the_switch_is_a_mode_and_the_setting_is_a_property():
    import ctypes as C
    L = _lib.lib()
    n = L.itsx_switch_registry(None, 0)
    b = C.create_string_buffer(int(n))
    L.itsx_switch_registry(b, n)
    reg = {line.split("\t")[0]: line.split("\t")[1] for line in b.value.decode().strip().split("\n")}
    assert reg["ITSX_SHARE_SAMPLES"] == "mode"                       # it changes no result: not a hook
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\| `ITSX_SHARE_SAMPLES` \| mode \|", doc)
    from itsxpress_amd.engine import Engine
    from itsxpress_amd.batch import SampleBatch
    e = Engine.__new__(Engine)                  # no context: the setting is remembered by the Python layer
    assert e.share_samples is False
    e.share_samples = True
    assert e.share_samples is True
    for bad in ("device", 1, 0, None, "on"):
        with pytest.raises(ValueError):
            e.share_samples = bad
    assert e.share_samples is True
    e.share_samples = False
    assert isinstance(SampleBatch.share_samples, property) and isinstance(Engine.share_samples, property)
    bt = SampleBatch.__new__(SampleBatch)
    bt.engine = e
    assert bt.share_samples is False
    bt.share_samples = True
    assert e.share_samples is True and bt.share_samples is True
    with pytest.raises(ValueError):
        bt.share_samples = "yes"
    e.share_samples = False

    class _S:
        seq_file, tempdir = "x.fq", "."
    b2 = SampleBatch([_S()], engine=e)
    assert b2.share_samples is False and e.share_samples is False    # off by default: making a batch leaves the engine's setting alone
    b2.share_samples = True
    assert b2.share_samples is True and e.share_samples is True
    with pytest.raises(ValueError):
        b2.share_samples = "device"
    e.share_samples = False


# ------------------------------------------------------------------ the model, on samples written by hand
A = "ACGTTGCAAGGCTTACCGGATTTACGCAGTCAA"          # 33 bases, not its own reverse complement
B = "GGGTTTCCCAAATTTGGGCCCAAAGGGTTTACGTACGTAA"
C_ = "TTGACCAGTAGGCATCAGGACTAGCATCGACTAGCTAC"


def _batch(samples):
    seqs = [s for x in samples for s in x]
    smp = np.concatenate([np.full(len(x), i, np.int32) for i, x in enumerate(samples)]) if seqs else np.zeros(0, np.int32)
    return seqs, smp


def test_classes_of_hand_written_samples():
    rcA = derep_exact.rc(A)
    assert rcA != A
    samples = [[A, B, A],                 # uniques 0 (A), 1 (B)
               [B, rcA, C_],              # 2 (B), 3 (rc A: this sample's only copy of A is the reverse complement), 4 (C)
               [],                        # an empty sample
               [rcA, A, C_.lower()],      # 5 (rc A; A joins it as a minus-strand member), 6 (C, lower case)
               [A]]                       # 7 (A)
    seqs, smp = _batch(samples)
    class_of, holder, off, members, usample = sce.batch_classes(seqs, smp)
    assert usample.tolist() == [0, 0, 1, 1, 1, 3, 3, 4]
    # classes in order of their holders: A {0, 7}, B {1, 2}, rc A {3, 5}, C {4, 6}
    assert class_of.tolist() == [0, 1, 1, 2, 3, 2, 3, 0]
    assert holder.tolist() == [0, 1, 3, 4]
    assert off.tolist() == [0, 2, 4, 6, 8] and members.tolist() == [0, 7, 1, 2, 3, 5, 4, 6]
    # the forward copy and the reverse complement never share a class, whichever sample holds which
    assert class_of[0] != class_of[3] and class_of[5] == class_of[3] and class_of[7] == class_of[0]
    # a holder is the smallest member, and members rise inside a class
    for c in range(len(holder)):
        m = members[off[c]:off[c + 1]]
        assert m[0] == holder[c] and np.all(np.diff(m) > 0) and np.all(class_of[m] == c)
    # one sample never holds two members of a class: its own dereplication merged them
    for c in range(len(holder)):
        s = usample[members[off[c]:off[c + 1]]]
        assert len(set(s.tolist())) == len(s)


def test_classes_tell_apart_what_the_packing_could_confuse():
    t = A + B                                            # 73 bases
    cases = [t, t[:-1] + ("C" if t[-1] != "C" else "G"), t + "A", "A" + t,
             t[:15] + "N" + t[16:], t[:15] + "A" + t[16:], t[:16] + "N" + t[17:], t[:16] + "A" + t[17:],
             t[:15] + "R" + t[16:], t.replace("T", "U"), t.lower()]
    samples = [[x] for x in cases]
    seqs, smp = _batch(samples)
    class_of, holder, off, members, usample = sce.batch_classes(seqs, smp)
    texts = [derep_exact.norm(x) for x in cases]
    want = [texts.index(x) for x in texts]               # equal normalised text, nothing else
    assert sce.same_partition(class_of, want)
    assert class_of[9] == class_of[0] and class_of[10] == class_of[0]           # U == T, case is not a difference
    assert len({int(class_of[i]) for i in (0, 1, 2, 3, 4, 6, 8)}) == 7          # last base, trailing / leading A, N and R at a position
    assert not sce.same_partition([0, 0, 1], [0, 1, 1]) and sce.same_partition([3, 3, 9], [0, 0, 1])


def test_members_inherit_exactly_what_an_unshared_run_gives():
    """expected_from_unshared on a hand-made row table: equal rows for the members of a class and per-sample counters pass; a
    member whose rows differ from its holder's, or a counter that misses a member, is reported"""
    dt = np.dtype([("rep", "<i8"), ("prof", "<i4"), ("dom_idx", "<i4"), ("seq_reported", "<i4"), ("dom_reported", "<i4"), ("bitscore", "<f4")])
    class_of, holder, usample = np.array([0, 1, 0]), np.array([0, 1]), np.array([0, 0, 1])
    rows = np.array([(0, 0, 0, 1, 1, 30.5), (0, 1, 0, 0, 0, 3.0), (1, 0, 0, 1, 1, 12.0), (2, 0, 0, 1, 0, 30.5), (2, 1, 0, 0, 0, 3.0)], dt)
    domz = np.array([[2, 0], [1, 0]])
    assert sce.expected_from_unshared(rows, domz, class_of, holder, usample, 2) == []          # dom_reported may differ inside a class
    worse = rows.copy()
    worse["bitscore"][3] = 30.4
    assert ("rows", 2, 0) in sce.expected_from_unshared(worse, domz, class_of, holder, usample, 2)
    assert ("domz",) in sce.expected_from_unshared(rows, np.array([[2, 0], [0, 0]]), class_of, holder, usample, 2)
