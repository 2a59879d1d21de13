"""The feature table of the trimmed regions without a GPU: the text model on a hand-written case, the C ABI's declarations, and the
host formatter of the two files (itsx_write_feature_files) byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feature_table_model import feature_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_trimmed_table", "itsx_trimmed_table_get", "itsx_trimmed_table_reads", "itsx_trimmed_table_seqs", "itsx_write_feature_files"]


def test_model_on_six_reads():
    #        0 counted GATTA   1 the same, other flanks, lower case, U   2 N is not A   3 not written   4 a prefix: another feature
    seqs = ["ccGATTAcc", "tgauuaG", "ccGNTTAcc", "GATTA", "GATTAC", "ttGATTA"]
    start = [2, 1, 2, -1, 0, 2]
    stop = [7, 6, 7, 5, 4, 99]                                  # 5: stop past the end is clamped
    samples = [0, 1, 1, 0, 1, 1]
    t = feature_table(seqs, start, stop, samples, n_samples=2)
    assert t["sequences"] == ["GATTA", "GNTTA", "GATT"]
    assert t["totals"] == [3, 1, 1]
    assert t["first_read"] == [0, 2, 4]                         # the tie of GNTTA and GATT goes to the earlier first read
    assert t["counts"] == [[1, 2], [0, 1], [0, 1]]
    assert t["feature_of_read"] == [0, 0, 1, -1, 2, 0]
    t5 = feature_table(seqs, start, stop, samples, n_samples=2, min_len=5)
    assert t5["sequences"] == ["GATTA", "GNTTA"] and t5["feature_of_read"] == [0, 0, 1, -1, -1, 0]
    one = feature_table(seqs, start, stop)
    assert one["counts"] == [[3], [1], [1]]


def test_header_and_exports_name_the_calls():
    from itsxpress_amd import _lib
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS, name
    assert "#define ITSX_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header)
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "Makefile")) as f:
        assert "k_ftable.o" in f.read()


def _blob(names):
    enc = [x.encode() for x in names]
    return b"".join(enc), np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int64)


@pytest.fixture(scope="module")
def writer():
    from itsxpress_amd import _lib
    try:
        L = C.CDLL(_lib.LIB_PATH)                               # the host formatter needs no device
    except OSError as e:
        pytest.fail("libitsx_hip.so is not built: %s" % e)
    fn = L.itsx_write_feature_files
    vp, cp = C.c_void_p, C.c_char_p
    fn.restype = C.c_int
    fn.argtypes = [cp, cp, C.c_int64, C.c_int, vp, vp, vp, vp, vp, cp, vp, cp, vp, cp, vp, cp, vp]
    L.itsx_writers_last_error.restype = cp
    # three features over three samples; the first reads are 4, 0 and 2
    tab = dict(totals=np.array([5, 2, 2], np.int32), first=np.array([4, 0, 2], np.int32), row_off=np.array([0, 2, 3, 5], np.int64),
               es=np.array([0, 2, 1, 0, 1], np.int32), ec=np.array([3, 2, 2, 1, 1], np.int32),
               bases=b"GATTACA" + b"NRY" + b"T", off=np.array([0, 7, 10, 11], np.int64))

    def call(fasta, tsv, labels=None, reads=None, samples=None):
        keep = [_blob(x) if x is not None else (None, None) for x in (labels, reads, samples)]
        args = []
        for b, o in keep:
            args += [b, None if o is None else o.ctypes.data]
        rc = fn(None if fasta is None else os.fsencode(fasta), None if tsv is None else os.fsencode(tsv), 3, 3,
                tab["totals"].ctypes.data, tab["first"].ctypes.data, tab["row_off"].ctypes.data, tab["es"].ctypes.data, tab["ec"].ctypes.data,
                tab["bases"], tab["off"].ctypes.data, *args)
        return rc, L.itsx_writers_last_error().decode()
    return call


def test_files_byte_for_byte(writer, tmp_path):
    fa, tsv = str(tmp_path / "f.fa"), str(tmp_path / "t.tsv")
    assert writer(fa, tsv, labels=["aa", "bb", "cc"], samples=["x.fq", "y.fq", "z.fq"])[0] == 0
    assert open(fa, "rb").read() == b">aa;size=5\nGATTACA\n>bb;size=2\nNRY\n>cc;size=2\nT\n"
    assert open(tsv, "rb").read() == b"#feature\tx.fq\ty.fq\tz.fq\naa\t3\t0\t2\nbb\t0\t2\t0\ncc\t1\t1\t0\n"


def test_null_labels_and_null_sample_names(writer, tmp_path):
    fa, tsv = str(tmp_path / "f.fa"), str(tmp_path / "t.tsv")
    reads = ["r0 comment", "r1", "r2\tx", "r3", "read4 1:N:0 more"]      # a label is the first read's title up to the first blank
    assert writer(fa, tsv, reads=reads)[0] == 0
    assert open(fa, "rb").read() == b">read4;size=5\nGATTACA\n>r0;size=2\nNRY\n>r2;size=2\nT\n"
    assert open(tsv, "rb").read() == b"#feature\ts0\ts1\ts2\nread4\t3\t0\t2\nr0\t0\t2\t0\nr2\t1\t1\t0\n"
    assert writer(fa, tsv)[0] == 0                              # reads without names
    assert open(fa, "rb").read() == b">r000000004;size=5\nGATTACA\n>r000000000;size=2\nNRY\n>r000000002;size=2\nT\n"
    assert open(tsv, "rb").read().split(b"\n")[1] == b"r000000004\t3\t0\t2"


def test_one_path_null(writer, tmp_path):
    fa, tsv = str(tmp_path / "only.fa"), str(tmp_path / "only.tsv")
    assert writer(fa, None, labels=["a", "b", "c"])[0] == 0
    assert os.path.exists(fa) and not os.path.exists(tsv)
    assert writer(None, tsv, labels=["a", "b", "c"])[0] == 0
    assert open(tsv, "rb").read() == b"#feature\ts0\ts1\ts2\na\t3\t0\t2\nb\t0\t2\t0\nc\t1\t1\t0\n"


def test_unwritable_directory_is_an_io_error_and_leaves_nothing(writer, tmp_path):
    missing = tmp_path / "no_such_dir"
    rc, msg = writer(str(missing / "f.fa"), str(tmp_path / "t.tsv"), labels=["a", "b", "c"])
    assert rc == -2 and "f.fa" in msg
    assert not missing.exists() and not (tmp_path / "t.tsv").exists()
    rc, msg = writer(str(tmp_path / "g.fa"), str(missing / "t.tsv"), labels=["a", "b", "c"])
    assert rc == -2 and "t.tsv" in msg and not missing.exists()
