"""The host formatter with alignment records (itsx_write_domtbl_arrays_ali): without records the bytes of itsx_write_domtbl_arrays;
with them the hmm / ali / acc columns are the records' values in hmmsearch's widths and every other byte of the line stays."""
import os

import numpy as np


def _rows():
    from itsxpress_amd._lib import DOMAIN_DTYPE
    # (prof, rep, dom_idx, reported, tlen, ienv, jenv, bitscore, dombias, lnP, seq_score, seq_bias), in no particular order
    spec = [(1, 0, 0, 1, 180, 101, 140, 31.5, 0.3, -21.25, 33.0, 0.5),
            (0, 2, 0, 1, 250, 7, 66, 45.25, 0.0, -30.5, 45.5, 0.0),
            (0, 0, 1, 0, 180, 90, 120, 2.5, 1.2, -1.5, 38.75, 1.5),
            (0, 0, 0, 1, 180, 3, 60, 36.0, 0.1, -25.0, 38.75, 1.5),
            (0, 0, 2, 1, 180, 130, 178, 12.75, 0.6, -9.0, 38.75, 1.5),
            (0, 3, 0, 0, 90, 10, 40, 1.25, 0.0, -0.75, 1.5, 0.25),
            (1, 1, 1, 1, 300, 200, 260, 22.0, 0.2, -14.5, 40.25, 0.75),
            (1, 1, 0, 1, 300, 20, 70, 18.5, 0.4, -11.75, 40.25, 0.75),
            (1, 1, -1, 1, 300, 1, 2, 99.0, 0.0, -99.0, 99.0, 0.0),          # dom_idx < 0: not a domain, never written
            (1, 2, 0, 1, 250, 5, 5, 11.0, 0.0, -8.0, 11.0, 0.0)]            # an envelope of one residue
    rows = np.zeros(len(spec), DOMAIN_DTYPE)
    for i, (p, t, d, rep, tlen, ie, je, bit, db, lnp, ss, sb) in enumerate(spec):
        rows[i] = (t, p, tlen, ie, je, d, 3, 0, 0.0, 0.0, db, bit, lnp, ss, sb, 1, rep)
    return rows


def _blob(labels):
    offs = np.zeros(len(labels) + 1, np.int64)
    np.cumsum([len(x) for x in labels], out=offs[1:])
    return b"".join(labels), offs


def _write(fn, path, rows, ali):
    from itsxpress_amd import _lib
    L = _lib.lib()
    pn, po = _blob([b"3_ITS2_start", b"4_ITS2_end_of_a_long_profile_name"])
    M = np.array([61, 44], np.int32)
    tau = np.array([-3.875, -4.25], np.float32)
    lam = np.array([0.6953125, 0.703125], np.float32)
    domz = np.array([3, 2], np.int64)
    tb, to = _blob([b"target_zero", b"t1", b"X" * 1500, b"t3"])
    args = [os.fsencode(path), rows.ctypes.data, len(rows), 7, domz.ctypes.data, 2, pn, po.ctypes.data, M.ctypes.data, tau.ctypes.data, lam.ctypes.data,
            tb, to.ctypes.data]
    if fn == "ali":
        rc = L.itsx_write_domtbl_arrays_ali(*args, ali.ctypes.data if ali is not None else None)
    else:
        rc = L.itsx_write_domtbl_arrays(*args)
    assert rc == 0, L.itsx_writers_last_error()
    with open(path, "rb") as f:
        return f.read()


def test_alignment_record_is_24_bytes():
    from itsxpress_amd._lib import ALIGNMENT_DTYPE
    assert ALIGNMENT_DTYPE.itemsize == 24
    assert [ALIGNMENT_DTYPE.fields[k][1] for k in ALIGNMENT_DTYPE.names] == [0, 4, 8, 12, 16, 20]


def test_null_records_write_todays_bytes(tmp_path):
    rows = _rows()
    assert _write("ali", tmp_path / "a.txt", rows, None) == _write("plain", tmp_path / "b.txt", rows, None)


def test_records_fill_five_columns_and_nothing_else(tmp_path):
    from itsxpress_amd._lib import ALIGNMENT_DTYPE
    rows = _rows()
    ali = np.zeros(len(rows), ALIGNMENT_DTYPE)
    rng = np.random.default_rng(5)
    for i, r in enumerate(rows):
        if r["dom_idx"] < 0 or i == 4:          # row 4 (reported) stays without a record: its placeholders must stay too
            continue
        a, b = sorted(int(x) for x in rng.integers(r["ienv"], r["jenv"] + 1, 2))
        k1, k2 = sorted(int(x) for x in rng.integers(1, 45, 2))
        Ld = int(r["jenv"] - r["ienv"] + 1)
        ali[i] = (k1, k2, a, b, np.float32(Ld * float(rng.uniform(0.3, 1.0))), 1)
    ali[3]["oasc"] = np.float32(58 * 0.995)      # rounds to 0.99 / 1.00 at the %4.2f edge like any double
    ali[9] = (7, 7, 5, 5, np.float32(1.0), 1)    # one residue, acc 1.00
    plain = _write("plain", tmp_path / "p.txt", rows, None).decode().split("\n")
    got = _write("ali", tmp_path / "a.txt", rows, ali).decode().split("\n")
    assert len(plain) == len(got) and plain[:2] == got[:2]
    # the file's order: profile, target, domain; reported rows only
    order = sorted((i for i in range(len(rows)) if rows[i]["dom_idx"] >= 0 and rows[i]["dom_reported"] == 1),
                   key=lambda i: (rows[i]["prof"], rows[i]["rep"], rows[i]["dom_idx"]))
    data = [(p, g) for p, g in zip(plain[2:], got[2:]) if p]
    assert len(data) == len(order)
    seen_placeholder = False
    for (p, g), i in zip(data, order):
        r, a = rows[i], ali[i]
        fp, fg = p.split(), g.split()
        assert len(fp) == len(fg) == 23
        assert [fp[c] for c in range(23) if c not in (15, 16, 17, 18, 21)] == [fg[c] for c in range(23) if c not in (15, 16, 17, 18, 21)]
        if a["aligned"] == 1:
            acc = float(a["oasc"]) / (1.0 + abs(int(r["jenv"]) - int(r["ienv"])))
            want = "%5d %5d %5d %5d %5d %5d %4.2f" % (a["hmm_from"], a["hmm_to"], a["ali_from"], a["ali_to"], r["ienv"], r["jenv"], acc)
        else:
            seen_placeholder = True
            assert g == p
            want = "%5d %5d %5d %5d %5d %5d %4.2f" % (1, [61, 44][r["prof"]], r["ienv"], r["jenv"], r["ienv"], r["jenv"], 0.0)
        # every other byte of the line is unchanged: the columns sit at the same place in both lines
        at = p.index("%5d %5d %5d %5d %5d %5d %4.2f" % (1, [61, 44][r["prof"]], r["ienv"], r["jenv"], r["ienv"], r["jenv"], 0.0))
        assert g[at:at + len(want)] == want, (g, want)
        assert g[:at] == p[:at] and g[at + len(want):] == p[at + len(want):]
    assert seen_placeholder
    assert any(" 1.00 -" in g for _, g in data)
