"""itsx_twriter_strands on a writer with a device (itsx_twriter_set_device): the unit's strands go up beside its coordinates, the plan
marks the flipped records and k_trim_copy<true, true> reads their lines backwards (csrc/k_trim.hip).  The catalogue and the model are
tests/twriter_strand_cases.py, as in tests/test_twriter_strands_cpu.py; the device's file must inflate to the model byte for byte.
`pytest -m gpu`."""
import gzip

import numpy as np
import pytest

import twriter_strand_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _units(monkeypatch):
    monkeypatch.setenv("ITSX_WRITE_UNIT_KB", str(tc.UNIT_KB))
    monkeypatch.setenv("ITSX_IO_THREADS", "4")


@pytest.fixture(scope="module")
def cat():
    text, recs, start, stop, strand, tags = tc.catalogue()
    return dict(text=text, recs=recs, start=start, stop=stop, strand=strand, tags=tags, ends=tc.record_ends(text),
                model={ccs: tc.model(recs, start, stop, strand, ccs) for ccs in (0, 1)})


@pytest.mark.parametrize("pieces", [False, True])
@pytest.mark.parametrize("ccs", [0, 1])
def test_edge_catalogue_on_the_device_equals_the_model(cat, tmp_path, ccs, pieces):
    from itsxpress_amd import Engine
    dev = Engine(0)
    try:
        out = tmp_path / "o.fq.gz"
        nw, tot = tc.write(out, cat["text"], cat["ends"], cat["start"], cat["stop"], cat["strand"], 1, ccs, pieces, ctx=dev)
        st = dev.stats()
    finally:
        dev.close()
    want, n, t = cat["model"][ccs]
    assert (nw, tot) == (n, t)
    assert gzip.decompress(out.read_bytes()) == want
    # the units went through the device's index, plan and copy; the one with the blank line was sliced on the host
    assert st["n_tw_units_device"] > 40 and st["n_tw_units_host"] >= 1
    assert st["n_tw_units_host"] <= 2


def test_a_writer_without_strands_and_one_with_none_flipped_write_the_same_bytes(cat, tmp_path):
    """the device file of a writer that never got strands = that of one whose strands are all +1 or 0 (its units take the copy kernel
    without the flipped branch), and both inflate to the model without flips"""
    from itsxpress_amd import Engine
    files = []
    for k, sd in enumerate((None, np.where(cat["strand"] < 0, 1, cat["strand"]).astype(np.int8))):
        dev = Engine(0)
        try:
            out = tmp_path / ("o%d.fq.gz" % k)
            tc.write(out, cat["text"], cat["ends"], cat["start"], cat["stop"], sd, 1, 0, False, ctx=dev)
        finally:
            dev.close()
        files.append(out.read_bytes())
    assert files[0] == files[1]
    assert gzip.decompress(files[0]) == tc.model(cat["recs"], cat["start"], cat["stop"], np.ones_like(cat["strand"]), 0)[0]
