"""The merge kernel (k_merge.hip) through Engine.merge_pairs and itsx_merge_pairs_load_files, held to the independent high-precision
model and its catalogue of decision edges (tests/merge_exact.py) exactly as the oracle is in tests/test_merge_edges_cpu.py, with
the bit-equality of engine and oracle asserted alongside.  `pytest -m gpu`."""
import os

import numpy as np
import pytest

import merge_exact as mx
import orc
from test_merge_edges_cpu import check_against_model

pytestmark = pytest.mark.gpu
E_FORMAT, E_UNSUPPORTED = -3, -5


def _run(engine, pairs, **kw):
    """pairs = [(Case, Result)] in one engine call with the parameters kw; every pair against the model and, bit for bit, the oracle"""
    cs = [c for c, _ in pairs]
    reason, merged, score, shift = engine.merge_pairs([c.f for c in cs], [c.fq for c in cs], [c.r for c in cs], [c.rq for c in cs], **kw)
    assert len(reason) == len(cs)
    memo = {}
    for i, (c, res) in enumerate(pairs):
        got = (orc.MERGE_REASONS[int(reason[i])],) + (merged[i] if merged[i] else (None, None)) + (float(score[i]), int(shift[i]))
        assert (merged[i] is not None) == (got[0] == "ok"), c.name
        check_against_model(c, res, got)
        key = (c.f, c.fq, c.r, c.rq)
        if key not in memo:
            memo[key] = orc.merge_pair(c.f, c.fq, c.r, c.rq, **kw)
        o = memo[key]
        assert got[0] == o[0] and got[4] == o[4] and np.float64(got[3]).view(np.uint64) == np.float64(o[3]).view(np.uint64), c.name
        if o[0] == "ok":
            assert merged[i] == (o[1], o[2]), c.name


def _by_parameters(pairs):
    """the pairs of each parameter set, in catalogue order"""
    out = {}
    for c, res in pairs:
        out.setdefault(tuple(sorted(c.kw.items())), []).append((c, res))
    return [(dict(k), v) for k, v in out.items()]


def test_catalogue_against_the_model(engine):
    for kw, pairs in _by_parameters(mx.catalogue()):
        _run(engine, pairs, **kw)


def test_sweep_against_the_model(engine):
    for kw, pairs in _by_parameters([(c, r) for c, r in mx.sweep() if not mx.thin(r)]):
        _run(engine, pairs, **kw)


def test_no_pairs_and_one_pair(engine):
    reason, merged, score, shift = engine.merge_pairs([], [], [], [])
    assert len(reason) == 0 and merged == []
    for c, res in mx.short_cases(8):
        _run(engine, [(c, res)])


@pytest.mark.parametrize("total", [4096, 4097])
def test_indexed_and_plain_variant(engine, total):
    """the batch's longest pair selects the kernel variant: 4096 bases in all takes the 5-mer index, 4097 the plain compare"""
    fill = mx.filler(total)
    assert len(fill.f) + len(fill.r) == total
    fres = mx.model_of(fill)
    assert fres.reason == "ok" and not mx.thin(fres)
    short = [(c, r) for c, r in mx.catalogue() if len(c.f) + len(c.r) <= 4096]
    assert len(short) > 100
    for kw, pairs in _by_parameters(short):
        assert max(len(c.f) + len(c.r) for c, _ in pairs) <= 4096
        _run(engine, pairs + ([(fill, fres)] if not kw else [(fill, mx.merge(fill.f, fill.fq, fill.r, fill.rq, **kw))]), **kw)


def test_length_limit(engine):
    from itsxpress_amd import EngineError
    ok = mx.filler(12000)
    res = mx.model_of(ok)
    assert res.reason == "ok" and not mx.thin(res) and len(ok.f) + len(ok.r) == 12000
    _run(engine, [(ok, res)])
    over = mx.filler(12001)
    with pytest.raises(EngineError) as ei:
        engine.merge_pairs([over.f], [over.fq], [over.r], [over.rq])
    assert ei.value.code == E_UNSUPPORTED
    _run(engine, mx.short_cases(5))                             # the same engine merges a normal pair afterwards


def test_quality_bytes_outside_33_126(engine):
    from itsxpress_amd import EngineError
    good = mx.short_cases(3)
    for name, f, fq, r, rq in mx.format_cases():
        with pytest.raises(EngineError) as ei:
            engine.merge_pairs([good[0][0].f, f], [good[0][0].fq, fq], [good[0][0].r, r], [good[0][0].rq, rq])
        assert ei.value.code == E_FORMAT, name
    _run(engine, good)


def test_grid_stride_past_65536_pairs(engine):
    """more pairs than the kernel launches blocks: every block takes a second pair and reuses its LDS"""
    base = mx.short_cases(50)
    assert 40 <= len(base) <= 50 and len({r.reason for _, r in base}) >= 4
    n = 65536 + 300
    _run(engine, [base[i % len(base)] for i in range(n)])


def _packed(s):
    """a read as the engine packs it (2 bits per base, exceptions as (position << 4 | code))"""
    code = {c: i for i, c in enumerate("ACGT-RYMKSWHBVDN")}
    w = np.zeros(max(1, (len(s) + 15) // 16), np.uint32)
    exc = []
    for i, ch in enumerate(s):
        c = code[ch]
        if c <= 3:
            w[i >> 4] |= np.uint32(c << (2 * (i & 15)))
        else:
            exc.append((i << 4) | c)
    return w, np.array(exc, np.uint32)


def test_files_of_two_samples(engine, tmp_path):
    """the short cases as two samples' R1 / R2 files through itsx_merge_pairs_load_files: the resident read set and the merged
    records written per sample are the model's"""
    cases = [(c, r) for c, r in mx.short_cases(50) if c.f and c.r and set((c.f + c.r).upper()) <= set("ACGTN")]
    assert len(cases) >= 30 and any(c.group == "lower" for c, _ in cases)
    assert sum(r.reason == "ok" for _, r in cases) >= 8 and sum(r.reason != "ok" for _, r in cases) >= 8
    half = len(cases) // 2
    samples = [cases[:half], cases[half:]]
    r1s, r2s, outs = [], [], []
    for s, part in enumerate(samples):
        for tag, recs in (("R1", [(c.name, c.f, c.fq) for c, _ in part]), ("R2", [(c.name, c.r, c.rq) for c, _ in part])):
            path = str(tmp_path / ("s%d_%s.fq" % (s, tag)))
            with open(path, "w") as f:
                f.write("".join("@%s %s\n%s\n+\n%s\n" % (n, tag, b, q) for n, b, q in recs))
            (r1s if tag == "R1" else r2s).append(path)
        outs.append(str(tmp_path / ("s%d_merged.fq" % s)))
    n, m = engine.merge_pairs_load_files(r1s, r2s, outs)
    want = [[(c, r) for c, r in part if r.reason == "ok"] for part in samples]
    assert list(n) == [len(p) for p in samples] and list(m) == [len(w) for w in want]
    flat = want[0] + want[1]
    assert engine.read_names() == [c.name for c, _ in flat]
    for i, (c, res) in enumerate(flat):
        w, e = engine.debug_packed_read(i)
        ew, ee = _packed(res.seq)
        assert np.array_equal(w, ew) and np.array_equal(e, ee), c.name
    idx = engine.merge_pair_index()
    assert [int(x >= 0) for x in idx] == [int(r.reason == "ok") for part in samples for _, r in part]
    for s in range(2):
        assert open(outs[s]).read() == "".join("@%s\n%s\n+\n%s\n" % (c.name, r.seq, r.qual) for c, r in want[s])
