"""The device deflate (csrc/k_deflate.hip, compression == 3 of the batch writers): what can be checked without a device.  The code
lengths come from csrc/deflate_codes.h, the header one lane of the kernel runs per block, through itsx_debug_huffman_lengths; the
Kraft sums are exact integers scaled by 2^maxbits."""
import heapq
import os
import re

import numpy as np
import pytest

from itsxpress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["itsx_deflate_block_bytes", "itsx_deflate_bound", "itsx_deflate_device", "itsx_debug_huffman_lengths"]


def _fib(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def _block_bytes():
    return int(_lib.lib().itsx_deflate_block_bytes())


def _cases():
    B = "B"                                     # a count of a block's size: itsx_deflate_block_bytes(), asked when the test runs
    only256 = [0] * 286
    only256[256] = 1
    return [("286 equal", [5] * 286, 15), ("two symbols", [0, 3, 0, 9], 15), ("fibonacci 30", _fib(30), 15), ("fibonacci 19", _fib(19), 7),
            ("one heavy among 285", [B] + [1] * 285, 15), ("symbol 256 alone", only256, 15)]


def _lengths(freq, maxbits):
    f = np.ascontiguousarray(freq, np.uint32)
    out = np.full(f.size, 255, np.uint8)
    rc = _lib.lib().itsx_debug_huffman_lengths(f.ctypes.data, int(f.size), int(maxbits), out.ctypes.data)
    assert rc == 0
    return [int(x) for x in out]


def _huffman_depths(freq):
    """an unlimited Huffman code's lengths, built with a heap of (count, tie, symbols)"""
    used = [i for i, f in enumerate(freq) if f]
    depth = dict.fromkeys(used, 0)
    heap = [(freq[i], i, [i]) for i in used]
    heapq.heapify(heap)
    tie = len(freq)
    while len(heap) > 1:
        fa, _, sa = heapq.heappop(heap)
        fb, _, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, tie, sa + sb))
        tie += 1
    return depth


@pytest.mark.parametrize("name,freq,maxbits", _cases(), ids=[c[0] for c in _cases()])
def test_code_lengths(name, freq, maxbits):
    freq = [_block_bytes() if f == "B" else f for f in freq]
    lens = _lengths(freq, maxbits)
    used = [i for i, f in enumerate(freq) if f]
    for i, f in enumerate(freq):
        assert (lens[i] == 0) == (f == 0), (name, i, f, lens[i])           # a zero count gets length 0, and nothing else does
    assert max(lens) <= maxbits
    if len(used) == 1:
        assert lens[used[0]] == 1
    if len(used) >= 2:
        kraft = sum(1 << (maxbits - lens[i]) for i in used)
        assert kraft == 1 << maxbits, (name, kraft)                          # complete: zlib takes neither more nor less
        depth = _huffman_depths(freq)
        print(name, "deepest unlimited", max(depth.values()), "deepest", max(lens))
        if max(depth.values()) <= maxbits:                                   # the unlimited code fits: nothing may cost more
            assert sum(freq[i] * lens[i] for i in used) == sum(freq[i] * depth[i] for i in used)


def test_the_limit_engages_on_the_fibonacci_counts():
    assert max(_huffman_depths(_fib(30)).values()) == 29 and max(_lengths(_fib(30), 15)) == 15
    assert max(_huffman_depths(_fib(19)).values()) == 18 and max(_lengths(_fib(19), 7)) == 7


def test_bad_arguments_are_refused():
    L = _lib.lib()
    f = np.ones(300, np.uint32)
    out = np.zeros(300, np.uint8)
    assert L.itsx_debug_huffman_lengths(f.ctypes.data, 300, 15, out.ctypes.data) == -1          # more symbols than any alphabet has
    assert L.itsx_debug_huffman_lengths(f.ctypes.data, 19, 4, out.ctypes.data) == -1            # 19 symbols cannot fit 4 bits
    assert L.itsx_debug_huffman_lengths(f.ctypes.data, 19, 16, out.ctypes.data) == -1
    assert L.itsx_debug_huffman_lengths(None, 19, 7, out.ctypes.data) == -1


def test_bound():
    L = _lib.lib()
    B = _block_bytes()
    assert 32768 < B <= 65536 * 2
    ns = [0, 1, 2, 65534, 65535, 65536, B - 1, B, B + 1, 2 * B + 1, 10 * B + 7, 3 * 10 ** 9 + 11]
    for r in (1, 2, 3, 400):
        for n in ns:
            bound = int(L.itsx_deflate_bound(n, r))
            # the fewest members n bytes in r ranges can take ...: one range of n bytes and r - 1 empty ones; stored blocks, 18 a member
            blocks = -(-n // B) if n else 0
            empty = r - 1 if n else r
            assert bound >= n + 5 * -(-n // 65535) + 18 * (blocks + empty), (n, r, bound)
            # ... and the most: every range but one a single byte more than whole blocks
            assert bound >= n + 5 * -(-n // 65535) + 18 * (n // B + r), (n, r, bound)
            assert int(L.itsx_deflate_bound(n + 1, r)) >= bound and int(L.itsx_deflate_bound(n, r + 1)) >= bound
    assert int(L.itsx_deflate_bound(0, 0)) == 0


def test_abi_names_the_new_symbols():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(itsx_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.EXPORTS)
    assert re.search(r"#define ITSX_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6          # additive: no new version
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert re.search(r"int64_t itsx_deflate_block_bytes\(void\);", header)
    assert re.search(r"int64_t itsx_deflate_bound\(int64_t nbytes, int32_t n_ranges\);", header)
    assert re.search(r"int itsx_debug_huffman_lengths\(const uint32_t \*freq, int32_t n, int32_t maxbits, uint8_t \*lengths\);", header)
    assert "ms_deflate" in _lib.STATS_DTYPE.names
    assert _lib.STATS_DTYPE.fields["ms_deflate"][1] == _lib.STATS_DTYPE.fields["ms_ensemble"][1] + 4          # where padding was


def test_the_switch_is_registered_and_the_host_writers_refuse_the_device_kind(tmp_path):
    with open(os.path.join(ROOT, "itsxpress_amd", "csrc", "switches.cpp")) as f:
        assert re.search(r'\{"ITSX_DEVICE_DEFLATE", SW_MODE, "=1: the batch writers deflate gzip output on the device', f.read())
    from itsxpress_amd.engine import _batch_compression
    assert _batch_compression(True, False, "device", "t") == 3 and _batch_compression(True, False, "host", "t") == 1
    assert _batch_compression(False, True, "host", "t") == 2 and _batch_compression(False, False, "host", "t") == 0
    for gz, zs in ((False, False), (False, True), (True, True)):
        with pytest.raises(ValueError, match="device"):
            _batch_compression(gz, zs, "device", "t")
    from itsxpress_amd.engine import Engine
    e = Engine.__new__(Engine)                  # no context: the setting is the Python layer's
    assert e.deflate == "host"
    e.deflate = "device"
    assert e.deflate == "device"
    with pytest.raises(ValueError):
        e.deflate = "gpu"
    assert e.deflate == "device"
    # the host-only writer has no device text: 3 is not a kind it knows
    L = _lib.lib()
    src = tmp_path / "in.fq"
    src.write_text("@r\nACGT\n+\nIIII\n")
    a, b = np.zeros(1, np.int32), np.full(1, 4, np.int32)
    nw, tot = np.zeros(1, np.int64), np.zeros(1, np.int64)
    rc = L.itsx_write_trimmed_fastq(os.fsencode(str(src)), os.fsencode(str(tmp_path / "out.fq.gz")), 3, 0, a.ctypes.data, b.ctypes.data, 1,
                                    nw.ctypes.data, tot.ctypes.data)
    assert rc == -1 and not os.path.exists(str(tmp_path / "out.fq.gz"))
