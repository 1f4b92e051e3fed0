"""Batched Snappy without a GPU: the restated emission rule (tests/snappy_cases.py) round-trips through the Python decoder
and, where pyarrow is installed, through stock Snappy; the golden file of stock streams decodes and regenerates; the bound
holds, its worst-case family included; the library exports the new names.  The argument checks of the entry points need a
context (every entry point refuses a NULL one first) and are in tests/test_snappy_gpu.py."""
import ctypes as C
import os
import sys

import pytest

import parse1_cases as P1
import snappy_cases as S
from compression_algorithms_amd import _lib, lz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_snappy_batch_bound_bytes", "mi_snappy_batch_max_blocks", "mi_snappy_encode_batch_dev", "mi_snappy_decode_batch_dev",
         "mi_snappy_batch_size_dev", "mi_snappy_encode_batch", "mi_snappy_decode_batch"]


def _stock(stream, n):
    import pyarrow as pa
    return pa.decompress(stream, decompressed_size=n, codec="snappy", asbytes=True) if n else b""


@pytest.mark.parametrize("parse", S.PARSES)
@pytest.mark.parametrize("block", S.BLOCKS)
def test_restatement_round_trips(block, parse):
    for name, data in P1.cases().items():
        s = S.restate(data, block, parse)
        assert S.decode(s) == (data, S.OK, len(data)), name
        assert len(s) <= S.bound(len(data), block), name


@pytest.mark.parametrize("parse", S.PARSES)
@pytest.mark.parametrize("block", S.BLOCKS)
def test_stock_snappy_reads_the_restatement(block, parse):
    pytest.importorskip("pyarrow")
    for name, data in P1.cases().items():
        assert _stock(S.restate(data, block, parse), len(data)) == data, name


def test_restatement_sizes_on_record():
    """the sizes the design was judged by (parse 1, one block size): a change of the rule shows here first"""
    c = P1.cases()
    assert [len(S.restate(c[k], 65536, 1)) for k in ("text", "zeros", "mixed", "rising")] == [140_487, 3_301, 7_053, 478]


def test_every_piece_of_a_split_is_at_least_4():
    for L in range(4, 259):
        pieces, r = [], L
        while r >= 68:
            pieces.append(64)
            r -= 64
        if r > 64:
            pieces.append(60)
            r -= 60
        pieces.append(r)
        assert sum(pieces) == L and min(pieces) >= 4 and max(pieces) <= 64, (L, pieces)


def test_golden_decodes():
    g = S.golden()
    assert len(g) >= 10 and os.path.getsize(S.GOLDEN) < 200_000
    for name, stream, data in g:
        assert len(data) <= S.GOLDEN_CUT
        assert S.decode(stream) == (data, S.OK, len(data)), name


def test_golden_regenerates():
    pytest.importorskip("pyarrow")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import gen_snappy_golden as G
    finally:
        sys.path.pop(0)
    with open(S.GOLDEN) as f:
        assert f.read() == G.text(G.document())


def test_handwritten_streams_are_what_they_claim():
    names = [n for n, _, _ in S.handwritten()]
    assert len(set(names)) == len(names)
    for name, stream, data in S.handwritten():
        assert S.decode(stream) == (data, S.OK, len(data)), name
    hw = {n: d for n, _, d in S.handwritten()}
    assert len(hw["copy4_far"]) == 140_000 and len(hw["lit_40000"]) > 40_000 > 32_768


def test_stock_snappy_agrees_on_the_handwritten_and_the_corrupt_streams():
    pytest.importorskip("pyarrow")
    for name, stream, data in S.handwritten():
        assert _stock(stream, len(data)) == data, name
    for name, stream in S.corrupt():
        with pytest.raises(Exception):
            _stock(stream, max(S.preamble(stream)[1], 1))
        assert S.decode(stream)[1] in (S.CORRUPT, S.ARG), name


def test_corrupt_verdicts():
    got = {name: S.decode(s)[1] for name, s in S.corrupt()}
    assert set(got.values()) == {S.CORRUPT}, got                # (2^32 does not fit 32 bits: corrupt, not merely too large)
    assert S.decode(S.varint(0x80000000) + b"\x00")[1] == S.ARG  # well-formed, above the per-item limit
    assert S.decode(S.varint(0xFFFFFFFF) + b"\x00")[1] == S.ARG
    s, d = S.stream_of([S.lit(b"abcdefgh")])
    assert S.decode(s, cap=7) == (None, S.CAPACITY, 8) and S.decode(s, cap=8)[1] == S.OK


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def test_bound_function():
    L = _lib.lib()
    for block in (1, 7, 1000, 4096, 65536):
        p = lz.params("deflate", block=block)
        for n in (0, 1, 60, 61, 62, 256, 257, 65535, 65536, 65537, 1 << 20, (1 << 31) - 1):
            assert int(L.mi_snappy_batch_bound_bytes(n, C.byref(p))) >= S.bound(n, block)
            assert int(L.mi_snappy_batch_max_blocks(n, 3, C.byref(p))) == int(L.mi_deflate_batch_max_blocks(n, 3, C.byref(p)))


@pytest.mark.parametrize("parse", S.PARSES)
def test_bound_worst_case_family(parse):
    """61 noise bytes and a 4-byte repeat, over and over: every run pays the second tag byte"""
    for block, n in ((65536, 65 * 400), (4096, 65 * 130), (1000, 65 * 40)):
        data = S.worst_case(n)
        s = S.restate(data, block, parse)
        assert S.decode(s)[0] == data
        assert len(data) < len(s) <= S.bound(n, block), (block, len(s))


@pytest.mark.parametrize("block,n", [(1, 40), (7, 300), (65536, 70_000)])
def test_bound_noise(block, n):
    data = P1.noise(n, 7)
    for parse in S.PARSES if block > 7 else (0,):                # (parse 1 of a block below 3 bytes is all literals either way)
        s = S.restate(data, block, parse)
        assert S.decode(s)[0] == data and len(s) <= S.bound(n, block)


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_exports():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "mi_codec.h")) as f:
        h = f.read()
    assert all(name + "(" in h for name in NAMES)


def test_null_context_is_refused():
    L, p = _lib.lib(), lz.params("deflate")
    assert L.mi_snappy_decode_batch_dev(None, 0, None, None, None, None, None, None, None, 0, None) == S.ARG
    assert L.mi_snappy_batch_size_dev(None, 0, None, None, None, None, None, None) == S.ARG
    assert L.mi_snappy_encode_batch_dev(None, C.byref(p), 0, None, None, 0, None, None, None, None, None, None) == S.ARG
    assert L.mi_snappy_encode_batch(None, C.byref(p), 0, None, None, None, None, None, None) == S.ARG
    assert L.mi_snappy_decode_batch(None, 0, None, None, None, None, None, None, 0) == S.ARG
