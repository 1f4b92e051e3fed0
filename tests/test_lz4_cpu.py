"""Batched LZ4 without a GPU: the restated emission rule (tests/lz4_cases.py) is read back by stock LZ4 — which enforces the
format's end rules, so this proves them before a GPU sees the rule — and by the Python decoder; the golden file of stock streams
and verdicts decodes, agrees with stock and regenerates; the bounds hold, their worst-case family included; the library exports
the new names.  The argument checks of the entry points need a context and are in tests/test_lz4_gpu.py."""
import ctypes as C
import hashlib
import os
import sys

import pytest

import lz4_cases as Z
import parse1_cases as P1
from compression_algorithms_amd import _lib, lz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_lz4_batch_bound_bytes", "mi_lz4_batch_max_blocks", "mi_lz4_encode_batch_dev", "mi_lz4_decode_batch_dev",
         "mi_lz4_batch_size_dev", "mi_lz4_encode_batch", "mi_lz4_decode_batch"]


def _gen():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import gen_lz4_golden as G
    finally:
        sys.path.pop(0)
    return G


def _stock_readers():
    """[(name, block reader, frame reader)]: whichever of pyarrow and liblz4 (LZ4_decompress_safe) is installed"""
    out = []
    try:
        import pyarrow as pa
        raw, fr = pa.Codec("lz4_raw"), pa.Codec("lz4")
        out.append(("pyarrow", lambda s, n: raw.decompress(s, decompressed_size=n, asbytes=True) if n else b"",
                    lambda s, n: fr.decompress(s, decompressed_size=n, asbytes=True) if n else b""))
    except ImportError:
        pass
    G = _gen()
    L = G.liblz4()
    if L is not None:
        def block(s, n):
            r, got = G.stock_block(L, s, n)
            assert r == n, f"LZ4_decompress_safe returned {r}"
            return got
        out.append(("liblz4", block, None))
    return out


@pytest.mark.parametrize("parse", Z.PARSES)
@pytest.mark.parametrize("block", Z.BLOCKS)
def test_restatement_round_trips(block, parse):
    for name, data in list(Z.cpu_items().items()) + list(P1.cases().items()):
        s = Z.restate(data, block, parse, "frame")
        assert Z.decode(s, "frame") == (data, Z.OK, len(data)), name
        assert len(s) <= Z.bound(len(data), block, "frame"), name
        if len(data) <= block:
            s = Z.restate(data, block, parse, "block")
            assert Z.decode(s, "block") == (data, Z.OK, len(data)), name
            assert len(s) <= Z.bound(len(data), block, "block"), name


@pytest.mark.parametrize("parse", Z.PARSES)
@pytest.mark.parametrize("block", Z.BLOCKS)
def test_stock_lz4_reads_the_restatement(block, parse):
    """stock decoders refuse a block whose last match ends at the block's end, or starts in its last 12 bytes: the end rules hold"""
    readers = _stock_readers()
    if not readers:
        pytest.skip("neither pyarrow nor liblz4 is installed")
    for name, data in Z.cpu_items().items():
        for who, block_reader, frame_reader in readers:
            if frame_reader:
                assert frame_reader(Z.restate(data, block, parse, "frame"), len(data)) == data, (who, name)
            if len(data) <= block:
                assert block_reader(Z.restate(data, block, parse, "block"), len(data)) == data, (who, name)


def test_the_end_rules_are_what_the_restatement_is_about():
    """a block whose second half repeats its first: the parse's match runs to the last byte, the record's does not"""
    data = Z.cpu_items()["repeat_to_the_end"]
    tokens = Z.S.block_tokens(data, 65536, 0)[0]
    p, ln, d = tokens[-1]
    assert ln >= 4 and p + ln == len(data)
    rec = Z.emit_block(data, tokens)
    assert any(rec.endswith(Z.last(data[-k:])) for k in range(5, 16))            # the closing sequence: five literals or more
    assert Z.decode(rec, "block")[0] == data and len(rec) < len(data)            # (and a match was written)
    assert all(Z.emit_block(data[:n], Z.S.block_tokens(data[:n], 65536, 0)[0]) == Z.last(data[:n]) for n in range(1, 13))
    assert Z.restate(b"", 65536, 0, "block") == b"\x00" and Z.restate(b"", 65536, 0, "frame") == Z.FRAME_HEADER + Z.END_MARK


def test_xxh32_short():
    assert Z.xxh32_short(b"") == 0x02CC5D05 and Z.xxh32_short(b"a") == 0x550D7456 and Z.xxh32_short(b"abc") == 0x32D153FF
    assert Z.frame_header() == Z.FRAME_HEADER


def test_golden_decodes():
    g = Z.golden()
    assert len(g["blocks"]) >= 10 and len(g["frames"]) >= 10 and os.path.getsize(Z.GOLDEN) < 100_000
    for kind, fmt in (("blocks", "block"), ("frames", "frame")):
        for name, stream, data in g[kind]:
            assert len(data) <= Z.GOLDEN_CUT
            assert Z.decode(stream, fmt) == (data, Z.OK, len(data)), name
            assert Z.size_of(stream, fmt) == (Z.OK, len(data)), name
    flags = {name: stream[4] for name, stream, _ in g["frames"]}
    if "lz4f_linked" in flags:                                                   # what LZ4F_compressFrame's preferences were for
        assert not flags["lz4f_linked"] & 32 and flags["lz4f_content_size"] & 8 and flags["lz4f_block_checksum"] & 16
        assert flags["lz4f_content_checksum"] & 4 and dict((n, s[5]) for n, s, _ in g["frames"])["lz4f_256k"] == 0x50
    assert any(not s[4] & 32 and len(d) > 65536 for _, s, d in g["frames"])      # a linked frame of two blocks


def test_golden_mutations_agree_with_stock():
    """where LZ4_decompress_safe accepted a mutated block, the recorded expectation is MI_OK with stock's size; the expectation
    itself is lz4_cases.decode's, here recomputed"""
    m = Z.golden()["mutations"]
    if not m:
        pytest.skip("the golden file was written without liblz4")
    verdicts = set()
    for name, stream, cap, stock, want, sha in m:
        out, st, n = Z.decode(stream, "block", cap)
        assert (st, n) == want and (hashlib.sha256(out).hexdigest()[:16] if out is not None else None) == sha, name
        if stock >= 0:
            assert want == (Z.OK, stock), name
        verdicts.add((stock >= 0, st))
    assert (True, Z.OK) in verdicts and (False, Z.CORRUPT) in verdicts


def test_golden_regenerates():
    pytest.importorskip("pyarrow")
    G = _gen()
    with open(Z.GOLDEN) as f:
        on_disk = f.read()
    have = G.liblz4() is not None
    if have:
        assert on_disk == G.text(G.document())
    else:                                                                        # what pyarrow alone can write
        import json
        doc, new = json.loads(on_disk), G.document(False)
        assert [e for e in doc["blocks"]] == new["blocks"]
        assert [e for e in doc["frames"] if e["writer"].startswith("pyarrow")] == new["frames"]


def test_handwritten_streams_are_what_they_claim():
    for fmt in Z.FORMATS:
        names = [n for n, _, _ in Z.handwritten(fmt)]
        assert len(set(names)) == len(names)
        for name, stream, data in Z.handwritten(fmt):
            assert Z.decode(stream, fmt) == (data, Z.OK, len(data)), name
            assert Z.size_of(stream, fmt) == (Z.OK, len(data)), name
    hw = {n: (s, d) for n, s, d in Z.handwritten("block")}
    assert hw["chain_255_then_0"][0][1:3] == b"\xFF\x00" and hw["chain_255_then_0"][0].endswith(b"\xFF\x00\x50tail!")
    assert len(hw["lit_40000_far"][1]) > 40_000 > 32_768 and hw["empty"] == (b"\x00", b"")


def test_stock_lz4_agrees_on_the_handwritten_streams():
    """(except where a stream is about something stock does differently: it verifies the checksums this decoder skips)"""
    readers = _stock_readers()
    if not readers:
        pytest.skip("neither pyarrow nor liblz4 is installed")
    for who, block_reader, frame_reader in readers:
        for name, stream, data in Z.handwritten("block"):
            assert block_reader(stream, len(data)) == data, (who, name)
        for name, stream, data in Z.handwritten("frame") if frame_reader else ():
            if name != "checksum_fields_skipped":
                assert frame_reader(stream, len(data)) == data, (who, name)


def test_corrupt_verdicts():
    for fmt in Z.FORMATS:
        names = [n for n, _ in Z.corrupt(fmt)]
        assert len(set(names)) == len(names)
        for name, s in Z.corrupt(fmt):
            want = Z.ARG if name.startswith("unsupported_") else Z.CORRUPT
            assert Z.decode(s, fmt) == (None, want, 0), name
            assert Z.size_of(s, fmt)[0] in (want, Z.OK), name                    # (OK: a content size answers before the body is seen)
    s, d = Z.handwritten("block")[0][1:]
    assert Z.decode(s, "block", cap=len(d) - 1) == (None, Z.CAPACITY, len(d)) and Z.decode(s, "block", cap=len(d))[1] == Z.OK
    assert Z.size_of(dict(Z.corrupt("frame"))["content_size_plus_1"], "frame") == (Z.OK, 110)


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------
def test_bound_function():
    L = _lib.lib()
    for block in (1, 7, 1000, 4096, 65536):
        p = lz.params("deflate", block=block)
        for n in (0, 1, 14, 15, 269, 270, 65535, 65536, 65537, 1 << 20, (1 << 31) - 1):
            for k, fmt in enumerate(Z.FORMATS):
                assert int(L.mi_lz4_batch_bound_bytes(n, C.byref(p), k)) == Z.bound(n, block, fmt)
            assert int(L.mi_lz4_batch_max_blocks(n, 3, C.byref(p))) == int(L.mi_deflate_batch_max_blocks(n, 3, C.byref(p)))


@pytest.mark.parametrize("parse", Z.PARSES)
def test_bound_worst_case_family(parse):
    """270 noise bytes and a 4-byte repeat, over and over (every run pays two chain bytes), and plain noise (a frame stores it: the
    frame bound is met exactly)"""
    for block, n in ((65536, 274 * 100), (4096, 4096), (1000, 1000)):
        data = Z.worst_case(n)
        s = Z.restate(data, block, parse, "block")
        assert Z.decode(s, "block")[0] == data and len(data) < len(s) <= Z.bound(n, block, "block"), (block, len(s))
        s = Z.restate(data, block, parse, "frame")
        assert Z.decode(s, "frame")[0] == data and len(s) <= Z.bound(n, block, "frame")
    for block, n in ((65536, 65536), (1000, 3001), (7, 300), (1, 40)):
        data = P1.noise(n, 7)
        if block < 8 and parse:
            continue                                                             # (parse 1 of a block below 3 bytes is all literals either way)
        s = Z.restate(data, block, parse, "frame")
        assert Z.decode(s, "frame")[0] == data and len(s) == Z.bound(n, block, "frame")
        if n <= block:
            s = Z.restate(data, block, parse, "block")
            assert len(s) == n + 1 + len(Z.chain(n)) <= Z.bound(n, block, "block")


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_exports():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "mi_codec.h")) as f:
        h = f.read()
    assert all(name + "(" in h for name in NAMES)
    assert lz.LZ4_FORMATS == {"block": 0, "frame": 1}


def test_null_context_is_refused():
    L, p = _lib.lib(), lz.params("deflate")
    assert L.mi_lz4_decode_batch_dev(None, 0, None, None, None, None, None, None, None, 0, 0, None) == Z.ARG
    assert L.mi_lz4_batch_size_dev(None, 0, None, None, None, None, None, 0, None) == Z.ARG
    assert L.mi_lz4_encode_batch_dev(None, C.byref(p), 0, 0, None, None, 0, None, None, None, None, None, None) == Z.ARG
    assert L.mi_lz4_encode_batch(None, C.byref(p), 0, 0, None, None, None, None, None, None) == Z.ARG
    assert L.mi_lz4_decode_batch(None, 0, None, None, None, None, None, None, 0, 0) == Z.ARG
