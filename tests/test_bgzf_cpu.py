"""BGZF without a GPU: the expected stream (the CPU oracle's mode-Z records in members) against Python's gzip, the serial
index walker and the foreign streams the GPU tests use, the refusal list against the walker, the exports and the bound."""
import gzip
import os
import re

import numpy as np
import pytest

import bgzf_cases as B
from compression_algorithms_amd import _lib, lz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi_bgzf_bound_bytes", "mi_bgzf_encode_dev", "mi_bgzf_encode", "mi_bgzf_index_dev", "mi_bgzf_inflate_dev", "mi_bgzf_inflate")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _check_expected(data, block):
    stream, table = B.expected_bgzf(data, block)
    assert gzip.decompress(stream) == data
    so, oo = B.walk(stream)
    nb = (len(data) + block - 1) // block
    assert len(so) == nb + 2 and [8 * s for s in so[:-1]] == table and so[-1] == len(stream)
    assert oo[:-1] == [min(b * block, len(data)) for b in range(nb + 1)] and oo[-1] == len(data)
    assert max(np.diff(so)) <= 65536
    assert stream.endswith(B.EOF) and len(stream) <= B.bound(len(data), block)
    return stream


@pytest.mark.parametrize("block", B.BLOCKS)
def test_expected_stream_is_gzip(block):
    for name, data in B.own_cases().items():
        if block == 257 and len(data) > 100_000:
            data = data[:40_000]                           # (1 200 blocks of 257 bytes would show nothing more)
        _check_expected(data, block)
    _check_expected(B.one_block(block), block)


def test_largest_member_and_empty_input():
    rnd = B.own_cases()["random"]
    so, _ = B.walk(B.expected_bgzf(rnd, 65280)[0])
    assert max(np.diff(so)) == 65318                       # the stored form of a 65 280-byte block
    so, _ = B.walk(B.expected_bgzf(rnd, 65498)[0])
    assert max(np.diff(so)) == 65536
    assert B.expected_bgzf(b"", 65280) == (B.EOF, [0]) and gzip.decompress(B.EOF) == b""


def test_foreign_streams_are_bgzf():
    names = set()
    for name, stream, want in B.foreign_set():
        so, oo = B.check_foreign(stream, want)
        names.add(name)
        if name.startswith("decoy"):
            # byte-exact member headers inside the members: more header patterns than members
            assert stream.count(B.HEAD[:4]) >= len(so) - 1 + 10
    assert {"decoy_stored", "decoy_twice", "no_eof", "only_eof"} <= names
    # the set holds empty members in the middle, XLEN > 6, stored blocks and several blocks per member
    stream = dict((n, s) for n, s, _ in B.foreign_set())["text"]
    so, oo = B.walk(stream)
    xlens = {B.parse_member(stream, s)[2] for s in so[:-1]}
    assert 6 in xlens and max(xlens) > 6
    assert any(a == b for a, b in zip(oo[:-2], oo[1:-1]))


def test_hard_streams_defeat_the_guess():
    """the streams the GPU index is checked on really make its per-chunk guess wrong, or leave it without one: the rule
    of k_bgzf_spec restated in Python (bgzf_cases.spec_model) against the walker"""
    for name, stream, want, planted, least_none in B.hard_set():
        B.check_foreign(stream, want)
        model = B.spec_model(stream)
        wrong = [c for c, guess, true, hi in model if guess is not None and guess != true]
        none = [c for c, guess, true, hi in model if guess is None and true < hi]
        assert set(planted) <= set(wrong), (name, planted, wrong)
        assert len(none) >= least_none, (name, none)
        for c, guess, true, hi in model:                   # a planted guess is a decoy 100 bytes into its chunk
            if c in planted:
                assert guess == c * B.CHUNK + 100 and true > guess
        if name == "planted_70_chunks":
            assert len(model) == 69 and {1, 33, 63, 64, 65, 69} <= set(wrong) and len(wrong) < len(model)
    # and the ordinary foreign streams do not: which is why they alone would not show the verify pass working
    for name, stream, want in B.foreign_set():
        if stream:
            assert all(guess == true for c, guess, true, hi in B.spec_model(stream) if true < hi), name


def test_late_refusals_lie_behind_chunk_one():
    for name, stream, stage in B.hard_rejects():
        assert stage == "index" and len(stream) > 3 * B.CHUNK
        with pytest.raises(B.Corrupt):
            B.walk(stream)
        so = [k * B.STORED_MEMBER for k in range(5)]       # five good members: chunks 0 and 1 are clean
        pos = 0
        for want in so:
            assert pos == want
            pos += B.parse_member(stream, pos)[0]
        assert pos >= 2 * B.CHUNK


def test_gzi_layout():
    stream, table = B.expected_bgzf(B.one_block(65280) * 3, 65280)
    g = B.gzi(stream)
    assert int.from_bytes(g[:8], "little") == 3 and len(g) == 8 + 3 * 16
    assert int.from_bytes(g[8:16], "little") == table[1] // 8 and int.from_bytes(g[16:24], "little") == 65280


def test_walker_refuses_what_the_index_must_refuse():
    for name, stream, stage in B.rejects():
        if stage == "index":
            with pytest.raises(B.Corrupt):
                B.walk(stream)
        else:
            B.walk(stream)
            with pytest.raises(Exception):
                gzip.decompress(stream)


def test_bgzf_symbols_exported(built):
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(built, s), s
    hdr = open(os.path.join(ROOT, "include", "mi_codec.h")).read()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\(", hdr), s
    assert re.search(r"#define\s+MI_BGZF_BLOCK\s+65280u\b", hdr) and re.search(r"#define\s+MI_BGZF_MAX_BLOCK\s+65498u\b", hdr)
    assert lz.BGZF_BLOCK == 65280 and lz.BGZF_MAX_BLOCK == 65498 and lz.BGZF_EOF == B.EOF


def test_bound_values(built):
    for block in (65498, 65280, 4096, 257, 1):
        p = lz.params("deflate", block=block)
        for n in (0, 1, block - 1, block, block + 1, 10**9):
            assert lz.bound_bytes_bgzf(n, p) == B.bound(n, block), (n, block)
    assert lz.bound_bytes_bgzf(0) == 28
    rnd = B.own_cases()["random"]
    for block in B.BLOCKS:
        assert lz.bound_bytes_bgzf(len(rnd), lz.params("deflate", block=block)) >= len(B.expected_bgzf(rnd, block)[0])
    # the all-stored stream meets the bound exactly
    assert lz.bound_bytes_bgzf(len(rnd), lz.params("deflate", block=65280)) == len(B.expected_bgzf(rnd, 65280)[0])
    # a block whose stored member would not fit 65 536 bytes is no BGZF parameter set: the function says 0
    assert B.bound(65498, 65498) - 28 == 65536
    for block in (65499, 65536, 0):
        assert lz.bound_bytes_bgzf(10, lz.params("deflate", block=block)) == 0
