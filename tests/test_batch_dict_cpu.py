"""Preset dictionaries for the batched inflate and deflate, the parts that need no device: the hand-made items of dict_cases against
stock zlib with zdict= (bytes and verdicts), the expected deflate streams (the walk against the oracle, stock zlib reading
them, matches into the dictionary, the two bounds), the conditions the GPU file relies on in its fixtures, the exported
symbols and the argument checks the Python wrappers make before they touch a device."""
import ctypes as C
import os
import zlib

import pytest

import dict_cases as D
from compression_algorithms_amd import _lib, lz

INFLATE = ("mi_inflate_batch_dict_dev", "mi_inflate_batch_dict_size_dev", "mi_inflate_batch_dict")
DEFLATE = ("mi_deflate_batch_dict_dev", "mi_deflate_batch_dict", "mi_deflate_batch_dict_max_blocks", "mi_deflate_batch_dict_bound_bytes")


def test_the_bit_writer_writes_what_stock_zlib_reads():
    data = D.text(3000)
    tok = D.literals(data) + [(3, 1), (258, 3000), (4, 2), (17, 32), (130, 3259)]
    assert D.stock_inflate(D.fixed_stream(tok), "raw") == D.expand(tok) and D.expand(tok)[:3000] == data
    for ln in (3, 10, 11, 12, 114, 115, 227, 257, 258):
        for d in (1, 4, 5, 6, 24, 25, 192, 193, 3000):
            tok = D.literals(data) + [(ln, d)]
            assert D.stock_inflate(D.fixed_stream(tok), "raw") == D.expand(tok), (ln, d)


@pytest.mark.parametrize("container", D.CONTAINERS)
@pytest.mark.parametrize("dl", D.DICT_LENGTHS)
def test_seam_items_have_stock_zlibs_bytes_and_verdicts(container, dl):
    zd = D.dictionary(dl)
    names = []
    for name, item, want in D.seam_items(container, dl):
        assert D.stock_inflate(item, container, zd) == want, name
        names.append(name)
    refused = [n for n, _, w in D.seam_items(container, dl) if w is None]
    assert refused == (["distance_e_plus_1", "later_distance_too_far"] if dl < D.WINDOW else [])
    for must in ("distance_e", "last_byte_repeated"):
        assert must in names
    if dl >= 300:
        assert "seam_d5_len20" in names and "seam_d100_len150" in names and "seam_d300_len258" in names


def test_the_first_token_of_every_seam_item_is_a_match_into_the_dictionary():
    for dl in D.DICT_LENGTHS:
        e = min(dl, D.WINDOW)
        for name, tok in D.seam_tokens(dl):
            if not name.startswith("later_"):
                assert len(tok[0]) == 2 and tok[0][1] >= 1, name
        exact = dict(D.seam_tokens(dl))["distance_e"]
        assert exact[0][1] == e and D.expand(exact, D.dictionary(dl))[:1] == D.window(D.dictionary(dl))[:1]


@pytest.mark.parametrize("ring", [4096, 32768])
def test_wrapped_ring_items(ring):
    zd, tok, want = D.wrapped_ring(ring)
    assert D.expand(tok, zd) == want and len(want) > ring // 2
    first = next(t for t in tok if len(t) == 2)
    at = sum(1 for t in tok[:tok.index(first)])
    assert first[1] == at + len(zd) and at == (5000 if ring == 4096 else 20000)           # E's first byte, from far behind
    for container in D.CONTAINERS:
        assert D.stock_inflate(D.frame(D.fixed_stream(tok), want, container, zd), container, zd) == want


def test_mixed_zlib_batch_has_stock_zlibs_verdicts():
    zd, items = D.mixed_zlib()
    for name, item, want in items:
        assert D.stock_inflate(item, "zlib", zd) == want, name
    assert [n for n, _, w in items if w is None] == ["other_dictionary", "no_fdict_distance_in_front", "fdict_truncated_header"]
    fd = {n: bool(i[1] & 0x20) for n, i, _ in items}
    assert fd["fdict"] and fd["other_dictionary"] and fd["fdict_distance_into_e"] and not fd["no_fdict"] and not fd["no_fdict_distance_in_front"]


@pytest.mark.parametrize("container", D.CONTAINERS)
def test_stock_items_use_the_dictionary(container):
    """stock zlib reads them back with the dictionary, and the text items do not read back without it"""
    for dl in (300, 40000):
        zd = D.dictionary(dl)
        for name, item, want in D.stock_items(container, dl):
            assert D.stock_inflate(item, container, zd) == want, name
            if container == "zlib" and want:
                assert item[1] & 0x20 and item[2:6] == zlib.adler32(zd).to_bytes(4, "big"), name
        name, item, want = [c for c in D.stock_items(container, dl) if c[0] == "text_700_level_9"][0]
        assert D.stock_inflate(item, container) != want


def test_library_exports_the_dictionary_entry_points():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi_codec.h")).read()
    for s in INFLATE + DEFLATE:
        assert s in _lib.EXPORTS and hasattr(L, s), s
        assert f"mi_status {s}(" in hdr or f"uint64_t  {s}(" in hdr


def test_wrappers_refuse_gzip_with_a_dictionary_before_touching_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the wrapper asked for a device before it checked its arguments")
    monkeypatch.setattr(lz, "default_context", no_device)
    for call in (lz.inflate_batch, lz.inflate_batch_sizes, lz.inflate_batch_host, lz.deflate_batch, lz.deflate_batch_host):
        with pytest.raises(ValueError):
            call([b"\x03\x00"], container="gzip", zdict=b"abc")
        with pytest.raises(ValueError):
            call([b"\x03\x00"], container="raw", zdict="abc")
        with pytest.raises(ValueError):
            call([b"\x03\x00"], container="raw", zdict=[1, 2, 3])


# ---- the deflate's expected streams ------------------------------------------------------------------------------------------------
def test_the_walk_without_a_dictionary_is_the_oracles_tokeniser():
    import numpy as np
    from oracle import orc
    for n in (1, 5, 700, 65536):
        t = D.text(n, seed=2)
        enc = orc.Deflate()
        enc.fresh()
        assert np.array_equal(D.walk(b"", t)[0], enc.block_encode(t)), n
    for block in D.BLOCKS:                                         # ... and the whole stream that of the oracle without one
        for name, item in D.deflate_items(block, 300):
            for c in D.CONTAINERS:
                assert D.expected_stream(item, b"", block, c)[0] == bytes(orc.defz_stream(item, block, c)[0]), (block, name, c)


@pytest.mark.parametrize("block", D.BLOCKS)
@pytest.mark.parametrize("dl", D.DICT_LENGTHS)
def test_expected_streams(block, dl):
    """stock zlib reads every one with zdict= in both containers; every case has matches whose source starts inside U; the
    helpers bound blocks and bytes, stored blocks included"""
    zd = D.dictionary(dl)
    p = lz.params("deflate", block=block)
    L = _lib.lib()
    items = D.deflate_items(block, dl)
    names = [n for n, _ in items]
    u = len(D.used(zd, block))
    assert u == min(dl, 32768, block // 2)
    for must in (f"text_{block - u - 1}", f"text_{block - u}", f"text_{block - u + 1}", f"text_{2 * block - u + 1}", "text_0", "text_1",
                 "text_3", "text_4", "text_5", "text_700", "zeros", "noise", "pages", "of_the_dictionary", "dictionary_tail_repeated"):
        assert must in names, must
    into = {}
    for name, item in items:
        for c in D.CONTAINERS:
            s, into[name] = D.expected_stream(item, zd, block, c)
            assert D.stock_inflate(s, c, zd) == item, (name, c)
            assert len(s) <= L.mi_deflate_batch_dict_bound_bytes(len(item), p, lz.CONTAINERS[c], dl), (name, c)
            if c == "zlib":
                assert s[:2] == b"\x78\xbb" and s[2:6] == zlib.adler32(zd).to_bytes(4, "big")
    assert into["dictionary_tail_repeated"] >= 1 and (dl < 300 or into["text_700"] >= 1), into
    assert [D.blocks_of(len(i), block, dl) for n, i in items if n == f"text_{2 * block - u + 1}"] == [3]
    total = sum(len(i) for _, i in items)
    assert sum(D.blocks_of(len(i), block, dl) for _, i in items) <= L.mi_deflate_batch_dict_max_blocks(total, len(items), p, dl)
    assert L.mi_deflate_batch_dict_max_blocks(total, len(items), p, 0) == L.mi_deflate_batch_max_blocks(total, len(items), p)
    assert lz.deflate_batch_max_blocks(total, len(items), p, dict_bytes=dl) == L.mi_deflate_batch_dict_max_blocks(total, len(items), p, dl)
    for n in (0, 1, block - u, block - u + 1, 3 * block):          # incompressible items: every block stored
        for c in D.CONTAINERS:
            assert len(D.expected_stream(D.noise(n, seed=21), zd, block, c)[0]) <= L.mi_deflate_batch_dict_bound_bytes(n, p, lz.CONTAINERS[c], dl)
            assert L.mi_deflate_batch_dict_bound_bytes(n, p, lz.CONTAINERS[c], 0) == L.mi_deflate_batch_bound_bytes(n, p, lz.CONTAINERS[c])
