"""The items of the batched-inflate tests against stock zlib, and the parts of the feature that need no device: the three
exported symbols and the argument checks the Python wrappers make before they touch one."""
import ctypes as C
import os
import zlib

import pytest

import inflate_batch_cases as K
from compression_algorithms_amd import _lib, lz

NEW = ("mi_inflate_batch_dev", "mi_inflate_batch_size_dev", "mi_inflate_batch")


@pytest.mark.parametrize("container", K.CONTAINERS)
def test_clean_items_inflate_with_stock_zlib(container):
    items = K.clean_items(container)
    names = [n for n, _, _ in items]
    for must in ("empty", "one_byte", "stored_only", "crafted_fixed_258_32768", "crafted_dynamic_15_bit_codes", "mix_level1",
                 "mix_level6", "mix_level9", "far_last_match", "run"):
        assert must in names
    for name, item, want in items:
        out, eof, rest = K.stock_inflate(item, container)
        assert out == want and eof and rest == b"", name
    assert ("rich_header" in names) == (container == "gzip")


def test_the_far_match_item_ends_with_distance_32768():
    name, raw, want = [c for c in K.clean_raw() if c[0] == "far_last_match"][0]
    assert 40_000 < len(want) < 41_000 and want[-258:] == want[-258 - 32768:-32768]
    name, raw, want = [c for c in K.clean_raw() if c[0] == "stored_only"][0]
    assert raw[:5] == b"\x00\xff\xff\x00\x00" and raw[5 + 65535: 5 + 65535 + 5] == b"\x00\x00\x00\xff\xff"      # 65 535, then LEN = 0


def test_refusals_are_refused_by_stock_zlib_too():
    lax = []
    for name, container, item, status in K.refusals():
        assert status == K.CORRUPT
        try:
            out, eof, rest = K.stock_inflate(item, container)
        except zlib.error:
            continue
        if not eof:
            continue                                         # zlib wants more input: a truncated stream
        assert rest != b"", f"{name}: stock zlib accepts this item whole"
        lax.append(name)                                     # the stream ended before the item did: zlib hands the rest back
    assert sorted(lax) == sorted(K.ZLIB_IS_LAXER)


def test_refusal_list_holds_what_the_contract_names():
    names = {r[0] for r in K.refusals()}
    for must in ("crc_one_bit", "adler_off_by_one", "isize_off_by_one", "trailing_byte_gzip", "two_gzip_members", "cut_inside_block",
                 "cut_inside_header", "cut_inside_trailer", "bfinal_never_set") + K.FROM_REJECTS:
        assert must in names
    assert K.CHECKSUM <= names and len(names) == len(K.refusals())


def test_library_exports_the_batch_entry_points():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in _lib.EXPORTS and hasattr(L, s), s
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi_codec.h")).read()
    for s in NEW:
        assert f"mi_status {s}(" in hdr


def test_wrappers_check_lengths_before_touching_a_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the wrapper asked for a device before it checked its arguments")
    monkeypatch.setattr(lz, "default_context", no_device)
    buf = b"".join(i for _, i, _ in K.clean_items("raw")[:3])
    with pytest.raises(ValueError):
        lz.inflate_batch((buf, []), container="raw")                          # count + 1 offsets: at least one
    with pytest.raises(ValueError):
        lz.inflate_batch((buf, [0, 5, 3]), container="raw")                   # decreasing
    with pytest.raises(ValueError):
        lz.inflate_batch((buf, [0, 2, len(buf) + 1]), container="raw")        # past the buffer
    with pytest.raises(ValueError):
        lz.inflate_batch_sizes((buf, [0, 5, 3]), container="raw")
    with pytest.raises(ValueError):
        lz.inflate_batch([b"\x03\x00", b"\x03\x00"], container="raw", caps=[16])
    with pytest.raises(ValueError):
        lz.inflate_batch((buf, [0, 2, 4]), container="raw", caps=[16, 16, 16])
