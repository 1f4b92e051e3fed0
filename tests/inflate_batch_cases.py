"""Items for the batched-inflate tests (a helper module, not a conftest): complete raw DEFLATE streams with the bytes they
stand for, their framing as raw / zlib / gzip items, and the fixed list of items a decoder must refuse, each with the
verdict expected.  Builders only; everything is deterministic."""
import functools
import struct
import zlib

import numpy as np

import inflate_cases as ic

OK, ARG, CAPACITY, CORRUPT = 0, 1, 4, 8
CONTAINERS = ("raw", "zlib", "gzip")
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}


def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def frame(raw, data, container, gzip_header=ic.GZIP_PLAIN):
    """a complete raw DEFLATE stream of `data` as an item of `container`"""
    if container == "raw":
        return raw
    if container == "zlib":
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))
    return gzip_header + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


# GZIP_RICH's optional fields (FEXTRA, FNAME, FCOMMENT, FHCRC) with the header CRC stock zlib checks (the decoder does not)
RICH = ic.GZIP_RICH[:-2] + struct.pack("<H", zlib.crc32(ic.GZIP_RICH[:-2]) & 0xFFFF)


def stock_inflate(stream, container):
    """stock zlib on one item -> (bytes, reached the end of the stream, bytes left over behind it); raises zlib.error"""
    d = zlib.decompressobj(WBITS[container])
    out = d.decompress(stream) + d.flush()
    return out, d.eof, d.unused_data


def small_text(n, seed):
    return ic.synth.enwik_like(n, seed=seed).numpy().tobytes()


@functools.lru_cache(maxsize=None)
def clean_raw():
    """[(name, complete raw DEFLATE stream, the bytes it stands for)]"""
    rng = np.random.default_rng(23)
    out = [("empty", b"\x03\x00", b""), ("one_byte", deflate(b"A"), b"A")]
    # stored blocks only: the longest one, an empty one, a short last one
    big, tail = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes(), rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    w = ic.BitWriter()
    ic.put_stored(w, big)
    ic.put_stored(w, b"")
    ic.put_stored(w, tail, final=1)
    out.append(("stored_only", w.bytes(), big + tail))
    for name, (stream, want) in ic.crafted().items():
        out.append(("crafted_" + name, stream, want))
    mixed = ic.mix(100_000)
    for level in (1, 6, 9):                                  # several dynamic blocks, matches across block boundaries
        out.append((f"mix_level{level}", deflate(mixed, level), mixed))
    # about 40 KB whose LAST match has distance 32 768: out of a 4 KiB ring, read back from the output buffer
    tok = [(int(b),) for b in rng.integers(0, 256, 40_000, dtype=np.uint8)] + [(258, 32768)]
    w = ic.BitWriter()
    ic.put_fixed(w, tok, final=1)
    w.align()
    out.append(("far_last_match", w.bytes(), ic.expand(tok)))
    out.append(("run", deflate(b"a" * 70_000), b"a" * 70_000))          # distance 1, length 258
    out.append(("text_2k", deflate(small_text(2000, 31)), small_text(2000, 31)))
    return out


def clean_items(container):
    """[(name, item, expected bytes)] in `container`; gzip adds an item with every optional header field"""
    out = [(n, frame(raw, want, container), want) for n, raw, want in clean_raw()]
    if container == "gzip":
        t = small_text(3000, 32)
        out.append(("rich_header", frame(deflate(t), t, "gzip", RICH), t))
    return out


SMALL = ("empty", "one_byte", "text_2k")


def small_items(container, count):
    """`count` items: the small clean ones over and over"""
    base = [c for c in clean_items(container) if c[0] in SMALL]
    return [base[i % len(base)] for i in range(count)]


# from inflate_cases.rejects(): the streams that mean something as ONE whole item (no table, no length given)
FROM_REJECTS = ("truncated_stream", "btype_11", "nlen_mismatch", "oversubscribed_lengths", "incomplete_lengths",
                "distance_before_segment", "bfinal_inside_segment", "wrong_adler32", "wrong_crc32", "wrong_isize", "bad_fcheck",
                "fdict_set", "trailing_bytes", "trailing_bytes_raw")
CHECKSUM = {"wrong_adler32", "wrong_crc32", "crc_one_bit", "adler_off_by_one"}       # what verify=False and the size pass let through


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, container, item, status)]: every one MI_ERR_CORRUPT — none of them is meant to fault"""
    R = []
    for name, container, block, stream, table, n, verify, status in ic.rejects():
        if name in FROM_REJECTS:
            R.append((name, container, stream, CORRUPT))
    assert [r[0] for r in R] == [n for n in FROM_REJECTS], "inflate_cases.rejects() changed"
    t = small_text(5000, 33)
    raw = deflate(t)
    g, z = frame(raw, t, "gzip"), frame(raw, t, "zlib")

    def flip(b, at, mask=1):
        b = bytearray(b)
        b[at] ^= mask
        return bytes(b)

    R.append(("crc_one_bit", "gzip", flip(g, len(g) - 8, 0x10), CORRUPT))
    R.append(("adler_off_by_one", "zlib", z[:-4] + struct.pack(">I", (zlib.adler32(t) + 1) & 0xFFFFFFFF), CORRUPT))
    R.append(("isize_off_by_one", "gzip", g[:-4] + struct.pack("<I", len(t) + 1), CORRUPT))
    R.append(("trailing_byte_raw", "raw", raw + b"\x00", CORRUPT))
    R.append(("trailing_byte_zlib", "zlib", z + b"\x00", CORRUPT))
    R.append(("trailing_byte_gzip", "gzip", g + b"\x00", CORRUPT))
    R.append(("two_gzip_members", "gzip", g + g, CORRUPT))
    R.append(("cut_inside_block", "raw", raw[:len(raw) // 2], CORRUPT))
    R.append(("cut_inside_block_gzip", "gzip", g[:len(g) // 2], CORRUPT))
    rich = frame(raw, t, "gzip", RICH)
    R.append(("cut_inside_header", "gzip", rich[:20], CORRUPT))
    R.append(("cut_inside_plain_header", "gzip", g[:6], CORRUPT))
    R.append(("cut_inside_trailer", "gzip", g[:-3], CORRUPT))
    R.append(("cut_inside_trailer_zlib", "zlib", z[:-2], CORRUPT))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    R.append(("bfinal_never_set", "raw", c.compress(t) + c.flush(zlib.Z_SYNC_FLUSH), CORRUPT))
    R.append(("zero_bytes", "raw", b"", CORRUPT))
    return R


# stock zlib is laxer than the item contract here: it stops at the end of the first stream and hands the rest back
ZLIB_IS_LAXER = ("trailing_bytes", "trailing_bytes_raw", "bfinal_inside_segment", "trailing_byte_raw", "trailing_byte_zlib",
                 "trailing_byte_gzip", "two_gzip_members")


def skewed(n_small=2000, n_big=3):
    """[(item, expected)] raw: n_small items of about 1 KB mixed with n_big of about 1 MiB"""
    rng = np.random.default_rng(29)
    text = small_text(1 << 20, 34)
    small = [text[a:a + 1000 + 7 * (k % 5)] for k, a in enumerate(rng.integers(0, (1 << 20) - 2000, 8))]
    small = [(deflate(s), s) for s in small]
    bigs = [bytes(text[k:]) + bytes(text[:k]) for k in range(n_big)]
    bigs = [(deflate(b, 1), b) for b in bigs]
    out = [small[i % len(small)] for i in range(n_small)]
    for k, b in enumerate(bigs):
        out.insert((k + 1) * n_small // (n_big + 1), b)
    return out
