"""Mode Z's parse 1 (include/mi_codec.h: one-step lazy matching, matches up to 255 bytes) restated on the CPU: a helper
module, not a conftest.  The rule in Python over the oracle's candidates, the expected streams of compress_z, compress_bgzf
and the batched deflate built from those tokens with the oracle's record writer, and the fixed list of inputs the CPU and
the GPU file share.  Nothing here touches the GPU library."""
import functools
import os
import struct
import zlib

import numpy as np

import bgzf_cases
import dict_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W = 1 << 15
MAX_LEN = 255
NONE = 0xFFFF                                                  # the oracle's "no candidate" is 0xFFFFFFFF; no position reaches 0xFFFF
CONTAINERS = ("raw", "zlib", "gzip")
BLOCKS = (65536, 65280, 4096, 1000)
BGZF_BLOCKS = (65280, 4096, 1000)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def len0(buf):
    """len0(p) for 0 <= p <= n of one block: the common prefix of in[cand[p]..] and in[p..], at most min(255, n - p), 0 below
    3 and where the literal rule rejects the candidate; len0(n) = 0 -> (int array of n + 1, the candidates)"""
    from oracle import orc
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = a.size
    cand = orc.find_all(a, 15, 20, True).astype(np.int64)
    p = np.arange(n, dtype=np.int64)
    lim = np.minimum(MAX_LEN, n - p)
    out = np.zeros(n + 1, dtype=np.int64)
    idx = np.flatnonzero((cand < NONE) & (p - cand < W - 1))
    k = 0
    while idx.size:
        live = lim[idx] > k                                    # no byte at or past n is compared
        out[idx[~live]] = k
        idx = idx[live]
        eq = a[cand[idx] + k] == a[idx + k]
        out[idx[~eq]] = k
        idx = idx[eq]
        k += 1
    out[out < 3] = 0
    return out, cand


@functools.lru_cache(maxsize=None)
def walk(buf, skip=0):
    """the parse of one block (bytes) -> ((position, length, distance), ...) with length 0 for a literal"""
    n = len(buf)
    l0, cand = len0(buf)
    eff = l0[:n].copy()
    eff[l0[1:] > l0[:n]] = 0                                   # the longer match one byte on wins
    out, p = [], skip
    while p < n:
        ln = int(eff[p])
        out.append((p, ln, p - int(cand[p]) if ln else 0))
        p += ln if ln else 1
    return tuple(out)


def tokens(buf, skip=0):
    """the oracle's byte tokens {0, c} / {1, dlo, dhi, len} of one block under parse 1"""
    buf = bytes(buf)
    tok = bytearray()
    for p, ln, d in walk(buf, skip):
        tok += bytes([1, d & 255, d >> 8, ln]) if ln else bytes([0, buf[p]])
    return np.frombuffer(bytes(tok), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def stream_tokens(data, block):
    """(token bytes, per-block sizes) of the whole buffer, in the form orc.defz_stream takes"""
    toks = [tokens(data[a:a + block]) for a in range(0, len(data), block)]
    sizes = np.array([t.size for t in toks] or [0], dtype=np.uint64)
    return (np.concatenate(toks) if toks else np.zeros(0, dtype=np.uint8)), sizes[: len(toks)] if toks else sizes


# ---- expected streams ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_z(data, block, container):
    """what compress_z(data, params(block=block, parse=1), container) must write -> (bytes, block table)"""
    from oracle import orc
    out, bits = orc.defz_stream(data, block, container, tokens=stream_tokens(data, block))
    return bytes(out), bits


@functools.lru_cache(maxsize=None)
def expected_bgzf(data, block):
    """bgzf_cases.expected_bgzf over the parse-1 records -> (bytes, member table in bits)"""
    raw, bits = expected_z(data, block, "raw")
    out, table = bytearray(), []
    for b in range(len(bits) - 1):
        rec = raw[bits[b] // 8: bits[b + 1] // 8]
        part = data[b * block:(b + 1) * block]
        table.append(8 * len(out))
        out += bgzf_cases.HEAD + struct.pack("<H", len(rec) + 28 - 1) + rec + b"\x03\x00"
        out += struct.pack("<II", zlib.crc32(part), len(part))
    table.append(8 * len(out))
    return bytes(out + bgzf_cases.EOF), table


@functools.lru_cache(maxsize=None)
def expected_item(item, zdict, block, container):
    """dict_cases.expected_stream under parse 1: the stream of `item` behind the preset dictionary `zdict`"""
    from oracle import orc
    u = dict_cases.used(zdict, block)
    head = item[:block - len(u)]
    rec = orc.defz_record(tokens(u + head, len(u)), head)[0] if head else b""
    rest = expected_z(item[len(head):], block, "raw")[0]                      # the later blocks' records and 03 00
    if container == "raw" or not u:
        hdr = b"" if container == "raw" else b"\x78\x9c"
    else:
        hdr = b"\x78\xbb" + struct.pack(">I", zlib.adler32(zdict))
    return hdr + rec + rest + (struct.pack(">I", zlib.adler32(item)) if container == "zlib" else b"")


def inflate(stream, container, zdict=None):
    """stock zlib / gzip on a whole stream (complete, nothing behind it) -> bytes"""
    if container == "gzip":
        import gzip
        return gzip.decompress(stream)
    return dict_cases.stock_inflate(stream, container, zdict)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_text():
    with open(os.path.join(GOLDEN, "enwik_like_300k.bin"), "rb") as f:
        return f.read()


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def mixed():
    t = golden_text()
    return t[:2000] + bytes(700) + t[5000:5063] + b"A" * 1000 + t[9000:11000] + noise(2000, 3) + t[20000:22000]


MATCH_AT = 64 * 9 + 63                                         # where the 255-byte match of "chunk_offset_63" starts


def chunk_offset_63():
    """a match of exactly 255 bytes that starts at offset 63 of a 64-position chunk (its source 255 random bytes at the
    front; the byte behind the copy differs), so that the next two chunks are entered at offsets 254 and 190"""
    r = noise(256, 21)
    front = r[:255] + bytes([r[255] ^ 1])
    fill = noise(MATCH_AT - len(front), 22)
    return front + fill + r[:255] + bytes([r[255] ^ 2]) + noise(200, 23)


def ends_at_n():
    """the last token is a match whose last byte is the block's last byte"""
    r = noise(120, 24)
    return r + noise(333, 25) + r[:100]


RISING_AT = 400                                                # where the run of deferring positions of "rising" starts


def rising():
    """len0 strictly rising over four consecutive positions (4 < 5 < 8 < 21): three positions in a row give way to the next.
    The final `a b c d E` meets `a b c d`, `b c d E[:2]`, `c d E[:6]` and `d E[:20]`, each cut off by a byte that differs;
    where a word occurs twice the oracle's candidate is the earlier copy, so the longest comes first (the CPU test checks len0)"""
    e = noise(40, 31)
    a, b, c, d = (bytes([v]) for v in (0xA1, 0xB2, 0xC3, 0xD4))
    sep = lambda k: noise(37, 40 + k)
    stop = lambda x: bytes([x ^ 0x55])
    head = (sep(0) + d + e[:20] + stop(e[20]) + sep(1) + c + d + e[:6] + stop(e[6]) + sep(2) + b + c + d + e[:2] + stop(e[2])
            + sep(3) + a + b + c + d + stop(e[0]) + sep(4))
    head += noise(RISING_AT - len(head), 50)
    return head + a + b + c + d + e + noise(50, 51)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> bytes"""
    t = golden_text()
    out = {"text": t[:200_000], "zeros": bytes(70_000), "period3": (b"abc" * 1667)[:5000], "mixed": mixed(),
           "chunk_offset_63": chunk_offset_63(), "ends_at_n": ends_at_n(), "rising": rising()}
    for n in (1, 2, 3, 4, 5):
        out[f"zeros_{n}"] = bytes(n)
        out[f"text_{n}"] = t[100:100 + n]
    return out


def batch_items():
    """the mixed list of the batch tests: an empty item, one byte, items around one and two blocks of 1000, zeros, text"""
    t = golden_text()
    return [b"", t[7:8], t[100:1099], t[2000:3000], t[4000:5001], t[6000:7999], t[9000:11000], t[12000:14001], bytes(3000),
            t[20000:24567], (b"abc" * 300)[:777], mixed()[:5000]]
