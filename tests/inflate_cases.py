"""Streams for the inflate tests (a helper module, not a conftest).

  * a small RFC 1951 bit writer: tokens -> stored / fixed-Huffman / dynamic-Huffman blocks (the dynamic header spells every
    code length out with a flat 4-bit code-length code: no run-length symbols, any length set can be written);
  * foreign streams: stock zlib with Z_FULL_FLUSH every `seg` input bytes gives byte-aligned segments that refer to nothing
    earlier, and the table of their bit offsets;
  * the zlib / gzip framing around raw segments;
  * the fixed list of streams a decoder must refuse.

Tokens are (byte,) for a literal and (length, distance) for a match, as in rfc1951_tokens.py.
"""
import struct
import zlib

import numpy as np

from rfc1951_tokens import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA

from compression_algorithms_amd import synth

PRIMARY_LUT_BITS = 10            # INF_LL_BITS of csrc/inflate.hip (test_inflate_cpu.py checks the two agree)
SYNC = b"\x00\x00\xff\xff"       # what is left of an empty stored block once its 3 header bits and the padding are written
CLOSE = b"\x03\x00"              # BFINAL = 1, fixed, end-of-block


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.nacc = bytearray(), 0, 0

    def put(self, v, k):                         # k bits of v, LSB first
        self.acc |= (v & ((1 << k) - 1)) << self.nacc
        self.nacc += k
        while self.nacc >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nacc -= 8

    def put_code(self, code, k):                 # a Huffman code: MSB first
        for i in range(k - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.nacc:
            self.put(0, 8 - self.nacc)

    def bytes(self):
        assert self.nacc == 0
        return bytes(self.out)


def canonical(lengths):
    """RFC 1951 3.2.2: symbol -> code"""
    mx = max(lengths)
    cnt = [0] * (mx + 2)
    for l in lengths:
        if l:
            cnt[l] += 1
    code, nxt = 0, [0] * (mx + 2)
    for l in range(1, mx + 1):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _len_sym(L):
    i = max(k for k in range(29) if LEN_BASE[k] <= L and (k < 28 or L == 258))
    if L == 258:
        i = 28
    return i, L - LEN_BASE[i]


def _dist_sym(d):
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, d - DIST_BASE[i]


def _put_tokens(w, tokens, ll, dl):
    lc, dc = canonical(ll), canonical(dl) if any(dl) else [0] * len(dl)
    for t in tokens:
        if len(t) == 1:
            w.put_code(lc[t[0]], ll[t[0]])
        else:
            i, x = _len_sym(t[0])
            w.put_code(lc[257 + i], ll[257 + i])
            w.put(x, LEN_EXTRA[i])
            j, y = _dist_sym(t[1])
            assert dl[j], "the distance code has no such symbol"
            w.put_code(dc[j], dl[j])
            w.put(y, DIST_EXTRA[j])
    w.put_code(lc[256], ll[256])


def put_fixed(w, tokens, final=0):
    w.put(final, 1)
    w.put(1, 2)
    _put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def put_dynamic(w, tokens, ll, dl, final=0):
    """ll: 257..286 literal/length code lengths, dl: 1..30 distance code lengths, written one by one"""
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(ll) - 257, 5)
    w.put(len(dl) - 1, 5)
    w.put(19 - 4, 4)
    cl = [4] * 16 + [0, 0, 0]                    # lengths 0..15 as 4-bit codes: the code is the length itself
    for s in CL_ORDER:
        w.put(cl[s], 3)
    for l in list(ll) + list(dl):
        w.put_code(l, 4)
    _put_tokens(w, tokens, list(ll), list(dl))


def put_stored(w, data, final=0):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(~len(data) & 0xFFFF, 16)
    w.out += data


def put_sync(w):
    put_stored(w, b"")


def flat_ll():
    """a complete literal/length code over all 286 symbols: 226 of 8 bits, 60 of 9"""
    return [8] * 226 + [9] * 60


def flat_dl():
    """a complete distance code over all 30 symbols: 2 of 4 bits, 28 of 5"""
    return [4, 4] + [5] * 28


def expand(tokens, before=b""):
    """the bytes the tokens stand for, behind `before`"""
    out = bytearray(before)
    for t in tokens:
        if len(t) == 1:
            out.append(t[0])
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out[len(before):])


# ---- crafted single segments: (name, raw segment + closing 03 00, expected bytes) ---------------------------------------
def crafted():
    rng = np.random.default_rng(11)
    lit = [(int(b),) for b in rng.integers(0, 256, 32768, dtype=np.uint8)]
    out = {}
    # stock zlib never emits a distance above 32 506: lengths 3..258 at distance 32 768, and the short distances
    tok = lit + [(258, 32768), (3, 32768), (257, 1), (258, 1), (4, 32767), (10, 24577), (11, 24576), (227, 2), (258, 3)]
    w = BitWriter()
    put_fixed(w, tok)
    put_sync(w)
    out["fixed_258_32768"] = (w.bytes() + CLOSE, expand(tok))
    # a dynamic block with ONE distance code (length 1: RFC 1951 3.2.7), here code 29
    tok = lit + [(258, 32768), (100, 24577)]
    w = BitWriter()
    put_dynamic(w, tok, flat_ll(), [0] * 29 + [1])
    put_sync(w)
    out["dynamic_single_distance"] = (w.bytes() + CLOSE, expand(tok))
    # a dynamic block whose distance lengths are all zero (HDIST = 1, length 0) and that holds literals only
    w = BitWriter()
    put_dynamic(w, lit[:5000], flat_ll(), [0])
    put_sync(w)
    out["dynamic_no_distance"] = (w.bytes() + CLOSE, expand(lit[:5000]))
    # 15-bit codes in both alphabets: a chain 1, 2, ..., 14, 15, 15 over the symbols that are used
    chain = list(range(1, 15)) + [15, 15]
    ll = [0] * 286
    for s, l in zip([65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 256, 257, 285, 76, 77], chain):
        ll[s] = l
    dl = [0] * 30
    for s, l in zip(range(16), chain):
        dl[s] = l
    tok = [(65 + k,) for k in range(11)] + [(76,), (77,)] * 20 + [(3, DIST_BASE[j]) for j in range(4)] * 5
    tok += [(258, 13 + k) for k in range(3)] + [(3, DIST_BASE[j]) for j in (14, 15, 13, 12) if DIST_BASE[j] <= 60]
    w = BitWriter()
    put_dynamic(w, tok, ll, dl)
    put_sync(w)
    out["dynamic_15_bit_codes"] = (w.bytes() + CLOSE, expand(tok))
    # all three block types in one segment, the stored one of 65 535 bytes
    st = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    w = BitWriter()
    put_fixed(w, lit[:100])
    put_stored(w, st)
    put_dynamic(w, lit[:300] + [(258, 400)], flat_ll(), flat_dl())
    put_fixed(w, [(20, 30000)])
    put_sync(w)
    exp = expand(lit[:100]) + st
    exp += expand(lit[:300] + [(258, 400)], exp)
    exp += expand([(20, 30000)], exp)
    out["three_types"] = (w.bytes() + CLOSE, bytes(exp))
    return out


# ---- foreign streams: stock zlib cut with Z_FULL_FLUSH ---------------------------------------------------------------
def zlib_segments(data, level, seg):
    """-> (raw DEFLATE bytes, table): table[s] is the bit offset of segment s, table[-1] where the closing 03 00 starts"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out, table = bytearray(), [0]
    for i in range(0, len(data), seg):
        out += c.compress(data[i:i + seg])
        out += c.flush(zlib.Z_FULL_FLUSH)
        table.append(8 * len(out))
    tail = c.flush(zlib.Z_FINISH)
    assert tail == CLOSE, tail.hex()
    return bytes(out) + tail, table


GZIP_PLAIN = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
# FEXTRA (6 bytes) + FNAME + FCOMMENT + FHCRC (not verified by the decoder: any two bytes)
GZIP_RICH = bytes([0x1F, 0x8B, 8, 2 | 4 | 8 | 16, 1, 2, 3, 4, 2, 3]) + struct.pack("<H", 6) + b"AB\x02\x00xy" + b"name.txt\0" + b"a comment\0" + b"\x12\x34"


def frame(raw, table, data, container, gzip_header=GZIP_PLAIN):
    """raw segments + table -> the stream in `container` and its table (shifted by the header)"""
    if container == "raw":
        return raw, list(table)
    if container == "zlib":
        head, tail = b"\x78\x9c", struct.pack(">I", zlib.adler32(data))
    else:
        head, tail = gzip_header, struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
    return head + raw + tail, [t + 8 * len(head) for t in table]


def mix(n, seed=5):
    """text / random / zeros / text with rare bytes, in stretches of 20 000 to 90 000 bytes"""
    rng = np.random.default_rng(seed)
    parts, total, k = [], 0, 0
    while total < n:
        m = int(rng.integers(20_000, 90_000))
        kind = k % 4
        if kind == 0:
            p = synth.enwik_like(m, seed=seed + k).numpy().tobytes()
        elif kind == 1:
            p = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
        elif kind == 2:
            p = bytes(m)
        else:
            t = bytearray(synth.enwik_like(m, seed=seed + k).numpy().tobytes())
            for v in range(128, 256):                       # every high byte value once or twice: long codes
                t[int(rng.integers(0, m))] = v
            p = bytes(t)
        parts.append(p)
        total += m
        k += 1
    return b"".join(parts)[:n]


def short_words(n, seed=7):
    """every 1 000 bytes a fresh 5-byte unit over and over: a handful of tokens per segment, for which zlib picks fixed blocks"""
    rng = np.random.default_rng(seed)
    return b"".join(rng.integers(0, 256, 5, dtype=np.uint8).tobytes() * 200 for _ in range((n + 999) // 1000))[:n]


def foreign_inputs():
    return {
        "text": synth.enwik_like(700_000, seed=4).numpy().tobytes(),
        "mix": mix(900_000),
        "zeros": bytes(400_000),                             # length 258 over and over
        "short": short_words(30_000),
    }


FOREIGN_LEVELS = (1, 6, 9)
FOREIGN_SEGS = (65536, 32768, 1000)


def foreign_set():
    """[(name, data, level, seg)]: every input x level x segment size, and one 1 MiB segment size"""
    inp = foreign_inputs()
    out = [(f"{k}-l{lv}-s{seg}", d, lv, seg) for k, d in inp.items() for lv in FOREIGN_LEVELS for seg in FOREIGN_SEGS
           if not (k == "short" and seg != 1000)]
    big = synth.enwik_like(2_500_000, seed=6).numpy().tobytes()
    out.append(("text-l6-s1048576", big, 6, 1 << 20))
    return out


# ---- streams a decoder must refuse ------------------------------------------------------------------------------------
def rejects():
    """[(name, container, block, stream, table, n, verify, status)]: status 8 = MI_ERR_CORRUPT, 1 = MI_ERR_ARG; `table` may
    be handed to the device entry point as it is (the host entry point would refuse some of them before any copy)"""
    data = synth.enwik_like(150_000, seed=12).numpy().tobytes()
    n = len(data)
    raw, table = zlib_segments(data, 6, 65536)
    R = []

    def add(name, container, stream, tab, nn=n, block=65536, verify=True, status=8):
        R.append((name, container, block, bytes(stream), list(tab), nn, verify, status))

    add("truncated_stream", "raw", raw[:len(raw) // 2], table)
    add("table_past_end", "raw", raw, table[:-1] + [8 * len(raw) + 64])
    add("table_not_multiple_of_8", "raw", raw, [table[0], table[1] + 3] + table[2:])
    add("table_decreasing", "raw", raw, [table[0], table[2], table[1], table[3]])
    add("btype_11", "raw", b"\x06" + raw[1:], table)
    w = BitWriter()
    put_stored(w, data[:1000])
    put_sync(w)
    good = w.bytes() + CLOSE
    badn = bytearray(good)
    badn[3] ^= 0x01                                            # NLEN
    add("nlen_mismatch", "raw", badn, [0, 8 * (len(good) - 2)], nn=1000)
    w = BitWriter()
    put_dynamic(w, [(65,)] * 10, [8] * 226 + [9] * 59 + [8], flat_dl())      # one 9 became 8: Kraft sum above 1
    put_sync(w)
    s = w.bytes() + CLOSE
    add("oversubscribed_lengths", "raw", s, [0, 8 * (len(s) - 2)], nn=10)
    w = BitWriter()
    put_dynamic(w, [(65,)] * 10, [8] * 226 + [9] * 59 + [0], flat_dl())      # one code missing: incomplete
    put_sync(w)
    s = w.bytes() + CLOSE
    add("incomplete_lengths", "raw", s, [0, 8 * (len(s) - 2)], nn=10)
    w = BitWriter()
    put_fixed(w, [(65,), (66,), (67,), (5, 4)])                              # reaches one byte before the segment
    put_sync(w)
    s = w.bytes() + CLOSE
    add("distance_before_segment", "raw", s, [0, 8 * (len(s) - 2)], nn=8)
    # the second segment starts with a match that would be fine in one stream: it reaches into segment 0
    w = BitWriter()
    put_fixed(w, [(int(b),) for b in data[:64]])
    put_sync(w)
    cut = len(w.out)
    put_fixed(w, [(64, 64)])
    put_sync(w)
    s = w.bytes() + CLOSE
    assert zlib.decompress(s, -15) == data[:64] * 2
    add("distance_into_previous_segment", "raw", s, [0, 8 * cut, 8 * (len(s) - 2)], nn=128, block=64)
    w = BitWriter()
    put_fixed(w, [(int(b),) for b in data[:99]])
    put_sync(w)
    s = w.bytes() + CLOSE
    add("segment_one_byte_short", "raw", s, [0, 8 * (len(s) - 2)], nn=100)
    w = BitWriter()
    put_fixed(w, [(int(b),) for b in data[:101]])
    put_sync(w)
    s = w.bytes() + CLOSE
    add("segment_one_byte_long", "raw", s, [0, 8 * (len(s) - 2)], nn=100)
    w = BitWriter()                                            # BFINAL = 1 in the first of two segments
    put_fixed(w, [(int(b),) for b in data[:64]], final=1)
    w.align()
    cut = len(w.out)
    put_fixed(w, [(int(b),) for b in data[64:128]])
    put_sync(w)
    s = w.bytes() + CLOSE
    add("bfinal_inside_segment", "raw", s, [0, 8 * cut, 8 * (len(s) - 2)], nn=128, block=64)
    # the frame
    z, zt = frame(raw, table, data, "zlib")
    g, gt = frame(raw, table, data, "gzip")
    add("wrong_adler32", "zlib", z[:-1] + bytes([z[-1] ^ 1]), zt)
    add("wrong_adler32_unverified", "zlib", z[:-1] + bytes([z[-1] ^ 1]), zt, verify=False, status=0)
    add("wrong_crc32", "gzip", g[:-8] + bytes([g[-8] ^ 1]) + g[-7:], gt)
    add("wrong_crc32_unverified", "gzip", g[:-8] + bytes([g[-8] ^ 1]) + g[-7:], gt, verify=False, status=0)
    add("wrong_isize", "gzip", g[:-1] + bytes([g[-1] ^ 1]), gt)
    add("wrong_isize_unverified", "gzip", g[:-1] + bytes([g[-1] ^ 1]), gt, verify=False)
    add("bad_fcheck", "zlib", b"\x78\x9d" + z[2:], zt)
    add("fdict_set", "zlib", b"\x78\xbb" + z[2:], zt)          # 0x78BB % 31 == 0 with FDICT
    add("trailing_bytes", "gzip", g + b"\x00", gt)
    add("trailing_bytes_raw", "raw", raw + b"\x00", table)
    add("table_starts_inside_header", "gzip", g, [gt[0] - 8] + gt[1:])
    add("unknown_container", 3, raw, table, status=1)
    add("block_zero", "raw", raw, table, block=0, status=1)
    return R
