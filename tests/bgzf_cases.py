"""Streams for the BGZF tests (a helper module, not a conftest): the expected stream built from the CPU oracle's mode-Z
records, a serial index walker in pure Python (the reference for the GPU index), foreign BGZF written with stock zlib —
several DEFLATE blocks per member, stored blocks, empty members, extra subfields, BGZF of a BGZF file (byte-exact decoy
headers inside stored blocks) — and the fixed list of streams the decoder must refuse."""
import gzip
import os
import struct
import zlib

import numpy as np

import defz_cases as D
import inflate_cases as ic

BGZF_BLOCK = 65280
BGZF_MAX_BLOCK = 65498
BLOCKS = (65280, 65498, 4096, 257)
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def member(deflate, payload, extra_before=b"", extra_after=b""):
    """one BGZF member around a complete raw DEFLATE stream of `payload`; extra_*: whole subfields around 'BC'"""
    xlen = len(extra_before) + 6 + len(extra_after)
    total = 12 + xlen + len(deflate) + 8
    assert total <= 65536 and len(payload) <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC\x02\x00" + struct.pack("<H", total - 1)
            + extra_after + deflate + struct.pack("<II", zlib.crc32(payload), len(payload)))


def expected_bgzf(data, block=BGZF_BLOCK):
    """the stream mi_bgzf_encode_dev must write -> (bytes, member table in bits): the records of oracle/orc_defz.c, each
    behind the 18-byte header and in front of 03 00, CRC-32 and ISIZE, then the EOF member"""
    from oracle import orc
    data = bytes(data)
    raw, bits = orc.defz_stream(data, block, "raw")
    out, table = bytearray(), []
    for b in range(len(bits) - 1):
        rec = raw[bits[b] // 8: bits[b + 1] // 8]
        table.append(8 * len(out))
        out += HEAD + struct.pack("<H", len(rec) + 28 - 1) + rec + b"\x03\x00"
        out += struct.pack("<II", zlib.crc32(data[b * block:(b + 1) * block]), len(data[b * block:(b + 1) * block]))
    table.append(8 * len(out))
    return bytes(out + EOF), table


def bound(n, block):
    """mi_bgzf_bound_bytes: per block mode Z's per-block bound, 03 00 and the 26 bytes of header and trailer; the EOF member"""
    nb = (n + block - 1) // block
    last = n - (nb - 1) * block if nb else 0
    mem = lambda b: b + 5 * ((b + 65534) // 65535) + 5 + 2 + 26
    return ((nb - 1) * mem(block) + mem(last) if nb else 0) + 28


def own_cases():
    """name -> bytes: the inputs of the issue's CPU check"""
    rng = np.random.default_rng(5)
    return {
        "golden300k": open(os.path.join(GOLDEN, "enwik_like_300k.bin"), "rb").read(),
        "random": rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes(),
        "zeros": bytes(200_000),
        "one_byte": b"\x41",
        "empty": b"",
    }


def one_block(block):
    return D.text(block, seed=6)


class Corrupt(ValueError):
    pass


def parse_member(buf, pos, end=None):
    """the member at `pos` inside buf[pos:end] -> (total bytes, ISIZE, XLEN) or Corrupt: the rule of include/mi_codec.h"""
    end = len(buf) if end is None else end
    if end - pos < 28:
        raise Corrupt("shorter than a member")
    if buf[pos:pos + 4] != b"\x1f\x8b\x08\x04":
        raise Corrupt("magic, CM or FLG")
    xlen = buf[pos + 10] | (buf[pos + 11] << 8)
    if 12 + xlen + 2 + 8 > end - pos:
        raise Corrupt("XLEN past the stream")
    q, bsize = 0, None
    while q + 4 <= xlen and bsize is None:
        f = pos + 12 + q
        slen = buf[f + 2] | (buf[f + 3] << 8)
        if buf[f:f + 2] == b"BC" and slen == 2 and q + 6 <= xlen:
            bsize = buf[f + 4] | (buf[f + 5] << 8)
        q += 4 + slen
    if bsize is None:
        raise Corrupt("no BC subfield")
    total = bsize + 1
    if total < xlen + 12 + 2 + 8 or total > end - pos:
        raise Corrupt("BSIZE")
    isize = int.from_bytes(buf[pos + total - 4: pos + total], "little")
    if isize > 65536:
        raise Corrupt("ISIZE")
    return total, isize, xlen


def walk(buf):
    """the serial walk from offset 0 -> (stream offsets, output offsets), members + 1 entries each"""
    buf = bytes(buf)
    pos, out, so, oo = 0, 0, [0], [0]
    while pos < len(buf):
        total, isize, _ = parse_member(buf, pos)
        pos += total
        out += isize
        so.append(pos)
        oo.append(out)
    return so, oo


def gzi(buf):
    """htslib's .gzi of the stream: u64 count, then the pairs of every member start but the first"""
    so, oo = walk(buf)
    pairs = list(zip(so, oo))[1:-1]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", s, o) for s, o in pairs)


def _deflate(payload, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(payload) + c.flush()


def foreign_bgzf(data, seed, levels=(0, 1, 6, 9), empties=True, extras=True, eof=True, max_payload=None):
    """`data` cut into members of 1..65 280 payload bytes, written by stock zlib at the levels in turn (several blocks per
    member, lengths to 258, stored blocks at level 0); a payload is halved until its member fits 65 536 bytes; empty
    members in the middle; some members with a subfield before 'BC' and one behind it (XLEN > 6); max_payload: only
    members that small"""
    rng = np.random.default_rng(seed)
    out, at, k = bytearray(), 0, 0
    while at < len(data):
        n = int(rng.choice([rng.integers(1, 300), rng.integers(1, 9000), rng.integers(1, 65281)]))
        if max_payload:
            n = 1 + n % max_payload
        n = min(n, len(data) - at)
        before = after = b""
        if extras and k % 3 == 1:
            before = b"XY" + struct.pack("<H", 5) + b"hello"
            after = b"BD" + struct.pack("<H", 2) + b"\x01\x02" if k % 2 else b""
        while True:
            payload = data[at:at + n]
            d = _deflate(payload, levels[k % len(levels)])
            if 12 + len(before) + 6 + len(after) + len(d) + 8 <= 65536:
                break
            n //= 2
        out += member(d, payload, before, after)
        at += n
        k += 1
        if empties and k % 5 == 2:
            out += EOF
    if eof:
        out += EOF
    return bytes(out)


def foreign_set():
    """(name, stream, expected bytes): each verified with gzip.decompress and the walker by the CPU test"""
    text = ic.mix(700_000, seed=15)
    rng = np.random.default_rng(8)
    rnd = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    out = [
        ("text", foreign_bgzf(text, 1), text),
        ("random", foreign_bgzf(rnd, 2), rnd),
        ("zeros_level9", foreign_bgzf(bytes(300_000), 3, levels=(9,)), bytes(300_000)),
        ("no_eof", foreign_bgzf(text[:150_000], 4, eof=False), text[:150_000]),
        ("plain", foreign_bgzf(text[:200_000], 5, empties=False, extras=False), text[:200_000]),
        ("only_eof", EOF, b""),
        ("empty_stream", b"", b""),
    ]
    # decoys: a BGZF file compressed again, its members coming out as stored blocks with byte-exact headers inside
    inner = foreign_bgzf(text[:400_000], 6)
    out.append(("decoy_stored", foreign_bgzf(inner, 7, levels=(0,)), inner))
    inner2 = foreign_bgzf(rnd, 9, levels=(0,), empties=False, extras=False)
    inner3 = foreign_bgzf(inner2, 10, levels=(0,))
    out.append(("decoy_twice", foreign_bgzf(inner3, 11, levels=(0, 1)), inner3))
    return out


# ---- streams that defeat the index's guesses.  csrc/bgzf.hip gives every CHUNK bytes of the stream a wave that guesses the
# chunk's entry: the first of at most TRIES header patterns in the chunk from which BSIZE hops reach the chunk's end.
# spec_model restates that rule, so the tests can show that these streams really make it guess wrong, or not at all. ---
CHUNK = 131072
TRIES = 8
MAGIC = b"\x1f\x8b\x08\x04"
STORED_PAYLOAD = 60000
STORED_MEMBER = 18 + 5 + STORED_PAYLOAD + 8


def stored_member(payload):
    """a member whose DEFLATE data is one stored block with BFINAL = 1: payload byte i is byte 23 + i of the member"""
    assert len(payload) <= 65535
    return member(b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload, payload)


def stored_bgzf(data, payload=STORED_PAYLOAD, eof=True):
    return b"".join(stored_member(data[i:i + payload]) for i in range(0, len(data), payload)) + (EOF if eof else b"")


def spec_model(buf):
    """[(chunk, guessed entry or None, true entry, chunk end)] for every chunk but the first of a VALID stream"""
    so, _ = walk(buf)
    n, out = len(buf), []
    for c in range(1, (n + CHUNK - 1) // CHUNK):
        lo, hi = c * CHUNK, min((c + 1) * CHUNK, n)
        true = min(x for x in so if x >= lo)
        guess, tries, p = None, 0, buf.find(MAGIC, lo)
        while p != -1 and p < hi and tries < TRIES and guess is None:
            tries += 1
            pos = p
            try:
                while pos < hi:
                    pos += parse_member(buf, pos)[0]
                guess = p
            except Corrupt:
                p = buf.find(MAGIC, p + 1)
        out.append((c, guess, true, hi))
    return out


def planted_stream(nchunks, plant_at, seed=31):
    """Stored members of random bytes over `nchunks` chunks.  In every chunk of `plant_at` the member that straddles the
    chunk's first byte gets, 100 bytes into the chunk, a byte-exact header whose BSIZE hop lands exactly on that member's
    end (where its own ISIZE passes for the decoy's): the guess survives every check a chunk can make on its own and is
    wrong, with one member and one ISIZE too many.  -> (stream, payload bytes, planted chunks)"""
    rng = np.random.default_rng(seed)
    nmem = (nchunks * CHUNK - 28) // STORED_MEMBER
    data = bytearray(rng.integers(0, 256, nmem * STORED_PAYLOAD, dtype=np.uint8).tobytes().replace(MAGIC, b"\0\0\0\0"))
    planted = []
    for c in plant_at:
        lo = c * CHUNK
        k = lo // STORED_MEMBER                                        # the member that holds byte lo
        mstart, mend, p = k * STORED_MEMBER, (k + 1) * STORED_MEMBER, lo + 100
        assert mstart + 23 <= p and p + 18 <= mend - 8 and mend - p >= 28, "chunk %d: no room for the decoy" % c
        i = k * STORED_PAYLOAD + (p - mstart - 23)
        data[i:i + 18] = HEAD + struct.pack("<H", mend - p - 1)
        planted.append(c)
    data = bytes(data)
    stream = stored_bgzf(data)
    assert (len(stream) + CHUNK - 1) // CHUNK == nchunks
    return stream, data, planted


def hard_set():
    """(name, stream, expected bytes, chunks whose guess must be wrong, least number of chunks without a guess)"""
    out = []
    s, d, pl = planted_stream(4, (1, 2))
    out.append(("planted_small", s, d, pl, 0))
    # more than 64 chunks (one verify round compares 64 guesses): wrong guesses at the start, in the middle, on both sides of
    # the round's edge and at the end
    s, d, pl = planted_stream(70, (1, 2, 33, 63, 64, 65, 69))
    out.append(("planted_70_chunks", s, d, pl, 0))
    # BGZF of a BGZF file whose members are tiny: behind a chunk's first byte come hundreds of inner headers, each of
    # whose hops breaks at the next outer member, before the first outer header: no guess at all
    inner = foreign_bgzf(ic.mix(400_000, seed=17), 12, max_payload=300)
    out.append(("tiny_inner_members", stored_bgzf(inner), inner, [], 2))
    return out


def hard_rejects():
    """index-stage refusals whose bad member lies in chunk 2: chunk 0's plain walk never meets it"""
    rng = np.random.default_rng(41)
    good = stored_bgzf(rng.integers(0, 256, 7 * STORED_PAYLOAD, dtype=np.uint8).tobytes().replace(MAGIC, b"\0\0\0\0"), eof=False)
    m5 = 5 * STORED_MEMBER
    assert len(good) == 7 * STORED_MEMBER and 2 * CHUNK <= m5 < 3 * CHUNK
    out = []
    b = bytearray(good)
    b[m5 + 1] ^= 0x10                                                  # chunk 2 guesses member 6; the walk from chunk 1 arrives at 5
    out.append(("late_bad_magic", bytes(b), "index"))
    b = bytearray(good)
    b[m5 + 16: m5 + 18] = struct.pack("<H", STORED_MEMBER - 1 + 9)        # lands 9 bytes into member 6: no guess in chunk 2
    out.append(("late_bsize_off", bytes(b), "index"))
    out.append(("late_truncated", good[:-5], "index"))
    out.append(("late_trailing_garbage", good + b"\x00" * 11, "index"))
    b = bytearray(good)
    b[m5 + STORED_MEMBER - 4: m5 + STORED_MEMBER] = struct.pack("<I", 65537)
    out.append(("late_isize_above_65536", bytes(b), "index"))
    return out


# ---- streams the decoder must refuse: (name, stream, stage) with stage "index" (mi_bgzf_index_dev refuses) or "inflate"
# (the index is the walker's, mi_bgzf_inflate_dev refuses) ------------------------------------------------------------
def rejects():
    text = D.text(150_000, seed=12)
    good = foreign_bgzf(text, 21, levels=(6,), empties=False, extras=False)
    so, _ = walk(good)
    last = so[-3]                                                      # the last data member (the EOF member follows it)
    mid = so[2]
    out = []

    def flip(at, mask=1):
        b = bytearray(good)
        b[at] ^= mask
        return bytes(b)

    out.append(("crc_flipped", flip(so[3] - 8), "inflate"))
    out.append(("isize_flipped", flip(so[3] - 4), "inflate"))
    big = bytearray(good)
    big[so[3] - 4: so[3]] = struct.pack("<I", 65537)
    out.append(("isize_above_65536", bytes(big), "index"))
    past = bytearray(good[:so[-2]])                                    # no EOF member: BSIZE of the last member too large
    past[last + 16: last + 18] = struct.pack("<H", (so[-2] - last) + 40 - 1)
    out.append(("bsize_past_stream", bytes(past), "index"))
    short = bytearray(good)
    short[mid + 16: mid + 18] = struct.pack("<H", 20)
    out.append(("bsize_shorter_than_header", bytes(short), "index"))
    nobc = bytearray(good)
    nobc[mid + 12: mid + 14] = b"BD"
    out.append(("no_bc_subfield", bytes(nobc), "index"))
    out.append(("truncated_last_member", good[:so[-2] - 5], "index"))
    out.append(("trailing_garbage", good + b"\x00" * 7, "index"))
    out.append(("flags_other_than_fextra", flip(mid + 3, 8), "index"))
    # a distance that reaches before the member's first byte
    w = ic.BitWriter()
    ic.put_fixed(w, [(65,), (66,), (5, 3)], final=1)
    w.align()
    out.append(("distance_before_member", good[:so[-2]] + member(w.bytes(), b"AB" + b"?" * 5) + EOF, "inflate"))
    # DEFLATE data that stops short of the trailer: two bytes between its end and the CRC
    d = _deflate(text[:1000], 6)
    out.append(("deflate_stops_short", good[:so[-2]] + member(d + b"\x00\x00", text[:1000]) + EOF, "inflate"))
    # no BFINAL = 1 block: the data ends with a sync flush
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(text[:1000]) + c.flush(zlib.Z_SYNC_FLUSH)
    out.append(("no_final_block", good[:so[-2]] + member(d, text[:1000]) + EOF, "inflate"))
    return out + hard_rejects()


def check_foreign(stream, want):
    assert gzip.decompress(stream) == want if stream else want == b""
    so, oo = walk(stream)
    assert so[-1] == len(stream) and oo[-1] == len(want)
    return so, oo
