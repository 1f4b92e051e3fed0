"""LZ4 on the CPU (a helper module, not a conftest): the batched encoder's emission rule restated in Python over the tokens of
tests/snappy_cases.block_tokens, a decoder for raw blocks and frames with exactly the verdicts of include/mi_codec.h ("Batched
LZ4"), XXH32 for inputs below 16 bytes (the frame header's HC), writers for handwritten sequences, blocks and frames, and the
handwritten and corrupt streams the CPU and the GPU file share.  Nothing here touches the GPU library, and nothing needs another
LZ4 implementation: tests/golden/lz4_stock.json (scripts/gen_lz4_golden.py) holds what stock LZ4 wrote and how it judged."""
import base64
import functools
import hashlib
import json
import os
import struct

import parse1_cases as P1
import snappy_cases as S

OK, ARG, CAPACITY, CORRUPT = 0, 1, 4, 8
MAX_BYTES = 0x7FFFFFFF
GOLDEN = os.path.join(P1.GOLDEN, "lz4_stock.json")
GOLDEN_CUT = S.GOLDEN_CUT
BLOCKS = S.BLOCKS
PARSES = S.PARSES
FORMATS = ("block", "frame")
FRAME_HEADER = bytes.fromhex("04224D18604082")                  # version 1, independent blocks, no checksums, no content size, 64 KiB
END_MARK = b"\x00\x00\x00\x00"
MUTATION_ROOM = 1024                                           # capacity given to a mutated stream: the original's size and this


# ---- XXH32 below 16 bytes ------------------------------------------------------------------------------------------------------------
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _rotl(v, k):
    return ((v << k) | (v >> (32 - k))) & _M


def xxh32_short(data, seed=0):
    """XXH32 of fewer than 16 bytes: no stripes, only whole words, single bytes and the avalanche"""
    assert len(data) < 16
    h = (seed + _P5 + len(data)) & _M
    words = len(data) // 4
    for k in range(words):
        h = (h + int.from_bytes(data[4 * k:4 * k + 4], "little") * _P3) & _M
        h = (_rotl(h, 17) * _P4) & _M
    for c in data[4 * words:]:
        h = (h + c * _P5) & _M
        h = (_rotl(h, 11) * _P1) & _M
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    return h ^ (h >> 16)


# ---- the writers -----------------------------------------------------------------------------------------------------------------------
def chain(v):
    """the bytes behind a length nibble for the value v: none below 15, else 255s and one byte below 255"""
    if v < 15:
        return b""
    v -= 15
    return b"\xFF" * (v // 255) + bytes([v % 255])


def seq(lits, offset, mlen):
    """one sequence with a match of mlen >= 4 bytes"""
    assert mlen >= 4 and 0 <= offset < 65536
    return bytes([(min(len(lits), 15) << 4) | min(mlen - 4, 15)]) + chain(len(lits)) + bytes(lits) + struct.pack("<H", offset) + chain(mlen - 4)


def last(lits, nibble=0):
    """the closing sequence: literals only (nibble: what its unused match nibble holds)"""
    return bytes([(min(len(lits), 15) << 4) | nibble]) + chain(len(lits)) + bytes(lits)


def word(v):
    return struct.pack("<I", v)


def frame_header(bmax=4, indep=True, bcheck=False, csize=None, ccheck=False, dict_id=None, version=1, reserved=0, bd_low=0,
                 hc=None, magic=0x184D2204):
    flg = (version << 6) | (indep << 5) | (bcheck << 4) | ((csize is not None) << 3) | (ccheck << 2) | (reserved << 1) | (dict_id is not None)
    desc = bytes([flg, (bmax << 4) | bd_low])
    if csize is not None:
        desc += struct.pack("<Q", csize)
    if dict_id is not None:
        desc += word(dict_id)
    return word(magic) + desc + bytes([(xxh32_short(desc) >> 8) & 0xFF if hc is None else hc])


def frame(blocks, tail=END_MARK, **header):
    """blocks: [(data, stored)]; with bcheck / ccheck every checksum field is four bytes that nobody verifies"""
    out = bytearray(frame_header(**header))
    for data, stored in blocks:
        out += word(len(data) | (0x80000000 if stored else 0)) + bytes(data)
        if header.get("bcheck"):
            out += b"\xC5\xC5\xC5\xC5"
    out += tail
    if header.get("ccheck"):
        out += b"\xCC\xCC\xCC\xCC"
    return bytes(out)


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
_GOOD, _BAD, _BIG = 0, 1, 2


def _chain(s, ip, bend, v):
    while True:
        if ip >= bend:
            return None, ip
        c = s[ip]
        ip += 1
        v += c
        if c != 255:
            return v, ip


def _sequences(s, ip, bend, out, floor, limit, over):
    """the sequences of s[ip:bend] appended to out -> _GOOD / _BAD / `over`; floor: the first position a match may reach; limit:
    where the output must end at the latest"""
    while True:
        if ip >= bend:
            return _BAD                                        # the block ends behind a match: no closing literals
        tok = s[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            ll, ip = _chain(s, ip, bend, ll)
            if ll is None:
                return _BAD
        if ll > bend - ip:
            return _BAD
        if ll > limit - len(out):
            return over
        out += s[ip:ip + ll]
        ip += ll
        if ip == bend:
            return _GOOD
        if bend - ip < 2:
            return _BAD
        d = s[ip] | (s[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        if ml == 15:
            ml, ip = _chain(s, ip, bend, ml)
            if ml is None:
                return _BAD
        ml += 4
        if d == 0 or d > len(out) - floor:
            return _BAD
        if ml > limit - len(out):
            return over
        if d >= ml:
            out += out[len(out) - d:len(out) - d + ml]
        else:
            piece = bytes(out[-d:])
            out += (piece * (ml // d + 1))[:ml]


def frame_info(s):
    """the header of a frame -> (verdict, dict(hb, bmax, indep, bcheck, ccheck, csize))"""
    if len(s) < 4:
        return CORRUPT, None
    magic = int.from_bytes(s[:4], "little")
    if magic != 0x184D2204:
        return (ARG if (magic & 0xFFFFFFF0) == 0x184D2A50 or magic == 0x184C2102 else CORRUPT), None
    if len(s) < 7:
        return CORRUPT, None
    flg, bd = s[4], s[5]
    if flg >> 6 != 1 or flg & 2 or bd & 0x8F or bd >> 4 < 4:
        return CORRUPT, None
    has_csize, has_dict = bool(flg & 8), bool(flg & 1)
    dl = 2 + 8 * has_csize + 4 * has_dict
    if 4 + dl + 1 > len(s):
        return CORRUPT, None
    if (xxh32_short(s[4:4 + dl]) >> 8) & 0xFF != s[4 + dl]:
        return CORRUPT, None
    csize = int.from_bytes(s[6:14], "little") if has_csize else None
    if has_dict or (has_csize and csize > MAX_BYTES):
        return ARG, None
    return OK, dict(hb=5 + dl, bmax=1 << (8 + 2 * (bd >> 4)), indep=bool(flg & 32), bcheck=bool(flg & 16), ccheck=bool(flg & 4), csize=csize)


def _frame_body(s, f, out):
    ip, end = f["hb"], len(s)
    while True:
        if end - ip < 4:
            return _BAD
        w = int.from_bytes(s[ip:ip + 4], "little")
        ip += 4
        if w == 0:
            break
        bs = w & 0x7FFFFFFF
        if bs == 0 or bs > f["bmax"] or bs > end - ip:              # (80 00 00 00 is neither the EndMark nor a block)
            return _BAD
        room = len(out) + f["bmax"]
        limit, over = (MAX_BYTES, _BIG) if room > MAX_BYTES else (room, _BAD)
        if w >> 31:
            if bs > limit - len(out):
                return over
            out += s[ip:ip + bs]
        else:
            st = _sequences(s, ip, ip + bs, out, len(out) if f["indep"] else 0, limit, over)
            if st != _GOOD:
                return st
        ip += bs
        if f["bcheck"]:
            if end - ip < 4:
                return _BAD
            ip += 4
    if f["ccheck"]:
        if end - ip < 4:
            return _BAD
        ip += 4
    if ip != end:
        return _BAD
    if f["csize"] is not None and f["csize"] != len(out):
        return _BAD
    return _GOOD


def decode(stream, fmt, cap=None):
    """-> (bytes or None, verdict, out_bytes) as mi_lz4_decode_batch_dev answers for one item"""
    stream = bytes(stream)
    if len(stream) > MAX_BYTES or (cap is not None and cap > MAX_BYTES):
        return None, ARG, 0
    if not stream:
        return None, CORRUPT, 0
    out = bytearray()
    if fmt == "frame":
        st, f = frame_info(stream)
        if st:
            return None, st, 0
        st = _frame_body(stream, f, out)
    else:
        st = _sequences(stream, 0, len(stream), out, 0, MAX_BYTES, _BIG)
    if st != _GOOD:
        return None, (ARG if st == _BIG else CORRUPT), 0
    if cap is not None and len(out) > cap:
        return None, CAPACITY, len(out)
    return bytes(out), OK, len(out)


def size_of(stream, fmt):
    """-> (verdict, out_bytes) as mi_lz4_batch_size_dev answers: the decoder's, but a frame with a content size from its header alone"""
    if fmt == "frame" and 0 < len(stream) <= MAX_BYTES:
        st, f = frame_info(bytes(stream))
        if st == OK and f["csize"] is not None:
            return OK, f["csize"]
    _, st, n = decode(stream, fmt)
    return st, n


# ---- the emission rule over the tokens ---------------------------------------------------------------------------------------------
def emit_block(part, tokens):
    """the record of one block of n bytes: a match at p joins the pending run when p + 12 > n or when min(L, n - 5 - p) < 4; any
    other match flushes the run and itself (at its possibly shortened length) as one sequence; the run left over closes the block"""
    n, out, run_from = len(part), bytearray(), 0
    for p, ln, d in tokens:
        if ln == 0 or p + 12 > n:
            continue
        ln = min(ln, n - 5 - p)                                # (mode Z's clip to n - p is the weaker one)
        if ln < 4:
            continue
        out += seq(part[run_from:p], d, ln)
        run_from = p + ln
    return bytes(out + last(part[run_from:]))


@functools.lru_cache(maxsize=None)
def restate(data, block=65536, parse=0, fmt="frame"):
    """what lz4_compress_batch must write for the item `data`"""
    tokens = S.block_tokens(data, block, parse)
    if fmt == "block":
        assert len(data) <= block
        return emit_block(data, tokens[0]) if data else b"\x00"
    out = bytearray(FRAME_HEADER)
    for k, t in enumerate(tokens):
        part = data[k * block:(k + 1) * block]
        rec = emit_block(part, t)
        out += word(len(part) | 0x80000000) + part if len(rec) >= len(part) else word(len(rec)) + rec
    return bytes(out + END_MARK)


def bound(n, block=65536, fmt="frame"):
    """mi_lz4_batch_bound_bytes, restated"""
    return 11 + n + 4 * ((n + block - 1) // block) if fmt == "frame" else n + n // 255 + 16


def worst_case(n):
    """270 noise bytes — the shortest run whose chain takes two bytes — then a repeat of four bytes from 300 back, over and over:
    the most a match can cost beside the literals it flushes"""
    out, k = bytearray(), 0
    while len(out) < n:
        out += P1.noise(270, 2000 + k)
        out += out[-300:-296] if len(out) >= 300 else out[-4:]
        k += 1
    return bytes(out[:n])


def cpu_items():
    """name -> bytes: the inputs the restatement is proven on before a GPU sees the rule.  Sizes around every threshold of the end
    rules, a run, noise, and a match that would end on the block's last byte (parse1_cases' "ends_at_n")"""
    t = P1.golden_text()
    out = {f"text_{n}": t[:n] for n in (0, 1, 4, 5, 12, 13, 17, 65536)}
    out.update({f"run_{n}": b"a" * n for n in (12, 13, 17, 300, 65536)})
    out["noise_70000"] = P1.noise(70_000, 7)
    out["noise_999"] = P1.noise(999, 8)
    out["ends_at_n"] = P1.cases()["ends_at_n"]
    out["repeat_to_the_end"] = P1.noise(40, 9) + P1.noise(40, 9)                # the second half matches to the last byte
    out["mixed"] = P1.cases()["mixed"]
    out["worst_3000"] = worst_case(3000)
    return out


# ---- stock LZ4's streams and verdicts -----------------------------------------------------------------------------------------------
def golden_inputs():
    """name -> bytes: what scripts/gen_lz4_golden.py compresses with stock LZ4 — the Snappy fixture's inputs with the text cut to
    12 000 bytes (the fixture stays small), noise, and 3 000 noise bytes repeated to 70 000: two blocks whose matches, in a linked
    frame, reach across the block boundary"""
    out = dict(S.golden_inputs())
    out["text"] = out["text"][:12_000]
    out["noise_1000"] = P1.noise(1000, 11)
    out["periodic_70000"] = (P1.noise(3000, 12) * 24)[:70_000]
    return out


MUTATED = ("mixed", "chunk_offset_63", "rising", "item_1999", "period3")
MUTATIONS_EACH = 48


def mutation_plan(name, stream):
    """[(position, xor mask)]: MUTATIONS_EACH one-byte changes of a stock block, from a hash of its name"""
    out = []
    for k in range(MUTATIONS_EACH):
        h = hashlib.sha256(f"{name}:{k}".encode()).digest()
        out.append((int.from_bytes(h[:4], "little") % len(stream), h[4] or 1))
    return out


def mutate(stream, at, mask):
    s = bytearray(stream)
    s[at] ^= mask
    return bytes(s)


@functools.lru_cache(maxsize=None)
def golden():
    """-> dict: "blocks" and "frames" [(name, stock stream, the bytes it decodes to)], "mutations" [(name, mutated block, capacity,
    stock's return value, expected (verdict, out_bytes), the first 16 hex digits of the expected bytes' SHA-256 or None)]"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    inputs = golden_inputs()
    out = {"blocks": [], "frames": [], "mutations": []}
    for kind in ("blocks", "frames"):
        for e in doc[kind]:
            data = inputs[e["input"]]
            assert hashlib.sha256(data).hexdigest()[:16] == e["sha256"], e["name"]
            out[kind].append((e["name"], base64.b64decode(e["stream"]), data))
    blocks = {name: (s, d) for name, s, d in out["blocks"]}
    for block, at, xor, stock, verdict, out_bytes, sha in doc["mutations"]:
        s, d = blocks[block]
        out["mutations"].append((f"{block}@{at}^{xor}", mutate(s, at, xor), len(d) + MUTATION_ROOM, stock, (verdict, out_bytes), sha))
    return out


# ---- handwritten streams -----------------------------------------------------------------------------------------------------------
def _made(fmt, stream):
    data, st, _ = decode(stream, fmt)
    assert st == OK, (fmt, st)
    return stream, data


@functools.lru_cache(maxsize=None)
def handwritten(fmt):
    """[(name, stream, bytes)]: the smallest shapes at which the decoder's paths differ"""
    nz = P1.noise
    blocks = []
    blocks.append(("chain_255_then_0", seq(nz(15 + 255, 60), 270, 4 + 15 + 255) + last(b"tail!")))       # both chains FF 00
    blocks.append(("chain_254", seq(nz(15 + 254, 61), 100, 4 + 15 + 254) + last(b"tail!")))               # both chains FE
    blocks.append(("nibble_14_and_15", seq(nz(14, 62), 14, 18) + seq(nz(15, 63), 1, 19) + last(b"12345")))     # 15: a chain of 00
    blocks.append(("overlap_1_70", b"".join(seq(nz(3, 64 + d), d, 70) for d in range(1, 71)) + last(b"12345")))
    blocks.append(("offset_65535", seq(nz(65_535, 65), 65_535, 64) + seq(b"", 65_535, 8) + last(b"12345")))
    blocks.append(("lit_5000", seq(nz(5000, 66), 4999, 30) + last(nz(5, 67))))
    blocks.append(("lit_40000_far", seq(nz(40_000, 68), 40_000, 3000) + seq(b"xyz", 39_000, 700) + last(b"12345")))   # past either ring
    blocks.append(("match_2000_d_100", seq(nz(100, 69), 100, 2000) + last(b"the end")))                       # d >= 64, pieces overlap
    blocks.append(("offset_eq_written", seq(nz(37, 70), 37, 11) + seq(b"", 48, 64) + last(b"12345")))
    blocks.append(("last_nibble_ignored", last(b"abc", nibble=9)))
    blocks.append(("only_literals_1", last(b"q")))
    blocks.append(("empty", b"\x00"))
    if fmt == "block":
        return [(name, *_made("block", s)) for name, s in blocks]
    big = ("offset_65535",)                                        # more than 64 KiB of block data or output: BD names 256 KiB
    out = [(name, *_made("frame", frame([(s, False)], bmax=5 if name in big else 4))) for name, s in blocks if name != "empty"]
    a, b = nz(300, 71), nz(200, 72)
    cross = seq(b, 400, 50) + last(b"12345")                       # reaches 100 bytes in front of its block
    out.append(("linked_match_across_blocks", *_made("frame", frame([(last(a), False), (cross, False)], indep=False))))
    out.append(("stored_and_compressed", *_made("frame", frame([(a, True), (seq(b, 150, 40) + last(b"12345"), False), (b, True)]))))
    out.append(("stored_65536", *_made("frame", frame([(nz(65_536, 73), True)]))))
    out.append(("empty_frame", *_made("frame", frame([]))))
    out.append(("content_size", *_made("frame", frame([(last(a), False)], csize=300))))
    out.append(("content_size_0", *_made("frame", frame([], csize=0))))
    out.append(("checksum_fields_skipped", *_made("frame", frame([(last(a), False), (b, True)], bcheck=True, ccheck=True, csize=500))))
    out.append(("bmax_7_block_100000", *_made("frame", frame([(last(nz(100_000, 74)), False)], bmax=7))))
    return out


@functools.lru_cache(maxsize=None)
def corrupt(fmt):
    """[(name, stream)]: each refused for exactly one reason (MI_ERR_CORRUPT, or MI_ERR_ARG where the name starts with unsupported_)"""
    nz = P1.noise(50, 95)
    good = seq(nz, 20, 8) + seq(b"abcdef", 33, 40) + last(b"12345")
    n_good = len(decode(good, "block")[0])
    blocks = [("offset_0", seq(nz, 0, 8) + last(b"12345")),
              ("offset_written_plus_1", seq(nz, 51, 8) + last(b"12345")),
              ("cut_in_literal_chain", bytes([0xF0, 0xFF])),
              ("cut_in_literals", good[:30]),
              ("cut_in_offset", seq(nz, 20, 8)[:-1]),
              ("cut_in_match_chain", seq(nz, 20, 300)[:-1]),
              ("ends_behind_a_match", seq(nz, 20, 8)),
              ("literals_past_the_end", bytes([0x50]) + b"abcd")]
    if fmt == "block":
        return blocks + [("zero_bytes", b"")]
    a, b = P1.noise(300, 71), P1.noise(200, 72)
    cross = seq(b, 400, 50) + last(b"12345")
    ok = frame([(good, False)])
    out = [(name, frame([(s, False)])) for name, s in blocks]
    out += [("indep_match_across_blocks", frame([(last(a), False), (cross, False)], indep=True)),
            ("version_0", frame([(good, False)], version=0)), ("version_2", frame([(good, False)], version=2)),
            ("reserved_flg_bit", frame([(good, False)], reserved=1)),
            ("bd_low_bits", frame([(good, False)], bd_low=1)), ("bd_top_bit", frame([(good, False)], bmax=12)),
            ("bd_block_maximum_3", frame([(good, False)], bmax=3)), ("bd_block_maximum_0", frame([(good, False)], bmax=0)),
            ("wrong_hc", frame([(good, False)], hc=0x83)),
            ("wrong_hc_with_content_size", frame([(good, False)], csize=n_good, hc=frame_header(csize=n_good)[-1] ^ 0x10)),
            ("content_size_plus_1", frame([(good, False)], csize=n_good + 1)), ("content_size_minus_1", frame([(good, False)], csize=n_good - 1)),
            ("trailing_byte", ok + b"\x00"), ("trailing_frame", ok + ok),
            ("end_mark_with_top_bit", frame([(good, False)], tail=word(0x80000000))),
            ("stored_block_of_0_bytes", frame([(good, False), (b"", True)])),
            ("no_end_mark", ok[:-4]), ("end_mark_cut", ok[:-1]),
            ("block_size_past_the_end", FRAME_HEADER + word(len(good) + 1) + good),
            ("block_data_above_maximum", frame([(P1.noise(65_537, 96), True)])),
            ("block_output_above_maximum", frame([(seq(nz, 1, 65_536) + last(b""), False)])),
            ("block_checksum_missing", frame([(good, False)], bcheck=True)[:-8] + END_MARK),
            ("content_checksum_missing", frame([(good, False)], ccheck=True)[:-4]),
            ("header_cut", FRAME_HEADER[:6]), ("magic_cut", FRAME_HEADER[:3]), ("wrong_magic", b"\x05" + ok[1:]),
            ("zero_bytes", b""),
            ("unsupported_dict_id", frame([(good, False)], dict_id=7)),
            ("unsupported_skippable_frame", word(0x184D2A53) + word(4) + b"skip"),
            ("unsupported_legacy_frame", word(0x184C2102) + word(len(good)) + good),
            ("unsupported_content_size_2_pow_31", frame([], csize=1 << 31))]
    return out


NEIGHBOURS = ("chain_255_then_0", "overlap_1_70", "lit_5000")


def among_good(fmt):
    """[(name, stream, bytes or None)]: every bad stream between good neighbours"""
    hw = {name: (s, d) for name, s, d in handwritten(fmt)}
    out = []
    for k, (name, s) in enumerate(corrupt(fmt)):
        g = NEIGHBOURS[k % len(NEIGHBOURS)]
        out += [(g, *hw[g]), (name, s, None)]
    g = NEIGHBOURS[0]
    return out + [(g, *hw[g])]
