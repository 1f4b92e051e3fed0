"""Raw Snappy on the CPU (a helper module, not a conftest): the batched encoder's emission rule restated in Python over the
oracle's tokens, a decoder with exactly the verdicts of include/mi_codec.h ("Batched Snappy"), an element writer for
handwritten streams, and the handwritten and corrupt streams the CPU and the GPU file share.  Nothing here touches the GPU
library, and nothing needs another Snappy implementation: tests/golden/snappy_stock.json (scripts/gen_snappy_golden.py) holds
what stock Snappy wrote."""
import base64
import functools
import hashlib
import json
import os

import parse1_cases as P1

OK, ARG, CAPACITY, CORRUPT = 0, 1, 4, 8
MAX_BYTES = 0x7FFFFFFF
GOLDEN = os.path.join(P1.GOLDEN, "snappy_stock.json")
GOLDEN_CUT = 70_000
BLOCKS = (65536, 4096, 1000)
PARSES = (0, 1)


# ---- the element writer ------------------------------------------------------------------------------------------------------------
def varint(n):
    out = bytearray()
    while True:
        out.append((n & 0x7F) | (0x80 if n > 0x7F else 0))
        n >>= 7
        if not n:
            return bytes(out)


def lit(data, form=None):
    """a literal element.  form None: the shortest (len - 1 in the tag below 60, else 60.. with as many length bytes as it
    needs); 60..63: that tag with its 1..4 length bytes, whatever the length"""
    v = len(data) - 1
    assert v >= 0
    if form is None:
        form = v if v < 60 else 59 + max(1, (v.bit_length() + 7) // 8)
    if form < 60:
        assert form == v
        return bytes([form << 2]) + bytes(data)
    return bytes([form << 2]) + v.to_bytes(form - 59, "little") + bytes(data)


def copy1(length, offset):
    assert 4 <= length <= 11 and 0 <= offset < 2048
    return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 255])


def copy2(length, offset):
    assert 1 <= length <= 64 and 0 <= offset < 65536
    return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")


def copy4(length, offset):
    assert 1 <= length <= 64 and 0 <= offset < 1 << 32
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
def preamble(stream):
    """-> (verdict, value, its bytes): at most five bytes, at most 32 bits (snappy's Varint::Parse32WithLimit); a well-formed
    value above 2^31 - 1 is ARG, the per-item limit"""
    v = 0
    for k in range(5):
        if k >= len(stream):
            return CORRUPT, 0, 0
        c = stream[k]
        v |= (c & 0x7F) << (7 * k)
        if c < 0x80:
            if v > 0xFFFFFFFF:
                return CORRUPT, 0, 0
            if v > MAX_BYTES:
                return ARG, 0, 0
            return OK, v, k + 1
    return CORRUPT, 0, 0


def _body(stream, ip, n):
    """the elements of stream[ip:] -> bytes, or None where they are malformed; n: the preamble (None: whatever they give)"""
    out, end = bytearray(), len(stream)
    room = lambda: (1 << 62) if n is None else n - len(out)
    while ip < end:
        tag = stream[ip]
        ip += 1
        kind = tag & 3
        extra = (max((tag >> 2) - 59, 0) if kind == 0 else 4 if kind == 3 else kind)
        if extra > end - ip:
            return None                                        # the input ends inside the element
        x = int.from_bytes(stream[ip:ip + extra], "little")
        ip += extra
        if kind == 0:
            ln = (x if extra else tag >> 2) + 1
            if ln > end - ip or ln > room():
                return None
            out += stream[ip:ip + ln]
            ip += ln
            continue
        if kind == 1:
            ln, d = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | x
        else:
            ln, d = (tag >> 2) + 1, x
        if d == 0 or d > len(out) or ln > room():
            return None
        if d >= ln:
            out += out[len(out) - d:len(out) - d + ln]
        else:
            for _ in range(ln):
                out.append(out[-d])
    return None if n is not None and len(out) != n else bytes(out)


def decode(stream, cap=None):
    """-> (bytes or None, verdict, out_bytes) as mi_snappy_decode_batch_dev answers for one item"""
    stream = bytes(stream)
    if len(stream) > MAX_BYTES or (cap is not None and cap > MAX_BYTES):
        return None, ARG, 0
    st, n, ip = preamble(stream)
    if st:
        return None, st, 0
    if cap is not None and n > cap:
        return None, CAPACITY, n
    out = _body(stream, ip, n)
    return (None, CORRUPT, 0) if out is None else (out, OK, n)


def stream_of(elements):
    """handwritten elements -> (stream, what it decodes to)"""
    body = b"".join(elements)
    data = _body(body, 0, None)
    assert data is not None
    return varint(len(data)) + body, data


# ---- the emission rule over the tokens ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_tokens(data, block, parse):
    """per block of `data`: ((position, length, distance), ...) with length 0 for a literal, before the clip.  Parse 1: the
    restated rule (parse1_cases.walk); parse 0: the oracle's tokens of independent blocks"""
    parts = [data[a:a + block] for a in range(0, len(data), block)]
    if parse == 1:
        return tuple(P1.walk(part) for part in parts)
    from oracle import orc
    tok, sizes = orc.deflate_stream(data, block, True)
    tok, out, at = tok.tobytes(), [], 0
    for size in (int(v) for v in sizes):
        t, p, i = [], 0, at
        while i < at + size:
            if tok[i] == 0:
                t.append((p, 0, 0))
                p, i = p + 1, i + 2
            else:
                t.append((p, tok[i + 3], tok[i + 1] | (tok[i + 2] << 8)))
                p, i = p + tok[i + 3], i + 4
        at += size
        out.append(tuple(t))
    return tuple(out)


def emit_block(part, tokens):
    """the record of one block: runs of literals and of matches shorter than 4, flushed by a match of 4 or more as ONE literal
    element; that match as copies of 64 while L >= 68, 60 if L > 64, the rest; copy-1 when 4 <= len <= 11 and d < 2048"""
    n, out, run_from = len(part), bytearray(), 0
    for p, ln, d in tokens:
        ln = min(ln, n - p)                                    # mode Z's clip of a last match that runs past the block
        if ln < 4:
            continue
        if p > run_from:
            out += lit(part[run_from:p])
        run_from = p + ln
        while ln >= 68:
            out += copy2(64, d)
            ln -= 64
        if ln > 64:
            out += copy2(60, d)
            ln -= 60
        out += copy1(ln, d) if ln <= 11 and d < 2048 else copy2(ln, d)
    if run_from < n:
        out += lit(part[run_from:])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def restate(data, block=65536, parse=0):
    """what snappy_compress_batch must write for the item `data`"""
    out = bytearray(varint(len(data)))
    for k, tokens in enumerate(block_tokens(data, block, parse)):
        out += emit_block(data[k * block:(k + 1) * block], tokens)
    return bytes(out)


def bound(n, block=65536):
    """mi_snappy_batch_bound_bytes, restated"""
    return 5 + n + n // 61 + 3 * ((n + block - 1) // block)


def worst_case(n):
    """61 noise bytes, then a repeat of four bytes from 2 100 back (the last four while there are not that many), over and
    over: every run takes the two-byte tag and every copy the three-byte form — 66 bytes for 65"""
    out, k = bytearray(), 0
    while len(out) < n:
        out += P1.noise(61, 1000 + k)
        out += out[-2100:-2096] if len(out) >= 2100 else out[-4:]
        k += 1
    return bytes(out[:n])


# ---- stock Snappy's streams ----------------------------------------------------------------------------------------------------------
def golden_inputs():
    """name -> bytes: what scripts/gen_snappy_golden.py compresses with stock Snappy, cut to GOLDEN_CUT bytes"""
    c = P1.cases()
    out = {k: c[k][:GOLDEN_CUT] for k in ("text", "zeros", "period3", "mixed", "chunk_offset_63", "rising", "zeros_1", "text_5")}
    items = P1.batch_items()
    out.update({"item_empty": items[0], "item_1999": items[5], "item_abc": items[10]})
    return out


@functools.lru_cache(maxsize=None)
def golden():
    """[(name, stock stream, the bytes it decodes to)]"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    inputs, out = golden_inputs(), []
    for e in doc["streams"]:
        data = inputs[e["name"]]
        assert hashlib.sha256(data).hexdigest() == e["sha256"], e["name"]
        out.append((e["name"], base64.b64decode(e["stream"]), data))
    return out


# ---- handwritten streams -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def handwritten():
    """[(name, stream, bytes)]: the smallest shapes at which the decoder's paths differ"""
    nz = lambda n, seed: P1.noise(n, seed)
    out = []
    # a copy-4 that reaches 100 000 bytes back, past either ring, in an item of 140 000 bytes: 64-byte copies are all it takes
    far = [lit(nz(40_000, 70))] + [copy2(64, 40_000)] * ((100_000 - 40_000) // 64 + 1) + [copy4(64, 100_000)]
    far += [copy2(64, 30_000)] * ((140_000 - len(_body(b"".join(far), 0, None))) // 64)
    far.append(lit(nz(140_000 - len(_body(b"".join(far), 0, None)), 71)))
    out.append(("copy4_far", far))
    for form, n in ((60, 17), (60, 256), (61, 300), (61, 5), (62, 70_000), (62, 9), (63, 12)):
        out.append((f"lit_tag{form}_{n}", [lit(nz(n, 72 + n % 7), form), copy1(4, 3)]))
    out.append(("lit_5000", [lit(nz(5000, 80)), copy2(30, 4999)]))
    out.append(("lit_40000", [lit(nz(40_000, 81)), copy2(64, 40_000), lit(b"xyz")]))
    el = [lit(nz(80, 82))]
    for d in range(1, 71):
        el += [copy2(64, d), lit(nz(3, 83 + d))]
    out.append(("overlap_1_70", el))
    out.append(("offset_eq_produced", [lit(nz(37, 90)), copy1(11, 37), copy2(64, 48), copy4(7, 112)]))
    out.append(("copy2_65535", [lit(nz(65_535, 91)), copy2(64, 65_535), copy2(1, 65_535)]))
    out.append(("empty", []))
    return [(name, *stream_of(e)) for name, e in out]


@functools.lru_cache(maxsize=None)
def corrupt():
    """[(name, stream)]: each malformed in exactly one way, and refused by every Snappy reader"""
    nz = P1.noise(50, 95)
    good = [lit(nz), copy1(8, 20), lit(b"abcdef"), copy2(40, 33)]
    body = b"".join(good)
    n = len(_body(body, 0, None))
    out = [("offset_0", varint(58) + lit(nz) + copy1(8, 0)),
           ("offset_produced_plus_1", varint(58) + lit(nz) + copy2(8, 51)),
           ("cut_in_length_bytes", varint(400) + lit(P1.noise(300, 96), 61)[:2]),
           ("cut_in_literal", varint(n) + body[:30]),
           ("cut_in_copy1", varint(58) + lit(nz) + copy1(8, 20)[:1]),
           ("cut_in_copy2", varint(58) + lit(nz) + copy2(8, 20)[:2]),
           ("cut_in_copy4", varint(58) + lit(nz) + copy4(8, 20)[:4]),
           ("preamble_plus_1", varint(n + 1) + body),
           ("preamble_minus_1", varint(n - 1) + body),
           ("trailing_bytes", varint(n) + body + lit(b"z")),
           ("trailing_zero_byte", varint(n) + body + b"\x00"),
           ("varint_6_bytes", b"\x80\x80\x80\x80\x80\x00" + body),
           ("varint_2_pow_32", b"\x80\x80\x80\x80\x10" + body),
           ("varint_cut", b"\x80\x80"),
           ("zero_bytes", b"")]
    return out


NEIGHBOURS = ("lit_tag60_17", "overlap_1_70", "lit_5000")


def among_good(bad):
    """[(name, stream, bytes or None)]: every bad stream between good neighbours"""
    hw = {name: (s, d) for name, s, d in handwritten()}
    out = []
    for k, (name, s) in enumerate(bad):
        g = NEIGHBOURS[k % len(NEIGHBOURS)]
        out += [(g, *hw[g]), (name, s, None)]
    g = NEIGHBOURS[0]
    return out + [(g, *hw[g])]
