"""Streams and ranges for the BGZF byte-range tests (a helper module, not a conftest).  The expected bytes of every range are
gzip.decompress(stream)[off:off + len]: stock Python, never the code under test.  Also a numpy model of the plan the device
makes (pieces per range, interior or edge, the slice of an edge piece's member) and the brute force it is checked against."""
import gzip
import zlib

import numpy as np

import bgzf_cases as B
from bgzf_cases import member, stored_member, walk

MI_OK, MI_ERR_ARG, MI_ERR_CORRUPT = 0, 1, 8
CANARY = 0xA5
GAPS = (1, 3, 15, 17)                                                  # bytes left free in front of slot i: every slot misaligned


def _deflate(payload, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(payload) + c.flush()


def s1_data():
    from compression_algorithms_amd import synth
    return synth.enwik_like(3 * 65280 + 1234, seed=11).numpy().tobytes()


def s1():
    """the library's own output (tests/test_bgzf_gpu.py pins the encoder to these bytes): 4 members and the EOF member"""
    data = s1_data()
    stream, _ = B.expected_bgzf(data, B.BGZF_BLOCK)
    return stream, data


def s2():
    """foreign, tiny and irregular: payloads of 1, 0, 7, 300, 0, 0 and 65 280 bytes, empty members in the middle and doubled,
    mixed zlib levels, level 0 (stored blocks) among them; the EOF member behind"""
    text = s1_data()
    sizes, levels = (1, 0, 7, 300, 0, 0, 65280), (6, 9, 0, 9, 1, 0, 1)
    out, at = bytearray(), 0
    for n, lv in zip(sizes, levels):
        payload = text[at:at + n]
        out += member(_deflate(payload, lv), payload)
        at += n
    out += B.EOF
    return bytes(out), text[:at]


def s3():
    """one member: 40 000 random bytes followed by a copy of the first 20 000, level 9.  (The copy lies 40 000 bytes behind
    its source, which is farther than DEFLATE reaches, so zlib writes it as literals: S3F below is the stream whose matches
    really are far.)"""
    rng = np.random.default_rng(77)
    head = rng.integers(0, 256, 40_000, dtype=np.uint8).tobytes()
    data = head + head[:20_000]
    return member(_deflate(data, 9), data) + B.EOF, data


def s3f():
    """the same shape with the copy in reach: 40 000 random bytes, then bytes [8 000, 28 000) again, at distance 32 000 —
    matches whose source lies outside the 4 KiB ring and outside the range [40 001, 59 999)"""
    rng = np.random.default_rng(78)
    head = rng.integers(0, 256, 40_000, dtype=np.uint8).tobytes()
    data = head + head[8_000:28_000]
    d = _deflate(data, 9)
    assert len(d) < 41_000, "the copy was not found"
    return member(d, data) + B.EOF, data


def s4():
    """S1 with member 1 as one stored block and one payload byte of it flipped behind the CRC's back: well-formed, only the
    CRC-32 of member 1 differs -> (stream, the bytes it inflates to when nobody checks, the member's number)"""
    stream, data = s1()
    so, oo = walk(stream)
    payload = data[oo[1]:oo[2]]
    m = bytearray(stored_member(payload))
    at = 31_000
    m[23 + at] ^= 0x40                                                 # (payload byte i is byte 23 + i of a stored member)
    flipped = bytearray(data)
    flipped[oo[1] + at] ^= 0x40
    return stream[:so[1]] + bytes(m) + stream[so[2]:], bytes(flipped), 1


def streams():
    """name -> (stream, expected bytes), each checked against gzip.decompress and the walker"""
    out = {"S1": s1(), "S2": s2(), "S3": s3(), "S3F": s3f()}
    for name, (stream, data) in out.items():
        assert gzip.decompress(stream) == data, name
        so, oo = walk(stream)
        assert so[-1] == len(stream) and oo[-1] == len(data), name
    assert len(walk(out["S1"][0])[0]) - 1 == 5
    return out


def ranges_for(stream, name=""):
    """the issue's list of (offset, length) for one stream, in the order given there"""
    so, oo = walk(stream)
    total, nm = oo[-1], len(oo) - 1
    ne = [m for m in range(nm) if oo[m + 1] > oo[m]]
    r = [(0, 0), (min(5, total), 0)]
    for m in ne:
        r += [(oo[m], 1), (oo[m + 1] - 1, 1)]                          # first and last byte of every member
    for x in sorted(set(oo[1:-1])):
        if 0 < x < total:
            r.append((x - 1, 2))                                       # across every boundary (and the empty members on it)
    for m in ne:
        r.append((oo[m], oo[m + 1] - oo[m]))                           # exactly one member
    for k in range(len(ne) - 2):
        a, b = oo[ne[k] + 1] - 1, oo[ne[k + 2]] + 1                    # two edge pieces around an interior one
        r.append((a, b - a))
    r.append((0, total))
    r += [(total - 1, 10), (total, 3), (total + 5, 3)]
    r += [r[len(r) // 2]] * 2                                          # the same range twice
    half = max(total // 3, 1)
    r += [(total // 5, half), (total // 5 + half // 2, half)]          # two that overlap
    r += sorted(r[2:10], reverse=True)                                 # descending
    if name in ("S3", "S3F"):
        r.append((40_001, 19_998))                                     # its source bytes lie outside the range
    return r


def expected(data, ranges):
    return [data[a:a + n] for a, n in ranges]


def layout(ranges, gaps=GAPS):
    """slot offsets with gaps[i % 4] free bytes in front of slot i -> (offsets, size of the buffer, a tail gap included)"""
    at, offs = 0, []
    for i, (_, n) in enumerate(ranges):
        at += gaps[i % len(gaps)]
        offs.append(at)
        at += n
    return offs, at + 19


# ---- the plan: what k_bgzr_members / k_bgzr_plan / k_bgzr_fill compute, in numpy ----------------------------------------------
def plan_model(oo, ranges):
    """per range the list of (member, 'interior' | 'edge', lo, hi): binary searches over the compacted non-empty members"""
    o = np.asarray(oo, dtype=np.int64)
    total = int(o[-1])
    nz = np.nonzero(o[1:] != o[:-1])[0]
    starts, ends = o[nz], o[nz + 1]
    out = []
    for a, n in ranges:
        if n == 0 or a >= total:
            out.append([])
            continue
        b = min(a + n, total)
        k0 = int(np.searchsorted(ends, a, side="right"))
        k1 = int(np.searchsorted(starts, b, side="left"))
        pieces = []
        for k in range(k0, k1):
            o0, o1 = int(starts[k]), int(ends[k])
            kind = "interior" if o0 >= a and o1 <= b else "edge"
            pieces.append((int(nz[k]), kind, max(o0, a) - o0, min(o1, b) - o0))
        out.append(pieces)
    return out


def plan_brute(oo, ranges):
    total = oo[-1]
    out = []
    for a, n in ranges:
        b = min(a + n, total)
        pieces = []
        for m in range(len(oo) - 1):
            o0, o1 = oo[m], oo[m + 1]
            if o1 > o0 and o0 < b and o1 > a and n > 0:
                pieces.append((m, "interior" if (a <= o0 and o1 <= b) else "edge", max(o0, a) - o0, min(o1, b) - o0))
        out.append(pieces)
    return out
