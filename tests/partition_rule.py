"""The rule by which stage 1 of the LDS-resident match finder cuts a block into parts, restated in numpy.

Written from the comments at the head of csrc/lz2_partition.hip and from DESIGN.md section 3, one group and one cut at a time, with
none of the kernel's machinery (no scans, no 64-way searches): tests/test_partition_cuts_gpu.py holds the device's parts against
it, tests/test_partition_rule.py checks it against the properties the rule promises.

  * position p of a block has home = mix32(little-endian word at p, zero bytes past the block's end) mod T, T = 2^tbits buckets;
    16 384 groups of Gw = T / 16 384 consecutive buckets; c[g] = positions whose home lies in group g;
  * at most out[g] = max(in[g] + c[g] - Gw, c[g] - 1, 0) entries overflow from group g into the next, in[g + 1] = out[g]; the
    lz77 flavour starts with in[0] = 0, the deflate flavour's table is a ring and in[0] is the fixed point of one lap;
    group g is certified where out[g] == 0: no probe cluster crosses its end;
  * deflate: the ring is cut behind the first certified group (base = its end), the groups are renumbered from there; a block
    without a certified group goes to the fallback pipeline.  lz77: base 0;
  * greedy cuts: a part ends behind the LAST certified group that keeps it within `cap` entries (2 048) and, for tables of up to
    2^20 buckets, within 2^16 homes; where there is none and the rest of the block is above 4 096 entries, behind the last one
    that keeps it within 4 096; where there is none either, the block goes to the fallback pipeline.  What is left when at most
    `cap` entries remain (or at most 4 096 with no cut within `cap`) is the last part.
"""
import numpy as np

NG_BITS = 14
NG = 1 << NG_BITS
CAP_WIDE = 4096
MAXPARTS = 128
M32 = 0xFFFFFFFF


def mix32(w):
    """the reference's hash() of a 32-bit word (numpy uint32 array in, uint32 array out)"""
    k = w.astype(np.uint64) * 0xcc9e2d51 & M32
    k = ((k << 15) | (k >> 17)) & M32
    k = k * 0x1b873593 & M32
    h = ((k << 13) | (k >> 19)) & M32
    h = (h * 5 + 0xe6546b64) & M32
    h ^= h >> 16
    h = h * 0x85ebca6b & M32
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M32
    h ^= h >> 16
    return h.astype(np.uint32)


def unmix32(h):
    """the word whose mix32 is h (mix32 is a bijection of the 32-bit words); python int in and out"""
    inv = lambda m: pow(m, -1, 1 << 32)
    ror = lambda x, r: ((x >> r) | (x << (32 - r))) & M32
    h ^= h >> 16
    h = h * inv(0xc2b2ae35) & M32
    h ^= (h >> 13) ^ (h >> 26)
    h = h * inv(0x85ebca6b) & M32
    h ^= h >> 16
    h = (h - 0xe6546b64) * inv(5) & M32
    k = ror(h, 13) * inv(0x1b873593) & M32
    return ror(k, 15) * inv(0xcc9e2d51) & M32


def group_counts(block, tbits):
    """entries per group of one block (uint8 array of 1 .. 65 536 bytes)"""
    n = len(block)
    b = np.concatenate([np.asarray(block, np.uint8), np.zeros(3, np.uint8)]).astype(np.uint32)
    words = b[:n] | (b[1:n + 1] << 8) | (b[2:n + 2] << 16) | (b[3:n + 3] << 24)
    home = mix32(words) & np.uint32((1 << tbits) - 1)
    return np.bincount(home >> (tbits - NG_BITS), minlength=NG).astype(np.int64)


def certified(c, tbits, deflate):
    """bool per group: nothing overflows out of it"""
    gw = 1 << (tbits - NG_BITS)

    def lap(x):
        out = np.empty(NG, np.int64)
        for g in range(NG):
            x = max(x + int(c[g]) - gw, int(c[g]) - 1, 0)
            out[g] = x
        return out

    if not deflate:
        return lap(0) == 0
    # one lap shrinks every carry (fewer entries than buckets): the lap that starts from the first lap's end is the fixed point
    first = lap(0)
    out = lap(int(first[-1]))
    assert out[-1] == first[-1]
    return out == 0


def parts(block, tbits, deflate, cap=2048):
    """the block's record as the rule has it: dict with n, nparts, base, fallback, part_lo, part_count, part_start, and
    `cuts`: per cut (first group of the part, boundary, group the part ends behind) in the renumbered order"""
    n = len(block)
    gshift = tbits - NG_BITS
    c = group_counts(block, tbits)
    safe = certified(c, tbits, deflate)
    if deflate and not safe.any():
        return dict(n=n, fallback=1)
    gstart = (int(np.flatnonzero(safe)[0]) + 1) % NG if deflate else 0
    c, safe = np.roll(c, -gstart), np.roll(safe, -gstart)
    cum = np.cumsum(c)                                     # entries in renumbered groups 0 .. g
    span = (65536 >> gshift) if gshift <= 6 else NG
    first, cuts, glo, cur = [0], [], 0, 0
    while n - cur > cap:
        end = min(glo + span, NG - 1)                      # the last group always belongs to the last part

        def last_certified(limit):
            boundary = min(int(np.searchsorted(cum, limit, side="right")), end)      # first group above the limit
            ok = np.flatnonzero(safe[glo:boundary])
            return (glo + int(ok[-1]) if ok.size else None), boundary

        g, boundary = last_certified(cur + cap)
        if g is None:
            if n - cur <= CAP_WIDE:
                break
            g, boundary = last_certified(cur + CAP_WIDE)
        if g is None or len(first) + 2 > MAXPARTS:
            return dict(n=n, fallback=1)
        cuts.append((glo, boundary, g))
        cur, glo = int(cum[g]), g + 1
        first.append(glo)
    start = np.array([int(cum[g - 1]) if g else 0 for g in first], np.int64)
    count = np.diff(np.append(start, n))
    return dict(n=n, nparts=len(first), base=gstart << gshift, fallback=int((count > CAP_WIDE).any()),
                part_lo=np.array(first, np.int64) << gshift, part_count=count, part_start=start, cuts=cuts,
                safe=safe, cum=cum, cap=cap, span=span)


def self_check(r, tbits):
    """what the rule promises of a record that does not fall back"""
    assert not r["fallback"]
    gshift = tbits - NG_BITS
    lo, cnt = r["part_lo"], r["part_count"]
    assert lo[0] == 0 and np.all(np.diff(lo) > 0) and lo[-1] < (1 << tbits), "the parts cover [0, T) in order"
    assert cnt.sum() == r["n"] and np.array_equal(np.cumsum(cnt) - cnt, r["part_start"]), "the counts sum to n"
    assert np.all(cnt <= CAP_WIDE), "no part above what stage 2 holds"
    for k, (glo, boundary, g) in enumerate(r["cuts"]):
        assert r["safe"][g] and glo <= g < boundary, "every cut lies on a certified group"
        if cnt[k] > r["cap"]:                              # a wide part: only where no certified group lay within the cap
            within = int(np.searchsorted(r["cum"], r["part_start"][k] + r["cap"], side="right"))
            assert not r["safe"][glo:min(within, glo + r["span"], NG - 1)].any(), "a part above the cap although a cut fitted"
        assert lo[k + 1] == (g + 1) << gshift
        assert (g + 1 - glo) <= r["span"], "a part of a small table stays within 2^16 homes"
        if cnt[k] <= r["cap"]:                             # greedy: the next certified group would not have fitted
            nxt = np.flatnonzero(r["safe"][g + 1:min(glo + r["span"], NG - 1)])
            assert nxt.size == 0 or r["cum"][g + 1 + nxt[0]] - r["part_start"][k] > r["cap"], "a part ends at the LAST cut that fits"


def lookback(r):
    """per cut: how many groups the part's last group lies below the boundary's predecessor (0: the group in front of the boundary)"""
    return [boundary - 1 - g for glo, boundary, g in r["cuts"]]


def block_with_distant_cut(seed=4, n=32768, tbits=20, band=(7000, 400)):
    """A block of n bytes for the deflate flavour in which one cut's last certified group lies at least 64 groups below the
    cut's boundary: every fourth word is free to choose (mix32 is inverted), and `band` = (first group, groups) gets two of
    them per group, in different buckets — c = 2 everywhere, so out = 1 and no group of the band is certified.  The other bytes
    are seeded noise, about two entries per group."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    gshift = tbits - NG_BITS
    g0, ng = band
    slots = rng.permutation(n // 4 - 1)[:2 * ng]
    for i, s in enumerate(slots):
        home = ((g0 + i // 2) << gshift) + (i % 2) * 17 + int(rng.integers(0, 16))
        w = unmix32(home | (int(rng.integers(0, 1 << (32 - tbits))) << tbits))
        data[4 * s:4 * s + 4] = np.frombuffer(int(w).to_bytes(4, "little"), np.uint8)
    return data
