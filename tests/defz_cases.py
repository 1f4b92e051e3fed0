"""Inputs for the mode-Z tests (a helper module, not a conftest): the case families, the clip blocks, the crafted limiter
blocks and the 100 seeded cases.  Shared by the CPU oracle tests and the GPU tests, so both see the same bytes."""
import numpy as np

from compression_algorithms_amd import synth

BLOCKS = (65536, 65535, 4096, 1000, 257)


def text(n, seed=1):
    return synth.enwik_like(n, seed=seed).numpy().tobytes()


def cases():
    """name -> bytes: text, zeros, one byte, random, periods 3 to 32767, the sizes 0..5 and 65535..65537, tail zeros"""
    rng = np.random.default_rng(3)
    c = {
        "text1m": text(1_000_000),
        "zeros": bytes(300_000),
        "one_byte": b"\x41" * 200_000,
        "random": rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes(),
    }
    for per in (3, 4, 16384, 16385, 32767):
        unit = rng.integers(0, 256, per, dtype=np.uint8).tobytes()
        c[f"period{per}"] = (unit * (200_000 // per + 2))[:200_000]
    for n in (0, 1, 2, 3, 4, 5, 65535, 65536, 65537, 3 * 65536 + 7):
        c[f"size{n}"] = text(n, seed=n % 7 + 1) if n else b""
    # a 0x00 run close to every block end: the last match runs into the zero tail and is clipped
    t = bytearray(text(5 * 4096 + 100, seed=9))
    for b in range(1, 6):
        for k in (1, 2, 3, 5):
            t[b * 4096 - k] = 0
    c["tail_zeros"] = bytes(t)
    return c


def clip_blocks(block=4096, seed=3):
    """four blocks whose last token is a match into the zero tail covering 1, 2, 3 and 4 real bytes: the tag of `keep`
    bytes is followed by 12 zeros early in the block and ends the block"""
    rng = np.random.default_rng(seed)
    out = []
    for keep in (1, 2, 3, 4):
        b = rng.integers(64, 256, block, dtype=np.uint8)
        tag = np.array([7, 9, 11, 13][:keep], dtype=np.uint8)
        b[100:100 + keep] = tag
        b[100 + keep:112 + keep] = 0
        b[block - keep:] = tag
        out.append(b)
    return np.concatenate(out).tobytes()


def skewed_block(k=14, filler=200, seed=0):
    """one 64 KiB block: bytes 1..k with Fibonacci counts 1, 2, 3, 5, ... (with end-of-block's single count an exact
    Fibonacci chain) spread among `filler` byte values of equal count.  Random order: no 4-byte word repeats, every token
    is a literal, and the unlimited Huffman tree is ~18 deep (the chain ~13 levels under a ~6-level tree of the filler):
    the literal/length code takes the limiter (15)."""
    rng = np.random.default_rng(seed)
    fib = [1, 2]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    rare = np.repeat(np.arange(1, k + 1, dtype=np.uint8), fib)
    m = 65536 - rare.size
    fill = np.repeat(np.arange(32, 32 + filler, dtype=np.uint8), (m + filler - 1) // filler)[:m]
    d = np.concatenate([rare, fill])
    rng.shuffle(d)
    return d.tobytes()


FIB11 = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89)
CL_PERM = (4, 6, 7, 2, 0, 3, 5, 10, 9, 8, 1)


def cl_limit_block(seed=0, perm=CL_PERM):
    """one 64 KiB block whose code-length code takes the 7-bit limiter.  Target literal code lengths 5..15 are given to
    byte values in the Fibonacci counts 1, 1, 2, ..., 89 (permuted by `perm`), the other byte values get 8; each byte
    value then occurs in proportion to 2^-target.  The literal/length lengths come out close to the targets, so the
    run-length symbols (one per length: no long runs in a shuffled assignment) carry counts near a Fibonacci chain, whose
    unlimited Huffman code is deeper than 7.  The seed was searched with the CPU oracle (tests/test_oracle_defz.py
    asserts that its flag fires)."""
    rng = np.random.default_rng(seed)
    counts = [FIB11[i] for i in perm]
    vals = list(range(5, 16)) + [8]
    counts = counts + [256 - sum(counts)]
    tl = np.concatenate([np.full(c, v) for v, c in zip(vals, counts)])
    rng.shuffle(tl)
    w = 2.0 ** (-tl.astype(float))
    f = np.maximum(1, np.round(w / w.sum() * 65535)).astype(np.int64)
    d = np.repeat(np.arange(256, dtype=np.uint8), f)
    rng.shuffle(d)
    return d[:65536].tobytes()


DIST_SEED = 3


def dist_limit_block(seed=DIST_SEED, codes=range(10, 27)):
    """one 64 KiB block whose distance code takes the limiter (15): random bytes with 6-byte copies (LZ semantics: a copy
    may overlap its source) at distance codes 10..26 in Fibonacci counts 1, 1, 2, ..., 1597, the rarest code the longest
    distance, 7 fresh bytes between copies.  Every copy's source is fresh bytes (the distance is chosen inside its code's
    range so), so the finder's match is that copy and the distance histogram is the chain: 17 codes, depth 16.  The seed
    was checked with the CPU oracle (tests/test_oracle_defz.py asserts the flag)."""
    from rfc1951_tokens import DIST_BASE, DIST_EXTRA
    rng = np.random.default_rng(seed)
    codes = list(codes)
    fib = [1, 1]
    while len(fib) < len(codes):
        fib.append(fib[-1] + fib[-2])
    seq = np.repeat(np.asarray(codes[::-1]), fib)             # the longest distance once, the shortest most often
    rng.shuffle(seq)
    d = rng.integers(0, 256, 65536, dtype=np.uint8)
    fresh = np.ones(65536, dtype=bool)
    p = 8300
    for c in seq:
        base, span = DIST_BASE[int(c)], 1 << DIST_EXTRA[int(c)]
        for dist in range(base, base + span):
            if fresh[p - dist:min(p, p - dist + 6)].all():
                break
        for k in range(6):
            d[p + k] = d[p + k - dist]
        fresh[p:p + 6] = False
        p += 6 + 7
    return d.tobytes()


def seeded_cases():
    """the 100 seeded cases of test_seeded_random_cases: (i, fam, data, block, container)"""
    rng = np.random.default_rng(20261016)
    out = []
    for i in range(100):
        fam = int(rng.integers(0, 4))
        n = int(rng.choice([rng.integers(0, 300), rng.integers(0, 70_000), rng.integers(0, 400_000)]))
        block = int(rng.choice([65536, 65535, 32768, 4096, 1000, 257]))
        if fam == 0:
            data = text(n, seed=i + 1) if n else b""
        elif fam == 1:
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif fam == 2:
            data = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
        else:
            unit = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            data = (unit * (n // len(unit) + 1))[:n]
        out.append((i, fam, data, block, ["raw", "zlib", "gzip"][i % 3]))
    return out
