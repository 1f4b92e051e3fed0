"""Mode Z on the GPU: standard DEFLATE streams that stock zlib / gzip inflate, with the reference's tokens."""
import ctypes as C
import gzip
import heapq
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import rfc1951_tokens as R
from compression_algorithms_amd import lz, synth

pytestmark = pytest.mark.gpu

HDR = {"raw": 0, "zlib": 2, "gzip": 10}


def _inflate(x, container):
    if container == "raw":
        return zlib.decompress(x, -15)
    if container == "zlib":
        return zlib.decompress(x)
    return gzip.decompress(x)


def _text(n, seed=1):
    return synth.enwik_like(n, seed=seed).numpy().tobytes()


def _encode(data, container="gzip", block=65536, **kw):
    st = lz.compress_z(data, lz.params("deflate", block=block), container, **kw)
    x = st.tobytes()
    return x, [int(v) for v in st.block_bits.cpu()]


def _t_tokens(data, block):
    """mode-T tokens per block (byte tokens {0,c} / {1,dlo,dhi,len})"""
    st = lz.compress(data, lz.params("deflate", block=block))
    raw, bits = st.tobytes(), [int(v) for v in st.block_bits.cpu()]
    out = []
    for b in range(len(bits) - 1):
        s, e = bits[b] // 8, bits[b + 1] // 8
        toks, i = [], s
        while i < e:
            if raw[i] == 0:
                toks.append((raw[i + 1],)); i += 2
            else:
                toks.append((raw[i + 3], raw[i + 1] | raw[i + 2] << 8)); i += 4
        out.append(toks)
    return out


def _clip(toks, data):
    """the mode-Z rule: the block's last match is clipped at the block end (>= 3: a match, else literals)"""
    pos = sum(1 if len(t) == 1 else t[0] for t in toks[:-1])
    t = toks[-1]
    if len(t) == 2 and pos + t[0] > len(data):
        L = len(data) - pos
        return toks[:-1] + ([(L, t[1])] if L >= 3 else [(c,) for c in data[pos:]])
    return toks


def _cases():
    rng = np.random.default_rng(3)
    c = {
        "text1m": _text(1_000_000),
        "zeros": bytes(300_000),
        "one_byte": b"\x41" * 200_000,
        "random": rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes(),
    }
    for per in (3, 4, 16384, 16385, 32767):
        unit = rng.integers(0, 256, per, dtype=np.uint8).tobytes()
        c[f"period{per}"] = (unit * (200_000 // per + 2))[:200_000]
    for n in (0, 1, 2, 3, 4, 5, 65535, 65536, 65537, 3 * 65536 + 7):
        c[f"size{n}"] = _text(n, seed=n % 7 + 1) if n else b""
    # a 0x00 run close to every block end: the last match runs into the zero tail and is clipped
    t = bytearray(_text(5 * 4096 + 100, seed=9))
    for b in range(1, 6):
        for k in (1, 2, 3, 5):
            t[b * 4096 - k] = 0
    c["tail_zeros"] = bytes(t)
    return c


CASES = _cases()


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_round_trip_stock_zlib(name, container):
    data = CASES[name]
    for block in (65536, 4096):
        x, bits = _encode(data, container, block)
        assert _inflate(x, container) == data, (name, block)
        assert len(x) <= lz.bound_bytes_z(len(data), lz.params("deflate", block=block), container)
        assert bits[0] == 8 * HDR[container] and all(v % 8 == 0 for v in bits)


def test_ten_megabytes_and_gzip_tool(tmp_path):
    data = _text(10_000_000, seed=5)
    x, _ = _encode(data, "gzip")
    assert gzip.decompress(x) == data
    assert len(x) < len(data) // 2
    if shutil.which("gzip") or os.path.exists("/usr/bin/gzip"):
        f = tmp_path / "t.gz"
        f.write_bytes(x)
        subprocess.check_call([shutil.which("gzip") or "/usr/bin/gzip", "-t", str(f)])


def test_incompressible_is_stored():
    data = np.random.default_rng(8).integers(0, 256, 3 * 65536 + 11, dtype=np.uint8).tobytes()
    x, bits = _encode(data, "raw")
    assert len(x) <= lz.bound_bytes_z(len(data), lz.params("deflate"), 0)
    assert zlib.decompress(x, -15) == data
    for b in range(3):                                       # (the 11-byte tail block is shorter as fixed Huffman)
        st = R.read(x[bits[b] // 8: bits[b + 1] // 8], stop_at_end=False)
        assert [k.btype for k in st.blocks] == [0, 0, 0]     # 65 535 + 1 bytes, then the sync flush
    assert bits[3] - bits[0] == 8 * 3 * (65536 + 15)


@pytest.mark.parametrize("name,block", [("text1m", 65536), ("tail_zeros", 4096), ("size196615", 65536), ("period3", 4096)])
def test_token_parity_and_codes(name, block):
    data = CASES[name][:300_000]
    x, bits = _encode(data, "raw", block)
    want = _t_tokens(data, block)
    assert len(bits) - 1 == len(want)
    for b in range(len(bits) - 1):
        blk = data[b * block:(b + 1) * block]
        st = R.read(x[bits[b] // 8: bits[b + 1] // 8], stop_at_end=False)
        assert st.data == blk
        assert st.blocks[-1].btype == 0 and not st.blocks[-1].tokens and x[bits[b + 1] // 8 - 4: bits[b + 1] // 8] == b"\0\0\xff\xff"
        body = st.blocks[:-1]
        if body[0].btype in (1, 2):
            assert len(body) == 1
            assert st.tokens == _clip(want[b], blk), (name, b)
        for k in body:
            if k.btype == 2:
                assert max(k.lit_lengths) <= 15 and max(k.dist_lengths) <= 15 and max(k.cl_lengths) <= 7
                for lens in (k.lit_lengths, k.dist_lengths, k.cl_lengths):
                    num, den = R.kraft(lens)
                    assert num == den, "incomplete or over-subscribed code"
                assert k.lit_lengths[256] > 0


def _huffman_depth(freq):
    """height of an unlimited Huffman tree over the nonzero frequencies (heapq order; ties among equal counts can move it
    by a level, the crafted block below has three to spare)"""
    h = [(f, i, 0) for i, f in enumerate(freq) if f]
    heapq.heapify(h)
    k = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        k += 1
        heapq.heappush(h, (a[0] + b[0], k, max(a[2], b[2]) + 1))
    return h[0][2]


def _rfc_histogram(toks):
    """literal/length histogram of a token list, end-of-block included"""
    f = [0] * 286
    for t in toks:
        f[t[0] if len(t) == 1 else 257 + max(i for i in range(28) if R.LEN_BASE[i] <= t[0])] += 1        # (lengths <= 255)
    f[256] += 1
    return f


def _skewed_block(k=14, filler=200, seed=0):
    """one 64 KiB block: bytes 1..k with Fibonacci counts 1, 2, 3, 5, ... (with end-of-block's single count an exact
    Fibonacci chain) spread among `filler` byte values of equal count.  Random order: no 4-byte word repeats, every token
    is a literal, and the unlimited Huffman tree is ~18 deep (the chain ~13 levels under a ~6-level tree of the filler)."""
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


def test_length_limiter_reached():
    data = _skewed_block()
    toks = _t_tokens(data, 65536)[0]
    assert _huffman_depth(_rfc_histogram(toks)) > 15, "the crafted block does not need the limiter"
    for container in ("raw", "zlib", "gzip"):
        x, bits = _encode(data, container)
        assert _inflate(x, container) == data
        st = R.read(x[bits[0] // 8: bits[1] // 8], stop_at_end=False)
        assert [b.btype for b in st.blocks] == [2, 0]
        k = st.blocks[0]
        assert max(k.lit_lengths) == 15 and max(k.dist_lengths) <= 15 and max(k.cl_lengths) <= 7
        for lens in (k.lit_lengths, k.dist_lengths, k.cl_lengths):
            num, den = R.kraft(lens)
            assert num == den, "incomplete or over-subscribed code"
        assert st.tokens == toks


def _clip_blocks(block=4096, seed=3):
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


def test_clip_both_kinds():
    block = 4096
    data = _clip_blocks(block)
    want = _t_tokens(data, block)
    x, bits = _encode(data, "raw", block)
    assert zlib.decompress(x, -15) == data
    for b, keep in enumerate((1, 2, 3, 4)):
        blk = data[b * block:(b + 1) * block]
        last = want[b][-1]
        pos = sum(1 if len(t) == 1 else t[0] for t in want[b][:-1])
        assert len(last) == 2 and pos == block - keep and last[0] > keep       # a match that overshoots the block end
        got = R.read(x[bits[b] // 8: bits[b + 1] // 8], stop_at_end=False).tokens
        assert got == _clip(want[b], blk)
        if keep < 3:
            assert got[-keep:] == [(c,) for c in blk[-keep:]] and got[:-keep] == want[b][:-1]      # literals
        else:
            assert got[-1] == (keep, last[1]) and got[:-1] == want[b][:-1]                          # a shorter match


def test_block_table_restart_points():
    data = _text(700_000, seed=2)
    for container in ("raw", "gzip"):
        x, bits = _encode(data, container)
        assert bits[0] == 8 * HDR[container]
        for b in range(len(bits) - 1):
            d = zlib.decompressobj(-15)
            assert d.decompress(x[bits[b] // 8: bits[b + 1] // 8]) == data[b * 65536:(b + 1) * 65536]
        assert x[bits[-1] // 8: bits[-1] // 8 + 2] == b"\x03\x00"


def test_checksums_match_zlib():
    ctx = lz.default_context()
    rng = np.random.default_rng(4)
    big = torch.from_numpy(rng.integers(0, 256, 3 * 65536 + 64, dtype=np.uint8)).cuda()
    hb = big.cpu().numpy().tobytes()
    res = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens = list(range(0, 71)) + [65535, 65536, 65537, 2 * 65536 - 1, 2 * 65536 + 1, 3 * 65536 + 1]
    for start in (0, 1, 3, 7):
        for n in lens:
            for fn, ref in (("mi_crc32_dev", zlib.crc32), ("mi_adler32_dev", zlib.adler32)):
                st = getattr(ctx.L, fn)(ctx.h, C.c_void_p(big.data_ptr() + start), n, C.c_void_p(res.data_ptr()), ctx.stream_ptr())
                assert st == 0
                assert int(res.item()) & 0xFFFFFFFF == ref(hb[start:start + n]), (fn, start, n)
    data = _text(100_000_000, seed=6)
    assert lz.crc32(data) == zlib.crc32(data)
    assert lz.adler32(data) == zlib.adler32(data)


def test_determinism_host_entry_and_large_input():
    data = _text(3_000_000, seed=7)
    for container in ("raw", "zlib", "gzip"):
        x1, b1 = _encode(data, container)
        x2, b2 = _encode(data, container)
        assert x1 == x2 and b1 == b2
        xh, bh = lz.compress_z_host(data, None, container)
        assert xh == x1 and bh == b1
    big = _text(100_000_000, seed=8)
    x, _ = _encode(big, "zlib")
    assert zlib.decompress(x) == big


def test_errors():
    ctx = lz.default_context()
    data = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    out = torch.empty(4096, dtype=torch.uint8, device="cuda")
    bits = torch.zeros(4, dtype=torch.int64, device="cuda")

    def enc(p, container, cap=4096):
        return ctx.L.mi_deflate_z_encode_dev(ctx.h, C.byref(p), container, C.c_void_p(data.data_ptr()), 1000, C.c_void_p(out.data_ptr()),
                                             cap, C.c_void_p(bits.data_ptr()), C.c_void_p(bits[3:].data_ptr()), ctx.stream_ptr())
    p = lz.params("deflate")
    assert enc(p, 0) == 0
    q = lz.params("deflate"); q.wbits = 16
    assert enc(q, 0) == 1
    assert enc(lz.params("lz77"), 0) == 1
    q = lz.params("deflate"); q.block = 65792
    assert enc(q, 0) == 1
    assert enc(p, 3) == 1
    for c in (0, 1, 2):
        bound = lz.bound_bytes_z(1000, p, c)
        assert enc(p, c, bound - 1) == 4
        assert enc(p, c, bound) == 0
    torch.cuda.synchronize()


def test_seeded_random_cases():
    rng = np.random.default_rng(20261016)
    for i in range(100):
        fam = int(rng.integers(0, 4))
        n = int(rng.choice([rng.integers(0, 300), rng.integers(0, 70_000), rng.integers(0, 400_000)]))
        block = int(rng.choice([65536, 65535, 32768, 4096, 1000, 257]))
        if fam == 0:
            data = _text(n, seed=i + 1) if n else b""
        elif fam == 1:
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif fam == 2:
            data = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
        else:
            unit = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            data = (unit * (n // len(unit) + 1))[:n]
        container = ["raw", "zlib", "gzip"][i % 3]
        x, _ = _encode(data, container, block)
        assert _inflate(x, container) == data, (i, fam, n, block, container)
