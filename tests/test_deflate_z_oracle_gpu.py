"""Mode Z on the GPU against the CPU oracle (oracle/orc_defz.c), byte for byte: every record, the block table, the
container header and trailer.  A round trip passes for any valid DEFLATE stream; these tests also see a wrong block type,
limiter, header trimming or run-length rule."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import defz_cases as D
from compression_algorithms_amd import lz
from oracle import orc

pytestmark = pytest.mark.gpu

CASES = D.cases()


def _gpu(data, container, block):
    st = lz.compress_z(data, lz.params("deflate", block=block), container)
    return st.tobytes(), [int(v) for v in st.block_bits.cpu()]


def _first_diff(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return k


def _same(data, block, tokens=None, containers=("raw", "zlib", "gzip"), what=""):
    tokens = tokens if tokens is not None else orc.deflate_stream(data, block, True)
    for c in containers:
        want, wbits = orc.defz_stream(data, block, c, tokens=tokens)
        got, gbits = _gpu(data, c, block)
        if got != want or gbits != wbits:
            bad = next((b for b in range(len(wbits)) if b >= len(gbits) or gbits[b] != wbits[b]), None)
            raise AssertionError(f"{what} block {block} {c}: {len(got)} vs {len(want)} bytes, first byte differing at "
                                 f"{_first_diff(got, want)}, first table entry differing {bad}")


@pytest.mark.parametrize("block", D.BLOCKS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_record_is_the_oracles(name, block):
    _same(CASES[name], block, what=name)


def test_clip_blocks_are_the_oracles():
    _same(D.clip_blocks(4096), 4096, what="clip")


def test_seeded_random_cases_are_the_oracles():
    for i, fam, data, block, container in D.seeded_cases():
        _same(data, block, containers=(container,), what=f"case {i} (family {fam}, n {len(data)})")


@pytest.mark.parametrize("name,flag", [("skewed", "lim_ll"), ("cl_limit", "lim_cl"), ("dist_limit", "lim_dc")])
def test_crafted_limiter_blocks(name, flag):
    """the literal/length (15), code-length (7) and distance (15) limiters, each on a block built to need it (the CPU
    test asserts the oracle's flag)"""
    data = {"skewed": D.skewed_block, "cl_limit": D.cl_limit_block, "dist_limit": D.dist_limit_block}[name]()
    tok = orc.deflate_stream(data, 65536, True)
    _, info = orc.defz_record(tok[0], data)
    assert info[flag] == 1
    _same(data, 65536, tokens=tok, what=name)


# ---------------------------------------------------------------- beyond 4 GiB
BIG = (1 << 32) + 4099
TILE = 1_000_003                                                       # (odd: the blocks of the tiled input all differ)


@pytest.fixture(scope="module")
def tiled():
    """a device buffer of BIG + 3 bytes: a text tile repeated (cheap to make, to checksum on the host and to cut blocks from)"""
    tile = D.text(TILE, seed=11)
    dev = torch.frombuffer(bytearray(tile), dtype=torch.uint8).cuda()
    buf = dev.repeat((BIG + 3 + TILE - 1) // TILE)[:BIG + 3]
    torch.cuda.synchronize()
    return tile, buf


def _host_range(tile, start, n):
    """the tiled bytes [start, start + n) in pieces of at most one tile"""
    at = start
    while at < start + n:
        k = at % TILE
        m = min(TILE - k, start + n - at)
        yield tile[k:k + m]
        at += m


def _zlib_of(tile, start, n, fn):
    v = fn(b"")
    for piece in _host_range(tile, start, n):
        v = fn(piece, v)
    return v


def test_checksums_beyond_4gib(tiled):
    tile, buf = tiled
    ctx = lz.default_context()
    res = torch.zeros(1, dtype=torch.int32, device="cuda")
    for start in (0, 3):
        for fn, ref in (("mi_crc32_dev", zlib.crc32), ("mi_adler32_dev", zlib.adler32)):
            st = getattr(ctx.L, fn)(ctx.h, C.c_void_p(buf.data_ptr() + start), BIG, C.c_void_p(res.data_ptr()), ctx.stream_ptr())
            assert st == 0
            assert int(res.item()) & 0xFFFFFFFF == _zlib_of(tile, start, BIG, ref), (fn, start)


def test_gzip_encode_beyond_4gib(tiled):
    tile, buf = tiled
    data = buf[:BIG]
    block = 65536
    st = lz.compress_z(data, lz.params("deflate", block=block), "gzip")
    nbytes = st.nbytes
    bits = st.block_bits.cpu().numpy()
    nblocks = (BIG + block - 1) // block
    assert len(bits) == nblocks + 1 and bits[0] == 80
    tail = st.data[nbytes - 10: nbytes].cpu().numpy().tobytes()
    assert tail[:2] == b"\x03\x00" and int(bits[-1]) // 8 == nbytes - 10
    assert int.from_bytes(tail[2:6], "little") == _zlib_of(tile, 0, BIG, zlib.crc32)
    assert int.from_bytes(tail[6:10], "little") == BIG % (1 << 32)
    rng = np.random.default_rng(4099)
    picks = sorted(set(rng.integers(0, nblocks, 6).tolist()) | {0, nblocks - 2, nblocks - 1, (1 << 32) // block})
    for b in picks:
        n = min(block, BIG - b * block)
        blk = b"".join(_host_range(tile, b * block, n))
        rec = st.data[int(bits[b]) // 8: int(bits[b + 1]) // 8].cpu().numpy().tobytes()
        assert zlib.decompressobj(-15).decompress(rec) == blk, b                 # inflates from its restart point
        tok, _ = orc.deflate_stream(blk, block, True)
        want, _ = orc.defz_record(tok, blk)
        assert rec == want, b
