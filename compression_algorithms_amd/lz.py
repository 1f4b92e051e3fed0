"""Host-side mirror of the reference's LZ77 interfaces over the HIP path.

  lz77 flavour     algorithms/lz77/lz77.h:55-63    lz77_compress / lz77_decompress
  deflate flavour  algorithms/deflate/lz77.h:47-53 per-block lz77_compress (fresh table per block)

Both are block-parallel: the input is cut into `block`-byte blocks that are encoded
independently exactly as the reference encodes a buffer of that size.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import as_device_bytes, default_context


def params(flavour="deflate", wbits=None, block=65536, parse=0):
    """parse: 0 the reference's greedy parse; 1 the lazy parse with matches up to 255 bytes, for the standard-DEFLATE writers
    only (compress_z, compress_bgzf, deflate_batch and their host forms; include/mi_codec.h, mode Z) and for
    snappy_compress_batch and lz4_compress_batch, which run the same pipeline"""
    if flavour == "deflate":
        return _lib.LzParams(15, 5, 20, 1, block, parse)
    if flavour == "lz77":
        wb = 14 if wbits is None else wbits
        return _lib.LzParams(wb, 4, wb + 6, 0, block, parse)
    raise ValueError(flavour)


def find_all(data, p, ctx=None):
    """find() at every position of every block -> uint16 tensor (0xFFFF = none)."""
    ctx = ctx or default_context()
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    cand = torch.empty(max(n, 1), dtype=torch.int16, device=ctx.device)
    st = ctx.L.mi_lz_find_all_dev(ctx.h, C.byref(p), C.c_void_p(d_in.data_ptr()), n, C.c_void_p(cand.data_ptr()),
                                  ctx.stream_ptr())
    _lib.check(st, "mi_lz_find_all_dev")
    return cand[:n]


def find_all32(data, p, ctx=None):
    """find() at every position of every block, for blocks above 64 KiB -> int32 tensor viewed as uint32 (0xFFFFFFFF = none)."""
    ctx = ctx or default_context()
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    cand = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device)
    st = ctx.L.mi_lz_find_all32_dev(ctx.h, C.byref(p), C.c_void_p(d_in.data_ptr()), n, C.c_void_p(cand.data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_lz_find_all32_dev")
    return cand[:n]


class LzStream:
    """A block-parallel LZ77 stream on the device.

    data        uint8 tensor, the concatenated block streams (lz77 flavour: bit-contiguous)
    block_bits  int64 tensor [nblocks+1], exclusive prefix of per-block lengths in BITS
    """

    def __init__(self, data, block_bits, n, p, ctx=None, violations_before=0):
        self.data, self.block_bits, self.n, self.p = data, block_bits, n, p
        self._ctx, self._v0 = ctx, violations_before

    def check_order(self):
        """mi_codec.h promises that a sort found out of (key, time) order is never silent: the asynchronous encoder cannot
        say so when it returns, so the first read of its result does — MiError(MI_ERR_UNSTABLE); the context ranks
        with ballots from then on, encode again."""
        if self._ctx is not None and self._ctx.order_violations() != self._v0:
            self._v0 = self._ctx.order_violations()
            raise _lib.MiError(10, "the encoder that wrote this stream reported a sort out of order")

    @property
    def total_bits(self):
        t = int(self.block_bits[-1])                       # (synchronises: the encoder has joined torch's stream)
        self.check_order()
        return t

    @property
    def nbytes(self):
        return (self.total_bits + 7) // 8

    def tobytes(self):
        return self.data[: self.nbytes].cpu().numpy().tobytes()


def bound_bytes(n, p):
    """mi_lz_bound_bytes of include/mi_codec.h (a static inline there)"""
    nblocks = (n + p.block - 1) // p.block
    if p.deflate:
        return 2 * n + 2 * nblocks + 8
    return (9 * n + nblocks * (p.wbits + p.lbits - 8) + 7) // 8 + 16


def compress(data, p, ctx=None):
    """Encode `data` as independent `p.block`-byte blocks (reference semantics per block)."""
    ctx = ctx or default_context()
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    nblocks = (n + p.block - 1) // p.block
    cap = bound_bytes(n, p) + 64
    out = torch.empty(cap, dtype=torch.uint8, device=ctx.device)
    bits = torch.zeros(nblocks + 1, dtype=torch.int64, device=ctx.device)
    v0 = ctx.order_violations()
    st = ctx.L.mi_lz_encode_dev(ctx.h, C.byref(p), C.c_void_p(d_in.data_ptr() if n else 0), n, C.c_void_p(out.data_ptr()), cap,
                                C.c_void_p(bits.data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_lz_encode_dev")
    return LzStream(out, bits, n, p, ctx, v0)


def decompress(stream, ctx=None):
    ctx = ctx or default_context()
    out = torch.empty(max(stream.n, 1), dtype=torch.uint8, device=ctx.device)
    st = ctx.L.mi_lz_decode_dev(ctx.h, C.byref(stream.p), C.c_void_p(stream.data.data_ptr()), stream.data.numel(),
                                C.c_void_p(stream.block_bits.data_ptr()), C.c_void_p(out.data_ptr()), stream.n, ctx.stream_ptr())
    _lib.check(st, "mi_lz_decode_dev")
    return out[: stream.n]


# ---- mode H: the reference's deflate token sequence, entropy coded per block (include/mi_codec.h) ----------------
def compress_h(data, p=None, ctx=None):
    """Deflate tokens (algorithms/deflate/lz77.c:199-280) + per-block dynamic Huffman over the 286-symbol
    alphabet the reference sketches (deflate/huffman.c:49-62).  Returns an LzStream whose `data` holds the
    concatenated block records and whose block_bits are record offsets in bits."""
    ctx = ctx or default_context()
    p = p or params("deflate")
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    nblocks = (n + p.block - 1) // p.block
    cap = int(ctx.L.mi_deflate_h_bound_bytes(n, C.byref(p))) + 64
    out = torch.empty(cap, dtype=torch.uint8, device=ctx.device)
    bits = torch.zeros(nblocks + 1, dtype=torch.int64, device=ctx.device)
    v0 = ctx.order_violations()
    st = ctx.L.mi_deflate_h_encode_dev(ctx.h, C.byref(p), C.c_void_p(d_in.data_ptr() if n else 0), n, C.c_void_p(out.data_ptr()),
                                       cap, C.c_void_p(bits.data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_deflate_h_encode_dev")
    return LzStream(out, bits, n, p, ctx, v0)


def decompress_h(stream, ctx=None):
    ctx = ctx or default_context()
    out = torch.empty(max(stream.n, 1), dtype=torch.uint8, device=ctx.device)
    st = ctx.L.mi_deflate_h_decode_dev(ctx.h, C.byref(stream.p), C.c_void_p(stream.data.data_ptr()), stream.data.numel(),
                                       C.c_void_p(stream.block_bits.data_ptr()), C.c_void_p(out.data_ptr()), stream.n,
                                       ctx.stream_ptr())
    _lib.check(st, "mi_deflate_h_decode_dev")
    return out[: stream.n]


# ---------------------------------------------------------------------------------------------------------------------
# the reference's first parser: lz77_compress_old (algorithms/lz77/lz77.h:51-54, lz77.c:185-262)
class WholeStream:
    """ONE lz77 stream over a whole buffer (no blocks): `data` uint8 tensor, `total_bits` = the reference's bit_index"""

    def __init__(self, data, total_bits, n, wbits, lbits):
        self.data, self.total_bits, self.n, self.wbits, self.lbits = data, total_bits, n, wbits, lbits

    @property
    def nbytes(self):
        return self.total_bits // 8 + 1                   # lz77.c:258

    def tobytes(self):
        return self.data[: self.nbytes].cpu().numpy().tobytes()


def compress_old(data, wbits=14, lbits=4, ctx=None):
    """lz77_compress_old on the GPU: longest match of the whole 2^wbits - 1 window at every token, first-longest wins, one
    stream over the whole buffer (lz_old.hip).  O(n * 2^wbits) like the reference."""
    ctx = ctx or default_context()
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    cap = int(ctx.L.mi_lz77_old_bound_bytes(n))
    out = torch.empty(cap, dtype=torch.uint8, device=ctx.device)
    bits = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    st = ctx.L.mi_lz77_old_encode_dev(ctx.h, wbits, lbits, C.c_void_p(d_in.data_ptr() if n else 0), n, C.c_void_p(out.data_ptr()), cap,
                                      C.c_void_p(bits.data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_lz77_old_encode_dev")
    return WholeStream(out, int(bits.item()), n, wbits, lbits)


def decompress_whole(stream, ctx=None):
    """decode a whole-buffer lz77 stream (lz77.c:347-377) on one wave"""
    ctx = ctx or default_context()
    out = torch.empty(max(stream.n, 1), dtype=torch.uint8, device=ctx.device)
    st = ctx.L.mi_lz77_whole_decode_dev(ctx.h, stream.wbits, stream.lbits, C.c_void_p(stream.data.data_ptr()), stream.data.numel(),
                                        stream.total_bits, C.c_void_p(out.data_ptr()), stream.n, ctx.stream_ptr())
    _lib.check(st, "mi_lz77_whole_decode_dev")
    return out[: stream.n]


# ---- mode Z: standard DEFLATE (RFC 1951) in a raw / zlib / gzip container (include/mi_codec.h) -------------------
CONTAINERS = {"raw": 0, "zlib": 1, "gzip": 2}


class ZStream:
    """A mode-Z stream on the device: `data` uint8 tensor, `block_bits` int64 tensor [nblocks+1] (bit offset of every
    record, the container header included; the last entry is where the closing 03 00 starts), `n` input bytes."""

    def __init__(self, data, block_bits, out_bytes, n, p, container, ctx=None, violations_before=0):
        self.data, self.block_bits, self._out_bytes, self.n, self.p = data, block_bits, out_bytes, n, p
        self.container = container
        self._ctx, self._v0 = ctx, violations_before

    @property
    def nbytes(self):
        b = int(self._out_bytes.item())                    # (synchronises: the encoder has joined torch's stream)
        if self._ctx is not None and self._ctx.order_violations() != self._v0:
            self._v0 = self._ctx.order_violations()
            raise _lib.MiError(10, "the encoder that wrote this stream reported a sort out of order")
        return b

    def tobytes(self):
        return self.data[: self.nbytes].cpu().numpy().tobytes()


def bound_bytes_z(n, p=None, container="gzip"):
    """mi_deflate_z_bound_bytes"""
    p = p or params("deflate")
    c = CONTAINERS.get(container, container)
    return int(_lib.lib().mi_deflate_z_bound_bytes(n, C.byref(p), c))


def compress_z(data, p=None, container="gzip", ctx=None, cap=None):
    """The reference's deflate tokens as standard DEFLATE that zlib.decompress / gzip.decompress read: one byte-aligned
    record per p.block input bytes, in container "raw" (RFC 1951), "zlib" (RFC 1950) or "gzip" (RFC 1952)."""
    ctx = ctx or default_context()
    p = p or params("deflate")
    c = CONTAINERS.get(container, container)
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    nblocks = (n + p.block - 1) // p.block if p.block else 0
    if cap is None:
        cap = bound_bytes_z(n, p, c) if c in CONTAINERS.values() else 64
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=ctx.device)
    bits = torch.zeros(nblocks + 2, dtype=torch.int64, device=ctx.device)
    v0 = ctx.order_violations()
    st = ctx.L.mi_deflate_z_encode_dev(ctx.h, C.byref(p), c, C.c_void_p(d_in.data_ptr() if n else 0), n, C.c_void_p(out.data_ptr()),
                                       cap, C.c_void_p(bits.data_ptr()), C.c_void_p(bits[nblocks + 1:].data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_deflate_z_encode_dev")
    return ZStream(out, bits[: nblocks + 1], bits[nblocks + 1:], n, p, c, ctx, v0)


def compress_z_host(data, p=None, container="gzip", ctx=None):
    """the host-buffer entry point (mi_deflate_z_encode) -> (bytes, block table as a list)"""
    ctx = ctx or default_context()
    p = p or params("deflate")
    c = CONTAINERS.get(container, container)
    buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    n = buf.size
    nblocks = (n + p.block - 1) // p.block
    cap = bound_bytes_z(n, p, c)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    bits = np.zeros(nblocks + 1, dtype=np.uint64)
    nb = C.c_uint64(0)
    st = ctx.L.mi_deflate_z_encode(ctx.h, C.byref(p), c, buf.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), cap,
                                   bits.ctypes.data_as(C.c_void_p), C.byref(nb))
    _lib.check(st, "mi_deflate_z_encode")
    return out[: nb.value].tobytes(), [int(x) for x in bits]


def _checksum(fn, data, ctx):
    ctx = ctx or default_context()
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    res = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    st = getattr(ctx.L, fn)(ctx.h, C.c_void_p(d_in.data_ptr() if n else 0), n, C.c_void_p(res.data_ptr()), ctx.stream_ptr())
    _lib.check(st, fn)
    return int(res.item()) & 0xFFFFFFFF


def crc32(data, ctx=None):
    """CRC-32 of the buffer on the GPU (the value zlib.crc32 gives)"""
    return _checksum("mi_crc32_dev", data, ctx)


def adler32(data, ctx=None):
    """Adler-32 of the buffer on the GPU (the value zlib.adler32 gives)"""
    return _checksum("mi_adler32_dev", data, ctx)


# ---- inflate: standard DEFLATE read back on the GPU from a table of restart points (include/mi_codec.h) -----------
MI_INFLATE_NO_CHECKSUM = 1


def _inflate_dev(ctx, c, block, d_stream, stream_bytes, d_bits, n, verify):
    out = torch.empty(max(n, 1), dtype=torch.uint8, device=ctx.device)
    st = ctx.L.mi_inflate_dev(ctx.h, c, block, C.c_void_p(d_stream.data_ptr()), stream_bytes, C.c_void_p(d_bits.data_ptr()),
                              C.c_void_p(out.data_ptr()), n, 0 if verify else MI_INFLATE_NO_CHECKSUM, ctx.stream_ptr())
    _lib.check(st, "mi_inflate_dev")
    return out[:n]


def decompress_z(stream, ctx=None, verify=True):
    """Inflate a ZStream on the GPU, one wave per record -> uint8 device tensor of stream.n bytes.  verify=False skips the
    comparison of the container's Adler-32 / CRC-32 with that of the decoded bytes."""
    ctx = ctx or default_context()
    return _inflate_dev(ctx, stream.container, stream.p.block, stream.data, stream.nbytes, stream.block_bits, stream.n, verify)


def gzip_header_bytes(buf):
    """length of the RFC 1952 member header at the start of `buf`"""
    if len(buf) < 10 or buf[0] != 0x1F or buf[1] != 0x8B:
        raise ValueError("not a gzip stream")
    flg, pos = buf[3], 10
    if flg & 4:
        pos += 2 + (buf[pos] | (buf[pos + 1] << 8))
    for f in (8, 16):
        if flg & f:
            pos = bytes(buf).index(b"\0", pos) + 1
    if flg & 2:
        pos += 2
    return pos


def inflate(data, n, seg_bits=None, block=None, container="gzip", ctx=None, verify=True):
    """Inflate standard DEFLATE from anywhere (bytes or a tensor) -> uint8 device tensor of n bytes.

    With seg_bits (list, array or tensor of ceil(n / block) + 1 bit offsets: the start of every segment, then the start of
    the closing part) and block: one wave per segment.  With seg_bits=None the stream is ONE segment (one wave: correct,
    slow): the wrapper finds the end of the container header, and takes the end of the DEFLATE data to be the stream's end
    without its trailer — less a closing 03 00 if the stream ends in one (mode Z, zlib's Z_FINISH after a flush); otherwise
    the last block of the stream must be the data block itself (zlib.compress).  Anything else needs a table."""
    ctx = ctx or default_context()
    c = CONTAINERS.get(container, container)
    d_stream = as_device_bytes(data, ctx.device)
    nbytes = d_stream.numel()
    if nbytes == 0:
        raise ValueError("an empty stream (the shortest DEFLATE stream is 03 00)")
    if seg_bits is None:
        if c not in CONTAINERS.values():
            raise ValueError(container)
        block = max(n, 1)
        head = bytes(d_stream[: min(nbytes, 65536 + 2048)].cpu().numpy().tobytes()) if c == 2 else b""
        start = gzip_header_bytes(head) if c == 2 else (2 if c == 1 else 0)
        end = nbytes - (8 if c == 2 else 4 if c == 1 else 0)
        if end < start:
            raise ValueError("the stream is shorter than its container")
        if n == 0:
            table = [8 * start]
        else:
            tail = bytes(d_stream[max(end - 2, start): end].cpu().numpy().tobytes())
            # 03 00 at the end is a closing block only if the data before it stops at a byte boundary, which cannot be told
            # without decoding: both readings are legal streams, so the closing-block reading is tried first
            tables = ([[8 * start, 8 * (end - 2)]] if tail == b"\x03\x00" else []) + [[8 * start, 8 * end]]
            last = None
            for t in tables:
                bits = torch.tensor(t, dtype=torch.int64, device=ctx.device)
                try:
                    return _inflate_dev(ctx, c, block, d_stream, nbytes, bits, n, verify)
                except _lib.MiError as e:
                    if e.status != 8:
                        raise
                    last = e
            raise ValueError("the stream does not inflate as one segment (corrupt, or its closing part is neither 03 00 nor "
                             "empty): pass seg_bits and block") from last
        bits = torch.tensor(table, dtype=torch.int64, device=ctx.device)
        return _inflate_dev(ctx, c, block, d_stream, nbytes, bits, n, verify)
    if not block:
        raise ValueError("seg_bits needs block")
    nseg = (n + block - 1) // block
    if torch.is_tensor(seg_bits):
        bits = seg_bits.to(device=ctx.device, dtype=torch.int64).contiguous()
    else:
        bits = torch.from_numpy(np.asarray(seg_bits, dtype=np.uint64).astype(np.int64)).to(ctx.device)
    if bits.numel() != nseg + 1:
        raise ValueError(f"seg_bits has {bits.numel()} entries, ceil(n / block) + 1 = {nseg + 1} expected")
    return _inflate_dev(ctx, c, block, d_stream, nbytes, bits, n, verify)


def decompress_z_host(data, table, n, block, container="gzip", ctx=None, verify=True):
    """the host-buffer entry point (mi_inflate), the twin of compress_z_host -> bytes"""
    ctx = ctx or default_context()
    c = CONTAINERS.get(container, container)
    buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    bits = np.ascontiguousarray(np.asarray(table, dtype=np.uint64))
    nseg = (n + block - 1) // block if block else 0
    if bits.size != nseg + 1:
        raise ValueError(f"the table has {bits.size} entries, ceil(n / block) + 1 = {nseg + 1} expected")
    out = np.zeros(max(n, 1), dtype=np.uint8)
    st = ctx.L.mi_inflate(ctx.h, c, block, buf.ctypes.data_as(C.c_void_p), buf.size, bits.ctypes.data_as(C.c_void_p),
                          out.ctypes.data_as(C.c_void_p), n, 0 if verify else MI_INFLATE_NO_CHECKSUM)
    _lib.check(st, "mi_inflate")
    return out[:n].tobytes()


# ---- BGZF: mode Z's records as independent gzip members that carry their own sizes (include/mi_codec.h) ------------
BGZF_BLOCK = 65280
BGZF_MAX_BLOCK = 65498
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class BgzfStream:
    """A BGZF stream on the device: `data` uint8 tensor, `member_bits` int64 tensor [nblocks+1] (bit offset of every
    member's first byte; the last entry is the EOF member), `n` input bytes."""

    def __init__(self, data, member_bits, out_bytes, n, p, ctx=None, violations_before=0):
        self.data, self.member_bits, self._out_bytes, self.n, self.p = data, member_bits, out_bytes, n, p
        self._ctx, self._v0 = ctx, violations_before

    @property
    def nbytes(self):
        b = int(self._out_bytes.item())                    # (synchronises: the encoder has joined torch's stream)
        if self._ctx is not None and self._ctx.order_violations() != self._v0:
            self._v0 = self._ctx.order_violations()
            raise _lib.MiError(10, "the encoder that wrote this stream reported a sort out of order")
        return b

    def tobytes(self):
        return self.data[: self.nbytes].cpu().numpy().tobytes()


def bound_bytes_bgzf(n, p=None):
    """mi_bgzf_bound_bytes (0 for a parameter set BGZF does not take)"""
    p = p or params("deflate", block=BGZF_BLOCK)
    return int(_lib.lib().mi_bgzf_bound_bytes(n, C.byref(p)))


def compress_bgzf(data, p=None, ctx=None, cap=None):
    """`data` as BGZF: what bgzip -d, samtools, gzip -d and gzip.decompress read, one member per p.block (65 280) input
    bytes, and what decompress_bgzf reads back from the bytes alone."""
    ctx = ctx or default_context()
    p = p or params("deflate", block=BGZF_BLOCK)
    d_in = as_device_bytes(data, ctx.device)
    n = d_in.numel()
    nblocks = (n + p.block - 1) // p.block if p.block else 0
    if cap is None:
        cap = bound_bytes_bgzf(n, p) or 64
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=ctx.device)
    bits = torch.zeros(nblocks + 2, dtype=torch.int64, device=ctx.device)
    v0 = ctx.order_violations()
    st = ctx.L.mi_bgzf_encode_dev(ctx.h, C.byref(p), C.c_void_p(d_in.data_ptr() if n else 0), n, C.c_void_p(out.data_ptr()), cap,
                                  C.c_void_p(bits.data_ptr()), C.c_void_p(bits[nblocks + 1:].data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_bgzf_encode_dev")
    return BgzfStream(out, bits[: nblocks + 1], bits[nblocks + 1:], n, p, ctx, v0)


def compress_bgzf_host(data, p=None, ctx=None):
    """the host-buffer entry point (mi_bgzf_encode) -> (bytes, member table as a list)"""
    ctx = ctx or default_context()
    p = p or params("deflate", block=BGZF_BLOCK)
    buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    n = buf.size
    nblocks = (n + p.block - 1) // p.block
    cap = bound_bytes_bgzf(n, p)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    bits = np.zeros(nblocks + 1, dtype=np.uint64)
    nb = C.c_uint64(0)
    st = ctx.L.mi_bgzf_encode(ctx.h, C.byref(p), buf.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), cap,
                              bits.ctypes.data_as(C.c_void_p), C.byref(nb))
    _lib.check(st, "mi_bgzf_encode")
    return out[: nb.value].tobytes(), [int(x) for x in bits]


class BgzfIndex(tuple):
    """(stream_offsets, out_offsets): int64 device tensors of members + 1 entries each, the last (stream bytes, total)"""

    def __new__(cls, stream_offsets, out_offsets, pairs):
        self = super().__new__(cls, (stream_offsets, out_offsets))
        self.pairs = pairs                                 # the [members + 1, 2] tensor mi_bgzf_inflate_dev takes
        return self

    @property
    def members(self):
        return self.pairs.shape[0] - 1

    def to_gzi(self):
        """htslib's .gzi: u64 count, then (compressed offset, uncompressed offset) of members 1..count, little-endian"""
        t = self.pairs.cpu().numpy().astype("<u8")
        count = max(self.members - 1, 0)
        return np.array([count], dtype="<u8").tobytes() + t[1:1 + count].tobytes()


def _bgzf_index_dev(ctx, d_stream, cap=None):
    nbytes = d_stream.numel()
    count = torch.zeros(2, dtype=torch.int64, device=ctx.device)
    ptr = C.c_void_p(d_stream.data_ptr() if nbytes else 0)
    if cap is None:
        st = ctx.L.mi_bgzf_index_dev(ctx.h, ptr, nbytes, None, 0, C.c_void_p(count.data_ptr()), ctx.stream_ptr())
        _lib.check(st, "mi_bgzf_index_dev")
        cap = int(count[0])
    pairs = torch.zeros((cap + 1, 2), dtype=torch.int64, device=ctx.device)
    st = ctx.L.mi_bgzf_index_dev(ctx.h, ptr, nbytes, C.c_void_p(pairs.data_ptr()), cap, C.c_void_p(count.data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_bgzf_index_dev")
    return pairs[: int(count[0]) + 1]


def bgzf_index(data, ctx=None, cap_members=None):
    """The members of a BGZF stream (bytes or a tensor), found on the GPU from the stream itself -> BgzfIndex, which unpacks
    as (stream_offsets, out_offsets) and has .to_gzi().  cap_members=None counts first."""
    ctx = ctx or default_context()
    pairs = _bgzf_index_dev(ctx, as_device_bytes(data, ctx.device), cap_members)
    return BgzfIndex(pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), pairs)


def decompress_bgzf(data, members=None, first=0, count=None, verify=True, ctx=None):
    """Inflate BGZF on the GPU from nothing but its bytes (`data`: bytes, a tensor or a BgzfStream; e.g. a file read from
    disk) -> uint8 device tensor.  members: a BgzfIndex from bgzf_index (made here if None); first / count: only that range
    of members (random access)."""
    ctx = ctx or default_context()
    if isinstance(data, BgzfStream):
        data = data.data[: data.nbytes]
    d_stream = as_device_bytes(data, ctx.device)
    if members is None:
        members = bgzf_index(d_stream, ctx)
    pairs = members.pairs if isinstance(members, BgzfIndex) else torch.stack([torch.as_tensor(members[0]), torch.as_tensor(members[1])], 1)
    pairs = pairs.to(device=ctx.device, dtype=torch.int64).contiguous()
    total = pairs.shape[0] - 1
    if count is None:
        count = total - first
    if first < 0 or count < 0 or first + count > total:
        raise ValueError(f"members [{first}, {first + count}) of {total}")
    n = int(pairs[first + count, 1] - pairs[first, 1])
    out = torch.empty(max(n, 1), dtype=torch.uint8, device=ctx.device)
    st = ctx.L.mi_bgzf_inflate_dev(ctx.h, C.c_void_p(d_stream.data_ptr()), d_stream.numel(), C.c_void_p(pairs.data_ptr()), first, count,
                                   C.c_void_p(out.data_ptr()), n, 0 if verify else MI_INFLATE_NO_CHECKSUM, ctx.stream_ptr())
    _lib.check(st, "mi_bgzf_inflate_dev")
    return out[:n]


def decompress_bgzf_host(data, ctx=None, verify=True, out_cap=None):
    """the host-buffer entry point (mi_bgzf_inflate: index + inflate), the twin of compress_bgzf_host -> bytes"""
    ctx = ctx or default_context()
    buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    if out_cap is None:                                    # the total of the members' ISIZE: a count-only index call
        count = torch.zeros(2, dtype=torch.int64, device=ctx.device)
        d = as_device_bytes(buf, ctx.device)
        st = ctx.L.mi_bgzf_index_dev(ctx.h, C.c_void_p(d.data_ptr() if buf.size else 0), buf.size, None, 0, C.c_void_p(count.data_ptr()),
                                     ctx.stream_ptr())
        _lib.check(st, "mi_bgzf_index_dev")
        out_cap = int(count[1])
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    nb = C.c_uint64(0)
    st = ctx.L.mi_bgzf_inflate(ctx.h, buf.ctypes.data_as(C.c_void_p), buf.size, out.ctypes.data_as(C.c_void_p), out_cap, C.byref(nb),
                               0 if verify else MI_INFLATE_NO_CHECKSUM)
    _lib.check(st, "mi_bgzf_inflate")
    return out[: nb.value].tobytes()


# ---- BGZF byte ranges: many (offset, length) slices of the uncompressed data in one call (include/mi_codec.h) ---------
class BgzfRead(tuple):
    """(out, out_offsets, got, status) of bgzf_read: the uint8 output, where every range's slot starts in it (int64), the
    bytes delivered per range (int64) and the verdict per range (int32), device tensors; .failed counts the ranges that are
    not MI_OK (reading it synchronises)."""

    def __new__(cls, out, out_offsets, got, status, failed):
        self = super().__new__(cls, (out, out_offsets, got, status))
        self._failed = failed
        return self

    @property
    def failed(self):
        return int(self._failed.item())


def _index_pairs(members, device):
    pairs = members.pairs if isinstance(members, BgzfIndex) else torch.stack([torch.as_tensor(members[0]), torch.as_tensor(members[1])], 1)
    return pairs.to(device=device, dtype=torch.int64).contiguous()


def bgzf_piece_counts(out_offsets, ranges):
    """The pieces of every range — one per non-empty member that holds a byte of it — from the members' output offsets
    (members + 1 entries, not decreasing) -> int64 tensor [R].  Pure torch, on whatever device the offsets live."""
    o = torch.as_tensor(out_offsets).to(torch.int64)
    r = torch.as_tensor(ranges).to(device=o.device, dtype=torch.int64).reshape(-1, 2)
    total = o[-1]
    keep = o[1:] != o[:-1]
    starts, ends = o[:-1][keep].contiguous(), o[1:][keep].contiguous()
    a = r[:, 0].contiguous()
    b = torch.minimum(a + r[:, 1], total)
    k0 = torch.searchsorted(ends, a, right=True)               # the first member that ends behind a
    k1 = torch.searchsorted(starts, b, right=False)            # the first member that starts at or behind b
    live = (r[:, 1] > 0) & (a < total)
    return torch.where(live, (k1 - k0).clamp(min=0), torch.zeros_like(k0))


def bgzf_read_max_pieces(count, total_len, min_member_bytes=BGZF_BLOCK):
    """mi_bgzf_read_max_pieces: a bound on the pieces of `count` ranges of `total_len` bytes together over members of at
    least `min_member_bytes` uncompressed bytes (bgzip: 65 280)"""
    return int(_lib.lib().mi_bgzf_read_max_pieces(count, total_len, min_member_bytes))


def bgzf_voffset_to_offset(index, voffsets):
    """htslib virtual offsets (coffset << 16 | uoffset: where the member starts in the file, and a position inside its
    uncompressed bytes) -> offsets into the uncompressed data, by the index (a BgzfIndex, or (stream offsets, output
    offsets)).  ValueError where coffset is not a member's start or uoffset exceeds that member's size.  Pure torch."""
    so, oo = torch.as_tensor(index[0]).to(torch.int64), torch.as_tensor(index[1]).to(torch.int64)
    v = torch.as_tensor(voffsets).to(device=so.device, dtype=torch.int64).reshape(-1)
    co, uo = v >> 16, v & 0xFFFF
    starts = so[:-1].contiguous()
    if starts.numel() == 0:
        if v.numel():
            raise ValueError("the index has no members")
        return v
    # (empty streams aside, member starts increase strictly: a member has at least 28 bytes)
    k = torch.searchsorted(starts, co.contiguous(), right=False).clamp(max=starts.numel() - 1)
    if bool((starts[k] != co).any()):
        bad = int(co[(starts[k] != co).nonzero()[0, 0]])
        raise ValueError(f"coffset {bad} is not the start of a member")
    size = oo[k + 1] - oo[k]
    if bool((uo > size).any()):
        i = int((uo > size).nonzero()[0, 0])
        raise ValueError(f"uoffset {int(uo[i])} exceeds the {int(size[i])} bytes of the member at {int(co[i])}")
    return oo[k] + uo


def bgzf_read(data, ranges, members=None, verify=True, ctx=None, max_pieces=None, out=None, out_offsets=None):
    """Many byte ranges of a BGZF stream's uncompressed data in one call -> BgzfRead, which unpacks as (out, out_offsets,
    got, status).  ranges: [R, 2] int64 (offset, length) tensor or array, in any order, overlapping or repeated as they
    like.  A range that ends past the end of the data is a short read (got < length, status MI_OK).  members: a BgzfIndex
    (made here if None).  max_pieces: the launch bound (None: the exact count, by torch.searchsorted over the index — one
    synchronisation; pass bgzf_read_max_pieces(...) to avoid it).  out / out_offsets: a uint8 device tensor to write into
    and where each range's slot starts in it (None: a new tensor with the slots packed back to back); slots must not
    overlap, and a slot that leaves `out` is MI_ERR_ARG for its range.  One bad range does not spoil the rest."""
    ctx = ctx or default_context()
    if isinstance(data, BgzfStream):
        data = data.data[: data.nbytes]
    if torch.is_tensor(data) and data.device == ctx.device and data.dtype == torch.uint8 and data.is_contiguous() and data.data_ptr() % 4 == 0:
        d_stream = data                                        # (the library asks for 4-byte alignment only)
    else:
        d_stream = as_device_bytes(data, ctx.device)
    if members is None:
        members = bgzf_index(d_stream, ctx)
    pairs = _index_pairs(members, ctx.device)
    r = torch.as_tensor(np.asarray(ranges, dtype=np.int64) if not torch.is_tensor(ranges) else ranges)
    r = r.to(device=ctx.device, dtype=torch.int64).reshape(-1, 2)
    count = r.shape[0]
    if bool((r < 0).any()) if count else False:
        raise ValueError("offsets and lengths must not be negative")
    d_off, d_len = r[:, 0].contiguous(), r[:, 1].contiguous()
    if out_offsets is None:
        d_at = torch.cumsum(d_len, 0) - d_len
    else:
        d_at = torch.as_tensor(out_offsets).to(device=ctx.device, dtype=torch.int64).reshape(-1).contiguous()
        if d_at.numel() != count:
            raise ValueError(f"out_offsets has {d_at.numel()} entries for {count} ranges")
    if out is None:
        need = int((d_at + d_len).max()) if count else 0
        out = torch.empty(max(need, 1), dtype=torch.uint8, device=ctx.device)
        out_bytes = need
    else:
        if not (torch.is_tensor(out) and out.device == ctx.device and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous uint8 tensor on the context's device")
        out_bytes = out.numel()
    if max_pieces is None:
        max_pieces = int(bgzf_piece_counts(pairs[:, 1], r).sum()) if count else 0
    got = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    failed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    st = ctx.L.mi_bgzf_read_ranges_dev(ctx.h, _ptr(d_stream), d_stream.numel(), C.c_void_p(pairs.data_ptr()), pairs.shape[0] - 1, count,
                                       _ptr(d_off), _ptr(d_len), C.c_void_p(out.data_ptr()), _ptr(d_at), out_bytes, max_pieces,
                                       _ptr(got), _ptr(status), _ptr(failed), 0 if verify else MI_INFLATE_NO_CHECKSUM, ctx.stream_ptr())
    _lib.check(st, "mi_bgzf_read_ranges_dev")
    return BgzfRead(out, d_at, got[:count], status[:count], failed)


def bgzf_read_host(data, ranges, ctx=None, verify=True, out=None, out_offsets=None):
    """the host-buffer entry point (mi_bgzf_read_ranges: copy up, index, read, copy down) -> (out as a numpy uint8 array,
    out_offsets, got, status as lists)"""
    ctx = ctx or default_context()
    buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
    if (r < 0).any():
        raise ValueError("offsets and lengths must not be negative")
    count = r.shape[0]
    off, ln = np.ascontiguousarray(r[:, 0]).astype(np.uint64), np.ascontiguousarray(r[:, 1]).astype(np.uint64)
    at = (np.cumsum(ln) - ln).astype(np.uint64) if out_offsets is None else np.ascontiguousarray(np.asarray(out_offsets, dtype=np.int64).reshape(-1)).astype(np.uint64)
    if at.size != count:
        raise ValueError(f"out_offsets has {at.size} entries for {count} ranges")
    if out is None:
        out_bytes = int((at + ln).max()) if count else 0
        out = np.zeros(max(out_bytes, 1), dtype=np.uint8)
    else:
        out_bytes = out.size
    got, status = np.zeros(max(count, 1), dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = ctx.L.mi_bgzf_read_ranges(ctx.h, vp(buf), buf.size, count, vp(off), vp(ln), vp(out), vp(at), out_bytes, vp(got), vp(status),
                                   0 if verify else MI_INFLATE_NO_CHECKSUM)
    _lib.check(st, "mi_bgzf_read_ranges")
    return out, [int(v) for v in at], [int(v) for v in got[:count]], [int(v) for v in status[:count]]


# ---- batched inflate: many independent raw / zlib / gzip streams in one launch (include/mi_codec.h) -------------------
def _is_packed(items):
    return (isinstance(items, tuple) and len(items) == 2 and not isinstance(items[1], (bytes, bytearray, memoryview))
            and not (torch.is_tensor(items[1]) and items[1].dtype == torch.uint8))


def _nbytes(x):
    return x.numel() if torch.is_tensor(x) else len(x)


def _batch_check(items, caps):
    """everything that can be refused without a device -> (packed?, offsets or None, count)"""
    if _is_packed(items):
        buf, offsets = items
        off = [int(v) for v in (offsets.cpu().tolist() if torch.is_tensor(offsets) else offsets)]
        if len(off) < 1:
            raise ValueError("offsets needs count + 1 entries: at least one")
        if off[0] < 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] > _nbytes(buf):
            raise ValueError(f"offsets must not decrease and must stay inside the buffer's {_nbytes(buf)} bytes")
        count = len(off) - 1
    else:
        off, count = None, len(items)
    if caps is not None and _nbytes(caps) != count:
        raise ValueError(f"caps has {_nbytes(caps)} entries for {count} items")
    return off, count


def _batch_inputs(ctx, items, off, count):
    """-> (tensors to keep alive, int64 device tensor of pointers, int64 device tensor of sizes)"""
    if off is not None:
        buf = as_device_bytes(items[0], ctx.device)
        base = buf.data_ptr()
        ptrs, sizes, keep = [base + a for a in off[:-1]], [b - a for a, b in zip(off, off[1:])], [buf]
    else:
        keep, ptrs, sizes = [], [0] * count, [0] * count
        host = [(i, bytes(x)) for i, x in enumerate(items) if not torch.is_tensor(x)]
        if host:                                               # the host items in one buffer, one copy up
            at, offs = 0, []
            for _, b in host:
                offs.append(at)
                at += (len(b) + 15) & ~15
            pack = np.zeros(max(at, 1), dtype=np.uint8)
            for (_, b), a in zip(host, offs):
                pack[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
            d = torch.from_numpy(pack).to(ctx.device)
            keep.append(d)
            for (i, b), a in zip(host, offs):
                ptrs[i], sizes[i] = d.data_ptr() + a, len(b)
        for i, x in enumerate(items):
            if torch.is_tensor(x):
                t = x.to(device=ctx.device, dtype=torch.uint8).contiguous()
                keep.append(t)
                ptrs[i], sizes[i] = (t.data_ptr() if t.numel() else 0), t.numel()
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=ctx.device) if v else torch.zeros(0, dtype=torch.int64, device=ctx.device)
    return keep, dev(ptrs), dev(sizes)


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t.numel() else 0)


def _zdict_check(zdict, c):
    """a preset dictionary (zlib's zdict: bytes or a uint8 tensor, or None) and the container: what can be refused without a device"""
    if zdict is None:
        return
    if torch.is_tensor(zdict):
        if zdict.dtype != torch.uint8 or zdict.dim() != 1:
            raise ValueError("zdict: bytes or a one-dimensional uint8 tensor")
    elif not isinstance(zdict, (bytes, bytearray, memoryview)):
        raise ValueError("zdict: bytes or a one-dimensional uint8 tensor")
    if _nbytes(zdict) and c == CONTAINERS["gzip"]:
        raise ValueError("gzip has no dictionary field: a preset dictionary goes with the raw or the zlib container")


def _zdict_dev(ctx, zdict):
    """-> the dictionary as a contiguous uint8 tensor on the context's device"""
    if torch.is_tensor(zdict):
        return zdict.to(device=ctx.device).contiguous()
    return as_device_bytes(bytes(zdict), ctx.device) if len(zdict) else torch.zeros(0, dtype=torch.uint8, device=ctx.device)


def _batch_sizes_dev(ctx, c, count, d_in, d_nb, d_dict=None):
    sizes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    if d_dict is None:
        st = ctx.L.mi_inflate_batch_size_dev(ctx.h, c, count, _ptr(d_in), _ptr(d_nb), _ptr(sizes), _ptr(status), None, 0, ctx.stream_ptr())
        _lib.check(st, "mi_inflate_batch_size_dev")
    else:
        st = ctx.L.mi_inflate_batch_dict_size_dev(ctx.h, c, count, _ptr(d_in), _ptr(d_nb), _ptr(sizes), _ptr(status), None, _ptr(d_dict),
                                                  d_dict.numel(), 0, ctx.stream_ptr())
        _lib.check(st, "mi_inflate_batch_dict_size_dev")
    return sizes[:count], status[:count]


def inflate_batch_sizes(items, container="gzip", ctx=None, zdict=None):
    """What every item of a batch inflates to, without writing a byte -> (sizes int64, status int32) device tensors.  `items`
    and `zdict` as for inflate_batch.  A checksum mismatch cannot be seen here (such an item is MI_OK)."""
    off, count = _batch_check(items, None)
    c = CONTAINERS.get(container, container)
    _zdict_check(zdict, c)
    ctx = ctx or default_context()
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    out = _batch_sizes_dev(ctx, c, count, d_in, d_nb, None if zdict is None else _zdict_dev(ctx, zdict))
    ctx.sync()                                                 # (the inputs in `keep` may go now)
    return out


class InflateBatch:
    """The result of inflate_batch: `outputs` (a list of uint8 device tensors, each cut to its size; empty where the item
    failed), `out_bytes` (int64) and `status` (int32) device tensors, `failed` (how many items are not MI_OK)."""

    def __init__(self, outputs, out_bytes, status, failed):
        self.outputs, self.out_bytes, self.status, self.failed = outputs, out_bytes, status, failed

    def raise_for_status(self):
        if self.failed:
            st = [int(v) for v in self.status.cpu()]
            i = next(k for k, v in enumerate(st) if v)
            raise _lib.MiError(st[i], f"inflate_batch: {self.failed} of {len(st)} items failed, the first one item {i}")
        return self


def inflate_batch(items, container="gzip", caps=None, verify=True, ctx=None, zdict=None):
    """Inflate many independent streams of one container ("raw", "zlib", "gzip") in one launch -> InflateBatch.

    items: a list of bytes or uint8 tensors, or a pair (buffer, offsets) for a packed buffer with count + 1 offsets (item i
    is buffer[offsets[i]:offsets[i + 1]]: no alignment needed).  caps: the output capacity of every item (list or tensor);
    None runs the size pass first and allocates one packed output.  An item that does not fit its capacity comes back
    MI_ERR_CAPACITY with out_bytes = the size it needs; one bad item does not spoil the rest.  zdict: one preset dictionary
    for all items (bytes or a uint8 device tensor), as zlib.decompressobj(wbits, zdict=...) takes it: every raw item uses
    it, a zlib item if its header names it (FDICT and the dictionary's Adler-32); gzip has no such field and is refused."""
    off, count = _batch_check(items, caps)
    c = CONTAINERS.get(container, container)
    _zdict_check(zdict, c)
    ctx = ctx or default_context()
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    d_dict = None if zdict is None else _zdict_dev(ctx, zdict)
    if caps is None:
        d_cap = _batch_sizes_dev(ctx, c, count, d_in, d_nb, d_dict)[0]
        cap = [int(v) for v in d_cap.cpu()]
    else:
        cap = [int(v) for v in (caps.cpu().tolist() if torch.is_tensor(caps) else caps)]
        d_cap = torch.tensor(cap, dtype=torch.int64, device=ctx.device) if count else torch.zeros(0, dtype=torch.int64, device=ctx.device)
    at, offs = 0, []
    for v in cap:
        offs.append(at)
        at += (min(v, 0x7FFFFFFF) + 15) & ~15                 # (a capacity above that is refused per item)
    out = torch.empty(max(at, 16), dtype=torch.uint8, device=ctx.device)
    d_out = torch.tensor([out.data_ptr() + a for a in offs], dtype=torch.int64, device=ctx.device) if count else d_cap
    nbytes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    failed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    flags = 0 if verify else MI_INFLATE_NO_CHECKSUM
    if d_dict is None:
        st = ctx.L.mi_inflate_batch_dev(ctx.h, c, count, _ptr(d_in), _ptr(d_nb), _ptr(d_out), _ptr(d_cap), _ptr(nbytes), _ptr(status),
                                        _ptr(failed), flags, ctx.stream_ptr())
        _lib.check(st, "mi_inflate_batch_dev")
    else:
        st = ctx.L.mi_inflate_batch_dict_dev(ctx.h, c, count, _ptr(d_in), _ptr(d_nb), _ptr(d_out), _ptr(d_cap), _ptr(nbytes), _ptr(status),
                                             _ptr(failed), _ptr(d_dict), d_dict.numel(), flags, ctx.stream_ptr())
        _lib.check(st, "mi_inflate_batch_dict_dev")
    ctx.sync()
    nb, stl = [int(v) for v in nbytes[:count].cpu()], [int(v) for v in status[:count].cpu()]
    outputs = [out[a:a + (n if s == 0 else 0)] for a, n, s in zip(offs, nb, stl)]
    return InflateBatch(outputs, nbytes[:count], status[:count], int(failed.item()) if count else 0)


def inflate_batch_host(items, container="gzip", ctx=None, verify=True, zdict=None):
    """the host-buffer entry point (mi_inflate_batch, called once for the sizes and once to inflate, so the inputs travel to
    the device twice: a convenience path): a list of bytes -> (list of bytes, None where the item failed; list of status
    codes).  zdict: a preset dictionary as for inflate_batch, here host bytes (mi_inflate_batch_dict)"""
    items = [bytes(x) for x in items]
    count = len(items)
    c = CONTAINERS.get(container, container)
    _zdict_check(zdict, c)
    ctx = ctx or default_context()
    if zdict is not None:
        hd = np.frombuffer(bytes(zdict.cpu().numpy().tobytes() if torch.is_tensor(zdict) else zdict), dtype=np.uint8)
        hdp = hd.ctypes.data_as(C.c_void_p) if hd.size else None
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in items]
    h_in = (C.c_void_p * max(count, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    h_nb = (C.c_uint64 * max(count, 1))(*[a.size for a in arrs])
    sizes, status = (C.c_uint64 * max(count, 1))(), (C.c_uint32 * max(count, 1))()
    flags = 0 if verify else MI_INFLATE_NO_CHECKSUM
    if zdict is None:
        call = lambda o, cp: ctx.L.mi_inflate_batch(ctx.h, c, count, h_in, h_nb, o, cp, sizes, status, flags)
    else:
        call = lambda o, cp: ctx.L.mi_inflate_batch_dict(ctx.h, c, count, h_in, h_nb, o, cp, sizes, status, hdp, hd.size, flags)
    st = call(None, None)
    _lib.check(st, "mi_inflate_batch")
    outs = [np.zeros(max(int(sizes[i]), 1), dtype=np.uint8) for i in range(count)]
    h_out = (C.c_void_p * max(count, 1))(*[o.ctypes.data for o in outs])
    h_cap = (C.c_uint64 * max(count, 1))(*[int(sizes[i]) for i in range(count)])
    st = call(h_out, h_cap)
    _lib.check(st, "mi_inflate_batch")
    return [outs[i][: int(sizes[i])].tobytes() if status[i] == 0 else None for i in range(count)], [int(status[i]) for i in range(count)]


# ---- batched deflate: many independent buffers, each a complete raw / zlib / gzip stream, in one call (include/mi_codec.h) ------
class DeflateBatch(InflateBatch):
    """The result of deflate_batch, shaped like InflateBatch: `outputs` (a list of uint8 device tensors, each cut to its stream;
    empty where the item failed), `out_bytes` (int64; the size needed where the status is MI_ERR_CAPACITY) and `status` (int32)
    device tensors, `failed` (how many items are not MI_OK)."""

    def raise_for_status(self):
        if self.failed:
            st = [int(v) for v in self.status.cpu()]
            i = next(k for k, v in enumerate(st) if v)
            raise _lib.MiError(st[i], f"deflate_batch: {self.failed} of {len(st)} items failed, the first one item {i}")
        return self


def deflate_batch_max_blocks(total_bytes, count, p=None, dict_bytes=0):
    """mi_deflate_batch_max_blocks: an upper bound on the blocks of `count` items of `total_bytes` together; dict_bytes: with a
    preset dictionary of that size (mi_deflate_batch_dict_max_blocks: an item's first block is shorter by the dictionary's tail)"""
    p = p or params("deflate")
    if dict_bytes:
        return int(_lib.lib().mi_deflate_batch_dict_max_blocks(total_bytes, count, C.byref(p), dict_bytes))
    return int(_lib.lib().mi_deflate_batch_max_blocks(total_bytes, count, C.byref(p)))


def deflate_batch_bound_bytes(n, p=None, container="gzip", dict_bytes=0):
    """mi_deflate_batch_dict_bound_bytes: the most an item of n bytes comes to, with a preset dictionary of dict_bytes"""
    p = p or params("deflate")
    return int(_lib.lib().mi_deflate_batch_dict_bound_bytes(n, C.byref(p), CONTAINERS.get(container, container), dict_bytes))


def _dict_blocks(n, block, dict_bytes):
    """the blocks of an item of n bytes behind a dictionary of dict_bytes (include/mi_codec.h)"""
    u = min(dict_bytes, 32768, block // 2)
    return 0 if n == 0 else 1 + (n - min(n, block - u) + block - 1) // block


def deflate_batch(items, p=None, container="gzip", caps=None, ctx=None, max_blocks=None, zdict=None):
    """Compress many independent buffers in one call -> DeflateBatch.  Item i's stream is byte for byte compress_z(item i).
    zdict: one preset dictionary for all items (bytes or a uint8 device tensor), as zlib.compressobj(..., zdict=...) takes it:
    the streams are what zlib.decompressobj(wbits, zdict=...) and inflate_batch(..., zdict=...) read; raw or zlib only.

    items: a list of bytes or uint8 tensors, or a pair (buffer, offsets) for a packed buffer with count + 1 offsets (item i
    is buffer[offsets[i]:offsets[i + 1]]: no alignment needed), as for inflate_batch.  caps: the output capacity of every
    item (list or tensor); None gives each item its bound in one packed output.  An item that does not fit its capacity
    comes back MI_ERR_CAPACITY with out_bytes = the size it needs; one bad item does not spoil the rest.  max_blocks: the
    launch bound (None: from the sizes, which are known here)."""
    off, count = _batch_check(items, caps)
    c = CONTAINERS.get(container, container)
    if c not in CONTAINERS.values():
        raise ValueError(f"container {container!r}: one of {sorted(CONTAINERS)}")
    _zdict_check(zdict, c)
    ctx = ctx or default_context()
    p = p or params("deflate")
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    d_dict = None if zdict is None else _zdict_dev(ctx, zdict)
    nd = 0 if d_dict is None else d_dict.numel()
    sizes = [int(v) for v in d_nb.cpu()] if count else []
    if caps is None:
        cap = [bound_bytes_z(n, p, c) if d_dict is None else deflate_batch_bound_bytes(n, p, c, nd) for n in sizes]
    else:
        cap = [int(v) for v in (caps.cpu().tolist() if torch.is_tensor(caps) else caps)]
    d_cap = torch.tensor(cap, dtype=torch.int64, device=ctx.device) if count else torch.zeros(0, dtype=torch.int64, device=ctx.device)
    at, offs = 0, []
    for v in cap:
        offs.append(at)
        at += (min(v, 0x7FFFFFFF) + 15) & ~15                 # (a capacity above that is refused per item)
    out = torch.empty(max(at, 16), dtype=torch.uint8, device=ctx.device)
    d_out = torch.tensor([out.data_ptr() + a for a in offs], dtype=torch.int64, device=ctx.device) if count else d_cap
    if max_blocks is None:
        max_blocks = sum(_dict_blocks(n, p.block, nd) for n in sizes if n <= 0x7FFFFFFF)
    nbytes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    failed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    v0 = ctx.order_violations()
    if d_dict is None:
        st = ctx.L.mi_deflate_batch_dev(ctx.h, C.byref(p), c, count, _ptr(d_in), _ptr(d_nb), max_blocks, _ptr(d_out), _ptr(d_cap),
                                        _ptr(nbytes), _ptr(status), _ptr(failed), ctx.stream_ptr())
        _lib.check(st, "mi_deflate_batch_dev")
    else:
        st = ctx.L.mi_deflate_batch_dict_dev(ctx.h, C.byref(p), c, count, _ptr(d_in), _ptr(d_nb), max_blocks, _ptr(d_out), _ptr(d_cap),
                                             _ptr(nbytes), _ptr(status), _ptr(failed), _ptr(d_dict), nd, ctx.stream_ptr())
        _lib.check(st, "mi_deflate_batch_dict_dev")
    ctx.sync()
    if ctx.order_violations() != v0:
        raise _lib.MiError(10, "the encoder that wrote this batch reported a sort out of order")
    nb, stl = [int(v) for v in nbytes[:count].cpu()], [int(v) for v in status[:count].cpu()]
    outputs = [out[a:a + (n if s == 0 else 0)] for a, n, s in zip(offs, nb, stl)]
    return DeflateBatch(outputs, nbytes[:count], status[:count], int(failed.item()) if count else 0)


def deflate_batch_host(items, p=None, container="gzip", ctx=None, zdict=None):
    """the host-buffer entry point (mi_deflate_batch): a list of bytes -> (list of bytes, None where the item failed; list of
    status codes).  zdict: a preset dictionary as for deflate_batch, here host bytes (mi_deflate_batch_dict)"""
    items = [bytes(x) for x in items]
    count = len(items)
    c = CONTAINERS.get(container, container)
    _zdict_check(zdict, c)
    ctx = ctx or default_context()
    p = p or params("deflate")
    hd = None if zdict is None else np.frombuffer(zdict.cpu().numpy().tobytes() if torch.is_tensor(zdict) else bytes(zdict), dtype=np.uint8)
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in items]
    h_in = (C.c_void_p * max(count, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    h_nb = (C.c_uint64 * max(count, 1))(*[a.size for a in arrs])
    caps = [bound_bytes_z(a.size, p, c) if hd is None else deflate_batch_bound_bytes(a.size, p, c, hd.size) for a in arrs]
    outs = [np.zeros(max(v, 1), dtype=np.uint8) for v in caps]
    h_out = (C.c_void_p * max(count, 1))(*[o.ctypes.data for o in outs])
    h_cap = (C.c_uint64 * max(count, 1))(*caps)
    sizes, status = (C.c_uint64 * max(count, 1))(), (C.c_uint32 * max(count, 1))()
    if hd is None:
        st = ctx.L.mi_deflate_batch(ctx.h, C.byref(p), c, count, h_in, h_nb, h_out, h_cap, sizes, status)
    else:
        st = ctx.L.mi_deflate_batch_dict(ctx.h, C.byref(p), c, count, h_in, h_nb, h_out, h_cap, sizes, status,
                                         hd.ctypes.data_as(C.c_void_p) if hd.size else None, hd.size)
    _lib.check(st, "mi_deflate_batch")
    return [outs[i][: int(sizes[i])].tobytes() if status[i] == 0 else None for i in range(count)], [int(status[i]) for i in range(count)]


# ---- batched Snappy: many independent RAW Snappy buffers (what snappy.compress / pyarrow's "snappy" codec write) per call ---------
class SnappyBatch(InflateBatch):
    """The result of snappy_compress_batch / snappy_decompress_batch, shaped like InflateBatch and DeflateBatch: `outputs` (a
    list of uint8 device tensors, each cut to its size; empty where the item failed), `out_bytes` (int64; the size needed where
    the status is MI_ERR_CAPACITY) and `status` (int32) device tensors, `failed` (how many items are not MI_OK)."""

    def raise_for_status(self):
        if self.failed:
            st = [int(v) for v in self.status.cpu()]
            i = next(k for k, v in enumerate(st) if v)
            raise _lib.MiError(st[i], f"snappy batch: {self.failed} of {len(st)} items failed, the first one item {i}")
        return self


def snappy_batch_bound_bytes(n, p=None):
    """mi_snappy_batch_bound_bytes: the most an item of n bytes comes to"""
    p = p or params("deflate")
    return int(_lib.lib().mi_snappy_batch_bound_bytes(n, C.byref(p)))


def _batch_outputs(ctx, cap, count):
    """one packed output for the capacities -> (buffer, its offsets, device tensors of pointers and capacities)"""
    d_cap = torch.tensor(cap, dtype=torch.int64, device=ctx.device) if count else torch.zeros(0, dtype=torch.int64, device=ctx.device)
    at, offs = 0, []
    for v in cap:
        offs.append(at)
        at += (min(v, 0x7FFFFFFF) + 15) & ~15                 # (a capacity above that is refused per item)
    out = torch.empty(max(at, 16), dtype=torch.uint8, device=ctx.device)
    d_out = torch.tensor([out.data_ptr() + a for a in offs], dtype=torch.int64, device=ctx.device) if count else d_cap
    return out, offs, d_out, d_cap


def _snappy_sizes_dev(ctx, count, d_in, d_nb):
    sizes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    st = ctx.L.mi_snappy_batch_size_dev(ctx.h, count, _ptr(d_in), _ptr(d_nb), _ptr(sizes), _ptr(status), None, ctx.stream_ptr())
    _lib.check(st, "mi_snappy_batch_size_dev")
    return sizes[:count], status[:count]


def snappy_batch_sizes(items, ctx=None):
    """The preamble of every item (what snappy's GetUncompressedLength answers) -> (sizes int64, status int32) device tensors.
    `items` as for snappy_decompress_batch.  The body is not validated: an item that is MI_OK here may still be corrupt."""
    off, count = _batch_check(items, None)
    ctx = ctx or default_context()
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    out = _snappy_sizes_dev(ctx, count, d_in, d_nb)
    ctx.sync()                                                 # (the inputs in `keep` may go now)
    return out


def snappy_decompress_batch(items, caps=None, ctx=None):
    """Decode many independent raw Snappy buffers in one launch -> SnappyBatch.

    items: a list of bytes or uint8 tensors, or a pair (buffer, offsets) for a packed buffer with count + 1 offsets (item i is
    buffer[offsets[i]:offsets[i + 1]]: no alignment needed).  caps: the output capacity of every item (list or tensor); None
    reads the preambles first and allocates one packed output.  An item whose preamble exceeds its capacity comes back
    MI_ERR_CAPACITY with out_bytes = the preamble and nothing written; a malformed one MI_ERR_CORRUPT; one bad item does not
    spoil the rest.  Raw Snappy only: not the framing format (.sz), not Hadoop's block wrapper."""
    off, count = _batch_check(items, caps)
    ctx = ctx or default_context()
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    if caps is None:
        cap = [int(v) for v in _snappy_sizes_dev(ctx, count, d_in, d_nb)[0].cpu()]
    else:
        cap = [int(v) for v in (caps.cpu().tolist() if torch.is_tensor(caps) else caps)]
    out, offs, d_out, d_cap = _batch_outputs(ctx, cap, count)
    nbytes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    failed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    st = ctx.L.mi_snappy_decode_batch_dev(ctx.h, count, _ptr(d_in), _ptr(d_nb), _ptr(d_out), _ptr(d_cap), _ptr(nbytes), _ptr(status),
                                          _ptr(failed), 0, ctx.stream_ptr())
    _lib.check(st, "mi_snappy_decode_batch_dev")
    ctx.sync()
    nb, stl = [int(v) for v in nbytes[:count].cpu()], [int(v) for v in status[:count].cpu()]
    outputs = [out[a:a + (n if s == 0 else 0)] for a, n, s in zip(offs, nb, stl)]
    return SnappyBatch(outputs, nbytes[:count], status[:count], int(failed.item()) if count else 0)


def snappy_compress_batch(items, p=None, caps=None, ctx=None, max_blocks=None):
    """Compress many independent buffers in one call, each to a raw Snappy buffer that stock Snappy reads -> SnappyBatch.

    items: as for snappy_decompress_batch.  p: params("deflate", block=..., parse=0 or 1) — the batched deflate's finder, parse
    and blocks; the format is chosen by this entry point, not by a parameter.  caps: the output capacity of every item; None
    gives each item its bound in one packed output.  An item that does not fit its capacity comes back MI_ERR_CAPACITY with
    out_bytes = the size it needs.  max_blocks: the launch bound (None: from the sizes, which are known here)."""
    off, count = _batch_check(items, caps)
    ctx = ctx or default_context()
    p = p or params("deflate")
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    sizes = [int(v) for v in d_nb.cpu()] if count else []
    if caps is None:
        cap = [snappy_batch_bound_bytes(n, p) for n in sizes]
    else:
        cap = [int(v) for v in (caps.cpu().tolist() if torch.is_tensor(caps) else caps)]
    out, offs, d_out, d_cap = _batch_outputs(ctx, cap, count)
    if max_blocks is None:
        max_blocks = sum((n + p.block - 1) // p.block for n in sizes if n <= 0x7FFFFFFF)
    nbytes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    failed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    v0 = ctx.order_violations()
    st = ctx.L.mi_snappy_encode_batch_dev(ctx.h, C.byref(p), count, _ptr(d_in), _ptr(d_nb), max_blocks, _ptr(d_out), _ptr(d_cap),
                                          _ptr(nbytes), _ptr(status), _ptr(failed), ctx.stream_ptr())
    _lib.check(st, "mi_snappy_encode_batch_dev")
    ctx.sync()
    if ctx.order_violations() != v0:
        raise _lib.MiError(10, "the encoder that wrote this batch reported a sort out of order")
    nb, stl = [int(v) for v in nbytes[:count].cpu()], [int(v) for v in status[:count].cpu()]
    outputs = [out[a:a + (n if s == 0 else 0)] for a, n, s in zip(offs, nb, stl)]
    return SnappyBatch(outputs, nbytes[:count], status[:count], int(failed.item()) if count else 0)


def _host_arrays(items):
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in items]
    count = len(arrs)
    h_in = (C.c_void_p * max(count, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    h_nb = (C.c_uint64 * max(count, 1))(*[a.size for a in arrs])
    return arrs, h_in, h_nb, (C.c_uint64 * max(count, 1))(), (C.c_uint32 * max(count, 1))()


def snappy_compress_batch_host(items, p=None, ctx=None):
    """the host-buffer entry point (mi_snappy_encode_batch): a list of bytes -> (list of bytes, None where the item failed; list
    of status codes)"""
    items = [bytes(x) for x in items]
    count = len(items)
    ctx = ctx or default_context()
    p = p or params("deflate")
    arrs, h_in, h_nb, sizes, status = _host_arrays(items)
    caps = [snappy_batch_bound_bytes(a.size, p) for a in arrs]
    outs = [np.zeros(max(v, 1), dtype=np.uint8) for v in caps]
    h_out = (C.c_void_p * max(count, 1))(*[o.ctypes.data for o in outs])
    h_cap = (C.c_uint64 * max(count, 1))(*caps)
    st = ctx.L.mi_snappy_encode_batch(ctx.h, C.byref(p), count, h_in, h_nb, h_out, h_cap, sizes, status)
    _lib.check(st, "mi_snappy_encode_batch")
    return [outs[i][: int(sizes[i])].tobytes() if status[i] == 0 else None for i in range(count)], [int(status[i]) for i in range(count)]


def snappy_decompress_batch_host(items, ctx=None):
    """the host-buffer entry point (mi_snappy_decode_batch, called once for the preambles and once to decode, so the inputs travel
    to the device twice: a convenience path): a list of bytes -> (list of bytes, None where the item failed; list of status codes)"""
    items = [bytes(x) for x in items]
    count = len(items)
    ctx = ctx or default_context()
    arrs, h_in, h_nb, sizes, status = _host_arrays(items)
    st = ctx.L.mi_snappy_decode_batch(ctx.h, count, h_in, h_nb, None, None, sizes, status, 0)
    _lib.check(st, "mi_snappy_decode_batch")
    outs = [np.zeros(max(int(sizes[i]), 1), dtype=np.uint8) for i in range(count)]
    h_out = (C.c_void_p * max(count, 1))(*[o.ctypes.data for o in outs])
    h_cap = (C.c_uint64 * max(count, 1))(*[int(sizes[i]) for i in range(count)])
    st = ctx.L.mi_snappy_decode_batch(ctx.h, count, h_in, h_nb, h_out, h_cap, sizes, status, 0)
    _lib.check(st, "mi_snappy_decode_batch")
    return [outs[i][: int(sizes[i])].tobytes() if status[i] == 0 else None for i in range(count)], [int(status[i]) for i in range(count)]


# ---- batched LZ4: many independent raw LZ4 blocks (LZ4_compress_default; Parquet LZ4_RAW) or LZ4 frames (the lz4 tool, Arrow IPC) per call
LZ4_FORMATS = {"block": 0, "frame": 1}                          # MI_LZ4_BLOCK, MI_LZ4_FRAME


class Lz4Batch(InflateBatch):
    """The result of lz4_compress_batch / lz4_decompress_batch: SnappyBatch's shape and meaning"""

    def raise_for_status(self):
        if self.failed:
            st = [int(v) for v in self.status.cpu()]
            i = next(k for k, v in enumerate(st) if v)
            raise _lib.MiError(st[i], f"lz4 batch: {self.failed} of {len(st)} items failed, the first one item {i}")
        return self


def _lz4_format(format):
    if format not in LZ4_FORMATS:
        raise ValueError(f"format must be one of {sorted(LZ4_FORMATS)}, not {format!r}")
    return LZ4_FORMATS[format]


def lz4_batch_bound_bytes(n, p=None, format="frame"):
    """mi_lz4_batch_bound_bytes: the most an item of n bytes comes to"""
    p = p or params("deflate")
    return int(_lib.lib().mi_lz4_batch_bound_bytes(n, C.byref(p), _lz4_format(format)))


def _lz4_sizes_dev(ctx, count, d_in, d_nb, fmt):
    sizes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    st = ctx.L.mi_lz4_batch_size_dev(ctx.h, count, _ptr(d_in), _ptr(d_nb), _ptr(sizes), _ptr(status), None, fmt, ctx.stream_ptr())
    _lib.check(st, "mi_lz4_batch_size_dev")
    return sizes[:count], status[:count]


def lz4_batch_sizes(items, format="frame", ctx=None):
    """What every item decodes to -> (sizes int64, status int32) device tensors.  `items` as for lz4_decompress_batch.  The walk of
    the decoder without its stores, with its verdicts — except that a frame which carries a content size answers from its header
    alone."""
    fmt = _lz4_format(format)
    off, count = _batch_check(items, None)
    ctx = ctx or default_context()
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    out = _lz4_sizes_dev(ctx, count, d_in, d_nb, fmt)
    ctx.sync()                                                 # (the inputs in `keep` may go now)
    return out


def _lz4_call(ctx, count, cap, what, call):
    """one device call `what` into a packed output of the capacities `cap` -> Lz4Batch; call(d_out, d_cap, nbytes, status, failed)"""
    out, offs, d_out, d_cap = _batch_outputs(ctx, cap, count)
    nbytes = torch.zeros(max(count, 1), dtype=torch.int64, device=ctx.device)
    status = torch.zeros(max(count, 1), dtype=torch.int32, device=ctx.device)
    failed = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    v0 = ctx.order_violations()
    _lib.check(call(_ptr(d_out), _ptr(d_cap), _ptr(nbytes), _ptr(status), _ptr(failed)), what)
    ctx.sync()
    if ctx.order_violations() != v0:
        raise _lib.MiError(10, "the encoder that wrote this batch reported a sort out of order")
    nb, stl = [int(v) for v in nbytes[:count].cpu()], [int(v) for v in status[:count].cpu()]
    outputs = [out[a:a + (n if s == 0 else 0)] for a, n, s in zip(offs, nb, stl)]
    return Lz4Batch(outputs, nbytes[:count], status[:count], int(failed.item()) if count else 0)


def _caps_list(caps):
    return [int(v) for v in (caps.cpu().tolist() if torch.is_tensor(caps) else caps)]


def lz4_decompress_batch(items, format="frame", caps=None, ctx=None):
    """Decode many independent LZ4 buffers in one launch -> Lz4Batch.

    items: a list of bytes or uint8 tensors, or a pair (buffer, offsets) for a packed buffer with count + 1 offsets (item i is
    buffer[offsets[i]:offsets[i + 1]]: no alignment needed).  format: "frame" (the lz4 tool's, Arrow IPC's) or "block" (a raw
    block: Parquet LZ4_RAW).  caps: the output capacity of every item (list or tensor); None runs the size walk first and
    allocates one packed output.  An item larger than its capacity comes back MI_ERR_CAPACITY with out_bytes = the size it needs
    and nothing written at or past the capacity; a malformed one MI_ERR_CORRUPT; one bad item does not spoil the rest.  Block and
    content checksums of a frame are skipped over, not verified."""
    fmt = _lz4_format(format)
    off, count = _batch_check(items, caps)
    ctx = ctx or default_context()
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    cap = _caps_list(_lz4_sizes_dev(ctx, count, d_in, d_nb, fmt)[0] if caps is None else caps)
    return _lz4_call(ctx, count, cap, "mi_lz4_decode_batch_dev", lambda *o: ctx.L.mi_lz4_decode_batch_dev(
        ctx.h, count, _ptr(d_in), _ptr(d_nb), *o, fmt, 0, ctx.stream_ptr()))


def lz4_compress_batch(items, p=None, format="frame", caps=None, ctx=None, max_blocks=None):
    """Compress many independent buffers in one call, each to an LZ4 frame or a raw LZ4 block that stock LZ4 reads -> Lz4Batch.

    items: as for lz4_decompress_batch.  p: params("deflate", block=..., parse=0 or 1) — the batched deflate's finder, parse and
    blocks.  format "frame": any size; one frame block per pipeline block, independent blocks, no checksums, no content size.
    format "block": an item is ONE block, so an item above p.block bytes comes back MI_ERR_ARG (alone).  caps: the output capacity
    of every item; None gives each item its bound in one packed output.  An item that does not fit its capacity comes back
    MI_ERR_CAPACITY with out_bytes = the size it needs.  max_blocks: the launch bound (None: from the sizes, which are known here;
    a raw-block item above the block size is refused and has no blocks)."""
    fmt = _lz4_format(format)
    off, count = _batch_check(items, caps)
    ctx = ctx or default_context()
    p = p or params("deflate")
    keep, d_in, d_nb = _batch_inputs(ctx, items, off, count)
    sizes = [int(v) for v in d_nb.cpu()] if count else []
    cap = [lz4_batch_bound_bytes(n, p, format) for n in sizes] if caps is None else _caps_list(caps)
    if max_blocks is None:
        max_blocks = sum((n + p.block - 1) // p.block for n in sizes if n <= 0x7FFFFFFF and (fmt or n <= p.block))
    return _lz4_call(ctx, count, cap, "mi_lz4_encode_batch_dev", lambda *o: ctx.L.mi_lz4_encode_batch_dev(
        ctx.h, C.byref(p), fmt, count, _ptr(d_in), _ptr(d_nb), max_blocks, *o, ctx.stream_ptr()))


def _lz4_host(count, caps, call):
    """one host-buffer call into outputs of the capacities `caps` -> (list of bytes, None where the item failed; list of status codes)"""
    outs = [np.zeros(max(v, 1), dtype=np.uint8) for v in caps]
    h_out = (C.c_void_p * max(count, 1))(*[o.ctypes.data for o in outs])
    sizes, status = call(h_out, (C.c_uint64 * max(count, 1))(*caps))
    return [outs[i][: int(sizes[i])].tobytes() if status[i] == 0 else None for i in range(count)], [int(status[i]) for i in range(count)]


def lz4_compress_batch_host(items, p=None, format="frame", ctx=None):
    """the host-buffer entry point (mi_lz4_encode_batch): a list of bytes -> (list of bytes, None where the item failed; list of
    status codes)"""
    fmt = _lz4_format(format)
    ctx = ctx or default_context()
    p = p or params("deflate")
    arrs, h_in, h_nb, sizes, status = _host_arrays([bytes(x) for x in items])

    def call(h_out, h_cap):
        _lib.check(ctx.L.mi_lz4_encode_batch(ctx.h, C.byref(p), fmt, len(arrs), h_in, h_nb, h_out, h_cap, sizes, status), "mi_lz4_encode_batch")
        return sizes, status
    return _lz4_host(len(arrs), [lz4_batch_bound_bytes(a.size, p, format) for a in arrs], call)


def lz4_decompress_batch_host(items, format="frame", ctx=None):
    """the host-buffer entry point (mi_lz4_decode_batch, called once for the sizes and once to decode, so the inputs travel to the
    device twice: a convenience path): a list of bytes -> (list of bytes, None where the item failed; list of status codes)"""
    fmt = _lz4_format(format)
    ctx = ctx or default_context()
    arrs, h_in, h_nb, sizes, status = _host_arrays([bytes(x) for x in items])

    def call(h_out, h_cap):
        _lib.check(ctx.L.mi_lz4_decode_batch(ctx.h, len(arrs), h_in, h_nb, h_out, h_cap, sizes, status, fmt, 0), "mi_lz4_decode_batch")
        return sizes, status
    call(None, None)
    return _lz4_host(len(arrs), [int(sizes[i]) for i in range(len(arrs))], call)
