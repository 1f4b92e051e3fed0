"""Batched LZ4 on the GPU, raw blocks and frames.  Encode: every item byte-equal to the emission rule restated on the CPU
(tests/lz4_cases.py), with capacities, refused items and a launch bound that is too small.  Decode: stock LZ4's streams from the
golden file, the encoder's own, handwritten streams at the shapes where the decoder's paths differ, under both ring sizes,
malformed streams among good neighbours, and one-byte mutations of stock blocks — each verdict the Python decoder's (for the
mutations: as recorded beside stock's own in the golden file), nothing written at or past a capacity."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import lz4_cases as Z
import parse1_cases as P1
import test_snappy_gpu as SG
from compression_algorithms_amd import lz
from test_snappy_gpu import _ptr, ctx  # noqa: F401  (the module's context fixture)

pytestmark = pytest.mark.gpu
FMT = {"block": 0, "frame": 1}


class Batch(SG.Batch):
    """test_snappy_gpu's layout of one device call (items at chosen alignments, outputs between guards of FILL) with the LZ4 calls"""

    def encode(self, p, fmt, max_blocks=None):
        if max_blocks is None:
            max_blocks = sum((len(x) + p.block - 1) // p.block for x in self.items if fmt == "frame" or len(x) <= p.block)
        st = self.ctx.L.mi_lz4_encode_batch_dev(self.ctx.h, C.byref(p), FMT[fmt], len(self.items), _ptr(self.d_ptr), _ptr(self.d_nb),
                                                max_blocks, _ptr(self.d_optr), _ptr(self.d_cap), _ptr(self.nbytes), _ptr(self.status),
                                                _ptr(self.failed), self.ctx.stream_ptr())
        assert st == 0, st
        return self.read()

    def decode(self, fmt):
        st = self.ctx.L.mi_lz4_decode_batch_dev(self.ctx.h, len(self.items), _ptr(self.d_ptr), _ptr(self.d_nb), _ptr(self.d_optr),
                                                _ptr(self.d_cap), _ptr(self.nbytes), _ptr(self.status), _ptr(self.failed), FMT[fmt], 0,
                                                self.ctx.stream_ptr())
        assert st == 0, st
        return self.read()


def _params(block, parse):
    return lz.params("deflate", block=block, parse=parse)


def _encode(ctx, items, block, parse, fmt, caps=None, **kw):
    p = _params(block, parse)
    caps = caps if caps is not None else [lz.lz4_batch_bound_bytes(len(x), p, fmt) for x in items]
    mb = kw.pop("max_blocks", None)
    return Batch(ctx, items, caps, **kw).encode(p, fmt, mb)


def _cases(block, fmt):
    """the parse's cases and the end rules' (a raw block holds at most one pipeline block: cut there)"""
    c = dict(P1.cases())
    c.update(Z.cpu_items())
    return {k: (v[:block] if fmt == "block" else v) for k, v in c.items()}


# ---- encode --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", Z.FORMATS)
@pytest.mark.parametrize("parse", Z.PARSES)
@pytest.mark.parametrize("block", Z.BLOCKS)
def test_encode_equals_the_restatement(ctx, block, parse, fmt):
    names, items = zip(*_cases(block, fmt).items())
    r = _encode(ctx, list(items), block, parse, fmt)
    assert r.st == [Z.OK] * len(items) and r.nfailed == 0 and r.guards_ok
    for name, item, got in zip(names, items, r.got):
        assert got == Z.restate(item, block, parse, fmt), name
        assert Z.decode(got, fmt) == (item, Z.OK, len(item)), name


@pytest.mark.parametrize("fmt", Z.FORMATS)
@pytest.mark.parametrize("parse", Z.PARSES)
def test_encode_batch_items_in_one_call(ctx, parse, fmt):
    """items of mixed sizes; in block format the ones above the block size are refused alone"""
    items = P1.batch_items()
    r = _encode(ctx, items, 1000, parse, fmt)
    fits = [fmt == "frame" or len(x) <= 1000 for x in items]
    assert r.st == [Z.OK if f else Z.ARG for f in fits] and r.nfailed == fits.count(False) and r.guards_ok
    for k, (x, f) in enumerate(zip(items, fits)):
        if f:
            assert r.got[k] == Z.restate(x, 1000, parse, fmt), k
        else:
            assert r.nb[k] == 0 and r.untouched(k), k
    assert r.got[0] == (b"\x00" if fmt == "block" else Z.FRAME_HEADER + Z.END_MARK)       # an empty item


def test_encode_block_format_refuses_block_plus_1(ctx):
    items = [P1.golden_text()[:4096], P1.golden_text()[:4097], P1.noise(4096, 3), b""]
    r = _encode(ctx, items, 4096, 0, "block")
    assert r.st == [Z.OK, Z.ARG, Z.OK, Z.OK] and r.nb[1] == 0 and r.untouched(1) and r.nfailed == 1 and r.guards_ok
    assert [r.got[k] for k in (0, 2, 3)] == [Z.restate(items[k], 4096, 0, "block") for k in (0, 2, 3)]


def test_encode_frame_stored_block(ctx):
    """2 * block + 1 bytes with the middle block incompressible: that block goes in stored, its neighbours do not"""
    t = P1.golden_text()
    item = t[:4096] + P1.noise(4096, 5) + t[4096:4097]
    r = _encode(ctx, [item, P1.noise(70_000, 7)], 4096, 1, "frame")
    assert r.st == [Z.OK, Z.OK] and r.guards_ok
    assert r.got == [Z.restate(item, 4096, 1, "frame"), Z.restate(P1.noise(70_000, 7), 4096, 1, "frame")]
    first = int.from_bytes(r.got[0][7:11], "little")
    assert first < 4096 and r.got[0][11 + first:15 + first] == Z.word(4096 | 0x80000000)
    assert len(r.got[1]) == Z.bound(70_000, 4096, "frame")                              # all stored: the bound, exactly


@pytest.mark.parametrize("fmt", Z.FORMATS)
def test_encode_worst_case_family_stays_inside_the_bound(ctx, fmt):
    items = [Z.worst_case(274 * 100), Z.worst_case(274 * 10), P1.noise(65_536, 7)]
    r = _encode(ctx, items, 65536, 0, fmt)
    assert r.st == [Z.OK] * 3 and r.guards_ok
    assert r.got == [Z.restate(x, 65536, 0, fmt) for x in items]


def test_encode_packed_buffer_every_address_residue(ctx):
    """(buffer, offsets): 16 items of 1 001 bytes, so that the items start at all 16 residues of the address"""
    t = P1.golden_text()
    items = [t[3000 * k:3000 * k + 1001] for k in range(16)]
    offsets = [1001 * k for k in range(17)]
    buf = torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).copy()).to(ctx.device)
    assert sorted((buf.data_ptr() + o) % 16 for o in offsets[:-1]) == list(range(16))
    for fmt in Z.FORMATS:
        for parse in Z.PARSES:
            r = lz.lz4_compress_batch((buf, offsets), _params(65536, parse), fmt, ctx=ctx).raise_for_status()
            assert [o.cpu().numpy().tobytes() for o in r.outputs] == [Z.restate(x, 65536, parse, fmt) for x in items]
    r = lz.lz4_compress_batch(items, _params(4096, 1), ctx=ctx).raise_for_status()
    assert [o.cpu().numpy().tobytes() for o in r.outputs] == [Z.restate(x, 4096, 1, "frame") for x in items]


@pytest.mark.parametrize("fmt", Z.FORMATS)
def test_encode_capacities(ctx, fmt):
    """size - 1, size and size + 1: the first is MI_ERR_CAPACITY with the size it needs, and nothing lands at or past a capacity"""
    items = [x[:1000] for x in P1.batch_items()[2:8]] if fmt == "block" else P1.batch_items()[2:8]
    want = [Z.restate(x, 1000, 1, fmt) for x in items]
    caps = [len(w) for w in want]
    caps[1] -= 1
    caps[4] -= 1
    caps[2] += 1
    r = _encode(ctx, items, 1000, 1, fmt, caps=caps)
    assert r.guards_ok
    for i, w in enumerate(want):
        if i in (1, 4):
            assert (r.st[i], r.nb[i]) == (Z.CAPACITY, len(w)), i
        else:
            assert (r.st[i], r.nb[i], r.got[i]) == (Z.OK, len(w), w), i
    assert r.nfailed == 2


def test_encode_refused_items(ctx):
    items = P1.batch_items()[2:7]
    r = _encode(ctx, items, 1000, 0, "frame", null_in=(2,))
    assert r.st == [Z.OK, Z.OK, Z.ARG, Z.OK, Z.OK] and r.nb[2] == 0 and r.nfailed == 1 and r.guards_ok and r.untouched(2)
    assert [g for i, g in enumerate(r.got) if i != 2] == [Z.restate(x, 1000, 0, "frame") for i, x in enumerate(items) if i != 2]
    blocks = [(len(x) + 999) // 1000 for x in items]
    r = _encode(ctx, items, 1000, 0, "frame", max_blocks=sum(blocks[:4]) - 1)     # item 3's last block does not fit
    assert r.st == [Z.OK, Z.OK, Z.OK, Z.ARG, Z.ARG] and r.nfailed == 2 and r.guards_ok
    assert r.got[:3] == [Z.restate(x, 1000, 0, "frame") for x in items[:3]] and r.untouched(3) and r.untouched(4)
    # over the per-item limit: a size of 2^31 (the pointer is never followed)
    b = Batch(ctx, items[:2], [lz.lz4_batch_bound_bytes(len(x), _params(1000, 0), "frame") for x in items[:2]])
    b.d_nb[1] = 1 << 31
    r = b.encode(_params(1000, 0), "frame", max_blocks=1)
    assert r.st == [Z.OK, Z.ARG] and r.untouched(1) and r.got[0] == Z.restate(items[0], 1000, 0, "frame")


def test_entry_point_arguments(ctx):
    L, h, s = ctx.L, ctx.h, ctx.stream_ptr()
    one = torch.zeros(8, dtype=torch.int64, device=ctx.device)
    a = _ptr(one)
    p = _params(65536, 0)
    assert L.mi_lz4_decode_batch_dev(h, 1, a, a, a, a, a, a, None, 0, 1, s) == Z.ARG               # flags must be 0
    assert L.mi_lz4_decode_batch_dev(h, 1, a, a, a, a, a, a, None, 2, 0, s) == Z.ARG               # no such format
    assert L.mi_lz4_decode_batch_dev(h, 1, None, a, a, a, a, a, None, 0, 0, s) == Z.ARG
    assert L.mi_lz4_decode_batch_dev(h, 1, a, a, a, a, a, None, None, 1, 0, s) == Z.ARG
    assert L.mi_lz4_decode_batch_dev(h, 0, None, None, None, None, None, None, None, 1, 0, s) == Z.OK
    assert L.mi_lz4_batch_size_dev(h, 1, a, None, a, a, None, 0, s) == Z.ARG
    assert L.mi_lz4_batch_size_dev(h, 1, a, a, a, a, None, 2, s) == Z.ARG
    assert L.mi_lz4_batch_size_dev(h, 0, None, None, None, None, None, 0, s) == Z.OK
    assert L.mi_lz4_encode_batch_dev(h, C.byref(p), 0, 1, a, a, 1, a, None, a, a, None, s) == Z.ARG
    assert L.mi_lz4_encode_batch_dev(h, C.byref(p), 2, 1, a, a, 1, a, a, a, a, None, s) == Z.ARG
    assert L.mi_lz4_encode_batch_dev(h, C.byref(p), 1, 0, None, None, 0, None, None, None, None, None, s) == Z.OK
    assert L.mi_lz4_encode_batch_dev(h, None, 0, 1, a, a, 1, a, a, a, a, None, s) == Z.ARG
    for bad in (lz.params("lz77", 14, 65536), lz.params("deflate", block=131072), lz.params("deflate", block=65536, parse=2)):
        assert L.mi_lz4_encode_batch_dev(h, C.byref(bad), 1, 1, a, a, 1, a, a, a, a, None, s) == Z.ARG
    with pytest.raises(ValueError):
        lz.lz4_compress_batch([b"x"], format="raw", ctx=ctx)
    ctx.sync()


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def _decode(ctx, streams, caps, fmt, **kw):
    return Batch(ctx, streams, caps, **kw).decode(fmt)


@pytest.mark.parametrize("kind,fmt", [("blocks", "block"), ("frames", "frame")])
def test_decode_stock_streams(ctx, kind, fmt):
    g = Z.golden()[kind]
    r = _decode(ctx, [s for _, s, _ in g], [len(d) for _, _, d in g], fmt, in_align=[(3 * k) % 16 for k in range(len(g))])
    assert r.st == [Z.OK] * len(g) and r.nfailed == 0 and r.guards_ok
    for (name, _, data), got in zip(g, r.got):
        assert got == data, name


@pytest.mark.parametrize("fmt", Z.FORMATS)
@pytest.mark.parametrize("parse", Z.PARSES)
def test_decode_the_encoders_own_output(ctx, parse, fmt):
    items = [x[:4096] if fmt == "block" else x for x in list(P1.cases().values()) + P1.batch_items()]
    enc = lz.lz4_compress_batch(items, _params(4096, parse), fmt, ctx=ctx).raise_for_status()
    dec = lz.lz4_decompress_batch(enc.outputs, fmt, ctx=ctx).raise_for_status()
    assert [o.cpu().numpy().tobytes() for o in dec.outputs] == items
    assert [int(v) for v in dec.out_bytes.cpu()] == [len(x) for x in items]


@pytest.mark.parametrize("fmt", Z.FORMATS)
@pytest.mark.parametrize("count", [0, 1100], ids=["ring32k", "ring4k"])
def test_decode_handwritten(ctx, count, fmt):
    """every handwritten stream at a different input alignment, once in a call of fewer than 1 024 items (the 32 KiB ring) and once
    padded to 1 100 items (the 4 KiB ring)"""
    hw = Z.handwritten(fmt)
    pad = [h for h in hw if h[0] in ("nibble_14_and_15", "only_literals_1", "offset_eq_written")]
    hw = hw + [pad[k % 3] for k in range(max(count - len(hw), 0))]
    r = _decode(ctx, [s for _, s, _ in hw], [len(d) for _, _, d in hw], fmt, in_align=[k % 16 for k in range(len(hw))])
    assert r.nfailed == 0 and r.guards_ok
    for k, ((name, _, data), got) in enumerate(zip(hw, r.got)):
        assert (r.st[k], r.nb[k]) == (Z.OK, len(data)), name
        assert got == data, name


@pytest.mark.parametrize("fmt", Z.FORMATS)
@pytest.mark.parametrize("count", [0, 1100], ids=["ring32k", "ring4k"])
def test_decode_corrupt_among_good(ctx, count, fmt):
    """every malformed stream between good neighbours: the Python decoder's verdict, the neighbours' results unchanged, nothing at
    or behind the item's capacity"""
    mix = Z.among_good(fmt)
    good = mix[0]
    mix = mix + [good] * max(count - len(mix), 0)
    caps = [len(d) if d is not None else 200 for _, _, d in mix]
    r = _decode(ctx, [s for _, s, _ in mix], caps, fmt, in_align=[(5 * k) % 16 for k in range(len(mix))])
    assert r.guards_ok
    for k, (name, s, d) in enumerate(mix):
        want = Z.decode(s, fmt, caps[k])
        assert (r.st[k], r.nb[k]) == (want[1], want[2]), name
        if d is not None:
            assert r.got[k] == d, name
    bad = [Z.decode(s, fmt)[1] for _, s, d in mix if d is None]
    assert r.nfailed == len(bad) == len(Z.corrupt(fmt)) and set(bad) == ({Z.CORRUPT} if fmt == "block" else {Z.CORRUPT, Z.ARG})


@pytest.mark.parametrize("fmt", Z.FORMATS)
def test_decode_capacities(ctx, fmt):
    """size - 1, size, size + 1 and 0: too small is MI_ERR_CAPACITY with the size needed, and nothing lands at or past the capacity"""
    hw = [h for h in Z.handwritten(fmt) if h[0] in ("lit_5000", "overlap_1_70", "chain_255_then_0", "offset_65535", "match_2000_d_100")]
    assert len(hw) == 5
    caps = [len(d) for _, _, d in hw]
    caps[1] -= 1
    caps[2] += 1
    caps[3] = 0
    caps[4] -= 1
    r = _decode(ctx, [s for _, s, _ in hw], caps, fmt)
    assert r.guards_ok and r.nfailed == 3
    for k, (name, _, data) in enumerate(hw):
        if k in (1, 3, 4):
            assert (r.st[k], r.nb[k]) == (Z.CAPACITY, len(data)), name
        else:
            assert (r.st[k], r.nb[k], r.got[k]) == (Z.OK, len(data), data), name
    assert r.untouched(3)


def test_decode_refused_items(ctx):
    hw = Z.handwritten("block")[1:4]
    r = _decode(ctx, [s for _, s, _ in hw], [len(d) for _, _, d in hw], "block", null_in=(1,))
    assert r.st == [Z.OK, Z.ARG, Z.OK] and r.nb[1] == 0 and r.untouched(1) and r.guards_ok


@pytest.mark.parametrize("fmt", Z.FORMATS)
def test_batch_sizes_agree_with_the_decode(ctx, fmt):
    g = Z.golden()["blocks" if fmt == "block" else "frames"]
    streams = [s for _, s, _ in Z.handwritten(fmt)] + [s for _, s in Z.corrupt(fmt)] + [s for _, s, _ in g]
    sizes, status = lz.lz4_batch_sizes(streams, fmt, ctx=ctx)
    want = [Z.size_of(s, fmt) for s in streams]
    assert [int(v) for v in status.cpu()] == [w[0] for w in want]
    assert [int(v) for v in sizes.cpu()] == [w[1] for w in want]
    caps = [w[1] for w in want]
    r = _decode(ctx, streams, caps, fmt)
    header_first = 0
    for k, s in enumerate(streams):
        dec = Z.decode(s, fmt, caps[k])
        assert (r.st[k], r.nb[k]) == (dec[1], dec[2]), k
        if want[k] != (dec[1], dec[2]):                                              # only where the header answered before the body
            assert fmt == "frame" and Z.frame_info(s)[1]["csize"] is not None, k
            header_first += 1
    assert header_first == (0 if fmt == "block" else 2)                              # content_size_plus_1 and content_size_minus_1


def test_packed_decode_and_python_verdicts(ctx):
    g = Z.golden()["frames"]
    streams = [s for _, s, _ in g] + [Z.corrupt("frame")[0][1]]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).tolist()
    r = lz.lz4_decompress_batch((b"".join(streams), offsets), ctx=ctx)
    assert r.failed == 1 and [int(v) for v in r.status.cpu()] == [Z.OK] * len(g) + [Z.CORRUPT]
    assert [o.cpu().numpy().tobytes() for o in r.outputs[:-1]] == [d for _, _, d in g]
    with pytest.raises(Exception):
        r.raise_for_status()
    caps = [len(d) for _, _, d in g] + [58]
    caps[0] -= 1
    r = lz.lz4_decompress_batch(streams, caps=caps, ctx=ctx)
    assert int(r.status[0]) == Z.CAPACITY and int(r.out_bytes[0]) == len(g[0][2]) and r.failed == 2


def test_decode_mutated_stock_blocks(ctx):
    """one-byte mutations of stock blocks: the verdict, size and bytes recorded in the golden file (lz4_cases.decode's, written
    by the generator beside LZ4_decompress_safe's own answer) — so wherever stock accepted, this is MI_OK with stock's bytes"""
    m = Z.golden()["mutations"]
    assert len(m) >= 200 and sum(1 for x in m if x[3] >= 0) >= 50
    r = _decode(ctx, [s for _, s, _, _, _, _ in m], [cap for _, _, cap, _, _, _ in m], "block", in_align=[(7 * k) % 16 for k in range(len(m))])
    assert r.guards_ok
    for k, (name, _, _, stock, want, sha) in enumerate(m):
        assert (r.st[k], r.nb[k]) == want, name
        if stock >= 0:
            assert (r.st[k], r.nb[k]) == (Z.OK, stock), name
        if sha is not None:
            assert hashlib.sha256(r.got[k]).hexdigest()[:16] == sha, name


def test_host_forms_round_trip(ctx):
    items = P1.batch_items()
    p = _params(1000, 1)
    enc, st = lz.lz4_compress_batch_host(items, p, ctx=ctx)
    assert st == [Z.OK] * len(items) and enc == [Z.restate(x, 1000, 1, "frame") for x in items]
    dec, st = lz.lz4_decompress_batch_host(enc + [Z.corrupt("frame")[1][1]], ctx=ctx)
    assert st == [Z.OK] * len(items) + [Z.CORRUPT] and dec[:-1] == items and dec[-1] is None
    enc, st = lz.lz4_compress_batch_host(items, p, "block", ctx=ctx)
    fits = [len(x) <= 1000 for x in items]
    assert st == [Z.OK if f else Z.ARG for f in fits]
    assert [e for e, f in zip(enc, fits) if f] == [Z.restate(x, 1000, 1, "block") for x, f in zip(items, fits) if f]
    dec, st = lz.lz4_decompress_batch_host([e for e in enc if e is not None], "block", ctx=ctx)
    assert set(st) == {Z.OK} and dec == [x for x, f in zip(items, fits) if f]
    assert lz.lz4_compress_batch_host([], p, ctx=ctx) == ([], []) and lz.lz4_decompress_batch_host([], ctx=ctx) == ([], [])
