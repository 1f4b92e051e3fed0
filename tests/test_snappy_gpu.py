"""Batched Snappy on the GPU.  Encode: every item byte-equal to the emission rule restated on the CPU (tests/snappy_cases.py),
with capacities, refused items and a launch bound that is too small.  Decode: stock Snappy's streams from the golden file, the
encoder's own, handwritten streams at the shapes where the decoder's paths differ, under both ring sizes, and malformed
streams among good neighbours — each verdict the Python decoder's, nothing written at or past a capacity."""
import ctypes as C

import numpy as np
import pytest
import torch

import parse1_cases as P1
import snappy_cases as S
from compression_algorithms_amd import lz
from compression_algorithms_amd.context import default_context

pytestmark = pytest.mark.gpu
GUARD, FILL = 32, 0xA5


@pytest.fixture(scope="module")
def ctx():
    return default_context()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t.numel() else 0)


class Batch:
    """One device call over host items laid out by hand: item i at a 16-byte boundary + in_align[i], its output at a 64-byte
    boundary + GUARD with GUARD bytes of FILL on both sides (and FILL inside: what a call leaves alone stays FILL)."""

    def __init__(self, ctx, items, caps, in_align=None, null_in=()):
        self.ctx, self.items, self.caps, n = ctx, items, list(caps), len(items)
        in_align = in_align or [0] * n
        at, self.in_off = 0, []
        for x, a in zip(items, in_align):
            at = (at + 15) & ~15
            self.in_off.append(at + a)
            at += a + len(x)
        h_in = np.full(at + 64, 0xEE, dtype=np.uint8)
        for x, o in zip(items, self.in_off):
            h_in[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
        at, self.out_off = 0, []
        for cap in self.caps:
            at = (at + 63) & ~63
            self.out_off.append(at + GUARD)
            at += GUARD + cap + GUARD
        dev = ctx.device
        self.d_in = torch.from_numpy(h_in).to(dev)
        self.d_out = torch.full((at + 64,), FILL, dtype=torch.uint8, device=dev)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        self.d_ptr = i64([0 if i in null_in else self.d_in.data_ptr() + o for i, o in enumerate(self.in_off)])
        self.d_nb = i64([len(x) for x in items])
        self.d_optr = i64([self.d_out.data_ptr() + o for o in self.out_off])
        self.d_cap = i64(self.caps)
        self.nbytes = torch.full((n,), -1, dtype=torch.int64, device=dev)
        self.status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.failed = torch.full((1,), -1, dtype=torch.int32, device=dev)

    def encode(self, p, max_blocks=None):
        if max_blocks is None:
            max_blocks = sum((len(x) + p.block - 1) // p.block for x in self.items)
        st = self.ctx.L.mi_snappy_encode_batch_dev(self.ctx.h, C.byref(p), len(self.items), _ptr(self.d_ptr), _ptr(self.d_nb), max_blocks,
                                                   _ptr(self.d_optr), _ptr(self.d_cap), _ptr(self.nbytes), _ptr(self.status),
                                                   _ptr(self.failed), self.ctx.stream_ptr())
        assert st == 0, st
        return self.read()

    def decode(self):
        st = self.ctx.L.mi_snappy_decode_batch_dev(self.ctx.h, len(self.items), _ptr(self.d_ptr), _ptr(self.d_nb), _ptr(self.d_optr),
                                                   _ptr(self.d_cap), _ptr(self.nbytes), _ptr(self.status), _ptr(self.failed), 0,
                                                   self.ctx.stream_ptr())
        assert st == 0, st
        return self.read()

    def read(self):
        self.ctx.sync()
        self.out = self.d_out.cpu().numpy()
        self.st = [int(v) for v in self.status.cpu()]
        self.nb = [int(v) for v in self.nbytes.cpu()]
        self.nfailed = int(self.failed.item())
        self.got = [self.out[o:o + min(n, cap)].tobytes() for o, n, cap in zip(self.out_off, self.nb, self.caps)]
        mask = np.ones(self.out.size, dtype=bool)
        for o, cap in zip(self.out_off, self.caps):
            mask[o:o + cap] = False
        self.guards_ok = bool((self.out[mask] == FILL).all())
        return self

    def untouched(self, i):
        """item i's whole output buffer is still FILL"""
        return bool((self.out[self.out_off[i]:self.out_off[i] + self.caps[i]] == FILL).all())


def _params(block, parse):
    return lz.params("deflate", block=block, parse=parse)


def _encode(ctx, items, block, parse, caps=None, **kw):
    p = _params(block, parse)
    caps = caps if caps is not None else [lz.snappy_batch_bound_bytes(len(x), p) for x in items]
    mb = kw.pop("max_blocks", None)
    return Batch(ctx, items, caps, **kw).encode(p, mb)


# ---- encode --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parse", S.PARSES)
@pytest.mark.parametrize("block", S.BLOCKS)
def test_encode_equals_the_restatement(ctx, block, parse):
    names, items = zip(*P1.cases().items())
    r = _encode(ctx, list(items), block, parse)
    assert r.st == [S.OK] * len(items) and r.nfailed == 0 and r.guards_ok
    for name, item, got in zip(names, items, r.got):
        assert got == S.restate(item, block, parse), name
        assert S.decode(got) == (item, S.OK, len(item)), name


@pytest.mark.parametrize("parse", S.PARSES)
def test_encode_batch_items_in_one_call(ctx, parse):
    items = P1.batch_items()
    r = _encode(ctx, items, 1000, parse)
    assert r.st == [S.OK] * len(items) and r.nfailed == 0 and r.guards_ok
    assert r.got == [S.restate(x, 1000, parse) for x in items]
    assert r.got[0] == b"\x00"                                   # an empty item is its preamble
    assert all(S.decode(g)[0] == x for g, x in zip(r.got, items))


def test_encode_worst_case_family_stays_inside_the_bound(ctx):
    items = [S.worst_case(65 * 400), S.worst_case(65 * 40), P1.noise(70_000, 7)]
    r = _encode(ctx, items, 65536, 0)
    assert r.st == [S.OK] * 3 and r.guards_ok
    assert r.got == [S.restate(x, 65536, 0) for x in items]


def test_encode_packed_buffer_every_address_residue(ctx):
    """(buffer, offsets): 16 items of 1 001 bytes, so that the items start at all 16 residues of the address"""
    t = P1.golden_text()
    items = [t[3000 * k:3000 * k + 1001] for k in range(16)]
    offsets = [1001 * k for k in range(17)]
    buf = torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).copy()).to(ctx.device)
    assert sorted((buf.data_ptr() + o) % 16 for o in offsets[:-1]) == list(range(16))
    for parse in S.PARSES:
        r = lz.snappy_compress_batch((buf, offsets), _params(65536, parse), ctx=ctx).raise_for_status()
        assert [o.cpu().numpy().tobytes() for o in r.outputs] == [S.restate(x, 65536, parse) for x in items]
    r = lz.snappy_compress_batch(items, _params(4096, 1), ctx=ctx).raise_for_status()
    assert [o.cpu().numpy().tobytes() for o in r.outputs] == [S.restate(x, 4096, 1) for x in items]


def test_encode_capacities(ctx):
    items = P1.batch_items()[2:8]
    want = [S.restate(x, 1000, 1) for x in items]
    caps = [len(w) for w in want]
    caps[1] -= 1
    caps[4] -= 1
    r = _encode(ctx, items, 1000, 1, caps=caps)
    assert r.guards_ok                                           # nothing at or behind any capacity
    for i, w in enumerate(want):
        if i in (1, 4):
            assert (r.st[i], r.nb[i]) == (S.CAPACITY, len(w)), i
        else:
            assert (r.st[i], r.nb[i], r.got[i]) == (S.OK, len(w), w), i
    assert r.nfailed == 2


def test_encode_refused_items(ctx):
    items = P1.batch_items()[2:7]
    r = _encode(ctx, items, 1000, 0, null_in=(2,))
    assert r.st == [S.OK, S.OK, S.ARG, S.OK, S.OK] and r.nb[2] == 0 and r.nfailed == 1 and r.guards_ok and r.untouched(2)
    assert [g for i, g in enumerate(r.got) if i != 2] == [S.restate(x, 1000, 0) for i, x in enumerate(items) if i != 2]
    blocks = [(len(x) + 999) // 1000 for x in items]
    r = _encode(ctx, items, 1000, 0, max_blocks=sum(blocks[:4]) - 1)         # item 3's last block does not fit
    assert r.st == [S.OK, S.OK, S.OK, S.ARG, S.ARG] and r.nfailed == 2 and r.guards_ok
    assert r.got[:3] == [S.restate(x, 1000, 0) for x in items[:3]] and r.untouched(3) and r.untouched(4)


def test_entry_point_arguments(ctx):
    L, h, s = ctx.L, ctx.h, ctx.stream_ptr()
    one = torch.zeros(8, dtype=torch.int64, device=ctx.device)
    a = _ptr(one)
    p = _params(65536, 0)
    assert L.mi_snappy_decode_batch_dev(h, 1, a, a, a, a, a, a, None, 1, s) == S.ARG               # flags must be 0
    assert L.mi_snappy_decode_batch_dev(h, 1, None, a, a, a, a, a, None, 0, s) == S.ARG
    assert L.mi_snappy_decode_batch_dev(h, 1, a, a, a, a, a, None, None, 0, s) == S.ARG
    assert L.mi_snappy_decode_batch_dev(h, 0, None, None, None, None, None, None, None, 0, s) == S.OK
    assert L.mi_snappy_batch_size_dev(h, 1, a, None, a, a, None, s) == S.ARG
    assert L.mi_snappy_batch_size_dev(h, 0, None, None, None, None, None, s) == S.OK
    assert L.mi_snappy_encode_batch_dev(h, C.byref(p), 1, a, a, 1, a, None, a, a, None, s) == S.ARG
    assert L.mi_snappy_encode_batch_dev(h, C.byref(p), 0, None, None, 0, None, None, None, None, None, s) == S.OK
    assert L.mi_snappy_encode_batch_dev(h, None, 1, a, a, 1, a, a, a, a, None, s) == S.ARG
    for bad in (lz.params("lz77", 14, 65536), lz.params("deflate", block=131072), lz.params("deflate", block=65536, parse=2)):
        assert L.mi_snappy_encode_batch_dev(h, C.byref(bad), 1, a, a, 1, a, a, a, a, None, s) == S.ARG
    ctx.sync()


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def _decode(ctx, streams, caps, **kw):
    return Batch(ctx, streams, caps, **kw).decode()


def test_decode_stock_streams(ctx):
    g = S.golden()
    r = _decode(ctx, [s for _, s, _ in g], [len(d) for _, _, d in g])
    assert r.st == [S.OK] * len(g) and r.nfailed == 0 and r.guards_ok
    for (name, _, data), got in zip(g, r.got):
        assert got == data, name


@pytest.mark.parametrize("parse", S.PARSES)
def test_decode_the_encoders_own_output(ctx, parse):
    items = list(P1.cases().values()) + P1.batch_items()
    enc = lz.snappy_compress_batch(items, _params(4096, parse), ctx=ctx).raise_for_status()
    dec = lz.snappy_decompress_batch(enc.outputs, ctx=ctx).raise_for_status()
    assert [o.cpu().numpy().tobytes() for o in dec.outputs] == items
    assert [int(v) for v in dec.out_bytes.cpu()] == [len(x) for x in items]


@pytest.mark.parametrize("count", [0, 1100], ids=["ring32k", "ring4k"])
def test_decode_handwritten(ctx, count):
    """every handwritten stream at every input alignment class it can meet, once in a call of fewer than 1 024 items (the 32 KiB
    ring) and once padded to 1 100 items (the 4 KiB ring)"""
    hw = S.handwritten()
    pad = [h for h in hw if h[0] in ("lit_tag60_17", "empty", "offset_eq_produced")]
    hw = hw + [pad[k % 3] for k in range(max(count - len(hw), 0))]
    r = _decode(ctx, [s for _, s, _ in hw], [len(d) for _, _, d in hw], in_align=[k % 16 for k in range(len(hw))])
    assert r.nfailed == 0 and r.guards_ok
    for k, ((name, _, data), got) in enumerate(zip(hw, r.got)):
        assert (r.st[k], r.nb[k]) == (S.OK, len(data)), name
        assert got == data, name


@pytest.mark.parametrize("count", [0, 1100], ids=["ring32k", "ring4k"])
def test_decode_corrupt_among_good(ctx, count):
    """every malformed stream between good neighbours: the Python decoder's verdict, the neighbours' results unchanged, and
    nothing at or behind the item's capacity (the size its preamble names)"""
    mix = S.among_good(S.corrupt())
    good = mix[0]
    mix = mix + [good] * max(count - len(mix), 0)
    caps = [len(d) if d is not None else max(S.preamble(s)[1], 0) for _, s, d in mix]
    r = _decode(ctx, [s for _, s, _ in mix], caps, in_align=[(5 * k) % 16 for k in range(len(mix))])
    assert r.guards_ok
    for k, (name, s, d) in enumerate(mix):
        want = S.decode(s, caps[k])
        assert (r.st[k], r.nb[k]) == (want[1], want[2]), name
        if d is not None:
            assert r.got[k] == d, name
    assert r.nfailed == sum(1 for _, _, d in mix if d is None) == len(S.corrupt())


def test_decode_capacities(ctx):
    hw = [h for h in S.handwritten() if h[0] in ("lit_5000", "overlap_1_70", "lit_tag61_300", "copy2_65535")]
    caps = [len(d) for _, _, d in hw]
    caps[1] -= 1
    caps[3] = 0
    r = _decode(ctx, [s for _, s, _ in hw], caps)
    assert r.guards_ok and r.nfailed == 2
    for k, (name, _, data) in enumerate(hw):
        if k in (1, 3):
            assert (r.st[k], r.nb[k]) == (S.CAPACITY, len(data)) and r.untouched(k), name
        else:
            assert (r.st[k], r.nb[k], r.got[k]) == (S.OK, len(data), data), name


def test_decode_refused_items(ctx):
    hw = S.handwritten()[1:4]
    r = _decode(ctx, [s for _, s, _ in hw], [len(d) for _, _, d in hw], null_in=(1,))
    assert r.st == [S.OK, S.ARG, S.OK] and r.nb[1] == 0 and r.untouched(1) and r.guards_ok
    big = [S.varint(0x80000000) + b"\x00", S.varint(0xFFFFFFFF) + b"\x00"]     # well-formed preambles above the per-item limit
    r = _decode(ctx, big, [64, 64])
    assert r.st == [S.ARG, S.ARG] and r.nb == [0, 0] and r.untouched(0) and r.untouched(1)


def test_batch_sizes(ctx):
    """the preamble alone: the header verdicts, and no look at the body"""
    streams = [s for _, s, _ in S.handwritten()] + [s for _, s in S.corrupt()] + [S.varint(0x80000000) + b"\x00"]
    sizes, status = lz.snappy_batch_sizes(streams, ctx=ctx)
    want = [(S.CORRUPT, 0, 0) if not len(s) else S.preamble(s) for s in streams]
    assert [int(v) for v in status.cpu()] == [w[0] for w in want]
    assert [int(v) for v in sizes.cpu()] == [w[1] if w[0] == S.OK else 0 for w in want]
    assert {S.OK, S.CORRUPT, S.ARG} == {w[0] for w in want}
    body_unseen = dict(zip([n for n, _ in S.corrupt()], want[len(S.handwritten()):]))
    assert body_unseen["offset_0"][0] == S.OK and body_unseen["trailing_bytes"][0] == S.OK


def test_packed_decode_and_python_verdicts(ctx):
    g = S.golden()
    streams = [s for _, s, _ in g] + [S.corrupt()[0][1]]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).tolist()
    r = lz.snappy_decompress_batch((b"".join(streams), offsets), ctx=ctx)
    assert r.failed == 1 and [int(v) for v in r.status.cpu()] == [S.OK] * len(g) + [S.CORRUPT]
    assert [o.cpu().numpy().tobytes() for o in r.outputs[:-1]] == [d for _, _, d in g]
    with pytest.raises(Exception):
        r.raise_for_status()
    caps = [len(d) for _, _, d in g] + [58]
    caps[0] -= 1
    r = lz.snappy_decompress_batch(streams, caps=caps, ctx=ctx)
    assert int(r.status[0]) == S.CAPACITY and int(r.out_bytes[0]) == len(g[0][2]) and r.failed == 2


def test_host_forms_round_trip(ctx):
    items = P1.batch_items()
    p = _params(1000, 1)
    enc, st = lz.snappy_compress_batch_host(items, p, ctx=ctx)
    assert st == [S.OK] * len(items) and enc == [S.restate(x, 1000, 1) for x in items]
    dec, st = lz.snappy_decompress_batch_host(enc + [S.corrupt()[1][1]], ctx=ctx)
    assert st == [S.OK] * len(items) + [S.CORRUPT] and dec[:-1] == items and dec[-1] is None
    assert lz.snappy_compress_batch_host([], p, ctx=ctx) == ([], []) and lz.snappy_decompress_batch_host([], ctx=ctx) == ([], [])
