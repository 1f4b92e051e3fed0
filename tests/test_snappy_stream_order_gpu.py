"""The three device entry points of the batched Snappy on a caller's own non-blocking stream, with the input arriving late and
poison right behind the call: the harness of tests/stream_cases.py, used as tests/test_stream_order_gpu.py uses it.  The
encoder runs the pipeline's side streams (an item straddles pipeline batches); the two readers are one launch each."""
import ctypes as C

import numpy as np
import pytest
import torch

import deflate_batch_cases as DB
import snappy_cases as S
import stream_cases as sc
from compression_algorithms_amd import lz
from compression_algorithms_amd.context import default_context

pytestmark = pytest.mark.gpu
GUARD, POISON = sc.GUARD, sc.OUT_POISON


@pytest.fixture(scope="module")
def ctx():
    return default_context()


@pytest.fixture(autouse=True)
def _drain_the_device():
    """whatever a failing case left running on an internal stream ends before the next case touches the workspace"""
    yield
    torch.cuda.synchronize()


def _i64(ctx, v):
    return torch.tensor([int(x) for x in v], dtype=torch.int64, device=ctx.device)


def _u32(a, count):
    return [int(v) for v in a[: 4 * count].view(np.uint32)]


def _i64s(a, count):
    return [int(v) for v in a[: 8 * count].view(np.int64)]


def _layout(items, caps):
    """items packed at 16-byte boundaries, outputs at 64-byte boundaries between guards -> (pack, in_off, out_off, out bytes)"""
    at, in_off = 0, []
    for x in items:
        at = (at + 15) & ~15
        in_off.append(at)
        at += len(x)
    pack = np.zeros(at + 16, dtype=np.uint8)
    for x, o in zip(items, in_off):
        pack[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    at, out_off = 0, []
    for cap in caps:
        at = (at + 63) & ~63
        out_off.append(at + GUARD)
        at += GUARD + cap + GUARD
    return pack, in_off, out_off, at + 64


def _check_outputs(got, out_off, caps, want, count):
    assert _u32(got["status"], count) == [S.OK] * count and _u32(got["failed"], 1) == [0]
    assert _i64s(got["nbytes"], count) == [len(w) for w in want]
    free = np.ones(got["out"].size, dtype=bool)
    for k, (o, w) in enumerate(zip(out_off, want)):
        assert got["out"][o:o + len(w)].tobytes() == w, f"item {k} differs"
        free[o:o + caps[k]] = False
    assert (got["out"][free] == POISON).all(), "bytes outside the items' buffers were written"


def _encode_case(ctx, items, block, parse):
    p = lz.params("deflate", block=block, parse=parse)
    count = len(items)
    caps = [lz.snappy_batch_bound_bytes(len(x), p) for x in items]
    pack, in_off, out_off, out_bytes = _layout(items, caps)
    c = sc.Case(ctx, f"snappy-encode-parse{parse}")
    d_in = c.late(pack, sc.data_poison(pack))
    d_out = c.out("out", out_bytes)
    nbytes, status, failed = c.out("nbytes", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    p_in, p_nb = _i64(ctx, [d_in.data_ptr() + o for o in in_off]), _i64(ctx, [len(x) for x in items])
    p_out, p_cap = _i64(ctx, [d_out.data_ptr() + o for o in out_off]), _i64(ctx, caps)
    max_blocks = sum((len(x) + block - 1) // block for x in items)
    call = lambda: ctx.L.mi_snappy_encode_batch_dev(ctx.h, C.byref(p), count, sc.ptr(p_in), sc.ptr(p_nb), max_blocks, sc.ptr(p_out),
                                                    sc.ptr(p_cap), sc.ptr(nbytes), sc.ptr(status), sc.ptr(failed), ctx.stream_ptr())
    want = [S.restate(x, block, parse) for x in items]
    c.check = lambda got: _check_outputs(got, out_off, caps, want, count)
    c.keepalive = (p_in, p_nb, p_out, p_cap)
    return c, call


def _decode_case(ctx, sizes_only):
    streams, want = zip(*[(s, d) for _, s, d in S.golden() + S.handwritten()[1:]])
    count = len(streams)
    caps = [len(w) for w in want]
    pack, in_off, out_off, out_bytes = _layout(streams, caps)
    c = sc.Case(ctx, f"snappy-{'size' if sizes_only else 'decode'}")
    d_in = c.late(pack, sc.zero_poison(pack))                       # (a zero byte is the preamble 0: nothing to write, no offset to follow)
    nbytes, status, failed = c.out("nbytes", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    p_in, p_nb = _i64(ctx, [d_in.data_ptr() + o for o in in_off]), _i64(ctx, [len(x) for x in streams])
    if sizes_only:
        call = lambda: ctx.L.mi_snappy_batch_size_dev(ctx.h, count, sc.ptr(p_in), sc.ptr(p_nb), sc.ptr(nbytes), sc.ptr(status),
                                                      sc.ptr(failed), ctx.stream_ptr())
        c.keepalive = (p_in, p_nb)

        def check(got):
            assert _u32(got["status"], count) == [S.OK] * count and _u32(got["failed"], 1) == [0]
            assert _i64s(got["nbytes"], count) == caps
        c.check = check
        return c, call
    d_out = c.out("out", out_bytes)
    p_out, p_cap = _i64(ctx, [d_out.data_ptr() + o for o in out_off]), _i64(ctx, caps)
    call = lambda: ctx.L.mi_snappy_decode_batch_dev(ctx.h, count, sc.ptr(p_in), sc.ptr(p_nb), sc.ptr(p_out), sc.ptr(p_cap), sc.ptr(nbytes),
                                                    sc.ptr(status), sc.ptr(failed), 0, ctx.stream_ptr())
    c.keepalive = (p_in, p_nb, p_out, p_cap)
    c.check = lambda got: _check_outputs(got, out_off, caps, list(want), count)
    return c, call


@pytest.mark.parametrize("parse", S.PARSES)
def test_snappy_encode_item_straddles_pipeline_batches(ctx, parse, monkeypatch):
    """an 11-block item among one-block items, four blocks per pipeline batch: the scratch sets rotate and the carry moves on"""
    monkeypatch.setenv("MI_LZ_BATCH", "4")
    items = DB.small(3) + [DB.text(10 * 1000 + 500, seed=6)] + DB.small(4, seed=10)
    sc.run(*_encode_case(ctx, items, 1000, parse))


def test_snappy_decode(ctx):
    sc.run(*_decode_case(ctx, False))


def test_snappy_batch_size(ctx):
    sc.run(*_decode_case(ctx, True))
