"""The three device entry points of the batched LZ4 on a caller's own non-blocking stream, with the input arriving late and
poison right behind the call: the harness of tests/stream_cases.py, used as tests/test_snappy_stream_order_gpu.py uses it.  The
encoder runs the pipeline's side streams (an item straddles pipeline batches); the two readers are one launch each."""
import ctypes as C

import pytest

import deflate_batch_cases as DB
import lz4_cases as Z
import stream_cases as sc
from compression_algorithms_amd import lz
from test_snappy_stream_order_gpu import _check_outputs, _drain_the_device, _i64, _i64s, _layout, _u32, ctx  # noqa: F401  (the layout,
#                                       the checks and the two fixtures are the Snappy file's: the verdict codes are the same)

pytestmark = pytest.mark.gpu
FMT = {"block": 0, "frame": 1}


def _encode_case(ctx, items, block, parse, fmt):
    p = lz.params("deflate", block=block, parse=parse)
    count = len(items)
    caps = [lz.lz4_batch_bound_bytes(len(x), p, fmt) for x in items]
    pack, in_off, out_off, out_bytes = _layout(items, caps)
    c = sc.Case(ctx, f"lz4-{fmt}-encode-parse{parse}")
    d_in = c.late(pack, sc.data_poison(pack))
    d_out = c.out("out", out_bytes)
    nbytes, status, failed = c.out("nbytes", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    p_in, p_nb = _i64(ctx, [d_in.data_ptr() + o for o in in_off]), _i64(ctx, [len(x) for x in items])
    p_out, p_cap = _i64(ctx, [d_out.data_ptr() + o for o in out_off]), _i64(ctx, caps)
    max_blocks = sum((len(x) + block - 1) // block for x in items)
    call = lambda: ctx.L.mi_lz4_encode_batch_dev(ctx.h, C.byref(p), FMT[fmt], count, sc.ptr(p_in), sc.ptr(p_nb), max_blocks, sc.ptr(p_out),
                                                 sc.ptr(p_cap), sc.ptr(nbytes), sc.ptr(status), sc.ptr(failed), ctx.stream_ptr())
    want = [Z.restate(x, block, parse, fmt) for x in items]
    c.check = lambda got: _check_outputs(got, out_off, caps, want, count)
    c.keepalive = (p_in, p_nb, p_out, p_cap)
    return c, call


def _decode_case(ctx, fmt, sizes_only):
    g = Z.golden()["blocks" if fmt == "block" else "frames"]
    streams, want = zip(*[(s, d) for _, s, d in g + Z.handwritten(fmt)])
    count = len(streams)
    caps = [len(w) for w in want]
    pack, in_off, out_off, out_bytes = _layout(streams, caps)
    c = sc.Case(ctx, f"lz4-{fmt}-{'size' if sizes_only else 'decode'}")
    d_in = c.late(pack, sc.zero_poison(pack))                       # (zero bytes: a block refused at its first offset, a frame at its magic — nothing is followed)
    nbytes, status, failed = c.out("nbytes", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    p_in, p_nb = _i64(ctx, [d_in.data_ptr() + o for o in in_off]), _i64(ctx, [len(x) for x in streams])
    if sizes_only:
        call = lambda: ctx.L.mi_lz4_batch_size_dev(ctx.h, count, sc.ptr(p_in), sc.ptr(p_nb), sc.ptr(nbytes), sc.ptr(status),
                                                   sc.ptr(failed), FMT[fmt], ctx.stream_ptr())
        c.keepalive = (p_in, p_nb)

        def check(got):
            assert _u32(got["status"], count) == [Z.OK] * count and _u32(got["failed"], 1) == [0]
            assert _i64s(got["nbytes"], count) == caps
        c.check = check
        return c, call
    d_out = c.out("out", out_bytes)
    p_out, p_cap = _i64(ctx, [d_out.data_ptr() + o for o in out_off]), _i64(ctx, caps)
    call = lambda: ctx.L.mi_lz4_decode_batch_dev(ctx.h, count, sc.ptr(p_in), sc.ptr(p_nb), sc.ptr(p_out), sc.ptr(p_cap), sc.ptr(nbytes),
                                                 sc.ptr(status), sc.ptr(failed), FMT[fmt], 0, ctx.stream_ptr())
    c.keepalive = (p_in, p_nb, p_out, p_cap)
    c.check = lambda got: _check_outputs(got, out_off, caps, list(want), count)
    return c, call


@pytest.mark.parametrize("parse", Z.PARSES)
def test_lz4_frame_encode_item_straddles_pipeline_batches(ctx, parse, monkeypatch):
    """an 11-block item among one-block items, four blocks per pipeline batch: the scratch sets rotate and the carry moves on"""
    monkeypatch.setenv("MI_LZ_BATCH", "4")
    items = DB.small(3) + [DB.text(10 * 1000 + 500, seed=6)] + DB.small(4, seed=10)
    sc.run(*_encode_case(ctx, items, 1000, parse, "frame"))


def test_lz4_block_encode_several_pipeline_batches(ctx, monkeypatch):
    monkeypatch.setenv("MI_LZ_BATCH", "4")
    items = [x[:1000] for x in DB.small(7) + DB.small(4, seed=10)]
    sc.run(*_encode_case(ctx, items, 1000, 1, "block"))


@pytest.mark.parametrize("fmt", Z.FORMATS)
def test_lz4_decode(ctx, fmt):
    sc.run(*_decode_case(ctx, fmt, False))


@pytest.mark.parametrize("fmt", Z.FORMATS)
def test_lz4_batch_size(ctx, fmt):
    sc.run(*_decode_case(ctx, fmt, True))
