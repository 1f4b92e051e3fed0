"""Stream order: the device entry points of include/mi_codec.h on a caller's own non-blocking stream (all but the multi-device
gather, which synchronises every device by contract and owns its streams).

The rest of the suite passes torch.cuda.current_stream(), which is HIP's legacy default stream: it waits for every blocking
stream and every synchronous copy, and the tests hand over inputs that were complete long before the call and read outputs
after a device-wide synchronisation.  A missing fork event, a join that forgets one internal stream, a memset on stream 0, a
scratch set reused a batch too early or a host read of a device word ahead of the stream all pass there.  Here every call
runs under the "late input / early poison" harness of tests/stream_cases.py (its docstring has the steps): the data arrives
on the stream behind a delay — after a call on the poison has left the workspace holding other intermediates than the
data's —, the outputs are copied and everything is overwritten with poison right behind the call, one synchronisation at the end, and the copies are compared with the CPU oracle, zlib or the original bytes — never with the
library's own default-stream output.

Host time of one warm call on a non-blocking stream (workspace grown) and the delay put in front of the late copy — four
times that, at least 5 ms, at most 250 ms — as measured on an MI355X (ROCm 7.0, torch 2.10); every run prints its own
("stream-order timing: ..."), and no case needed the second, fourfold delay:

    call (ms on the host)                                                       delay (ms)
    0.13 - 0.20   one batch: tokens, lz77 W 16 / 64 KiB, mode H, mode Z, BGZF          5
    0.08          mi_lz_find_all_dev                                                   5
    0.57 - 0.58   five batches of three: tokens, mode H, mode Z, BGZF                  5
    0.57          mi_deflate_batch_dev, 8 items, four blocks per batch                 5
    0.40 - 6.7    64 blocks of "pages", batches of 16 (6.7: a fresh process)      5 - 26.7
    0.63 - 1.24   two text encodes of 41 and 36 blocks back to back                    5
    1.02          three encodes back to back (14, 3, 14 blocks)                        5
    0.50 + 0.53   two contexts on two streams                                          5
    3.4 / 4.9     lz77 on 256 KiB / 128 KiB blocks (synchronises per batch)      13.5 / 19.5
    0.05 / 0.03   Huffman in three steps / in one call                                 5
    0.014 0.007   FSE encode, mi_fse_normalise_dev                                     5
    0.010 0.009   mi_crc32_dev, mi_adler32_dev                                         5
    0.05          lz77_compress_old's device entry point                               5
    0.01 - 0.04   mi_inflate_batch_dev, mi_inflate_batch_size_dev                      5
    0.09          mi_bgzf_read_ranges_dev                                              5
    0.9 - 26      the decoders (they synchronise: the time includes the kernels)   5 - 104
    14.3 / 5.7    mode Z -> inflate / BGZF -> index -> range read on the device   57.3 / 22.8

189 of the 192 block encodes of the "pages" input fell back (the precondition of the fallback case).  The negative control
showed the difference for five of the six stream pairs (20 ms delay); the sixth pair shared a hardware queue.

What the net catches, from scratch builds with one wait removed (never committed): without the final join of the pipeline
(the ev_fork wait, lz_emit.hip) the four five-batch cases, the batched-deflate case and the busy-default-stream case fail on
content.  Without the ev_replay[0] wait or the ev_fb[0] wait of the one-batch split, every one-batch case still passes — also
"solo-pages-tokens", whose blocks all take the fallback chain, and also with the workspace scrubbed: stale intermediates do
not explain it.  In that split the caller's stream runs the wave / row replays itself between the fork and the join, which
on these inputs outlast the lane replays on the side stream and the fallback chain on fb, so the parse behind them finds the
work done: a dependency whose producer always finishes first cannot be made visible by delaying the INPUT, and the harness
has no way to delay an internal stream.  (Sixteen hardware queues instead of four change nothing: it is not queue sharing.)

The negative control puts the late copy and the encode on two different streams with no event between them and requires the
stream to differ from the oracle's for at least one of the pairs among four fresh streams.  Its limit is the harness's limit:
two streams that share a hardware queue (the process has four) serialise by accident, so a dependency missed on an internal
stream that happens to share S's queue can still hide from these cases.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import bgzf_cases as B
import bgzf_range_cases as R
import deflate_batch_cases as DB
import inflate_batch_cases as K
import stream_cases as sc
from compression_algorithms_amd import _lib, fse, huffman, lz
from compression_algorithms_amd.context import Context, default_context
from oracle import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c[0]: c for c in sc.ENCODER_CASES}
GUARD, POISON = sc.GUARD, sc.OUT_POISON

@pytest.fixture(scope="module")
def ctx():
    return default_context()


@pytest.fixture(autouse=True)
def _drain_the_device():
    """whatever a failing case left running on an internal stream ends before the next case touches the workspace"""
    yield
    torch.cuda.synchronize()


def _encoder(ctx, name, **kw):
    _, kind, recipe, block, wbits, container = CASES[name]
    return sc.encoder_case(ctx, name, kind, recipe, block, wbits, container, **kw)


def _i64(ctx, v):
    return torch.tensor([int(x) for x in v], dtype=torch.int64, device=ctx.device)


def _u32(a, count):
    return [int(v) for v in a[: 4 * count].view(np.uint32)]


def _i64s(a, count):
    return [int(v) for v in a[: 8 * count].view(np.int64)]


# ---- 1. one batch: the "solo" split (replays on side and parse, fallback chain on fb) ----------------------------------------------
@pytest.mark.parametrize("name", ["solo-tokens", "solo-lz77-w14", "solo-lz77-w16", "solo-h", "solo-z-gzip", "solo-bgzf", "solo-find",
                                  "solo-pages-tokens"])
def test_one_batch_solo_split(ctx, name, monkeypatch):
    monkeypatch.delenv("MI_LZ_BATCH", raising=False)
    sc.run(*_encoder(ctx, name))


# ---- 2. the three-stream pipeline with rotating scratch sets ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pipe-tokens", "pipe-h", "pipe-z-zlib", "pipe-bgzf"])
def test_pipeline_five_batches_three_sets(ctx, name, monkeypatch):
    """14 blocks, three per batch: ev_done[k] is waited on and every scratch set is used again"""
    monkeypatch.setenv("MI_LZ_BATCH", "3")
    sc.run(*_encoder(ctx, name))


def _deflate_batch_case(ctx, items, block, container):
    p, cid = lz.params("deflate", block=block), lz.CONTAINERS[container]
    count = len(items)
    at, in_off = 0, []
    for x in items:
        at = (at + 15) & ~15
        in_off.append(at)
        at += len(x)
    pack = np.zeros(at + 16, dtype=np.uint8)
    for x, o in zip(items, in_off):
        pack[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    caps = [lz.bound_bytes_z(len(x), p, cid) for x in items]
    at, out_off = 0, []
    for cap in caps:
        at = (at + 63) & ~63
        out_off.append(at + GUARD)
        at += GUARD + cap + GUARD
    c = sc.Case(ctx, f"deflate-batch-{container}")
    d_in = c.late(pack, sc.data_poison(pack))
    d_out = c.out("out", at + 64)
    nbytes, status, failed = c.out("nbytes", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    p_in, p_nb = _i64(ctx, [d_in.data_ptr() + o for o in in_off]), _i64(ctx, [len(x) for x in items])
    p_out, p_cap = _i64(ctx, [d_out.data_ptr() + o for o in out_off]), _i64(ctx, caps)
    max_blocks = sum((len(x) + block - 1) // block for x in items)
    call = lambda: ctx.L.mi_deflate_batch_dev(ctx.h, C.byref(p), cid, count, sc.ptr(p_in), sc.ptr(p_nb), max_blocks, sc.ptr(p_out),
                                              sc.ptr(p_cap), sc.ptr(nbytes), sc.ptr(status), sc.ptr(failed), ctx.stream_ptr())
    want = [bytes(orc.defz_stream(x, block, container)[0]) for x in items]

    def check(got):
        assert _u32(got["status"], count) == [0] * count and _u32(got["failed"], 1) == [0]
        assert _i64s(got["nbytes"], count) == [len(w) for w in want]
        free = np.ones(got["out"].size, dtype=bool)
        for k, (o, w) in enumerate(zip(out_off, want)):
            assert got["out"][o:o + len(w)].tobytes() == w, f"item {k} differs from the oracle's stream"
            free[o:o + caps[k]] = False
        assert (got["out"][free] == POISON).all(), "bytes outside the items' buffers were written"
    c.check = check
    c.keepalive = (p_in, p_nb, p_out, p_cap)
    return c, call


def test_deflate_batch_item_straddles_pipeline_batches(ctx, monkeypatch):
    """the items of test_item_straddles_pipeline_batches: an 11-block item among one-block items, four blocks per batch"""
    monkeypatch.setenv("MI_LZ_BATCH", "4")
    items = DB.small(3) + [DB.text(10 * 1000 + 500, seed=6)] + DB.small(4, seed=10)
    sc.run(*_deflate_batch_case(ctx, items, 1000, "gzip"))


# ---- 3. the fallback stream and the hint-driven fourth stream -----------------------------------------------------------------------
@pytest.mark.parametrize("fb2_side", [None, "0", "1"])
def test_fallback_hint_and_second_fallback_stream(fb2_side, monkeypatch, tmp_path):
    """stream_cases.fallback_sequence.  With the switch unset the library decides from the hint alone where the odd batches'
    fallback chains go (with batches of 16 always the side stream: a hint above 8 is more than half a batch);
    MI_LZ_FB2_SIDE=0 makes the hint create the second fallback stream, which both text encodes then carry chains on; =1
    sends the chains to the side stream.  The release of that stream is not exercised (fallback_sequence says why).  Those
    two run in a child process (the switch is read with every call: the child is for a fresh context and hint)."""
    monkeypatch.setenv("MI_LZ_BATCH", "16")
    if fb2_side is None:
        monkeypatch.delenv("MI_LZ_FB2_SIDE", raising=False)
        sc.fallback_sequence()
        return
    for name in ("pages-tokens", "fb-a-tokens", "fb-b-h"):
        sc.expected(*CASES[name][1:])
    sc.save_expected(str(tmp_path / "expected.pickle"))             # (the oracle's streams, worked out once for all three variants)
    env = dict(os.environ, MI_LZ_BATCH="16", MI_LZ_FB2_SIDE=fb2_side, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    body = f"import stream_cases as sc; sc.load_expected({str(tmp_path / 'expected.pickle')!r}); sc.fallback_sequence()"
    r = subprocess.run([sys.executable, "-c", body], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 4. blocks above 64 KiB (lzs.hip / lzw.hip): synchronises once per batch by contract --------------------------------------------
@pytest.mark.parametrize("name", ["wide-lz77-w16", "wide-lz77-w14"])
def test_blocks_above_64k(ctx, name, monkeypatch):
    monkeypatch.delenv("MI_LZ_BATCH", raising=False)
    sc.run(*_encoder(ctx, name, asynchronous=False))


def test_blocks_above_64k_whole_block_finder(ctx, monkeypatch):
    """lzw.hip's own fork (ev_fork onto side / parse / fb) and join (ev_replay[0..2]): text flags no block, so the sliced
    finder of lzs.hip answers the two cases above alone; MI_LZW_SLICED=0 (read on every call) selects the whole-block finder.
    A profiled call afterwards confirms which finder's kernels ran."""
    monkeypatch.delenv("MI_LZ_BATCH", raising=False)
    monkeypatch.setenv("MI_LZW_SLICED", "0")
    c, call = _encoder(ctx, "wide-lz77-w16", asynchronous=False)
    c.name = "wide-lz77-w16-lzw"
    sc.run(c, call)
    S = torch.cuda.Stream()
    ctx.set_profiling(True)
    try:
        ctx.kernel_times()
        with torch.cuda.stream(S):
            c.load()
            assert call() == 0
            ctx.sync()
        names = {k["name"] for k in ctx.kernel_times()}
    finally:
        ctx.set_profiling(False)
    assert "k_lzw_resolve" in names and not any(n.startswith("k_lzs") for n in names), names


def test_find_all32_on_blocks_above_64k(ctx, monkeypatch):
    monkeypatch.delenv("MI_LZ_BATCH", raising=False)
    _, _, recipe, block, wbits, _ = CASES["wide-lz77-w16"]
    data = sc.make(recipe)
    n, p = data.size, sc.lz_params("L", block, wbits)
    c = sc.Case(ctx, "find-all32", asynchronous=False)
    d_in = c.late(data, sc.data_poison(data))
    cand = c.out("cand", 4 * n)
    want = np.concatenate([orc.find_all(data[a:a + block], wbits, wbits + 6, False) for a in range(0, n, block)])

    def check(got):
        bad = np.flatnonzero(got["cand"][: 4 * n].view(np.uint32) != want)
        assert bad.size == 0, f"{bad.size} candidates differ, first at {bad[:5]}"
    c.check = check
    sc.run(c, lambda: ctx.L.mi_lz_find_all32_dev(ctx.h, C.byref(p), sc.ptr(d_in), n, sc.ptr(cand), ctx.stream_ptr()))


# ---- 5. whole-buffer codecs ---------------------------------------------------------------------------------------------------------
def _huffman_check(name, n, three_steps):
    want = sc.expected("HUFF", sc.WHOLE, 0)
    nw = (want["bits"] + 31) // 32

    def check(got):
        info = _lib.HuffmanInfo.from_buffer_copy(got["info"][: C.sizeof(_lib.HuffmanInfo)].tobytes())
        tree = _lib.HuffmanTree.from_buffer_copy(got["tree"][: C.sizeof(_lib.HuffmanTree)].tobytes())
        assert info.status == 0 and info.total_bits == want["bits"], (name, info.status, info.total_bits)
        assert np.ctypeslib.as_array(tree.code).tobytes() == want["codes"] and np.ctypeslib.as_array(tree.length).tobytes() == want["lens"]
        assert got["words"][: 4 * nw].tobytes() == want["words"], f"{name}: the word stream differs from the oracle's"
        if three_steps:
            assert got["hist"][:2048].tobytes() == want["hist"]
    return nw, check


def test_huffman_hist_build_encode_chained(ctx):
    data = sc.make(sc.WHOLE)
    n, ntiles = data.size, int(ctx.L.mi_huffman_num_tiles(data.size))
    nw, check = _huffman_check("huffman-3-steps", n, True)
    c = sc.Case(ctx, "huffman-3-steps")
    d_in = c.late(data, sc.data_poison(data))
    hist, tile_hist = c.out("hist", 2048), c.out("tile_hist", ntiles * 1024)
    info, tree = c.out("info", C.sizeof(_lib.HuffmanInfo)), c.out("tree", C.sizeof(_lib.HuffmanTree))
    words, tile_off = c.out("words", 4 * (nw + 2)), c.out("tile_off", 8 * (ntiles + 1), table=True)
    L, h, sp = ctx.L, ctx.h, ctx.stream_ptr
    c.check = check
    sc.run(c, sc.chain(
        lambda: L.mi_huffman_hist_dev(h, sc.ptr(d_in), n, sc.ptr(hist), sc.ptr(tile_hist), sp()),
        lambda: L.mi_huffman_build_dev(h, sc.ptr(hist), sc.ptr(info), sc.ptr(tree), sp()),
        lambda: L.mi_huffman_encode_with_tree_dev(h, sc.ptr(d_in), n, sc.ptr(tree), sc.ptr(tile_hist), 0, sc.ptr(words), nw + 2,
                                                  sc.ptr(info), sc.ptr(tile_off), sp())))


def test_huffman_one_call(ctx):
    data = sc.make(sc.WHOLE)
    n, ntiles = data.size, int(ctx.L.mi_huffman_num_tiles(data.size))
    nw, check = _huffman_check("huffman", n, False)
    c = sc.Case(ctx, "huffman")
    d_in = c.late(data, sc.data_poison(data))
    info, tree = c.out("info", C.sizeof(_lib.HuffmanInfo)), c.out("tree", C.sizeof(_lib.HuffmanTree))
    words, tile_off = c.out("words", 4 * (nw + 2)), c.out("tile_off", 8 * (ntiles + 1), table=True)
    c.check = check
    sc.run(c, lambda: ctx.L.mi_huffman_encode_dev(ctx.h, sc.ptr(d_in), n, sc.ptr(words), nw + 2, sc.ptr(info), sc.ptr(tree),
                                                  sc.ptr(tile_off), ctx.stream_ptr()))


def test_fse_encode(ctx):
    data = sc.make(sc.WHOLE)
    n, p = data.size, fse.params()
    nblocks = (n + p.block - 1) // p.block
    cap = nblocks * fse.block_bound(p, ctx)
    c = sc.Case(ctx, "fse")
    d_in = c.late(data, sc.data_poison(data))
    out, offs = c.out("out", cap), c.out("offsets", 8 * (nblocks + 1), table=True)
    want = sc.expected("FSE", sc.WHOLE, 65536)["records"]

    def check(got):
        o = _i64s(got["offsets"], nblocks + 1)
        assert o == [0] + [8 * int(v) for v in np.cumsum([len(r) for r in want])], "record offsets"
        for b, r in enumerate(want):
            assert got["out"][o[b] // 8: o[b + 1] // 8].tobytes() == r, f"fse record {b} differs from the oracle's"
    c.check = check
    sc.run(c, lambda: ctx.L.mi_fse_encode_dev(ctx.h, C.byref(p), sc.ptr(d_in), n, sc.ptr(out), cap, sc.ptr(offs), ctx.stream_ptr()))


def test_fse_normalise(ctx):
    freq, stand_in = sc.fse_histograms()
    c = sc.Case(ctx, "fse-normalise")
    d_freq = c.late(freq.view(np.uint8), stand_in.view(np.uint8))
    cnt = c.out("cnt", 1024)
    want = orc.fse_normalise(freq, 8)

    def check(got):
        assert _u32(got["cnt"], 256) == [int(v) for v in want]
    c.check = check
    sc.run(c, lambda: ctx.L.mi_fse_normalise_dev(ctx.h, sc.ptr(d_freq), 8, sc.ptr(cnt), ctx.stream_ptr()))


@pytest.mark.parametrize("which", ["crc32", "adler32"])
def test_checksums(ctx, which):
    data = sc.make(sc.WHOLE)
    c = sc.Case(ctx, which)
    d_in = c.late(data, sc.data_poison(data))
    res = c.out("value", 4)
    want = sc.expected("CRC" if which == "crc32" else "ADLER", sc.WHOLE, 0)["value"]

    def check(got):
        assert _u32(got["value"], 1) == [want]
    c.check = check
    fn = getattr(ctx.L, f"mi_{which}_dev")
    sc.run(c, lambda: fn(ctx.h, sc.ptr(d_in), data.size, sc.ptr(res), ctx.stream_ptr()))


def test_lz77_old(ctx):
    data = sc.make(sc.OLD)
    n = data.size
    cap = int(ctx.L.mi_lz77_old_bound_bytes(n))
    c = sc.Case(ctx, "lz77-old")
    d_in = c.late(data, sc.data_poison(data))
    out, bits = c.out("out", cap), c.out("bits", 8, table=True)
    want = sc.expected("OLD", sc.OLD, 0, 14)

    def check(got):
        assert _i64s(got["bits"], 1) == [want["bits"]]
        assert got["out"][: len(want["out"])].tobytes() == want["out"], "lz77_compress_old's stream differs from the oracle's"
    c.check = check
    sc.run(c, lambda: ctx.L.mi_lz77_old_encode_dev(ctx.h, 14, 4, sc.ptr(d_in), n, sc.ptr(out), cap, sc.ptr(bits), ctx.stream_ptr()))


# ---- 6. asynchronous readers ----------------------------------------------------------------------------------------------------------
def _inflate_batch_case(ctx, container, sizes_only):
    items = K.clean_items(container)
    count, cid = len(items), lz.CONTAINERS[container]
    at, in_off = 0, []
    for _, x, _ in items:
        at = (at + 15) & ~15
        in_off.append(at)
        at += len(x)
    pack = np.zeros(at + 16, dtype=np.uint8)
    for (_, x, _), o in zip(items, in_off):
        pack[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    caps = [len(w) for _, _, w in items]
    at, out_off = 0, []
    for cap in caps:
        at = (at + 63) & ~63
        out_off.append(at + GUARD)
        at += GUARD + cap + GUARD
    c = sc.Case(ctx, f"inflate-batch{'-size' if sizes_only else ''}-{container}")
    d_in = c.late(pack, sc.zero_poison(pack))
    nbytes, status, failed = c.out("nbytes", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    p_in, p_nb = _i64(ctx, [d_in.data_ptr() + o for o in in_off]), _i64(ctx, [len(x) for _, x, _ in items])
    if sizes_only:
        call = lambda: ctx.L.mi_inflate_batch_size_dev(ctx.h, cid, count, sc.ptr(p_in), sc.ptr(p_nb), sc.ptr(nbytes), sc.ptr(status),
                                                       sc.ptr(failed), 0, ctx.stream_ptr())
        c.keepalive = (p_in, p_nb)
    else:
        d_out = c.out("out", at + 64)
        p_out, p_cap = _i64(ctx, [d_out.data_ptr() + o for o in out_off]), _i64(ctx, caps)
        call = lambda: ctx.L.mi_inflate_batch_dev(ctx.h, cid, count, sc.ptr(p_in), sc.ptr(p_nb), sc.ptr(p_out), sc.ptr(p_cap), sc.ptr(nbytes),
                                                  sc.ptr(status), sc.ptr(failed), 0, ctx.stream_ptr())
        c.keepalive = (p_in, p_nb, p_out, p_cap)

    def check(got):
        assert _u32(got["status"], count) == [K.OK] * count and _u32(got["failed"], 1) == [0]
        assert _i64s(got["nbytes"], count) == caps
        if sizes_only:
            return
        free = np.ones(got["out"].size, dtype=bool)
        for (name, _, w), o in zip(items, out_off):
            assert got["out"][o:o + len(w)].tobytes() == w, name
            free[o:o + len(w)] = False
        assert (got["out"][free] == POISON).all(), "bytes outside the items' buffers were written"
    c.check = check
    return c, call


@pytest.mark.parametrize("container", ["raw", "gzip"])
def test_inflate_batch(ctx, container):
    sc.run(*_inflate_batch_case(ctx, container, False))


def test_inflate_batch_size(ctx):
    sc.run(*_inflate_batch_case(ctx, "zlib", True))


def _range_arrays(ctx, so, oo, ranges):
    offs, size = R.layout(ranges)
    pairs = _i64(ctx, [v for pair in zip(so, oo) for v in pair])
    d_off, d_len, d_at = _i64(ctx, [a for a, _ in ranges]), _i64(ctx, [n for _, n in ranges]), _i64(ctx, offs)
    max_pieces = sum(len(p) for p in R.plan_model(oo, ranges))
    return offs, size, pairs, d_off, d_len, d_at, max_pieces


def _range_check(data, ranges, offs):
    want = R.expected(data, ranges)

    def check(got):
        count = len(ranges)
        assert _u32(got["status"], count) == [R.MI_OK] * count and _u32(got["failed"], 1) == [0]
        assert _i64s(got["got"], count) == [len(w) for w in want]
        free = np.ones(got["out"].size, dtype=bool)
        for i, (at, w) in enumerate(zip(offs, want)):
            assert got["out"][at:at + len(w)].tobytes() == w, (i, ranges[i])
            free[at:at + len(w)] = False
        assert (got["out"][free] == POISON).all(), "bytes that no range delivered were written"
    return check


def test_bgzf_read_ranges(ctx):
    """the ranges of bgzf_range_cases over its four-member stream: members cut at both ends, whole ones, past the end"""
    stream, data = R.s1()
    so, oo = R.walk(stream)
    ranges = R.ranges_for(stream, "S1")
    offs, size, pairs, d_off, d_len, d_at, max_pieces = _range_arrays(ctx, so, oo, ranges)
    count = len(ranges)
    c = sc.Case(ctx, "bgzf-read-ranges")
    d_s = c.late(np.frombuffer(stream, dtype=np.uint8), sc.zero_poison(stream), pad=16)
    out, got, status, failed = c.out("out", size), c.out("got", 8 * count, table=True), c.out("status", 4 * count), c.out("failed", 4)
    c.check = _range_check(data, ranges, offs)
    read = lambda at, pieces: ctx.L.mi_bgzf_read_ranges_dev(ctx.h, sc.ptr(d_s), len(stream), sc.ptr(pairs), len(so) - 1, count, sc.ptr(at),
                                                            sc.ptr(d_len), sc.ptr(out), sc.ptr(d_at), size, pieces, sc.ptr(got),
                                                            sc.ptr(status), sc.ptr(failed), 0, ctx.stream_ptr())
    # the cells of the workspace (members cut by a range are decoded there) must not hold these ranges' members from the
    # warm-up: the scrub reads the same slots from the real stream 30 011 bytes further on
    moved = [(a + 30_011 if n else a, n) for a, n in ranges]
    d_moved, moved_pieces = _i64(ctx, [a for a, _ in moved]), sum(len(p) for p in R.plan_model(oo, moved))

    def scrub_more():
        c.load()
        read(d_moved, moved_pieces)
    c.scrub_more = scrub_more
    sc.run(c, lambda: read(d_off, max_pieces))


# ---- 7. decoders: they synchronise inside, so late input only, and nothing outside [out, out + n) is written -------------------------
def _decoder_case(ctx, name, stream, data, make_call, extra_outs=()):
    stream, data = sc.as_np(stream), sc.as_np(data)
    c = sc.Case(ctx, name, asynchronous=False)
    d_s = c.late(stream, sc.zero_poison(stream), pad=16)
    out = c.out("out", data.size + 2 * GUARD)
    extra = {k: c.out(k, nbytes, table=True) for k, nbytes in extra_outs}
    call = make_call(d_s, sc.ptr(out, GUARD), extra)

    def check(got):
        o = got["out"]
        assert o[GUARD:GUARD + data.size].tobytes() == data.tobytes(), f"{name}: the decoded bytes differ"
        assert (o[:GUARD] == POISON).all() and (o[GUARD + data.size:] == POISON).all(), f"{name}: bytes outside [out, out + n) were written"
    c.check = check
    return c, call


@pytest.mark.parametrize("name", ["solo-tokens", "solo-lz77-w14", "solo-h"])
def test_block_decoders(ctx, name):
    _, kind, recipe, block, wbits, _ = CASES[name]
    data, want = sc.make(recipe), sc.expected(kind, recipe, block, wbits)
    p = sc.lz_params(kind, block, wbits)
    table = _i64(ctx, want["bits"])
    nbytes = (want["bits"][-1] + 7) // 8
    fn = ctx.L.mi_deflate_h_decode_dev if kind == "H" else ctx.L.mi_lz_decode_dev
    c, call = _decoder_case(ctx, "decode-" + name, want["out"][:nbytes], data, lambda d_s, d_out, _:
                            lambda: fn(ctx.h, C.byref(p), sc.ptr(d_s), nbytes, sc.ptr(table), d_out, data.size, ctx.stream_ptr()))
    sc.run(c, call)


def test_inflate_with_table(ctx):
    _, kind, recipe, block, _, container = CASES["solo-z-gzip"]
    data, want = sc.make(recipe), sc.expected(kind, recipe, block, None, container)
    table = _i64(ctx, want["bits"])
    c, call = _decoder_case(ctx, "inflate-table", want["out"], data, lambda d_s, d_out, _:
                            lambda: ctx.L.mi_inflate_dev(ctx.h, lz.CONTAINERS[container], block, sc.ptr(d_s), want["nbytes"], sc.ptr(table),
                                                         d_out, data.size, 0, ctx.stream_ptr()))
    sc.run(c, call)


def test_inflate_without_table(ctx):
    """zlib.compress's stream as ONE segment whose last block has BFINAL = 1 (one wave: a short input)"""
    data = sc.make(sc.OLD)
    stream = zlib.compress(data.tobytes(), 6)
    table = _i64(ctx, [16, 8 * (len(stream) - 4)])
    c, call = _decoder_case(ctx, "inflate-one-segment", stream, data, lambda d_s, d_out, _:
                            lambda: ctx.L.mi_inflate_dev(ctx.h, 1, data.size, sc.ptr(d_s), len(stream), sc.ptr(table), d_out, data.size, 0,
                                                         ctx.stream_ptr()))
    sc.run(c, call)


def test_bgzf_index_then_inflate(ctx):
    _, kind, recipe, block, _, _ = CASES["solo-bgzf"]
    data, want = sc.make(recipe), sc.expected(kind, recipe, block)
    so, oo = B.walk(want["out"])
    members = len(so) - 1

    def make_call(d_s, d_out, extra):
        L, h, n = ctx.L, ctx.h, want["nbytes"]
        return sc.chain(lambda: L.mi_bgzf_index_dev(h, sc.ptr(d_s), n, sc.ptr(extra["pairs"]), members, sc.ptr(extra["count"]), ctx.stream_ptr()),
                        lambda: L.mi_bgzf_inflate_dev(h, sc.ptr(d_s), n, sc.ptr(extra["pairs"]), 0, members, d_out, data.size, 0, ctx.stream_ptr()))
    c, call = _decoder_case(ctx, "bgzf-index-inflate", want["out"], data, make_call, [("pairs", 16 * (members + 1)), ("count", 16)])
    inner = c.check

    def check(got):
        assert _i64s(got["count"], 2) == [members, data.size]
        assert _i64s(got["pairs"], 2 * (members + 1)) == [v for pair in zip(so, oo) for v in pair], "the index differs from the serial walk"
        inner(got)
    c.check = check
    sc.run(c, call)


def test_lz77_whole_decode(ctx):
    """the whole-buffer stream of lz77_compress_old (the oracle's), decoded on one wave"""
    data, want = sc.make(sc.OLD), sc.expected("OLD", sc.OLD, 0, 14)
    nbytes = len(want["out"])
    c, call = _decoder_case(ctx, "lz77-whole-decode", want["out"], data, lambda d_s, d_out, _:
                            lambda: ctx.L.mi_lz77_whole_decode_dev(ctx.h, 14, 4, sc.ptr(d_s), nbytes, want["bits"], d_out, data.size,
                                                                   ctx.stream_ptr()))
    sc.run(c, call)


def test_fse_decode(ctx):
    data = sc.make(sc.WHOLE)
    st = fse.compress(data, ctx=ctx)
    nbytes, offsets, p = st.nbytes, st.offsets.clone(), st.p
    c, call = _decoder_case(ctx, "fse-decode", st.data[:nbytes].cpu().numpy(), data, lambda d_s, d_out, _:
                            lambda: ctx.L.mi_fse_decode_dev(ctx.h, C.byref(p), sc.ptr(d_s), nbytes, sc.ptr(offsets), d_out, data.size,
                                                            ctx.stream_ptr()))
    sc.run(c, call)


@pytest.mark.parametrize("tiles", [True, False])
def test_huffman_decode(ctx, tiles):
    data = sc.make(sc.WHOLE)[:100_000] if not tiles else sc.make(sc.WHOLE)          # (without tile offsets one lane walks it all)
    r = huffman.huffman_compress(data, ctx=ctx)
    words = r._words_padded.cpu().numpy().view(np.uint8)
    d_tree, tile_off = r._d_tree, r.tile_off
    c, call = _decoder_case(ctx, f"huffman-decode-{'tiles' if tiles else 'serial'}", words, data, lambda d_s, d_out, _:
                            lambda: ctx.L.mi_huffman_decode_dev(ctx.h, sc.ptr(d_s), r.total_bits, sc.ptr(d_tree), r.n_nodes,
                                                                sc.ptr(tile_off) if tiles else None, d_out, data.size, ctx.stream_ptr()))
    sc.run(c, call)


# ---- 8. chains on one stream with no synchronisation ----------------------------------------------------------------------------------
def test_three_encodes_back_to_back(ctx, monkeypatch):
    """A (14 blocks: the pipeline), B (3 blocks: one batch, the solo split), A again in another mode, one sync at the end"""
    monkeypatch.setenv("MI_LZ_BATCH", "3")
    cases = [_encoder(ctx, "pipe-tokens"), _encoder(ctx, "short-z-raw"), _encoder(ctx, "pipe-h")]
    sc.run(sc.merge(ctx, "chain-A-B-A", [c for c, _ in cases]), sc.chain(*[f for _, f in cases]))


def test_round_trip_z_on_the_device(ctx, monkeypatch):
    """mode Z -> mi_inflate_dev on S: the decoder reads the encoder's stream and table where the encoder left them; the host
    knows the stream's length from the oracle alone"""
    monkeypatch.setenv("MI_LZ_BATCH", "3")
    enc, enc_call = _encoder(ctx, "pipe-z-zlib")
    _, kind, recipe, block, _, container = CASES["pipe-z-zlib"]
    data, want = sc.make(recipe), sc.expected(kind, recipe, block, None, container)
    out = enc.out("back", data.size + 2 * GUARD)
    d_stream, d_bits = enc.outs["out"][0], enc.outs["bits"][0]
    call = sc.chain(enc_call, lambda: ctx.L.mi_inflate_dev(ctx.h, lz.CONTAINERS[container], block, sc.ptr(d_stream), want["nbytes"], sc.ptr(d_bits),
                                                           sc.ptr(out, GUARD), data.size, 0, ctx.stream_ptr()))
    inner = enc.check

    def check(got):
        inner(got)
        o = got["back"]
        assert o[GUARD:GUARD + data.size].tobytes() == data.tobytes()
        assert (o[:GUARD] == POISON).all() and (o[GUARD + data.size:] == POISON).all()
    enc.check, enc.asynchronous, enc.name = check, False, "round-trip-z"
    sc.run(enc, call)


def test_round_trip_bgzf_on_the_device(ctx, monkeypatch):
    """BGZF encode -> index -> range read on S, each stage reading what the stage before left on the device"""
    monkeypatch.setenv("MI_LZ_BATCH", "3")
    enc, enc_call = _encoder(ctx, "pipe-bgzf")
    _, kind, recipe, block, _, _ = CASES["pipe-bgzf"]
    data, want = sc.make(recipe), sc.expected(kind, recipe, block)
    so, oo = B.walk(want["out"])
    members, total = len(so) - 1, len(data)
    ranges = [(0, 1), (oo[1] - 7, 15), (oo[2] + 100, 2 * block), (oo[5] - 1, oo[8] - oo[5] + 2), (total - 10, 50), (total, 4), (3, 0)]
    offs, size, _, d_off, d_len, d_at, max_pieces = _range_arrays(ctx, so, oo, ranges)
    count = len(ranges)
    pairs, cnt = enc.out("pairs", 16 * (members + 1), table=True), enc.out("count", 16, table=True)
    out, got, status, failed = enc.out("rout", size), enc.out("got", 8 * count, table=True), enc.out("status", 4 * count), enc.out("failed", 4)
    d_stream, L, h, n = enc.outs["out"][0], ctx.L, ctx.h, want["nbytes"]
    call = sc.chain(enc_call,
                    lambda: L.mi_bgzf_index_dev(h, sc.ptr(d_stream), n, sc.ptr(pairs), members, sc.ptr(cnt), ctx.stream_ptr()),
                    lambda: L.mi_bgzf_read_ranges_dev(h, sc.ptr(d_stream), n, sc.ptr(pairs), members, count, sc.ptr(d_off), sc.ptr(d_len),
                                                      sc.ptr(out), sc.ptr(d_at), size, max_pieces, sc.ptr(got), sc.ptr(status), sc.ptr(failed),
                                                      0, ctx.stream_ptr()))
    inner, ranges_check = enc.check, _range_check(data.tobytes(), ranges, offs)

    def check(g):
        inner(g)
        assert _i64s(g["count"], 2) == [members, total]
        ranges_check(dict(g, out=g["rout"]))
    enc.check, enc.asynchronous, enc.name = check, False, "round-trip-bgzf"
    sc.run(enc, call)


# ---- 9. two contexts, two streams; a busy default stream ------------------------------------------------------------------------------
def test_two_contexts_on_two_streams(monkeypatch):
    """include/mi_codec.h: one context per concurrent stream — two pipeline encodes of different data in different modes,
    queued interleaved on two streams, both late, both poisoned early, both the oracle's"""
    monkeypatch.setenv("MI_LZ_BATCH", "3")
    ctxs = [Context(0), Context(0)]
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pairs = [sc.encoder_case(ctxs[0], *CASES["pipe-tokens"]), sc.encoder_case(ctxs[1], *CASES["pipe-bgzf"])]
        t = [sc.warm_and_time(c, f, S) for (c, f), S in zip(pairs, streams)]
        for (c, f), S in zip(pairs, streams):
            sc.scrub(c, f, S)
        delay_ms = sc.delay_for(max(t) * 2)
        for attempt in (0, 1):
            for (c, _), S in zip(pairs, streams):
                with torch.cuda.stream(S):
                    c.poison()
            torch.cuda.synchronize()
            events = []
            for (c, _), S in zip(pairs, streams):
                with torch.cuda.stream(S):
                    sc.Delay.get()(delay_ms)
                    c.load()
                    ev = torch.cuda.Event()
                    ev.record()
                    events.append(ev)
            rcs = []
            for (c, f), S in zip(pairs, streams):
                with torch.cuda.stream(S):
                    rcs.append(f())
            late = [not ev.query() for ev in events]
            for (c, _), S in zip(pairs, streams):
                with torch.cuda.stream(S):
                    c.keep()
                    c.poison()
            for (c, _), S in zip(pairs, streams):
                with torch.cuda.stream(S):
                    c.ctx.sync()
            assert rcs == [0, 0]
            if all(late) or attempt:
                break
            delay_ms *= 4
        print(f"stream-order timing: two-contexts: calls {1e3 * t[0]:.3f} + {1e3 * t[1]:.3f} ms on the host, delay {delay_ms:.1f} ms")
        assert all(late), f"vacuous — a late copy had finished when the calls returned (delay {delay_ms:.1f} ms)"
        for c, _ in pairs:
            c.check(c.kept())
    finally:
        for c in ctxs:
            c.close()


def test_call_beside_a_busy_default_stream(ctx, monkeypatch):
    """the same case while unrelated copies keep the default stream busy: nothing of the call may be ordered behind them, and
    nothing of it may lean on them"""
    monkeypatch.setenv("MI_LZ_BATCH", "3")
    a = torch.empty(1 << 28, dtype=torch.uint8, device=ctx.device)
    b = torch.empty_like(a)

    def background():
        for _ in range(300):
            b.copy_(a)
    sc.run(*_encoder(ctx, "pipe-z-zlib"), background=background)
    torch.cuda.synchronize()


# ---- the negative control ---------------------------------------------------------------------------------------------------------------
def test_negative_control_a_missing_dependency_shows(ctx, monkeypatch):
    """the late copy on one stream, the deflate-token encode on another, NO event between them: the encoder must see the
    poison (any bytes are a valid input to it) and its stream must differ from the oracle's for the data.  Two streams can
    share one of the process's hardware queues and serialise by accident, so the pairs among four fresh streams are tried
    and one that shows the difference is enough."""
    monkeypatch.delenv("MI_LZ_BATCH", raising=False)
    c, call = _encoder(ctx, "solo-tokens")
    want = sc.expected(*CASES["solo-tokens"][1:])
    w = np.frombuffer(want["out"], dtype=np.uint8)
    streams = [torch.cuda.Stream() for _ in range(4)]
    t = sc.warm_and_time(c, call, streams[0])
    sc.scrub(c, call, streams[0])
    delay_ms = max(sc.delay_for(t), 20.0)
    seen = {}
    for i, j in itertools.combinations(range(4), 2):
        with torch.cuda.stream(streams[j]):
            c.poison()
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[i]):
            sc.Delay.get()(delay_ms)
            c.load()
        with torch.cuda.stream(streams[j]):
            rc = call()
            c.keep()
        torch.cuda.synchronize()
        assert rc == 0
        got = c.kept()
        seen[(i, j)] = bool((got["out"][: w.size] != w).any()) or _i64s(got["bits"], len(want["bits"])) != list(want["bits"])
    print(f"stream-order negative control: differs per stream pair {seen} (delay {delay_ms:.1f} ms)")
    assert any(seen.values()), f"no pair of streams showed the missing dependency: {seen}"
