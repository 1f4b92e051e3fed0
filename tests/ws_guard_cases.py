"""The cases of test_ws_guard_gpu.py, run in ONE child process on the test build of the library (lib_test, -DMI_TEST_HOOKS):
every device entry point that works in the context workspace, on inputs that are tiny but take every layout the entry point
has (one set and one batch; three sets in rotation plus the tail; the sliced and the whole-block wide finder; a block redone in
its own rows).  Per case: a fresh context, reset -> the call (it grows the workspace) -> arm -> the same call again -> check.
A case is ONE entry point: the guard lies behind the largest request since the reset, so whatever a decoder or a later step of
a sequence needs as input (an encoded stream, an index, a tree) is made beforehand on ANOTHER context.
Prints one JSON object {case: [offset of the first changed guard byte or -1, outputs of both calls equal]}."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESET, ARM, CHECK = 0, 1, 2


def _b(t):
    return t.cpu().numpy().tobytes()


def _inputs():
    from compression_algorithms_amd import synth
    text = synth.enwik_like(6 * 65536 + 17, seed=161).numpy()
    wide = synth.enwik_like(300_000, seed=162).numpy()
    flagged = synth.enwik_like(6 * 131072, seed=71).numpy().copy()   # test_lz_wide_gpu.py::test_one_flagged_block_is_redone_alone
    flagged[3 * 131072 + 5000: 3 * 131072 + 45000] = 0
    flagged[5 * 131072 + 100: 5 * 131072 + 130] = 7
    return text, wide, flagged


def cases(pctx):
    """-> {name: (environment of the call, fn(ctx) -> list of bytes)}; pctx: the context that prepares inputs"""
    from compression_algorithms_amd import _lib, fse, huffman, lz
    text, wide, flagged = _inputs()
    one, many = text[: 3 * 65536 + 17], text                         # one batch and one set; with MI_LZ_BATCH=2 seven blocks
    pd, p14, pw = lz.params("deflate"), lz.params("lz77", 14), lz.params("lz77", 16, 131072)
    out = {}
    for tag, x, env in (("", one, {}), ("_batch2", many, {"MI_LZ_BATCH": "2"})):
        out["tokens" + tag] = (env, lambda ctx, x=x: [lz.compress(x, pd, ctx).tobytes()])
        out["h" + tag] = (env, lambda ctx, x=x: [lz.compress_h(x, pd, ctx).tobytes()])
        out["z_zlib" + tag] = (env, lambda ctx, x=x: [lz.compress_z(x, pd, "zlib", ctx).tobytes()])
        out["bgzf" + tag] = (env, lambda ctx, x=x: [lz.compress_bgzf(x, ctx=ctx).tobytes()])
        out["lz77w14" + tag] = (env, lambda ctx, x=x: [lz.compress(x, p14, ctx).tobytes()])

    items = [text[:0], text[:1], text[:65536], text[:70000], text[:200000]]

    def deflate_batch(ctx):
        r = lz.deflate_batch(items, ctx=ctx)
        return [_b(o) for o in r.outputs] + [_b(r.status)]
    out["deflate_batch"] = ({}, deflate_batch)

    out["wide_sliced"] = ({}, lambda ctx: [lz.compress(wide, pw, ctx).tobytes()])
    out["wide_whole_block"] = ({"MI_LZW_SLICED": "0"}, lambda ctx: [lz.compress(wide, pw, ctx).tobytes()])
    out["wide_one_block_redone"] = ({}, lambda ctx: [lz.compress(flagged, pw, ctx).tobytes()])
    out["find_all"] = ({}, lambda ctx: [_b(lz.find_all(one, pd, ctx))])
    out["find_all32"] = ({}, lambda ctx: [_b(lz.find_all32(wide, pw, ctx))])

    def huff(n):
        def fn(ctx):
            try:
                h = huffman.huffman_compress(text[:n], ctx)
            except _lib.MiError as e:                                # (no symbol at all: the reference gives up too)
                return [b"status %d" % e.status]
            return [_b(h.words), b"%d" % h.total_bits]
        return fn

    def huff3(n, step):                                               # (the histogram step takes nothing from the workspace)
        eng = huffman.HipShardEngine(pctx)
        hist, state = eng.hist(text[:n])
        try:
            tree = eng.build(hist)
            bits = eng.shard_bits(hist, tree)
        except _lib.MiError:
            tree = None                                              # (no symbol: there is no tree to encode with)

        def build(ctx):
            try:
                t = huffman.HipShardEngine(ctx).build(hist)
            except _lib.MiError as e:
                return [b"status %d" % e.status]
            return [_b(t["d_tree"])]

        def encode(ctx):
            if tree is None:
                return [b"no tree"]
            words, tile_off = huffman.HipShardEngine(ctx).encode(state, tree, 0, bits)
            return [_b(words), _b(tile_off)]
        return build if step == "build" else encode
    for n in (100_000, 0):
        out["huffman_%d" % n] = ({}, huff(n))
        out["huffman_build_%d" % n] = ({}, huff3(n, "build"))
        out["huffman_with_tree_%d" % n] = ({}, huff3(n, "encode"))
    out["fse"] = ({}, lambda ctx: [fse.compress(text[: 65536 + 4000], ctx=ctx).tobytes()])
    out["compress_old"] = ({}, lambda ctx: [lz.compress_old(text[:5000], ctx=ctx).tobytes()])

    old = lz.compress_old(text[:5000], ctx=pctx)
    out["decompress_whole"] = ({}, lambda ctx: [_b(lz.decompress_whole(old, ctx))])

    zs = lz.compress_z(one, pd, "zlib", pctx)                        # (the checksum of the decoded bytes inside the call)
    zs.nbytes
    out["decompress_z"] = ({}, lambda ctx: [_b(lz.decompress_z(zs, ctx, verify=True))])

    bg = lz.compress_bgzf(text[: 2 * 65280 + 1000], ctx=pctx).tobytes()          # three members
    idx = lz.bgzf_index(bg, pctx)
    assert idx.members >= 3, idx.members
    ranges = [[65000, 1000], [65279, 2], [130000, 1500], [100, 131000]]          # four ranges that cut members
    out["bgzf_index"] = ({}, lambda ctx: [_b(lz.bgzf_index(bg, ctx).pairs)])
    out["decompress_bgzf"] = ({}, lambda ctx: [_b(lz.decompress_bgzf(bg, idx, ctx=ctx))])

    def bgzf_read(ctx):
        r = lz.bgzf_read(bg, ranges, idx, ctx=ctx)
        return [_b(r[0]), _b(r[2]), _b(r[3])]
    out["bgzf_read"] = ({}, bgzf_read)

    streams = [_b(o) for o in lz.deflate_batch(items, ctx=pctx).outputs]

    def inflate_batch(ctx):
        r = lz.inflate_batch(streams, caps=[len(x) for x in items], ctx=ctx)
        return [_b(o) for o in r.outputs] + [_b(r.status)]
    out["inflate_batch_ordered"] = ({"MI_INFLATE_BATCH_ORDER": "1"}, inflate_batch)
    return out


def main():
    from compression_algorithms_amd.context import Context
    results = {}
    pctx = Context(0)
    for name, (env, fn) in cases(pctx).items():
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            ctx = Context(0)
            guard = ctx.L.mi_test_ws_guard
            guard.restype, guard.argtypes = C.c_int64, [C.c_void_p, C.c_int]
            assert guard(ctx.h, RESET) == -1
            first = fn(ctx)
            assert guard(ctx.h, ARM) == -1, "arming the guard failed"
            second = fn(ctx)
            at = int(guard(ctx.h, CHECK))
            ctx.sync()
            results[name] = [at, first == second]
            ctx.close()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        torch.cuda.synchronize()
    print("WS_GUARD " + json.dumps(results))


if __name__ == "__main__":
    main()
