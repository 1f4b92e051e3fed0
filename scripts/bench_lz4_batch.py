"""Batched LZ4 (mi_lz4_encode_batch_dev, mi_lz4_decode_batch_dev), raw blocks and frames, on bench.py's corpus cut into
65 536-byte pages, against the Snappy batch and the DEFLATE batches (raw container) on the SAME items in the SAME process: GB/s of
uncompressed bytes, warm, HIP events, the median of alternating runs with min, max and spread.

The decoders read what the encoders of this run wrote.  `ratio` is compressed / uncompressed bytes; `stock_lz4_ratio` is what
pyarrow's "lz4_raw" codec (LZ4_compress_default) makes of the same pages, and `stock_reads` whether pyarrow's "lz4_raw" and "lz4"
codecs decode the first, middle and last item of this run to the input (both null where pyarrow is not installed); `restated`
compares those items' bytes with the emission rule restated on the CPU (tests/lz4_cases.py; null where the oracle library is not
built).  --dump DIR writes those items (input, block, frame) as files, for a stock reader elsewhere.  One JSON line: the line that
belongs in profiles/.

    python scripts/bench_lz4_batch.py [--bytes 100000000] [--repeats 7] [--parse 0] [--dump DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from bench_snappy_batch import ITEM, Arrays, summary, timed  # noqa: E402  (the timing loop and the batch's arrays)
from compression_algorithms_amd import lz, synth  # noqa: E402


def run_set(ctx, p, pieces, repeats, dump):
    sizes = [len(pc) for pc in pieces]
    n, count = sum(sizes), len(pieces)
    at, offs = 0, []
    for sz in sizes:
        at = (at + 15) & ~15
        offs.append(at)
        at += sz
    h = np.zeros(at + 64, dtype=np.uint8)
    for pc, o in zip(pieces, offs):
        h[o:o + len(pc)] = np.frombuffer(pc, dtype=np.uint8)
    d_x = torch.from_numpy(h).to(ctx.device)
    in_ptrs = [d_x.data_ptr() + o for o in offs]
    q = lambda t: C.c_void_p(t.data_ptr())
    L, hnd, s = ctx.L, ctx.h, ctx.stream_ptr()
    max_blocks = sum((sz + p.block - 1) // p.block for sz in sizes)
    enc = {"lz4_block": Arrays(ctx, in_ptrs, sizes, [lz.lz4_batch_bound_bytes(sz, p, "block") for sz in sizes]),
           "lz4_frame": Arrays(ctx, in_ptrs, sizes, [lz.lz4_batch_bound_bytes(sz, p, "frame") for sz in sizes]),
           "snappy": Arrays(ctx, in_ptrs, sizes, [lz.snappy_batch_bound_bytes(sz, p) for sz in sizes]),
           "deflate": Arrays(ctx, in_ptrs, sizes, [lz.bound_bytes_z(sz, p, 0) for sz in sizes])}
    encoders = {
        "lz4_block": lambda a: L.mi_lz4_encode_batch_dev(hnd, C.byref(p), 0, count, q(a.p_in), q(a.p_nb), max_blocks, *a.args(), s),
        "lz4_frame": lambda a: L.mi_lz4_encode_batch_dev(hnd, C.byref(p), 1, count, q(a.p_in), q(a.p_nb), max_blocks, *a.args(), s),
        "snappy": lambda a: L.mi_snappy_encode_batch_dev(hnd, C.byref(p), count, q(a.p_in), q(a.p_nb), max_blocks, *a.args(), s),
        "deflate": lambda a: L.mi_deflate_batch_dev(hnd, C.byref(p), 0, count, q(a.p_in), q(a.p_nb), max_blocks, *a.args(), s)}
    decoders = {
        "lz4_block": lambda a: L.mi_lz4_decode_batch_dev(hnd, count, q(a.p_in), q(a.p_nb), *a.args(), 0, 0, s),
        "lz4_frame": lambda a: L.mi_lz4_decode_batch_dev(hnd, count, q(a.p_in), q(a.p_nb), *a.args(), 1, 0, s),
        "snappy": lambda a: L.mi_snappy_decode_batch_dev(hnd, count, q(a.p_in), q(a.p_nb), *a.args(), 0, s),
        "deflate": lambda a: L.mi_inflate_batch_dev(hnd, 0, count, q(a.p_in), q(a.p_nb), *a.args(), 0, s)}
    nb, dec = {}, {}
    for m, a in enc.items():
        assert encoders[m](a) == 0, m
        nb[m] = a.results()
        dec[m] = Arrays(ctx, a.out_ptrs, nb[m], sizes)            # the decoders read the encoders' outputs where they lie
        assert decoders[m](dec[m]) == 0, m
        assert dec[m].results() == sizes, m
    picks = sorted({0, count // 2, count - 1})
    for m in enc:                                                # a sanity check, not a test
        for k in picks:
            assert dec[m].item(k, sizes[k]) == pieces[k], (m, k)
    fmts = (("lz4_block", "block"), ("lz4_frame", "frame"))
    restated = None
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lz4_cases as Z
        restated = all(enc[m].item(k, nb[m][k]) == Z.restate(pieces[k], p.block, p.parse, f) for m, f in fmts for k in picks)
    except (ImportError, OSError):
        pass
    stock_ratio = stock_reads = None
    try:
        import pyarrow as pa
        raw, fr = pa.Codec("lz4_raw"), pa.Codec("lz4")
        stock_ratio = round(sum(len(raw.compress(pc, asbytes=True)) for pc in pieces) / n, 4)
        stock_reads = all(raw.decompress(enc["lz4_block"].item(k, nb["lz4_block"][k]), decompressed_size=sizes[k], asbytes=True) == pieces[k] and
                          fr.decompress(enc["lz4_frame"].item(k, nb["lz4_frame"][k]), decompressed_size=sizes[k], asbytes=True) == pieces[k]
                          for k in picks)
    except ImportError:
        pass
    if dump:
        os.makedirs(dump, exist_ok=True)
        for k in picks:
            with open(os.path.join(dump, f"item{k}.bin"), "wb") as f:
                f.write(pieces[k])
            for m, fmt in fmts:
                with open(os.path.join(dump, f"item{k}.{fmt}.lz4"), "wb") as f:
                    f.write(enc[m].item(k, nb[m][k]))
    res = dict(items=count, bytes=n, restated=restated, stock_reads=stock_reads, stock_lz4_ratio=stock_ratio)
    for m in enc:
        res[m + "_out_bytes"] = sum(nb[m])
        res[m + "_ratio"] = round(sum(nb[m]) / n, 4)
    modes = [(m + "_encode", (lambda m=m: encoders[m](enc[m]))) for m in enc] + [(m + "_decode", (lambda m=m: decoders[m](dec[m]))) for m in enc]
    for m, v in timed(modes, repeats).items():
        res[m] = summary(v, n)
    for m, _ in fmts:
        res[f"encode_{m}_over_snappy"] = round(res[m + "_encode"]["gbps"] / res["snappy_encode"]["gbps"], 3)
        res[f"encode_{m}_over_deflate"] = round(res[m + "_encode"]["gbps"] / res["deflate_encode"]["gbps"], 3)
        res[f"decode_{m}_over_snappy"] = round(res[m + "_decode"]["gbps"] / res["snappy_decode"]["gbps"], 3)
    if stock_ratio:
        res["size_lz4_block_over_stock"] = round(res["lz4_block_ratio"] / stock_ratio, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parse", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    ctx = lz.default_context()
    p = lz.params("deflate", parse=a.parse)
    x = synth.enwik_like(a.bytes, seed=a.seed).numpy().tobytes()
    pages = [x[i:i + ITEM] for i in range(0, a.bytes, ITEM)]
    res = dict(bench="lz4_batch", device=torch.cuda.get_device_name(0), parse=a.parse, block=p.block, repeats=a.repeats,
               pages=run_set(ctx, p, pages, a.repeats, a.dump))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
