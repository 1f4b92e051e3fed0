"""BGZF against mode Z (gzip) on bench.py's corpus: GB/s and ratio, warm, HIP events, the median of alternating runs in one
process.  Encode: mi_bgzf_encode_dev (block 65 280) against mi_deflate_z_encode_dev (gzip, block 65 536).  Decode:
mi_bgzf_index_dev and mi_bgzf_inflate_dev, timed separately, against mi_inflate_dev on the mode-Z gzip stream of the same
input with its table.  One JSON line.

    python scripts/bench_bgzf.py [--bytes 1000000000] [--repeats 5] [--parse {0,1}]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compression_algorithms_amd import lz, synth  # noqa: E402


def timed(modes, repeats):
    times = {m: [] for m, _ in modes}
    for _ in range(repeats):
        for m, f in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1))
    return {m: sorted(t) for m, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=12345)            # bench.py's corpus
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parse", type=int, choices=(0, 1), default=0)   # the parse of both encoders (include/mi_codec.h, mode Z)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = lz.default_context()
    pz, pb = lz.params("deflate", parse=a.parse), lz.params("deflate", block=lz.BGZF_BLOCK, parse=a.parse)
    x = synth.enwik_like(a.bytes, seed=a.seed, device=dev)
    n = x.numel()
    nbz, nbb = (n + pz.block - 1) // pz.block, (n + pb.block - 1) // pb.block
    bits = torch.zeros(max(nbz, nbb) + 2, dtype=torch.int64, device=dev)
    s = ctx.stream_ptr()
    cap = max(lz.bound_bytes_z(n, pz, 2), lz.bound_bytes_bgzf(n, pb)) + 64
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    xp, op, bp = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(bits.data_ptr())

    def enc_z():
        assert ctx.L.mi_deflate_z_encode_dev(ctx.h, C.byref(pz), 2, xp, n, op, cap, bp, C.c_void_p(bits[nbz + 1:].data_ptr()), s) == 0

    def enc_b():
        assert ctx.L.mi_bgzf_encode_dev(ctx.h, C.byref(pb), xp, n, op, cap, bp, C.c_void_p(bits[nbb + 1:].data_ptr()), s) == 0

    streams = {}
    for m, f, nb in (("mode_z_gzip", enc_z, nbz), ("bgzf", enc_b, nbb)):     # warm: workspace, code objects; keep the streams
        f()
        size = int(bits[nb + 1].item())
        streams[m] = (out[:size].clone(), bits[: nb + 1].clone(), size)
    res = {}
    for m, t in timed([("mode_z_gzip", enc_z), ("bgzf", enc_b)], a.repeats).items():
        med = t[len(t) // 2]
        res[m + "_encode"] = dict(ms_median=round(med, 3), ms_min=round(t[0], 3), gbps=round(n / med / 1e6, 3),
                                  ratio=round(n / streams[m][2], 4), bytes_out=streams[m][2])
    # one profiled encode of each (events around every launch: its own run, not part of the timings above)
    ctx.set_profiling(True)
    for m, f in (("mode_z_gzip", enc_z), ("bgzf", enc_b)):
        ctx.kernel_times()
        f()
        torch.cuda.synchronize()
        res[m + "_encode_kernels_ms"] = {k["name"]: round(k["ms"] * k["launches"], 3) for k in ctx.kernel_times()}
    ctx.set_profiling(False)
    res["bgzf_encode_over_mode_z_gzip"] = round(res["bgzf_encode"]["ms_median"] / res["mode_z_gzip_encode"]["ms_median"], 4)
    # ---- decode
    y = torch.empty(n, dtype=torch.uint8, device=dev)
    yp = C.c_void_p(y.data_ptr())
    dz, tz, bz = streams["mode_z_gzip"]
    db, _, bb = streams["bgzf"]
    members = nbb + 1
    pairs = torch.zeros((members + 1, 2), dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)

    def dec_z(flags):
        def f():
            assert ctx.L.mi_inflate_dev(ctx.h, 2, pz.block, C.c_void_p(dz.data_ptr()), bz, C.c_void_p(tz.data_ptr()), yp, n, flags, s) == 0
        return f

    def index():
        assert ctx.L.mi_bgzf_index_dev(ctx.h, C.c_void_p(db.data_ptr()), bb, C.c_void_p(pairs.data_ptr()), members, C.c_void_p(cnt.data_ptr()), s) == 0

    def count():
        assert ctx.L.mi_bgzf_index_dev(ctx.h, C.c_void_p(db.data_ptr()), bb, None, 0, C.c_void_p(cnt.data_ptr()), s) == 0

    def dec_b(flags):
        def f():
            assert ctx.L.mi_bgzf_inflate_dev(ctx.h, C.c_void_p(db.data_ptr()), bb, C.c_void_p(pairs.data_ptr()), 0, members, yp, n, flags, s) == 0
        return f

    index()
    assert [int(v) for v in cnt.cpu()] == [members, n]
    nock = lz.MI_INFLATE_NO_CHECKSUM
    decs = [("mode_z_gzip_inflate", dec_z(0)), ("bgzf_index", index), ("bgzf_count_only", count), ("bgzf_inflate", dec_b(0)),
            ("mode_z_gzip_inflate_no_checksum", dec_z(nock)), ("bgzf_inflate_no_checksum", dec_b(nock))]
    for m, f in decs:                                           # warm, and right
        y.zero_()
        f()
        if "inflate" in m:
            assert torch.equal(y, x), m
    for m, t in timed(decs, a.repeats).items():
        med = t[len(t) // 2]
        res[m] = dict(ms_median=round(med, 3), ms_min=round(t[0], 3), gbps=round(n / med / 1e6, 3))
    res["bgzf_index_over_inflate"] = round(res["bgzf_index"]["ms_median"] / res["bgzf_inflate"]["ms_median"], 4)
    res["bgzf_index_plus_inflate_over_mode_z_inflate"] = round(
        (res["bgzf_index"]["ms_median"] + res["bgzf_inflate"]["ms_median"]) / res["mode_z_gzip_inflate"]["ms_median"], 4)
    res["members"] = members
    res["device"] = torch.cuda.get_device_name(0)
    res["bytes"] = n
    res["repeats"] = a.repeats
    res["parse"] = a.parse
    print(json.dumps(res))


if __name__ == "__main__":
    main()
