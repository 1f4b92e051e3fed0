"""Mode Z (standard DEFLATE) against mode H on bench.py's corpus: GB/s and ratio, warm, HIP events, alternating encodes in
one process; zlib.compress levels 1 and 6 on one host core as the CPU baseline.  Then the decoders, the same way: the GPU
inflater (mi_inflate_dev) on the raw and gzip streams, with and without its checksum pass, against mode H's decoder, and
zlib.decompress on one host core.

    python scripts/bench_deflate_z.py [--bytes 1000000000] [--repeats 5] [--cpu-bytes 100000000] [--parse {0,1}]

--parse 1: mode Z with the lazy parse and matches up to 255 bytes (mode H keeps the reference's tokens).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compression_algorithms_amd import lz, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=12345)            # bench.py's corpus
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-bytes", type=int, default=100_000_000)
    ap.add_argument("--parse", type=int, choices=(0, 1), default=0)   # mode Z's parse (include/mi_codec.h)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = lz.default_context()
    p, pz = lz.params("deflate"), lz.params("deflate", parse=a.parse)          # mode H, mode Z
    x = synth.enwik_like(a.bytes, seed=a.seed, device=dev)
    n = x.numel()
    nblocks = (n + p.block - 1) // p.block
    bits = torch.zeros(nblocks + 2, dtype=torch.int64, device=dev)
    s = ctx.stream_ptr()
    cap_h = int(ctx.L.mi_deflate_h_bound_bytes(n, C.byref(p))) + 64
    cap_z = max(lz.bound_bytes_z(n, pz, c) for c in (0, 2)) + 64
    out = torch.empty(max(cap_h, cap_z), dtype=torch.uint8, device=dev)
    xp, op, bp, ob = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(bits.data_ptr()), C.c_void_p(bits[nblocks + 1:].data_ptr())

    def run_h():
        assert ctx.L.mi_deflate_h_encode_dev(ctx.h, C.byref(p), xp, n, op, cap_h, bp, s) == 0
        return lambda: int(bits[nblocks].item()) // 8

    def run_z(c):
        def f():
            assert ctx.L.mi_deflate_z_encode_dev(ctx.h, C.byref(pz), c, xp, n, op, cap_z, bp, ob, s) == 0
            return lambda: int(bits[nblocks + 1].item())
        return f

    modes = [("mode_h", run_h), ("mode_z_raw", run_z(0)), ("mode_z_gzip", run_z(2))]
    for _, f in modes:                                         # warm: workspace, code objects
        f()()
    times = {m: [] for m, _ in modes}
    size = {}
    for _ in range(a.repeats):
        for m, f in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            sz = f()
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1))
            size[m] = sz()
    res = {}
    for m, _ in modes:
        t = sorted(times[m])
        med = t[len(t) // 2]
        res[m] = dict(ms_median=round(med, 3), ms_min=round(t[0], 3), gbps=round(n / med / 1e6, 3), ratio=round(n / size[m], 4),
                      bytes_out=size[m])
    # ---- decoders: every stream in a buffer of its own, the output compared once, then timed alternating
    streams = {}
    for m, f in modes:
        nb = f()()
        streams[m] = (out[:nb].clone(), bits[: nblocks + 1].clone(), nb)
    y = torch.empty(n, dtype=torch.uint8, device=dev)
    yp = C.c_void_p(y.data_ptr())

    def dec_h():
        d, t, nb = streams["mode_h"]
        assert ctx.L.mi_deflate_h_decode_dev(ctx.h, C.byref(p), C.c_void_p(d.data_ptr()), nb, C.c_void_p(t.data_ptr()), yp, n, s) == 0

    def dec_z(m, c, flags):
        def f():
            d, t, nb = streams[m]
            assert ctx.L.mi_inflate_dev(ctx.h, c, p.block, C.c_void_p(d.data_ptr()), nb, C.c_void_p(t.data_ptr()), yp, n, flags, s) == 0
        return f

    decs = [("mode_h_decode", dec_h), ("mode_z_decode_raw", dec_z("mode_z_raw", 0, 0)),
            ("mode_z_decode_gzip", dec_z("mode_z_gzip", 2, 0)),
            ("mode_z_decode_gzip_no_checksum", dec_z("mode_z_gzip", 2, lz.MI_INFLATE_NO_CHECKSUM))]
    for m, f in decs:                                           # warm, and right
        y.zero_()
        f()
        assert torch.equal(y, x), m
    dtimes = {m: [] for m, _ in decs}
    for _ in range(a.repeats):
        for m, f in decs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            dtimes[m].append(e0.elapsed_time(e1))
    for m, _ in decs:
        t = sorted(dtimes[m])
        med = t[len(t) // 2]
        res[m] = dict(ms_median=round(med, 3), ms_min=round(t[0], 3), gbps=round(n / med / 1e6, 3))
    res["mode_z_decode_over_mode_h_decode"] = round(res["mode_z_decode_raw"]["gbps"] / res["mode_h_decode"]["gbps"], 3)
    cpu = x[: a.cpu_bytes].cpu().numpy().tobytes()
    zc = streams["mode_z_gzip"][0].cpu().numpy().tobytes() if a.cpu_bytes >= n else lz.compress_z(x[: a.cpu_bytes], pz, "gzip").tobytes()
    t0 = time.perf_counter()
    back = zlib.decompress(zc, 31)
    dt = time.perf_counter() - t0
    assert len(back) == len(cpu)
    res["zlib_decompress_1core"] = dict(bytes_out=len(cpu), gbps=round(len(cpu) / dt / 1e9, 4))
    for lvl in (1, 6):
        t0 = time.perf_counter()
        z = zlib.compress(cpu, lvl)
        dt = time.perf_counter() - t0
        res[f"zlib_level{lvl}_1core"] = dict(bytes_in=len(cpu), gbps=round(len(cpu) / dt / 1e9, 4), ratio=round(len(cpu) / len(z), 4))
    res["device"] = torch.cuda.get_device_name(0)
    res["bytes"] = n
    res["repeats"] = a.repeats
    res["parse"] = a.parse
    print(json.dumps(res))


if __name__ == "__main__":
    main()
