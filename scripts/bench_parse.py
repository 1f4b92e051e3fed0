"""Mode Z's two parses side by side on inputs that are sparse or repetitive: the `zeros` input and the `runs` and `pages`
families of synth.py (and `text` as the yardstick), raw container, 64 KiB blocks.  Per family and parse: the output size, the
COLD time (the first encode of that input by this process: the context has met neither the input nor, for parse 0 / 1 of
the first family, the parse's code objects' first launch) and the WARM time (median of --repeats further encodes, HIP
events), alternating the two parses.  One JSON line.

    python scripts/bench_parse.py [--bytes 100000000] [--repeats 5] [--families zeros,runs,pages]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compression_algorithms_amd import lz, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--families", default="zeros,runs,pages")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = lz.default_context()
    ps = {k: lz.params("deflate", parse=k) for k in (0, 1)}
    n = a.bytes
    nblocks = (n + 65535) // 65536
    cap = lz.bound_bytes_z(n, ps[0], 0) + 64
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    bits = torch.zeros(nblocks + 2, dtype=torch.int64, device=dev)
    s = ctx.stream_ptr()
    res = dict(device=torch.cuda.get_device_name(0), bytes=n, repeats=a.repeats)

    def timed(x, parse):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        st = ctx.L.mi_deflate_z_encode_dev(ctx.h, C.byref(ps[parse]), 0, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), cap,
                                           C.c_void_p(bits.data_ptr()), C.c_void_p(bits[nblocks + 1:].data_ptr()), s)
        assert st == 0, st
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), int(bits[nblocks + 1].item())

    for fam in a.families.split(","):
        h = np.zeros(n, dtype=np.uint8) if fam == "zeros" else np.ascontiguousarray(synth.family(fam, a.seed, n))
        x = torch.from_numpy(h).to(dev)
        r = {}
        for parse in (0, 1):
            ms, size = timed(x, parse)
            r[f"parse{parse}"] = dict(bytes_out=size, ratio=round(n / size, 3), cold_ms=round(ms, 3), cold_gbps=round(n / ms / 1e6, 3))
        warm = {0: [], 1: []}
        for _ in range(a.repeats):
            for parse in (0, 1):
                warm[parse].append(timed(x, parse)[0])
        for parse in (0, 1):
            t = sorted(warm[parse])
            r[f"parse{parse}"].update(warm_ms_median=round(t[len(t) // 2], 3), warm_ms_min=round(t[0], 3), warm_ms_max=round(t[-1], 3),
                                      warm_gbps=round(n / t[len(t) // 2] / 1e6, 3))
        # a sanity check, not a test: the parse-1 stream inflates to the input
        ms, size = timed(x, 1)
        y = lz.inflate(out[:size], n, bits[: nblocks + 1], 65536, "raw", ctx=ctx)
        assert torch.equal(y, x), fam
        res[fam] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
