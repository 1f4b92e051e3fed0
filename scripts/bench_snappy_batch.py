"""Batched Snappy (mi_snappy_encode_batch_dev, mi_snappy_decode_batch_dev) on bench.py's corpus, against the DEFLATE batches
(mi_deflate_batch_dev, mi_inflate_batch_dev; raw container) on the SAME items in the SAME process: GB/s of uncompressed bytes,
warm, HIP events, the median of alternating runs with min, max and spread.  The item sets of bench_deflate_batch.py and
bench_inflate_batch.py:

  uniform   the corpus cut into 65 536-byte pages
  skewed    10 000 items of 4 KiB plus four of 1 MiB

The decoders read what the encoders of this run wrote.  `ratio` is compressed / uncompressed bytes; `restated` compares the
first, middle and last item's Snappy bytes with the emission rule restated on the CPU (tests/snappy_cases.py; null where the
oracle library is not built).  One JSON line: the line that belongs in profiles/.

    python scripts/bench_snappy_batch.py [--bytes 100000000] [--repeats 7] [--parse 0]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from compression_algorithms_amd import lz, synth  # noqa: E402

ITEM = 65536


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


def summary(t, nbytes):
    med = t[len(t) // 2]
    return dict(ms_median=round(med, 3), ms_min=round(t[0], 3), ms_max=round(t[-1], 3), gbps=round(nbytes / med / 1e6, 3),
                spread=round((t[-1] - t[0]) / med, 4))


class Arrays:
    """pointer, size, capacity and result arrays of one batch whose item k reads `sizes[k]` bytes at in_ptrs[k]"""

    def __init__(self, ctx, in_ptrs, sizes, caps):
        dev = ctx.device
        self.ctx, self.count, self.caps = ctx, len(sizes), caps
        self.oo = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in caps])])
        self.out = torch.empty(int(self.oo[-1]) + 16, dtype=torch.uint8, device=dev)
        i64 = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)
        self.p_in, self.p_nb = i64(in_ptrs), i64(sizes)
        self.out_ptrs = [self.out.data_ptr() + int(a) for a in self.oo[:-1]]
        self.p_out, self.p_cap = i64(self.out_ptrs), i64(caps)
        self.nbytes = torch.zeros(self.count, dtype=torch.int64, device=dev)
        self.status = torch.zeros(self.count, dtype=torch.int32, device=dev)
        self.failed = torch.zeros(1, dtype=torch.int32, device=dev)

    def args(self):
        q = lambda t: C.c_void_p(t.data_ptr())
        return q(self.p_out), q(self.p_cap), q(self.nbytes), q(self.status), q(self.failed)

    def results(self):
        torch.cuda.synchronize()
        assert int(self.failed[0]) == 0, [int(v) for v in self.status.cpu()][:16]
        return [int(v) for v in self.nbytes.cpu()]

    def item(self, k, n):
        return self.out[int(self.oo[k]):int(self.oo[k]) + n].cpu().numpy().tobytes()


def run_set(ctx, p, name, pieces, repeats):
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
    sn = Arrays(ctx, in_ptrs, sizes, [lz.snappy_batch_bound_bytes(sz, p) for sz in sizes])
    df = Arrays(ctx, in_ptrs, sizes, [lz.bound_bytes_z(sz, p, 0) for sz in sizes])

    def snappy_encode():
        assert L.mi_snappy_encode_batch_dev(hnd, C.byref(p), count, q(sn.p_in), q(sn.p_nb), max_blocks, *sn.args(), s) == 0

    def deflate_encode():
        assert L.mi_deflate_batch_dev(hnd, C.byref(p), 0, count, q(df.p_in), q(df.p_nb), max_blocks, *df.args(), s) == 0
    snappy_encode()
    sn_nb = sn.results()
    deflate_encode()
    df_nb = df.results()
    # the decoders read the encoders' outputs where they lie
    sd = Arrays(ctx, sn.out_ptrs, sn_nb, sizes)
    dd = Arrays(ctx, df.out_ptrs, df_nb, sizes)

    def snappy_decode():
        assert L.mi_snappy_decode_batch_dev(hnd, count, q(sd.p_in), q(sd.p_nb), *sd.args(), 0, s) == 0

    def inflate():
        assert L.mi_inflate_batch_dev(hnd, 0, count, q(dd.p_in), q(dd.p_nb), *dd.args(), 0, s) == 0
    snappy_decode()
    inflate()
    assert sd.results() == sizes and dd.results() == sizes
    picks = sorted({0, count // 2, count - 1})
    for k in picks:                                              # a sanity check, not a test
        assert sd.item(k, sizes[k]) == pieces[k] and dd.item(k, sizes[k]) == pieces[k], k
    restated = None
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import snappy_cases as S
        restated = all(sn.item(k, sn_nb[k]) == S.restate(pieces[k], p.block, p.parse) for k in picks)
    except (ImportError, OSError):
        pass
    res = dict(items=count, bytes=n, snappy_out_bytes=sum(sn_nb), deflate_out_bytes=sum(df_nb),
               snappy_ratio=round(sum(sn_nb) / n, 4), deflate_ratio=round(sum(df_nb) / n, 4), restated=restated)
    t = timed([("snappy_encode", snappy_encode), ("deflate_encode", deflate_encode), ("snappy_decode", snappy_decode),
               ("inflate", inflate)], repeats)
    for m, v in t.items():
        res[m] = summary(v, n)
    res["encode_snappy_over_deflate"] = round(res["snappy_encode"]["gbps"] / res["deflate_encode"]["gbps"], 3)
    res["decode_snappy_over_inflate"] = round(res["snappy_decode"]["gbps"] / res["inflate"]["gbps"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parse", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skew-small", type=int, default=10_000)
    ap.add_argument("--skew-big", type=int, default=4)
    a = ap.parse_args()
    ctx = lz.default_context()
    p = lz.params("deflate", parse=a.parse)
    x = synth.enwik_like(max(a.bytes, a.skew_small * 4096, 1 << 20), seed=a.seed).numpy().tobytes()
    uniform = [x[i:i + ITEM] for i in range(0, a.bytes, ITEM)]
    skewed = [x[i * 4096:(i + 1) * 4096] for i in range(a.skew_small)]
    for k in range(a.skew_big):                                   # the large items spread over the batch, none of them first
        skewed.insert((k + 1) * a.skew_small // (a.skew_big + 1) + k, x[:1 << 20][k:] + x[:k])
    res = dict(bench="snappy_batch", device=torch.cuda.get_device_name(0), parse=a.parse, block=p.block, repeats=a.repeats,
               uniform=run_set(ctx, p, "uniform", uniform, a.repeats), skewed=run_set(ctx, p, "skewed", skewed, a.repeats))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
