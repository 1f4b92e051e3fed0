"""Batched deflate (mi_deflate_batch_dev) on bench.py's corpus: GB/s of input bytes, warm, HIP events, the median of
alternating runs with min, max and spread.  Every configuration runs in a child process of its own (a context, its
workspace and the encoders' fallback hint are per process), and prints its own JSON line.  Three cases:

  (a) uniform   the corpus cut into 65 536-byte items (gzip), against mi_deflate_z_encode_dev on the same bytes as ONE buffer
                in the same run: the yardstick — the same blocks; the batch adds descriptors and per-item framing
  (b) aligned   the same items at 16-byte aligned addresses against the same items at addresses offset by 1..15: what the
                register-shifted loads of the descriptor path are worth
  (c) skewed    10 000 items of 4 KiB plus four of 1 MiB

One JSON line.

    python scripts/bench_deflate_batch.py [--bytes 100000000] [--repeats 7]

--dict: the preset-dictionary variant INSTEAD of the three cases.  The corpus behind its first 32 768 bytes (the dictionary)
cut into --dict-item byte items (zlib container): the same items through mi_deflate_batch_dev and through
mi_deflate_batch_dict_dev, alternating in one process, with the compressed bytes of both; and, with --parent-lib PATH (a
libmi_codec.so built from the parent commit, loaded through MI_CODEC_LIB in a child of its own), mi_deflate_batch_dev of that
library on the same items: `no_dict_over_parent` is the ratio of the medians, to be read against the two spreads.

    python scripts/bench_deflate_batch.py --dict [--dict-item 700] [--repeats 3] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


class Batch:
    """the device arrays of one batch over items at (offset, size) of one device buffer; call() launches it (asynchronous)"""

    def __init__(self, ctx, p, container, buf, offs, sizes):
        dev = ctx.device
        self.ctx, self.p, self.c, self.count, self.sizes = ctx, p, lz.CONTAINERS[container], len(offs), sizes
        self.caps = [lz.bound_bytes_z(n, p, self.c) for n in sizes]
        oo = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in self.caps])])
        self.out = torch.empty(int(oo[-1]) + 16, dtype=torch.uint8, device=dev)
        self.oo = oo
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        self.p_in, self.p_nb = i64([buf.data_ptr() + int(a) for a in offs]), i64(sizes)
        self.p_out, self.p_cap = i64([self.out.data_ptr() + int(a) for a in oo[:-1]]), i64(self.caps)
        self.nbytes = torch.zeros(self.count, dtype=torch.int64, device=dev)
        self.status = torch.zeros(self.count, dtype=torch.int32, device=dev)
        self.failed = torch.zeros(1, dtype=torch.int32, device=dev)
        self.max_blocks = sum((n + p.block - 1) // p.block for n in sizes)

    def with_dict(self, d_dict):
        """the same items behind a preset dictionary: capacities and the launch bound follow it"""
        nd = d_dict.numel()
        self.d_dict = d_dict
        self.caps = [lz.deflate_batch_bound_bytes(n, self.p, self.c, nd) for n in self.sizes]
        oo = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in self.caps])])
        self.out = torch.empty(int(oo[-1]) + 16, dtype=torch.uint8, device=self.ctx.device)
        self.oo = oo
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=self.ctx.device)
        self.p_out, self.p_cap = i64([self.out.data_ptr() + int(a) for a in oo[:-1]]), i64(self.caps)
        self.max_blocks = lz.deflate_batch_max_blocks(sum(self.sizes), self.count, self.p, dict_bytes=nd)
        return self

    def call_dict(self):
        q = lambda t: C.c_void_p(t.data_ptr())
        st = self.ctx.L.mi_deflate_batch_dict_dev(self.ctx.h, C.byref(self.p), self.c, self.count, q(self.p_in), q(self.p_nb), self.max_blocks,
                                                  q(self.p_out), q(self.p_cap), q(self.nbytes), q(self.status), q(self.failed),
                                                  q(self.d_dict), self.d_dict.numel(), self.ctx.stream_ptr())
        assert st == 0, st

    def call(self):
        q = lambda t: C.c_void_p(t.data_ptr())
        st = self.ctx.L.mi_deflate_batch_dev(self.ctx.h, C.byref(self.p), self.c, self.count, q(self.p_in), q(self.p_nb), self.max_blocks,
                                             q(self.p_out), q(self.p_cap), q(self.nbytes), q(self.status), q(self.failed), self.ctx.stream_ptr())
        assert st == 0, st

    def check(self, host, offs):
        """a sanity check, not a test: every item MI_OK; the first, middle and last item read back by Python's gzip"""
        import gzip
        torch.cuda.synchronize()
        assert int(self.failed[0]) == 0
        nb = [int(v) for v in self.nbytes.cpu()]
        for k in (0, self.count // 2, self.count - 1):
            a = int(self.oo[k])
            assert gzip.decompress(self.out[a:a + nb[k]].cpu().numpy().tobytes()) == host[offs[k]:offs[k] + self.sizes[k]], k
        return sum(nb)


def layout(sizes, shift):
    """offsets of the items in one buffer: each at a 16-byte boundary + shift(k)"""
    at, offs = 0, []
    for k, n in enumerate(sizes):
        at = (at + 15) & ~15
        offs.append(at + shift(k))
        at += shift(k) + n
    return offs, at + 64


def place(ctx, pieces, offs, total):
    h = np.zeros(total, dtype=np.uint8)
    for pc, o in zip(pieces, offs):
        h[o:o + len(pc)] = np.frombuffer(pc, dtype=np.uint8)
    return torch.from_numpy(h).to(ctx.device), h.tobytes()


DICT_BYTES = 32768


def dict_child(a):
    """--dict in this process (under whatever MI_CODEC_LIB the parent set): prints its own JSON line"""
    import zlib
    ctx = lz.default_context()
    p = lz.params("deflate", parse=a.parse)
    x = synth.enwik_like(a.bytes, seed=a.seed).numpy().tobytes()
    zd, body = x[:DICT_BYTES], x[DICT_BYTES:]
    offs = list(range(0, len(body) - a.dict_item + 1, a.dict_item))
    sizes = [a.dict_item] * len(offs)
    n = sum(sizes)
    d_x = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to(ctx.device)
    res = dict(case=a.child, items=len(offs), item_bytes=a.dict_item, bytes=n, dict_bytes=len(zd), lib=os.environ.get("MI_CODEC_LIB", "tree"))

    def out_bytes(b, zdict):
        """a sanity check, not a test: every item MI_OK; the first, middle and last item read back by stock zlib"""
        torch.cuda.synchronize()
        assert int(b.failed[0]) == 0
        nb = [int(v) for v in b.nbytes.cpu()]
        for k in (0, b.count // 2, b.count - 1):
            s = b.out[int(b.oo[k]):int(b.oo[k]) + nb[k]].cpu().numpy().tobytes()
            d = zlib.decompressobj(15, zdict=zdict) if zdict else zlib.decompressobj(15)
            assert d.decompress(s) + d.flush() == body[offs[k]:offs[k] + sizes[k]], k
        return sum(nb)
    plain = Batch(ctx, p, "zlib", d_x, offs, sizes)
    plain.call()
    res["no_dict_out_bytes"] = out_bytes(plain, None)
    modes = [("no_dict", plain.call)]
    if a.child == "dict":
        d_dict = torch.from_numpy(np.frombuffer(zd, dtype=np.uint8).copy()).to(ctx.device)
        withd = Batch(ctx, p, "zlib", d_x, offs, sizes).with_dict(d_dict)
        withd.call_dict()
        res["dict_out_bytes"] = out_bytes(withd, zd)
        modes.append(("dict", withd.call_dict))
    for m, t in timed(modes, a.repeats).items():
        res[m] = summary(t, n)
    print(json.dumps(res))


def child(a):
    if a.child in ("dict", "dict-parent"):
        return dict_child(a)
    ctx = lz.default_context()
    p = lz.params("deflate", parse=a.parse)
    if a.child == "skewed":
        x = synth.enwik_like(max(a.skew_small * 4096, a.skew_big << 20), seed=a.seed).numpy().tobytes()
        pieces = [x[i * 4096:(i + 1) * 4096] for i in range(a.skew_small)]
        for k in range(a.skew_big):                               # the large items spread over the batch, none of them first
            pieces.insert((k + 1) * a.skew_small // (a.skew_big + 1) + k, x[:1 << 20][k:] + x[:k])
    else:
        x = synth.enwik_like(a.bytes, seed=a.seed).numpy().tobytes()
        pieces = [x[i:i + ITEM] for i in range(0, len(x), ITEM)]
    sizes = [len(pc) for pc in pieces]
    n = sum(sizes)
    res = dict(case=a.child, items=len(pieces), bytes=n)
    modes = []
    if a.child == "uniform":
        d_x = torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).to(ctx.device)
        b = Batch(ctx, p, "gzip", d_x, list(range(0, len(x), ITEM)), sizes)
        b.call()
        res["batch_out_bytes"] = b.check(x, list(range(0, len(x), ITEM)))
        one = lz.compress_z(d_x, p, "gzip", ctx=ctx)
        res["one_buffer_out_bytes"] = one.nbytes
        modes = [("one_buffer", lambda: lz.compress_z(d_x, p, "gzip", ctx=ctx)), ("batch", b.call)]
    elif a.child == "aligned":
        keep = []
        for tag, shift in (("aligned16", lambda k: 0), ("offset_1_15", lambda k: 1 + k % 15)):
            offs, total = layout(sizes, shift)
            buf, host = place(ctx, pieces, offs, total)
            b = Batch(ctx, p, "gzip", buf, offs, sizes)
            b.call()
            b.check(host, offs)
            keep.append(buf)
            modes.append((tag, b.call))
    else:
        offs, total = layout(sizes, lambda k: 0)
        buf, host = place(ctx, pieces, offs, total)
        b = Batch(ctx, p, "gzip", buf, offs, sizes)
        b.call()
        res["batch_out_bytes"] = b.check(host, offs)
        res["max_blocks"] = b.max_blocks
        modes = [("skewed", b.call)]
    for m, t in timed(modes, a.repeats).items():
        res[m] = summary(t, n)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--seed", type=int, default=12345)            # bench.py's corpus
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skew-small", type=int, default=10_000)
    ap.add_argument("--skew-big", type=int, default=4)
    ap.add_argument("--child", choices=("uniform", "aligned", "skewed", "dict", "dict-parent"))
    ap.add_argument("--dict", action="store_true")
    ap.add_argument("--dict-item", type=int, default=700)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parse", type=int, choices=(0, 1), default=0)   # the parse of every encode (include/mi_codec.h, mode Z)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = dict(device=torch.cuda.get_device_name(0), bytes=a.bytes, repeats=a.repeats, parse=a.parse)
    if a.dict:
        for case in ("dict", "dict-parent") if a.parent_lib else ("dict",):
            env = dict(os.environ, MI_CODEC_LIB=os.path.abspath(a.parent_lib)) if case == "dict-parent" else dict(os.environ)
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--bytes", str(a.bytes), "--repeats", str(a.repeats),
                                "--seed", str(a.seed), "--dict-item", str(a.dict_item), "--parse", str(a.parse)], capture_output=True, text=True, timeout=900, env=env)
            assert c.returncode == 0, c.stderr[-2000:]
            res[case.replace("-", "_")] = json.loads(c.stdout.strip().splitlines()[-1])
        res["dict_over_no_dict"] = round(res["dict"]["dict"]["ms_median"] / res["dict"]["no_dict"]["ms_median"], 4)
        if a.parent_lib:
            res["no_dict_over_parent"] = round(res["dict"]["no_dict"]["ms_median"] / res["dict_parent"]["no_dict"]["ms_median"], 4)
        print(json.dumps(res))
        return
    for case in ("uniform", "aligned", "skewed"):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--bytes", str(a.bytes), "--repeats", str(a.repeats),
                            "--seed", str(a.seed), "--skew-small", str(a.skew_small), "--skew-big", str(a.skew_big), "--parse", str(a.parse)],
                           capture_output=True, text=True, timeout=900)
        assert c.returncode == 0, c.stderr[-2000:]
        res[case] = json.loads(c.stdout.strip().splitlines()[-1])
    res["batch_over_one_buffer"] = round(res["uniform"]["batch"]["ms_median"] / res["uniform"]["one_buffer"]["ms_median"], 4)
    res["offset_over_aligned"] = round(res["aligned"]["offset_1_15"]["ms_median"] / res["aligned"]["aligned16"]["ms_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
