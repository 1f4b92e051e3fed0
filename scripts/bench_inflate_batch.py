"""Batched inflate (mi_inflate_batch_dev) on bench.py's corpus: GB/s of inflated bytes, warm, HIP events, the median of
alternating runs in one process, with min and max so that the run-to-run spread can be read off.  Three cases:

  (a) uniform   the corpus cut into 65 280-byte pieces, each compressed by stock zlib (level 6) into a raw / zlib / gzip item,
                the items packed back to back (unaligned); the size pass on the gzip items as well
  (b) bgzf      the raw-DEFLATE payloads of a compress_bgzf stream as raw items BY POINTER into that stream, and
                mi_bgzf_inflate_dev on the same stream in the same run: the yardstick — the same per-member work
  (c) skewed    thousands of 4 KiB items plus a handful of 1 MiB items, in a child process each with MI_INFLATE_BATCH_ORDER
                =1 and =0 (the switch is read at call time; a child keeps the two settings from sharing anything)

One JSON line.

    python scripts/bench_inflate_batch.py [--bytes 100000000] [--repeats 7]

--dict: the preset-dictionary variant INSTEAD of the three cases.  The corpus behind its first 32 768 bytes (the dictionary)
cut into --dict-item byte items, each compressed by stock zlib (level 6, zlib container) without and with zdict=: the
former through mi_inflate_batch_dev, the latter through mi_inflate_batch_dict_dev, alternating in one process; and, with
--parent-lib PATH (a libmi_codec.so built from the parent commit, loaded through MI_CODEC_LIB in a child of its own),
mi_inflate_batch_dev of that library on the same items: `no_dict_over_parent` is the ratio of the medians, to be read against
the two spreads.

    python scripts/bench_inflate_batch.py --dict [--dict-item 700] [--repeats 3] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compression_algorithms_amd import lz, synth  # noqa: E402

PIECE = 65280


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


def frame(raw, data, container):
    if container == "raw":
        return raw
    if container == "zlib":
        return b"\x78\x9c" + raw + zlib.adler32(data).to_bytes(4, "big")
    return bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF]) + raw + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


class Batch:
    """the device arrays of one batch; call() launches it on the current stream (asynchronous)"""

    def __init__(self, ctx, container, ptrs, sizes, out_sizes):
        dev = ctx.device
        self.ctx, self.c, self.count = ctx, lz.CONTAINERS[container], len(ptrs)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        offs = np.concatenate([[0], np.cumsum([(n + 15) & ~15 for n in out_sizes])])
        self.out = torch.empty(int(offs[-1]) + 16, dtype=torch.uint8, device=dev)
        self.offs, self.out_sizes = offs, out_sizes
        self.p_in, self.p_nb = i64(ptrs), i64(sizes)
        self.p_out, self.p_cap = i64([self.out.data_ptr() + int(a) for a in offs[:-1]]), i64(out_sizes)
        self.nbytes = torch.zeros(self.count, dtype=torch.int64, device=dev)
        self.status = torch.zeros(self.count, dtype=torch.int32, device=dev)
        self.failed = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(self, flags=0):
        p = lambda t: C.c_void_p(t.data_ptr())
        st = self.ctx.L.mi_inflate_batch_dev(self.ctx.h, self.c, self.count, p(self.p_in), p(self.p_nb), p(self.p_out), p(self.p_cap),
                                             p(self.nbytes), p(self.status), p(self.failed), flags, self.ctx.stream_ptr())
        assert st == 0, st

    def call_dict(self, d_dict):
        p = lambda t: C.c_void_p(t.data_ptr())
        st = self.ctx.L.mi_inflate_batch_dict_dev(self.ctx.h, self.c, self.count, p(self.p_in), p(self.p_nb), p(self.p_out), p(self.p_cap),
                                                  p(self.nbytes), p(self.status), p(self.failed), p(d_dict), d_dict.numel(), 0,
                                                  self.ctx.stream_ptr())
        assert st == 0, st

    def sizes(self):
        p = lambda t: C.c_void_p(t.data_ptr())
        st = self.ctx.L.mi_inflate_batch_size_dev(self.ctx.h, self.c, self.count, p(self.p_in), p(self.p_nb), p(self.nbytes), p(self.status),
                                                  p(self.failed), 0, self.ctx.stream_ptr())
        assert st == 0, st

    def check(self, want):
        """after a call: every item MI_OK with its expected length, and — a sanity check, not a test — the first, middle and
        last item byte for byte against `want` (a uint8 device tensor of the items back to back)"""
        torch.cuda.synchronize()
        assert int(self.failed[0]) == 0 and [int(v) for v in self.nbytes.cpu()] == list(self.out_sizes)
        for k in (0, self.count // 2, self.count - 1):
            a, n = int(self.offs[k]), self.out_sizes[k]
            at = sum(self.out_sizes[:k])
            assert torch.equal(self.out[a:a + n], want[at:at + n]), k


def packed(ctx, items):
    buf = torch.from_numpy(np.frombuffer(b"".join(items), dtype=np.uint8).copy()).to(ctx.device)
    offs = np.concatenate([[0], np.cumsum([len(i) for i in items])])
    return buf, [buf.data_ptr() + int(a) for a in offs[:-1]], [len(i) for i in items]


def skewed_child(a):
    """case (c) in this process, under whatever MI_INFLATE_BATCH_ORDER the parent set: prints its own JSON line"""
    ctx = lz.default_context()
    x = synth.enwik_like(max(a.skew_small * 4096, a.skew_big << 20), seed=a.seed).numpy().tobytes()
    small = [x[i * 4096:(i + 1) * 4096] for i in range(a.skew_small)]
    big = [x[:1 << 20][k:] + x[:k] for k in range(a.skew_big)]
    data = list(small)
    for k, b in enumerate(big):                                # the large items spread over the batch, none of them first
        data.insert((k + 1) * len(small) // (len(big) + 1) + k, b)
    items = [deflate(d) for d in data]
    buf, ptrs, sizes = packed(ctx, items)
    b = Batch(ctx, "raw", ptrs, sizes, [len(d) for d in data])
    b.call()
    b.check(torch.from_numpy(np.frombuffer(b"".join(data), dtype=np.uint8).copy()).to(ctx.device))
    # and a uniform batch under the same setting: what the three ordering kernels cost where they cannot help
    y = synth.enwik_like(a.child_uniform, seed=a.seed + 1).numpy().tobytes()
    pieces = [y[i:i + PIECE] for i in range(0, len(y), PIECE)]
    ubuf, uptrs, usizes = packed(ctx, [deflate(p) for p in pieces])
    u = Batch(ctx, "raw", uptrs, usizes, [len(p) for p in pieces])
    u.call()
    u.check(torch.from_numpy(np.frombuffer(y, dtype=np.uint8).copy()).to(ctx.device))
    t = timed([("skewed", b.call), ("uniform", u.call)], a.repeats)
    print(json.dumps(dict(summary(t["skewed"], sum(len(d) for d in data)), items=len(items), uniform=summary(t["uniform"], len(y)),
                          uniform_items=len(pieces), order=os.environ.get("MI_INFLATE_BATCH_ORDER", "unset"))))


DICT_BYTES = 32768


def dict_child(a):
    """--dict in this process (under whatever MI_CODEC_LIB the parent set): prints its own JSON line"""
    ctx = lz.default_context()
    x = synth.enwik_like(a.bytes, seed=a.seed).numpy().tobytes()
    zd, body = x[:DICT_BYTES], x[DICT_BYTES:]
    pieces = [body[i:i + a.dict_item] for i in range(0, len(body) - a.dict_item + 1, a.dict_item)]
    n = sum(len(p) for p in pieces)
    want = torch.from_numpy(np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()).to(ctx.device)
    res = dict(case=a.dict_child, items=len(pieces), item_bytes=a.dict_item, bytes=n, dict_bytes=len(zd), lib=os.environ.get("MI_CODEC_LIB", "tree"))

    def stock(p, zdict):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, zdict) if zdict else zlib.compressobj(6, zlib.DEFLATED, 15)
        return c.compress(p) + c.flush()
    items = [stock(p, None) for p in pieces]
    res["no_dict_in_bytes"] = sum(len(i) for i in items)
    buf, ptrs, sizes = packed(ctx, items)
    plain = Batch(ctx, "zlib", ptrs, sizes, [len(p) for p in pieces])
    plain.call()
    plain.check(want)
    modes = [("no_dict", plain.call)]
    if a.dict_child == "dict":
        d_dict = torch.from_numpy(np.frombuffer(zd, dtype=np.uint8).copy()).to(ctx.device)
        ditems = [stock(p, zd) for p in pieces]
        res["dict_in_bytes"] = sum(len(i) for i in ditems)
        dbuf, dptrs, dsizes = packed(ctx, ditems)
        withd = Batch(ctx, "zlib", dptrs, dsizes, [len(p) for p in pieces])
        withd.call_dict(d_dict)
        withd.check(want)
        modes.append(("dict", lambda: withd.call_dict(d_dict)))
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
    ap.add_argument("--child-uniform", type=int, default=64_000_000)
    ap.add_argument("--skewed-child", action="store_true")
    ap.add_argument("--dict", action="store_true")
    ap.add_argument("--dict-item", type=int, default=700)
    ap.add_argument("--dict-child", choices=("dict", "dict-parent"))
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.skewed_child:
        return skewed_child(a)
    if a.dict_child:
        return dict_child(a)
    if a.dict:
        res = dict(device=torch.cuda.get_device_name(0), bytes=a.bytes, repeats=a.repeats)
        for case in ("dict", "dict-parent") if a.parent_lib else ("dict",):
            env = dict(os.environ, MI_CODEC_LIB=os.path.abspath(a.parent_lib)) if case == "dict-parent" else dict(os.environ)
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--dict-child", case, "--bytes", str(a.bytes), "--repeats", str(a.repeats),
                                "--seed", str(a.seed), "--dict-item", str(a.dict_item)], capture_output=True, text=True, timeout=900, env=env)
            assert c.returncode == 0, c.stderr[-2000:]
            res[case.replace("-", "_")] = json.loads(c.stdout.strip().splitlines()[-1])
        res["dict_over_no_dict"] = round(res["dict"]["dict"]["ms_median"] / res["dict"]["no_dict"]["ms_median"], 4)
        if a.parent_lib:
            res["no_dict_over_parent"] = round(res["dict"]["no_dict"]["ms_median"] / res["dict_parent"]["no_dict"]["ms_median"], 4)
        print(json.dumps(res))
        return
    dev = torch.device("cuda", 0)
    ctx = lz.default_context()
    x = synth.enwik_like(a.bytes, seed=a.seed, device=dev)
    n = x.numel()
    res = dict(device=torch.cuda.get_device_name(0), bytes=n, repeats=a.repeats)
    # ---- (a) uniform: stock zlib items, packed back to back
    host = x.cpu().numpy().tobytes()
    pieces = [host[i:i + PIECE] for i in range(0, n, PIECE)]
    raws = [deflate(p) for p in pieces]
    res["uniform_items"] = len(pieces)
    modes, keep = [], []
    for container in ("raw", "zlib", "gzip"):
        buf, ptrs, sizes = packed(ctx, [frame(r, p, container) for r, p in zip(raws, pieces)])
        b = Batch(ctx, container, ptrs, sizes, [len(p) for p in pieces])
        b.call()
        b.check(x)
        keep.append((buf, b))
        modes.append((f"uniform_{container}", b.call))
        if container == "gzip":
            b.sizes()
            torch.cuda.synchronize()
            assert int(b.failed[0]) == 0 and [int(v) for v in b.nbytes.cpu()] == [len(p) for p in pieces]
            modes.append(("uniform_gzip_no_checksum", lambda b=b: b.call(lz.MI_INFLATE_NO_CHECKSUM)))
            modes.append(("uniform_gzip_size_pass", b.sizes))
    for m, t in timed(modes, a.repeats).items():
        res[m] = summary(t, n)
    del keep, modes
    # ---- (b) BGZF payloads by pointer, against mi_bgzf_inflate_dev on the same stream in the same run
    s = lz.compress_bgzf(x)
    stream = s.data[: s.nbytes]
    idx = lz.bgzf_index(stream)
    so = [int(v) for v in idx[0].cpu()]
    oo = [int(v) for v in idx[1].cpu()]
    members = len(so) - 1
    base = stream.data_ptr()
    b = Batch(ctx, "raw", [base + so[i] + 18 for i in range(members)], [so[i + 1] - 8 - so[i] - 18 for i in range(members)],
              [oo[i + 1] - oo[i] for i in range(members)])
    g = Batch(ctx, "gzip", [base + so[i] for i in range(members)], [so[i + 1] - so[i] for i in range(members)],
              [oo[i + 1] - oo[i] for i in range(members)])
    y = torch.empty(n, dtype=torch.uint8, device=dev)

    def bgzf(flags):
        def f():
            st = ctx.L.mi_bgzf_inflate_dev(ctx.h, C.c_void_p(base), stream.numel(), C.c_void_p(idx.pairs.data_ptr()), 0, members,
                                           C.c_void_p(y.data_ptr()), n, flags, ctx.stream_ptr())
            assert st == 0, st
        return f

    for bb in (b, g):
        bb.call()
        bb.check(x)
    bgzf(0)()
    assert torch.equal(y, x)
    nock = lz.MI_INFLATE_NO_CHECKSUM
    t = timed([("bgzf_inflate_dev_no_checksum", bgzf(nock)), ("batch_raw_payloads", b.call), ("bgzf_inflate_dev", bgzf(0)),
               ("batch_gzip_members", g.call)], a.repeats)
    for m, v in t.items():
        res[m] = summary(v, n)
    res["members"] = members
    # raw items carry no checksum: the like-for-like pairs are raw against no-checksum, gzip members against the checked call
    res["batch_raw_over_bgzf_no_checksum"] = round(res["batch_raw_payloads"]["ms_median"] / res["bgzf_inflate_dev_no_checksum"]["ms_median"], 4)
    res["batch_gzip_over_bgzf"] = round(res["batch_gzip_members"]["ms_median"] / res["bgzf_inflate_dev"]["ms_median"], 4)
    # ---- (c) skewed, one child per setting
    for tag, val in (("skewed_ordered", "1"), ("skewed_identity", "0")):
        env = dict(os.environ, MI_INFLATE_BATCH_ORDER=val)
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--skewed-child", "--repeats", str(a.repeats), "--seed", str(a.seed),
                            "--skew-small", str(a.skew_small), "--skew-big", str(a.skew_big), "--child-uniform", str(a.child_uniform)], env=env, capture_output=True, text=True,
                           timeout=600)
        assert c.returncode == 0, c.stderr[-2000:]
        res[tag] = json.loads(c.stdout.strip().splitlines()[-1])
    res["skewed_ordered_over_identity"] = round(res["skewed_ordered"]["ms_median"] / res["skewed_identity"]["ms_median"], 4)
    res["uniform_ordered_over_identity"] = round(res["skewed_ordered"]["uniform"]["ms_median"] / res["skewed_identity"]["uniform"]["ms_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
