"""Batched inflate on the device (mi_inflate_batch_dev, mi_inflate_batch_size_dev, mi_inflate_batch): clean items of every
block type against stock zlib in the three containers, at every alignment, across the ring switch at 1 024 items, at and
below their capacity, by pointer into a BGZF stream, in both dispatch orders, queued back to back, from host buffers.

Then ONE batch that interleaves every item the decoder must refuse with clean ones, run only after the clean cases of
this file have passed: the refused items must be refused cleanly and leave their neighbours alone.

Every output sits between 64 guard bytes of a known pattern on both sides, and every run checks them.
"""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys
import textwrap
import zlib

import numpy as np
import pytest
import torch

import bgzf_cases as B
import inflate_batch_cases as K
import inflate_cases as ic
from compression_algorithms_amd import _lib, lz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, PATTERN = 64, 0xA5
CID = {"raw": 0, "zlib": 1, "gzip": 2}
_CLEAN = {"ran": 0, "failed": 0}


def clean(fn):
    """marks a clean case: the refusal batch looks at how these went"""
    @functools.wraps(fn)
    def run(*a, **k):
        _CLEAN["ran"] += 1
        try:
            return fn(*a, **k)
        except BaseException:
            _CLEAN["failed"] += 1
            raise
    return run


def _i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda") if len(v) else torch.zeros(0, dtype=torch.int64, device="cuda")


class Run:
    """one call of mi_inflate_batch_dev over `items` (bytes), each output between guards; in_res(i) / out_res(i): the
    residue of item i's input address mod 4 and of its output address mod 16"""

    def __init__(self, items, container, caps, verify=True, in_res=lambda i: 0, out_res=lambda i: 0, ctx=None, sync=True, launch=True):
        self.ctx = ctx or lz.default_context()
        self.container, self.verify = container, verify
        self.count = count = len(items)
        at, self.in_off = 0, []
        for i, b in enumerate(items):
            at = (at + 15) // 16 * 16 + in_res(i)
            self.in_off.append(at)
            at += len(b)
        pack = np.zeros(at + 16, dtype=np.uint8)
        for b, a in zip(items, self.in_off):
            pack[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.d_in = torch.from_numpy(pack).cuda()
        assert self.d_in.data_ptr() % 16 == 0
        at, self.out_off = 0, []
        for i, c in enumerate(caps):
            at = (at + GUARD + 15) // 16 * 16 + out_res(i)
            self.out_off.append(at)
            at += c
        self.caps = list(caps)
        self.d_out = torch.full((at + GUARD + 16,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.d_out.data_ptr() % 16 == 0
        self.p_in = _i64([self.d_in.data_ptr() + a for a in self.in_off])
        self.p_nb = _i64([len(b) for b in items])
        self.p_out = _i64([self.d_out.data_ptr() + a for a in self.out_off])
        self.p_cap = _i64(self.caps)
        self.nbytes = torch.full((count + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((count + 1,), -1, dtype=torch.int32, device="cuda")
        self.failed = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        if launch:
            self.launch()
            if sync:
                self.finish()

    def launch(self):
        """the C call alone: every device array exists already, nothing here touches the stream but the call itself"""
        p = lambda t: C.c_void_p(t.data_ptr())
        self.rc = self.ctx.L.mi_inflate_batch_dev(self.ctx.h, CID.get(self.container, self.container), self.count, p(self.p_in), p(self.p_nb),
                                                  p(self.p_out), p(self.p_cap), p(self.nbytes), p(self.status), p(self.failed),
                                                  0 if self.verify else lz.MI_INFLATE_NO_CHECKSUM, self.ctx.stream_ptr())
        return self

    def finish(self):
        assert self.rc == 0, _lib.STATUS.get(self.rc, self.rc)
        self.ctx.sync()
        o = self.d_out.cpu().numpy()
        self.nb = [int(v) for v in self.nbytes.cpu()]
        self.st = [int(v) for v in self.status.cpu()]
        assert self.nb[-1] == -1 and self.st[-1] == -1 and int(self.failed[1]) == -1, "the result arrays were written past `count`"
        self.nb, self.st, self.nfailed = self.nb[:-1], self.st[:-1], int(self.failed[0])
        inside = np.zeros(o.size, dtype=bool)
        for a, c in zip(self.out_off, self.caps):
            inside[a:a + c] = True
        assert bool((o[~inside] == PATTERN).all()), "bytes outside an item's [d_out, d_out + cap) were written"
        self.out = [o[a:a + (n if s == 0 else 0)].tobytes() for a, n, s in zip(self.out_off, self.nb, self.st)]
        return self


def _all_ok(r, want, what):
    assert r.st == [0] * len(want), (what, [(i, s) for i, s in enumerate(r.st) if s][:5])
    assert r.nb == [len(w) for w in want], what
    for i, w in enumerate(want):
        assert r.out[i] == w, (what, i)
    assert r.nfailed == 0, what


# ---- 1. all clean items, the three containers, across the ring switch -------------------------------------------------
@clean
@pytest.mark.parametrize("container", K.CONTAINERS)
def test_all_clean_items_in_one_call(container):
    items = K.clean_items(container)
    want = [w for _, _, w in items]
    _all_ok(Run([i for _, i, _ in items], container, [len(w) for w in want]), want, container)
    r = lz.inflate_batch([i for _, i, _ in items], container=container)           # the Python surface: size pass, then inflate
    assert r.failed == 0 and [int(v) for v in r.status.cpu()] == [0] * len(want) and [int(v) for v in r.out_bytes.cpu()] == [len(w) for w in want]
    assert [t.cpu().numpy().tobytes() for t in r.outputs] == want
    assert r.raise_for_status() is r
    # the same items among small ones, 1 024 and more in all: the 4 KiB ring decodes the far matches and the long items too
    pad = K.small_items(container, 1030)
    many = pad[:500] + items + pad[500:]
    _all_ok(Run([i for _, i, _ in many], container, [len(w) for _, _, w in many]), [w for _, _, w in many], (container, "padded"))


@clean
@pytest.mark.parametrize("count", (1, 2, 1023, 1024, 1025))
def test_counts_across_the_ring_switch(count):
    for container in K.CONTAINERS:
        items = K.small_items(container, count)
        want = [w for _, _, w in items]
        _all_ok(Run([i for _, i, _ in items], container, [len(w) for w in want]), want, (container, count))


# ---- 2. alignment -----------------------------------------------------------------------------------------------------
@clean
@pytest.mark.parametrize("container", K.CONTAINERS)
def test_every_input_and_output_alignment(container):
    base = K.clean_items(container)
    items = [base[i % len(base)] for i in range(max(len(base), 16) + 3)]
    want = [w for _, _, w in items]
    for shift in (0, 1):                                     # every item meets several residues over the two rounds
        r = Run([i for _, i, _ in items], container, [len(w) for w in want], in_res=lambda i: (i + shift) % 4,
                out_res=lambda i: (5 * i + shift) % 16)
        assert {(a + r.d_in.data_ptr()) % 4 for a in r.in_off} == {0, 1, 2, 3}
        assert {(a + r.d_out.data_ptr()) % 16 for a in r.out_off} == set(range(16))
        _all_ok(r, want, (container, shift))
    # the packed form of the Python surface: items back to back, unaligned by nature
    buf = b"".join(i for _, i, _ in items)
    offs = np.cumsum([0] + [len(i) for _, i, _ in items]).tolist()
    r = lz.inflate_batch((buf, offs), container=container)
    assert r.failed == 0 and [t.cpu().numpy().tobytes() for t in r.outputs] == want


# ---- 3. capacity ------------------------------------------------------------------------------------------------------
@clean
@pytest.mark.parametrize("container", ("raw", "gzip"))
def test_capacity(container):
    items = K.clean_items(container)
    streams, want = [i for _, i, _ in items], [w for _, _, w in items]
    n = [len(w) for w in want]
    # n - 100 cuts far_last_match and run inside a match of 258; n // 2 and n - 1 cut the 100 KB items wherever they fall
    for what, caps in (("n-1", [max(v - 1, 0) for v in n]), ("0", [0] * len(n)), ("n-100", [max(v - 100, 0) for v in n]),
                       ("n/2", [v // 2 for v in n])):
        r = Run(streams, container, caps, out_res=lambda i: i % 16)
        for i, (name, _, _) in enumerate(items):
            if n[i] <= caps[i]:
                assert (r.st[i], r.nb[i]) == (0, n[i]) and r.out[i] == want[i], (what, name)
            else:
                assert (r.st[i], r.nb[i]) == (K.CAPACITY, n[i]), (what, name, r.st[i], r.nb[i])
        assert r.nfailed == sum(1 for v, c in zip(n, caps) if v > c), what
    # with 1 024 items and more the 4 KiB ring instance flips into counting inside a match as well
    pad = K.small_items(container, 1030)
    many = pad[:300] + items + pad[300:]
    caps = [max(len(w) - 100, 0) for _, _, w in many]
    r = Run([i for _, i, _ in many], container, caps, out_res=lambda i: i % 16)
    for i, (name, _, w) in enumerate(many):
        if len(w) <= caps[i]:
            assert (r.st[i], r.nb[i]) == (0, len(w)) and r.out[i] == w, ("padded", name)
        else:
            assert (r.st[i], r.nb[i]) == (K.CAPACITY, len(w)), ("padded", name, r.st[i], r.nb[i])
    assert r.nfailed == sum(1 for (_, _, w), c in zip(many, caps) if len(w) > c)


# ---- 4. size pass -----------------------------------------------------------------------------------------------------
@clean
@pytest.mark.parametrize("container", K.CONTAINERS)
def test_size_pass_equals_zlib(container):
    items = K.clean_items(container)
    sizes, status = lz.inflate_batch_sizes([i for _, i, _ in items], container=container)
    assert [int(v) for v in sizes.cpu()] == [len(zlib.decompress(i, K.WBITS[container])) for _, i, _ in items]
    assert [int(v) for v in status.cpu()] == [0] * len(items)
    many = K.small_items(container, 1500)
    sizes, status = lz.inflate_batch_sizes([i for _, i, _ in many], container=container)
    assert [int(v) for v in sizes.cpu()] == [len(w) for _, _, w in many] and not bool(status.any())


# ---- 6. BGZF cross-check ----------------------------------------------------------------------------------------------
@clean
def test_bgzf_payloads_by_pointer_and_members_as_gzip_items():
    data = ic.mix(300_000)
    s = lz.compress_bgzf(data)
    stream = s.data[: s.nbytes]
    want = lz.decompress_bgzf(stream).cpu().numpy().tobytes()
    assert want == data
    so, oo = B.walk(stream.cpu().numpy().tobytes())
    payloads = [stream[so[i] + 18: so[i + 1] - 8] for i in range(len(so) - 1)]      # views: pointers into the stream itself
    assert all(p.data_ptr() == stream.data_ptr() + so[i] + 18 for i, p in enumerate(payloads))
    r = lz.inflate_batch(payloads, container="raw")
    assert r.failed == 0 and b"".join(t.cpu().numpy().tobytes() for t in r.outputs) == want
    r = lz.inflate_batch((stream, so), container="gzip")
    assert r.failed == 0 and b"".join(t.cpu().numpy().tobytes() for t in r.outputs) == want
    assert [int(v) for v in r.out_bytes.cpu()] == [b - a for a, b in zip(oo, oo[1:])]


# ---- 7. skew and order ------------------------------------------------------------------------------------------------
def _skew_digest():
    items = K.skewed()
    r = lz.inflate_batch([i for i, _ in items], container="raw")
    h = hashlib.sha256()
    for t in r.outputs:
        h.update(t.cpu().numpy().tobytes())
    h.update(r.status.cpu().numpy().tobytes() + r.out_bytes.cpu().numpy().tobytes())
    return h.hexdigest(), r


@clean
def test_skewed_batch_is_the_same_in_both_orders():
    items = K.skewed()
    digest, r = _skew_digest()
    assert r.failed == 0 and [t.cpu().numpy().tobytes() for t in r.outputs] == [w for _, w in items]
    # the switch is read at call time: one child runs the identity order and then the size-class order
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    body = ("import os\nimport test_inflate_batch_gpu as t\n"
            "for v in ('0', '1'):\n    os.environ['MI_INFLATE_BATCH_ORDER'] = v\n    print('digest', v, t._skew_digest()[0])\n")
    c = subprocess.run([sys.executable, "-c", body], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    assert ("digest 0 " + digest) in c.stdout, "the identity order gives other outputs or statuses"
    assert ("digest 1 " + digest) in c.stdout, "the size-class order gives other outputs or statuses"


# ---- 8. asynchrony ----------------------------------------------------------------------------------------------------
@clean
def test_two_batches_back_to_back_on_one_stream(monkeypatch):
    """Both batches are prepared first (every upload done and waited for), then the two C calls follow each other with
    nothing in between, then ONE mi_sync.  The size-class order is forced on, so both calls build `order[]` in the one
    workspace of the context; the second batch is the smaller one, so the workspace does not grow between them (growing
    would synchronise)."""
    monkeypatch.setenv("MI_INFLATE_BATCH_ORDER", "1")
    a, b = K.small_items("zlib", 1100), K.clean_items("gzip")
    warm = Run([i for _, i, _ in a], "zlib", [len(w) for _, _, w in a])            # the workspace has its size now
    ra = Run([i for _, i, _ in a], "zlib", [len(w) for _, _, w in a], launch=False)
    rb = Run([i for _, i, _ in b], "gzip", [len(w) for _, _, w in b], launch=False)
    torch.cuda.synchronize()
    ra.launch()
    rb.launch()                                                                    # no host synchronisation in between
    ra.finish()                                                                    # mi_sync, once: the second finish finds the stream idle
    rb.finish()
    _all_ok(ra, [w for _, _, w in a], "first")
    _all_ok(rb, [w for _, _, w in b], "second")


# ---- 9. host form -----------------------------------------------------------------------------------------------------
@clean
@pytest.mark.parametrize("container", K.CONTAINERS)
def test_host_form_equals_zlib(container):
    items = K.clean_items(container)
    outs, status = lz.inflate_batch_host([i for _, i, _ in items], container=container)
    assert status == [0] * len(items) and outs == [zlib.decompress(i, K.WBITS[container]) for _, i, _ in items]


def test_host_form_with_mixed_verdicts():
    """mi_inflate_batch by hand (lz.inflate_batch_host sizes its own outputs and cannot express a short capacity): good, a
    byte short, truncated, NULL with a size, good — the call is MI_OK, every item has its own verdict, only the good ones are
    written; then the size-only call on the same five"""
    ctx = lz.default_context()
    _, item, want = next(c for c in K.clean_items("raw") if c[0] == "text_2k")
    n = len(want)
    streams = [item, item, item[:-3], item, item]
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in streams]
    h_in = (C.c_void_p * 5)(*[a.ctypes.data for a in arrs])
    h_in[3] = None
    h_nb = (C.c_uint64 * 5)(*[a.size for a in arrs])
    caps = [n, n - 1, n, n, n]
    outs = [np.full(n, PATTERN, dtype=np.uint8) for _ in range(5)]
    h_out = (C.c_void_p * 5)(*[o.ctypes.data for o in outs])
    h_cap = (C.c_uint64 * 5)(*caps)
    sizes, status = (C.c_uint64 * 5)(), (C.c_uint32 * 5)()
    assert ctx.L.mi_inflate_batch(ctx.h, CID["raw"], 5, h_in, h_nb, h_out, h_cap, sizes, status, 0) == 0
    assert list(status) == [0, K.CAPACITY, K.CORRUPT, K.ARG, 0]
    assert sizes[0] == n and sizes[1] == n and sizes[4] == n
    assert outs[0].tobytes() == want == zlib.decompress(item, -15) and outs[4].tobytes() == want
    assert bool((outs[1] == PATTERN).all()), "an item that did not fit was written"
    sizes, status = (C.c_uint64 * 5)(), (C.c_uint32 * 5)()
    assert ctx.L.mi_inflate_batch(ctx.h, CID["raw"], 5, h_in, h_nb, None, None, sizes, status, 0) == 0
    assert list(status) == [0, 0, K.CORRUPT, K.ARG, 0]
    assert sizes[0] == n and sizes[1] == n and sizes[4] == n


# ---- 10. arguments ----------------------------------------------------------------------------------------------------
@clean
def test_arguments():
    ctx = lz.default_context()
    L, s = ctx.L, ctx.stream_ptr()
    one = torch.zeros(4, dtype=torch.int64, device="cuda")
    p = C.c_void_p(one.data_ptr())
    assert L.mi_inflate_batch_dev(ctx.h, 0, 0, None, None, None, None, None, None, None, 0, s) == 0          # count == 0: nothing to do
    assert L.mi_inflate_batch_size_dev(ctx.h, 2, 0, None, None, None, None, None, 0, s) == 0
    assert L.mi_inflate_batch_dev(ctx.h, 3, 1, p, p, p, p, p, p, None, 0, s) == 1                             # unknown container
    assert L.mi_inflate_batch_dev(ctx.h, 0, 1, p, p, p, p, p, p, None, 2, s) == 1                             # unknown flag
    assert L.mi_inflate_batch_dev(ctx.h, 0, 1, None, p, p, p, p, p, None, 0, s) == 1                          # a NULL array
    assert L.mi_inflate_batch_dev(ctx.h, 0, 1 << 31, p, p, p, p, p, p, None, 0, s) == 1                       # count > 2^31 - 1
    # per item: sizes above 2^31 - 1 and NULL pointers with a size, between two good items; arrays built by hand
    good = K.clean_items("raw")[1]
    r = Run([good[1]] * 5, "raw", [len(good[2])] * 5, sync=False)
    ctx.sync()
    r.p_nb[1] = 1 << 31
    r.p_cap[2] = (1 << 31) + 5
    r.p_in[3] = 0
    q = lambda t: C.c_void_p(t.data_ptr())
    r.rc = L.mi_inflate_batch_dev(ctx.h, 0, 5, q(r.p_in), q(r.p_nb), q(r.p_out), q(r.p_cap), q(r.nbytes), q(r.status), q(r.failed), 0, s)
    r.caps[2] = len(good[2])                                          # (what the guard check may treat as item 2's own bytes)
    r.finish()
    assert r.st == [0, 1, 1, 1, 0] and r.nb == [len(good[2]), 0, 0, 0, len(good[2])] and r.nfailed == 3
    assert r.out[0] == good[2] and r.out[4] == good[2]
    sizes, status = lz.inflate_batch_sizes([good[1]], container="raw")
    assert int(sizes[0]) == len(good[2]) and int(status[0]) == 0


# ---- 5. isolation: the refusal batch, once, after the clean cases ------------------------------------------------------
def _need_clean_cases():
    if _CLEAN["failed"]:
        pytest.fail("a clean case of this file failed: the refusal batch is not run on a decoder that is wrong on good items")
    if not _CLEAN["ran"]:                                            # selected alone: one clean batch first
        test_all_clean_items_in_one_call("gzip")


def _payload(item, container):
    """what the DEFLATE data of an item whose trailer is wrong stands for"""
    return zlib.decompressobj(-15).decompress(item[{"zlib": 2, "gzip": 10}[container]:])


@pytest.mark.parametrize("container", K.CONTAINERS)
def test_refused_items_do_not_touch_their_neighbours(container):
    _need_clean_cases()
    bad = [r for r in K.refusals() if r[1] == container]
    assert bad
    good = K.small_items(container, len(bad) + 1)
    items, want, expect, names = [], [], [], []
    for k, (name, _, item, status) in enumerate(bad):               # clean, refused, clean, refused, ..., clean
        items += [good[k][1], item]
        want += [good[k][2], None]
        expect += [0, status]
        names += ["clean", name]
    items.append(good[-1][1]); want.append(good[-1][2]); expect.append(0); names.append("clean")
    caps = [len(w) if w is not None else 200_000 for w in want]
    r = Run(items, container, caps, in_res=lambda i: i % 4, out_res=lambda i: (3 * i) % 16)
    assert r.st == expect, [(n, s, e) for n, s, e in zip(names, r.st, expect) if s != e]
    assert r.nfailed == len(bad)
    for i, w in enumerate(want):
        assert r.nb[i] == (len(w) if w is not None else 0) and (w is None or r.out[i] == w), names[i]
    # verify=False lets exactly the checksum refusals through, with the right bytes — not the ISIZE ones
    r = Run(items, container, caps, verify=False)
    lax = [0 if n in K.CHECKSUM else e for n, e in zip(names, expect)]
    assert r.st == lax, [(n, s, e) for n, s, e in zip(names, r.st, lax) if s != e]
    assert r.nfailed == sum(1 for e in lax if e)
    for i, n in enumerate(names):
        if n in K.CHECKSUM:
            assert r.out[i] == _payload(items[i], container), n
        elif lax[i] == 0:
            assert r.out[i] == want[i]
    # the size pass gives the verdicts of the full call, except that it cannot see a checksum mismatch
    sizes, status = lz.inflate_batch_sizes(items, container=container)
    assert [int(v) for v in status.cpu()] == lax
    assert [int(v) for v in sizes.cpu()] == [len(o) if s == 0 else 0 for o, s in zip(r.out, lax)]
    # and the Python surface reports them
    b = lz.inflate_batch(items, container=container)
    assert b.failed == len(bad) and [int(v) for v in b.status.cpu()] == expect
    with pytest.raises(_lib.MiError) as e:
        b.raise_for_status()
    assert e.value.status == K.CORRUPT
