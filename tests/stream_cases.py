"""The "late input / early poison" harness of the stream-order tests (a helper module, not a conftest), with the input
recipes and the expected-value builders it needs.  tests/test_stream_order_gpu.py runs it on the device;
tests/test_stream_cases_cpu.py checks on the CPU what it takes for granted.

include/mi_codec.h promises that the device entry points are ordered on the caller's stream and on nothing else.  On HIP's
legacy default stream, which waits for every blocking stream and every synchronous copy, and with inputs that were complete
long before the call and outputs read after a device-wide synchronisation, a missing dependency cannot show.  Here every
call runs on a non-blocking stream S (torch.cuda.Stream()), and one case is, with NO host synchronisation between the steps:

  1. late input    the payload buffers hold POISON; S gets a delay (GPU work of a calibrated duration), then the
                   device-to-device copies that put the real bytes there.  Only data bytes arrive late: whatever a kernel uses
                   as an address, count, offset, capacity or length (pointer / size arrays, block tables, the BGZF index, the
                   ranges) is valid from the start, so that no case can fault even where the library is wrong.
  2. the call      on S, through the C ABI.
  3. early poison  at once, on S: every output is copied into a tensor made beforehand, then inputs AND outputs are
                   overwritten with poison.
  4. one mi_sync, and the copies are compared with values that do not come from the code under test.

A fork that does not wait for S reads poison; a join that misses an internal stream lets step 3 into that stream's reads or
leaves the copy incomplete.  For an asynchronous entry point the case also asserts that the event recorded right behind the
late copy has not happened when the call returns (the data really was late); the delay is four times the measured host time
of one warm call, at least 5 ms and at most 250 ms, and is quadrupled once before the case fails as vacuous.

Poison: for uncompressed inputs a fixed pseudo-random buffer that differs from the data in every 64-byte line (any bytes are
a valid input to an encoder); for compressed inputs zero bytes (refused by every container's header check, and a valid —
wrong — stream of literal tokens for the LZ decoders); 0x5A for outputs, except the u64 tables of offsets, sizes and counts,
whose every entry is 64: the library reads some of them back as the place to write to (Case.out).
"""
import ctypes as C
import functools
import math
import time
import zlib

import numpy as np

from compression_algorithms_amd import synth

OUT_POISON = 0x5A
TABLE_POISON = 64                                              # every u64 of an offset / size / count output: 64 bits, 8 bytes
GUARD = 64
DELAY_FLOOR_MS, DELAY_CEIL_MS = 5.0, 250.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def as_np(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def make(recipe):
    """("text" | a synth family, n, seed) -> read-only uint8 array"""
    kind, n, seed = recipe
    a = synth.enwik_like(n, seed=seed).numpy() if kind == "text" else synth.family(kind, seed, n)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


def data_poison(data):
    """pseudo-random bytes of the same length that differ from `data` in every 64-byte line"""
    d = as_np(data)
    p = np.random.default_rng(0x5A5A).integers(0, 256, d.size, dtype=np.uint8)
    at = np.arange(0, d.size, 64)
    p[at] = d[at] ^ 0xFF
    return p


def zero_poison(stream):
    return np.zeros(len(stream), dtype=np.uint8)


SOLO = ("text", 3 * 65536 + 777, 61)                           # one batch: the "solo" split
PIPE = ("text", 13 * 65536 + 4321, 62)                         # 14 blocks: five batches of three
PIPE_BGZF = ("text", 13 * 65280 + 4321, 63)
SHORT = ("text", 2 * 65536 + 99, 64)                           # 3 blocks
SOLO_PAGES = ("pages", 3 * 65536 + 777, 5)                     # one batch whose blocks fall back: the chain on fb has work
PAGES = ("pages", 64 * 65536, 5)                               # blocks that fall back (giant clusters)
FB_A = ("text", 40 * 65536 + 11, 65)                           # three batches of 16
FB_B = ("text", 35 * 65536 + 3, 66)
WIDE = ("text", 3 * 262144 + 777, 67)                          # four blocks of 256 KiB
WHOLE = ("text", 300_000, 68)
OLD = ("text", 20_000, 69)

# (name, kind, recipe, block, wbits, container): every encoder case of the GPU file; kinds below
ENCODER_CASES = [
    ("solo-tokens", "T", SOLO, 65536, None, None), ("solo-lz77-w14", "L", SOLO, 65536, 14, None),
    ("solo-lz77-w16", "L", SOLO, 65536, 16, None), ("solo-h", "H", SOLO, 65536, None, None),
    ("solo-z-gzip", "Z", SOLO, 65536, None, "gzip"), ("solo-bgzf", "BGZF", ("text", 3 * 65280 + 777, 61), 65280, None, None),
    ("solo-find", "FIND", SOLO, 65536, None, None), ("solo-pages-tokens", "T", SOLO_PAGES, 65536, None, None),
    ("pipe-tokens", "T", PIPE, 65536, None, None), ("pipe-h", "H", PIPE, 65536, None, None),
    ("pipe-z-zlib", "Z", PIPE, 65536, None, "zlib"), ("pipe-bgzf", "BGZF", PIPE_BGZF, 65280, None, None),
    ("short-z-raw", "Z", SHORT, 65536, None, "raw"),
    ("pages-tokens", "T", PAGES, 65536, None, None), ("fb-a-tokens", "T", FB_A, 65536, None, None),
    ("fb-b-h", "H", FB_B, 65536, None, None),
    ("wide-lz77-w16", "L", WIDE, 262144, 16, None), ("wide-lz77-w14", "L", ("text", 3 * 131072 + 777, 70), 131072, 14, None),
    ("huffman", "HUFF", WHOLE, 0, None, None), ("fse", "FSE", WHOLE, 65536, None, None),
    ("crc32", "CRC", WHOLE, 0, None, None), ("adler32", "ADLER", WHOLE, 0, None, None), ("lz77-old", "OLD", OLD, 0, 14, None),
]


# ---- expected values: the CPU oracle, zlib, numpy — never the library ---------------------------------------------------------
def _concat_bits(blocks):
    """[(stream bytes, bits)] -> (bit-contiguous bytes with zero pad bits, table of bit offsets)"""
    total = sum(nb for _, nb in blocks)
    bits = np.zeros(total, dtype=np.uint8)
    at, table = 0, [0]
    for s, nb in blocks:
        bits[at:at + nb] = np.unpackbits(s, bitorder="little")[:nb]
        at += nb
        table.append(at)
    return np.packbits(bits, bitorder="little").tobytes(), table


def expected_of(kind, data, block, wbits=None, container=None):
    """what the entry point of `kind` must write for `data` -> dict of the outputs the cases compare"""
    from oracle import orc
    data = as_np(data)
    if kind == "T":
        tok, sizes = orc.deflate_stream(data, block, True)
        return dict(out=tok.tobytes(), bits=[0] + [int(v) * 8 for v in np.cumsum(sizes)])
    if kind == "L":
        out, table = _concat_bits([orc.lz77_encode(data[a:a + block].tobytes(), wbits, 4, wbits + 6) for a in range(0, len(data), block)])
        return dict(out=out, bits=table)
    if kind == "H":
        d = orc.Deflate(block)
        recs = []
        for a in range(0, len(data), block):
            d.fresh()
            recs.append(orc.defh_encode_block(d.block_encode(data[a:a + block])).tobytes())
        return dict(out=b"".join(recs), bits=[0] + [int(v) * 8 for v in np.cumsum([len(r) for r in recs])])
    if kind == "Z":
        out, table = orc.defz_stream(data, block, container)
        return dict(out=bytes(out), bits=table, nbytes=len(out))
    if kind == "BGZF":
        import bgzf_cases
        out, table = bgzf_cases.expected_bgzf(data.tobytes(), block)
        return dict(out=out, bits=table, nbytes=len(out))
    if kind == "FIND":
        cand = np.concatenate([orc.find_all(data[a:a + block], 15, 20, True) for a in range(0, len(data), block)])
        return dict(cand=np.where(cand == 0xFFFFFFFF, 0xFFFF, cand).astype(np.uint16).tobytes())
    if kind == "HUFF":
        o = orc.huff_encode(data)
        return dict(words=o["words"].tobytes(), bits=o["bits"], codes=o["codes"].tobytes(), lens=o["lens"].tobytes(),
                    hist=np.bincount(data, minlength=256).astype(np.uint64).tobytes())
    if kind == "FSE":
        return dict(records=[orc.fse_encode_block(data[a:a + block], 8, 64, 1).tobytes() for a in range(0, len(data), block)])
    if kind == "CRC":
        return dict(value=zlib.crc32(data.tobytes()))
    if kind == "ADLER":
        return dict(value=zlib.adler32(data.tobytes()))
    if kind == "OLD":
        s, nb = orc.lz77_old_encode(data, wbits, 4)
        return dict(out=s.tobytes(), bits=int(nb))
    raise ValueError(kind)


_EXPECTED = {}


def expected(kind, recipe, block, wbits=None, container=None):
    key = (kind, recipe, block, wbits, container)
    if key not in _EXPECTED:
        _EXPECTED[key] = expected_of(kind, make(recipe), block, wbits, container)
    return _EXPECTED[key]


def save_expected(path):
    """what expected() has worked out so far, for a child process (the oracle takes seconds on inputs that fall back)"""
    import pickle
    with open(path, "wb") as f:
        pickle.dump(_EXPECTED, f)


def load_expected(path):
    import pickle
    with open(path, "rb") as f:
        _EXPECTED.update(pickle.load(f))


def fse_histograms():
    """(the histogram whose normalisation is checked, the histogram that stands in for it until the late copy: both are valid
    counts, since a count is not a data byte)"""
    freq = np.bincount(make(WHOLE), minlength=256).astype(np.uint64)
    return freq, (freq[::-1] + 1).copy()


# ---- the device side ------------------------------------------------------------------------------------------------------------
class Delay:
    """GPU work of a calibrated duration on the current stream: torch.cuda._sleep where this torch has it, else a chain of
    large device copies; calibrated once per process with events (the faster of two runs, so that it never comes out short)"""
    _inst = None

    def __init__(self):
        import torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        if self.sleep is None:
            self.a = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
            self.b = torch.empty_like(self.a)
        unit = 4_000_000 if self.sleep else 16
        self._work(unit)
        best = math.inf
        for _ in range(2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._work(unit)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        self.units_per_ms = unit / max(best, 1e-3)

    def _work(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.b.copy_(self.a)

    def __call__(self, ms):
        self._work(math.ceil(ms * self.units_per_ms))

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst


class Case:
    """the buffers of one case.  late(): a payload buffer that holds poison until load() copies the data in; out(): an output
    buffer (uint8, any other type is a view on the host) that holds 0x5A, with a twin keep() copies it into."""

    def __init__(self, ctx, name, asynchronous=True):
        self.ctx, self.name, self.asynchronous = ctx, name, asynchronous
        import torch
        self.lates, self.outs, self.tables, self.check, self._i64 = [], {}, set(), None, torch.int64
        self.scrub_more = None                                 # a further call that leaves other intermediates behind (scrub)

    def late(self, data, poison, pad=0):
        import torch
        d, p = as_np(data), as_np(poison)
        assert d.size == p.size
        tail = np.zeros(pad, dtype=np.uint8)
        src = torch.from_numpy(np.concatenate([d, tail])).to(self.ctx.device)
        poi = torch.from_numpy(np.concatenate([p, tail])).to(self.ctx.device)
        buf = poi.clone()
        self.lates.append((buf, src, poi))
        return buf

    def out(self, name, nbytes, table=False):
        """table: an array of u64 offsets, sizes or counts.  The library reads some of these back in stream order as the place
        to write to (k_defz_finish and k_bgzf_finish take the end of the records from the caller's block table), so under a
        missing join their poison becomes an address: it is TABLE_POISON in every entry, a small valid offset, not 0x5A."""
        import torch
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.ctx.device)
        assert not table or t.numel() % 8 == 0
        self.outs[name] = (t, torch.empty_like(t))
        self.tables.add(name) if table else None
        self._fill(name)
        return t

    def _fill(self, name):
        t = self.outs[name][0]
        if name in self.tables:
            t.view(dtype=self._i64).fill_(TABLE_POISON)
        else:
            t.fill_(OUT_POISON)

    def load(self):
        for buf, src, _ in self.lates:
            buf.copy_(src)

    def poison(self):
        for buf, _, poi in self.lates:
            buf.copy_(poi)
        for name in self.outs:
            self._fill(name)

    def keep(self):
        for t, twin in self.outs.values():
            twin.copy_(t)

    def kept(self):
        """the twins on the host: name -> uint8 array"""
        return {k: twin.cpu().numpy() for k, (_, twin) in self.outs.items()}


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset)


def delay_for(call_seconds):
    return min(max(4e3 * call_seconds, DELAY_FLOOR_MS), DELAY_CEIL_MS)


def warm_and_time(case, call, stream):
    """one call that grows the workspace, then the host time of a second one, both with the data in place -> seconds"""
    import torch
    with torch.cuda.stream(stream):
        case.load()
        rc = call()
        assert rc == 0, (case.name, rc)
        case.ctx.sync()
        torch.cuda.synchronize()                               # (nothing of the first call is left anywhere: one call is timed)
        t0 = time.perf_counter()
        rc = call()
        t = time.perf_counter() - t0
        assert rc == 0, (case.name, rc)
        case.ctx.sync()
        torch.cuda.synchronize()
    return t


def scrub(case, call, stream):
    """The warm-up calls leave the context's workspace holding the right intermediates for exactly the data under test, at
    the same addresses: a consumer that ran ahead of its producer on an internal stream would read values identical to
    those about to be written, and pass.  So one more call runs on the POISON (a valid input to every encoder, whose stream
    differs: tests/test_stream_cases_cpu.py; the readers and decoders refuse theirs), and case.scrub_more where a case has
    one; the status is not looked at.  Afterwards the workspace holds what the measured call must not be seen to use."""
    import torch
    with torch.cuda.stream(stream):
        case.poison()
        call()
        if case.scrub_more:
            case.scrub_more()
        try:
            case.ctx.sync()
        finally:
            torch.cuda.synchronize()


def run(case, call, stream=None, background=None, call_seconds=None):
    """late input, the call, early poison, one sync on a non-blocking stream; then case.check(the copies).  background: a
    function that queues unrelated work on the default stream just before.  call_seconds: the host time of a warm call where
    the caller has measured it (neither warm-up nor scrub calls are made here then)."""
    import torch
    S = stream or torch.cuda.Stream()
    if call_seconds is None:
        t = warm_and_time(case, call, S)
        scrub(case, call, S)
    else:
        t = call_seconds
    delay_ms = delay_for(t)
    for attempt in (0, 1):
        with torch.cuda.stream(S):
            case.poison()
        torch.cuda.synchronize()
        if background:
            background()
        with torch.cuda.stream(S):
            Delay.get()(delay_ms)
            case.load()
            ev = torch.cuda.Event()
            ev.record()
            rc = call()
            late = not ev.query()
            case.keep()
            case.poison()
            case.ctx.sync()
        assert rc == 0, (case.name, rc)
        if late or not case.asynchronous or attempt:
            break
        delay_ms *= 4
    print(f"stream-order timing: {case.name}: call {1e3 * t:.3f} ms on the host, delay {delay_ms:.1f} ms")
    if case.asynchronous:
        assert late, f"{case.name}: vacuous — the late copy had finished when the call returned (delay {delay_ms:.1f} ms, call {1e3 * t:.3f} ms)"
    case.check(case.kept())


# ---- encoders ---------------------------------------------------------------------------------------------------------------------
def _table(a, count):
    return [int(v) for v in a[: 8 * count].view(np.int64)]


def lz_params(kind, block, wbits):
    from compression_algorithms_amd import lz
    return lz.params("lz77", wbits, block) if kind == "L" else lz.params("deflate", None, block)


def encoder_case(ctx, name, kind, recipe, block, wbits=None, container=None, asynchronous=True):
    """one LZ-family encode (T deflate tokens, L lz77, H, Z, BGZF, FIND) -> (case, call)"""
    from compression_algorithms_amd import lz
    data = make(recipe)
    n = data.size
    p = lz_params(kind, block, wbits)
    nblocks = (n + block - 1) // block
    c = Case(ctx, name, asynchronous)
    d_in = c.late(data, data_poison(data))
    L, h = ctx.L, ctx.h
    if kind == "FIND":
        cand = c.out("cand", 2 * n)
        call = lambda: L.mi_lz_find_all_dev(h, C.byref(p), ptr(d_in), n, ptr(cand), ctx.stream_ptr())
        want = expected(kind, recipe, block, wbits, container)

        def check(got):
            bad = np.flatnonzero(got["cand"][: 2 * n].view(np.uint16) != np.frombuffer(want["cand"], dtype=np.uint16))
            assert bad.size == 0, f"{name}: {bad.size} candidates differ, first at {bad[:5]}"
        c.check = check
        return c, call
    if kind in ("T", "L"):
        cap = lz.bound_bytes(n, p) + 64
    elif kind == "H":
        cap = int(L.mi_deflate_h_bound_bytes(n, C.byref(p))) + 64
    elif kind == "Z":
        cid = lz.CONTAINERS[container]
        cap = lz.bound_bytes_z(n, p, cid)
    else:
        cap = lz.bound_bytes_bgzf(n, p)
    cap = (cap + 3) & ~3
    out, bits = c.out("out", cap), c.out("bits", 8 * (nblocks + 1), table=True)
    if kind in ("T", "L"):
        call = lambda: L.mi_lz_encode_dev(h, C.byref(p), ptr(d_in), n, ptr(out), cap, ptr(bits), ctx.stream_ptr())
    elif kind == "H":
        call = lambda: L.mi_deflate_h_encode_dev(h, C.byref(p), ptr(d_in), n, ptr(out), cap, ptr(bits), ctx.stream_ptr())
    elif kind == "Z":
        nb = c.out("nbytes", 8, table=True)
        call = lambda: L.mi_deflate_z_encode_dev(h, C.byref(p), cid, ptr(d_in), n, ptr(out), cap, ptr(bits), ptr(nb), ctx.stream_ptr())
    else:
        nb = c.out("nbytes", 8, table=True)
        call = lambda: L.mi_bgzf_encode_dev(h, C.byref(p), ptr(d_in), n, ptr(out), cap, ptr(bits), ptr(nb), ctx.stream_ptr())
    want = expected(kind, recipe, block, wbits, container)

    def check(got):
        assert _table(got["bits"], nblocks + 1) == list(want["bits"]), f"{name}: the block table differs"
        if "nbytes" in want:
            assert _table(got["nbytes"], 1) == [want["nbytes"]], f"{name}: out_bytes"
        w = np.frombuffer(want["out"], dtype=np.uint8)
        bad = np.flatnonzero(got["out"][: w.size] != w)
        assert bad.size == 0, f"{name}: the stream differs from the oracle's at byte {bad[:5]} of {w.size} ({bad.size} bytes)"
        if kind == "BGZF":
            import gzip
            assert gzip.decompress(got["out"][: w.size].tobytes()) == data.tobytes(), f"{name}: gzip does not give back the data"
    c.check = check
    return c, call


def chain(*calls):
    """several C calls one behind the other with no synchronisation -> the first status that is not MI_OK"""
    def call():
        for f in calls:
            rc = f()
            if rc:
                return rc
        return 0
    return call


def merge(ctx, name, cases, asynchronous=True):
    """several cases of one context as one: loaded, kept, poisoned and checked together"""
    m = Case(ctx, name, asynchronous)
    for k, c in enumerate(cases):
        m.lates += c.lates
        for key, v in c.outs.items():
            m.outs[f"{k}.{key}"] = v
            if key in c.tables:
                m.tables.add(f"{k}.{key}")

    def check(got):
        for k, c in enumerate(cases):
            c.check({key[len(f"{k}."):]: v for key, v in got.items() if key.startswith(f"{k}.")})
    m.check = check
    return m


# ---- the fallback stream and the hint-driven fourth stream ----------------------------------------------------------------------
def fallback_sequence():
    """On a fresh context, MI_LZ_BATCH=16 (the caller sets it): 64 blocks of the "pages" family, which leave the hint that
    blocks fall back; then two multi-batch text encodes back to back on one stream with no synchronisation between them.
    Both are queued before a batch of the first has run, so both read the hint the pages left: both send the fallback chains
    of their odd batches where that hint says (the side stream, or with MI_LZ_FB2_SIDE=0 a second fallback stream that the
    first call creates and the second finds in place), and the three streams are compared with the oracle's.  What this does
    NOT exercise: the release of that stream (hipStreamQuery in lz_emit.hip) — a call decides on it only once the hint is
    low again, which needs the text batches to have FINISHED, and then the input would no longer be late; it runs only in the
    unchecked warm-up calls, on an idle stream.  The encoder reads MI_LZ_FB2_SIDE with every call (csrc/lz_plan.h); the variants
    with it set run this in a child process (python -c ... fallback_sequence()) all the same: a fresh process has a fresh
    context, stream pool and hint."""
    import torch
    from compression_algorithms_amd.context import Context
    ctx = Context(0)
    try:
        S = torch.cuda.Stream()
        c0, call0 = encoder_case(ctx, "fb-pages", "T", PAGES, 65536)
        before = ctx.path_stats()["fallback_blocks"]
        run(c0, call0, S)
        fell = ctx.path_stats()["fallback_blocks"] - before
        print(f"stream-order fallback: {fell} block encodes of the pages input fell back in 3 calls of 4 batches of 16")
        assert fell > 3 * 4 * 8, f"precondition: more than 8 blocks of a batch must fall back, {fell} in 12 batches did"
        ca, call_a = encoder_case(ctx, "fb-a", "T", FB_A, 65536)
        cb, call_b = encoder_case(ctx, "fb-b", "H", FB_B, 65536)
        # the workspace grows with the text calls; the hint is what the LAST finished batch left, so the pages go once more
        t = warm_and_time(ca, call_a, S) + warm_and_time(cb, call_b, S)
        scrub(ca, call_a, S)
        scrub(cb, call_b, S)
        warm_and_time(c0, call0, S)
        run(merge(ctx, "fb-pair", [ca, cb]), chain(call_a, call_b), S, call_seconds=t)
    finally:
        ctx.close()
