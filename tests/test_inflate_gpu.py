"""The GPU inflater (mi_inflate_dev / mi_inflate, lz.decompress_z / lz.inflate) on the device.

Clean streams first: this library's own mode-Z streams, the CPU oracle's golden bytes, foreign streams written by stock zlib
with Z_FULL_FLUSH (inflate_cases.py), crafted blocks, a plain zlib.compress stream as one segment, 10^8 bytes.  Then a fixed
list of streams the decoder must refuse, each run once and only after the clean cases of this file have passed: they check
that the decoder refuses, with the bytes around its output buffer untouched.
"""
import ctypes as C
import functools
import gzip
import json
import os
import zlib

import numpy as np
import pytest
import torch

import defz_cases as D
import inflate_cases as ic
from compression_algorithms_amd import _lib, lz, synth

pytestmark = pytest.mark.gpu

CONTAINERS = ("raw", "zlib", "gzip")
_CLEAN = {"ran": 0, "failed": 0}


def clean(fn):
    """marks a clean case: the refusal cases look at how these went"""
    @functools.wraps(fn)
    def run(*a, **k):
        _CLEAN["ran"] += 1
        try:
            return fn(*a, **k)
        except BaseException:
            _CLEAN["failed"] += 1
            raise
    return run


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if len(b) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _roundtrip(data, block, container):
    x = _dev(data)
    s = lz.compress_z(x, lz.params("deflate", block=block), container)
    for verify in (True, False):
        y = lz.decompress_z(s, verify=verify)
        assert y.numel() == len(data) and torch.equal(y, x), (len(data), block, container, verify)
    return s


@pytest.fixture(scope="module")
def cases():
    return D.cases()


@clean
@pytest.mark.parametrize("block", (65536, 4096))
@pytest.mark.parametrize("container", CONTAINERS)
def test_own_streams_roundtrip(cases, container, block):
    for name, data in cases.items():
        _roundtrip(data, block, container)


@clean
def test_limiter_and_clip_blocks_roundtrip():
    for data in (D.skewed_block(), D.cl_limit_block(), D.dist_limit_block()):
        _roundtrip(data, 65536, "gzip")
    for c in CONTAINERS:
        _roundtrip(D.clip_blocks(), 4096, c)


@clean
def test_seeded_cases_roundtrip():
    for i, fam, data, block, container in D.seeded_cases():
        _roundtrip(data, block, container)


@clean
def test_empty_input():
    for c in CONTAINERS:
        s = _roundtrip(b"", 65536, c)
        assert lz.inflate(s.tobytes(), 0, seg_bits=[int(s.block_bits[0])], block=65536, container=c).numel() == 0
        assert lz.inflate(s.tobytes(), 0, container=c).numel() == 0
        assert lz.decompress_z_host(s.tobytes(), [int(s.block_bits[0])], 0, 65536, c) == b""


@clean
def test_host_entry_points_give_the_same_bytes(cases):
    for name in ("text1m", "random", "size65537", "size1", "tail_zeros"):
        for c, block in (("raw", 65536), ("zlib", 4096), ("gzip", 65536)):
            data = cases[name]
            stream, table = lz.compress_z_host(data, lz.params("deflate", block=block), c)
            assert lz.decompress_z_host(stream, table, len(data), block, c) == data, (name, c)
            assert lz.inflate(stream, len(data), seg_bits=table, block=block, container=c).cpu().numpy().tobytes() == data


@clean
def test_oracle_golden_records_inflate(golden_dir):
    z = json.load(open(os.path.join(golden_dir, "defz.json")))["kat_small"]
    kat = json.load(open(os.path.join(golden_dir, "kat_small.json")))
    assert z
    for name, e in z.items():
        want = bytes.fromhex(kat[name]["input_hex"])
        raw, table = bytes.fromhex(e["raw_hex"]), e["block_bits"]
        assert len(table) == (len(want) + 65535) // 65536 + 1
        got = lz.inflate(raw, len(want), seg_bits=table, block=65536, container="raw")
        assert got.cpu().numpy().tobytes() == want, name


@pytest.fixture(scope="module")
def foreign():
    return ic.foreign_set()


@clean
@pytest.mark.parametrize("container", CONTAINERS)
def test_foreign_zlib_streams(foreign, container):
    for name, data, level, seg in foreign:
        raw, table = ic.zlib_segments(data, level, seg)
        stream, tab = ic.frame(raw, table, data, container)
        if container == "zlib":
            assert zlib.decompress(stream) == data
        elif container == "gzip":
            assert gzip.decompress(stream) == data
        x = _dev(data)
        for verify in (True, False):
            y = lz.inflate(stream, len(data), seg_bits=tab, block=seg, container=container, verify=verify)
            assert torch.equal(y, x), (name, container, verify)
    name, data, level, seg = foreign[0]
    raw, table = ic.zlib_segments(data, level, seg)
    stream, tab = ic.frame(raw, table, data, container)
    assert lz.decompress_z_host(stream, tab, len(data), seg, container) == data


@clean
def test_gzip_header_with_name_extra_comment_and_crc(foreign):
    name, data, level, seg = foreign[0]
    raw, table = ic.zlib_segments(data, level, seg)
    stream, tab = ic.frame(raw, table, data, "gzip", ic.GZIP_RICH)
    assert gzip.decompress(stream) == data and tab[0] == 8 * len(ic.GZIP_RICH)
    assert lz.inflate(stream, len(data), seg_bits=tab, block=seg, container="gzip").cpu().numpy().tobytes() == data
    assert lz.inflate(stream, len(data), container="gzip").cpu().numpy().tobytes() == data      # one segment, header found on the host


@clean
def test_crafted_blocks():
    for name, (stream, want) in ic.crafted().items():
        table = [0, 8 * (len(stream) - 2)]
        for c in CONTAINERS:
            s, t = ic.frame(stream, table, want, c)
            got = lz.inflate(s, len(want), seg_bits=t, block=len(want), container=c)
            assert got.cpu().numpy().tobytes() == want, (name, c)
    # the same segments decoded with the 4 KiB ring (many segments): the stream is 1 100 copies of the crafted one
    reps = 1100
    for name, (stream, want) in ic.crafted().items():
        body = stream[:-2]
        table = [8 * len(body) * k for k in range(reps + 1)]
        got = lz.inflate(body * reps + ic.CLOSE, len(want) * reps, seg_bits=table, block=len(want), container="raw")
        assert torch.equal(got, _dev(want * reps)), name


@clean
def test_plain_zlib_compress_as_one_segment():
    data = synth.enwik_like(300_000, seed=21).numpy().tobytes()
    assert lz.inflate(zlib.compress(data, 9), len(data), seg_bits=None, container="zlib").cpu().numpy().tobytes() == data
    assert lz.inflate(gzip.compress(data, 6), len(data), container="gzip").cpu().numpy().tobytes() == data
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    assert lz.inflate(raw, len(data), container="raw").cpu().numpy().tobytes() == data
    # mode Z's own stream without its table: 03 00 behind the last record
    s = lz.compress_z(_dev(data[:60_000]), container="gzip")
    assert lz.inflate(s.tobytes(), 60_000, container="gzip").cpu().numpy().tobytes() == data[:60_000]


@clean
def test_1e8_roundtrip():
    x = synth.enwik_like(100_000_000, seed=31, device="cuda")
    s = lz.compress_z(x, container="gzip")
    assert torch.equal(lz.decompress_z(s), x)
    assert torch.equal(lz.decompress_z(s, verify=False), x)


# ---------------------------------------------------------------------------------------------------------------------
# refusal.  Each case once; the output buffer sits between 4 KiB of a known pattern.
GUARD = 4096
REJECTS = ic.rejects()


def _need_clean_cases():
    if _CLEAN["failed"]:
        pytest.fail("a clean case of this file failed: the refusal cases are not run on a decoder that is wrong on good streams")
    if not _CLEAN["ran"]:                                            # selected alone: one clean round trip first
        test_plain_zlib_compress_as_one_segment()


def _guarded(container, block, stream, table, n, verify):
    ctx = lz.default_context()
    d_stream = _dev(stream)
    bits = torch.tensor(table, dtype=torch.int64, device="cuda")
    buf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    c = lz.CONTAINERS.get(container, container)
    st = ctx.L.mi_inflate_dev(ctx.h, c, block, C.c_void_p(d_stream.data_ptr()), len(stream), C.c_void_p(bits.data_ptr()),
                              C.c_void_p(buf.data_ptr() + GUARD), n, 0 if verify else lz.MI_INFLATE_NO_CHECKSUM, ctx.stream_ptr())
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all())
    return st, buf[GUARD:GUARD + n], intact


@pytest.mark.parametrize("case", REJECTS, ids=[r[0] for r in REJECTS])
def test_refused(case):
    _need_clean_cases()
    name, container, block, stream, table, n, verify, status = case
    st, out, intact = _guarded(container, block, stream, table, n, verify)
    assert intact, "bytes outside the output buffer were written"
    assert st == status, (name, _lib.STATUS.get(st, st))


def test_refused_arguments():
    _need_clean_cases()
    ctx = lz.default_context()
    data = b"abc" * 100
    stream = zlib.compress(data)
    d = _dev(b"\0" + stream)                                           # an odd address for the stream
    bits = torch.tensor([16, 8 * (len(stream) - 4)], dtype=torch.int64, device="cuda")
    out = torch.zeros(512, dtype=torch.uint8, device="cuda")
    vp = C.c_void_p
    call = lambda *a: ctx.L.mi_inflate_dev(ctx.h, *a, ctx.stream_ptr())
    assert call(1, 300, vp(d.data_ptr() + 1), len(stream), vp(bits.data_ptr()), vp(out.data_ptr()), 300, 0) == 1
    assert call(1, 300, vp(d.data_ptr() + 4), len(stream), vp(bits.data_ptr()), vp(out.data_ptr()), 300, 2) == 1     # unknown flag
    assert call(1, 300, None, len(stream), vp(bits.data_ptr()), vp(out.data_ptr()), 300, 0) == 1
    assert call(1, 300, vp(d.data_ptr() + 4), len(stream), None, vp(out.data_ptr()), 300, 0) == 1
    assert call(1, 300, vp(d.data_ptr() + 4), len(stream), vp(bits.data_ptr()), None, 300, 0) == 1
    assert call(1, 1 << 31, vp(d.data_ptr() + 4), len(stream), vp(bits.data_ptr()), vp(out.data_ptr()), 300, 0) == 1


def test_host_entry_point_checks_the_table_first():
    _need_clean_cases()
    for name, container, block, stream, table, n, verify, status in REJECTS:
        if name.startswith("table_") and name != "table_starts_inside_header":
            with pytest.raises(_lib.MiError) as e:
                lz.decompress_z_host(stream, table, n, block, container)
            assert e.value.status == 8, name


def test_one_segment_wrapper_asks_for_a_table():
    _need_clean_cases()
    data = synth.enwik_like(200_000, seed=5).numpy().tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(data[:100_000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[100_000:]) + c.flush(zlib.Z_SYNC_FLUSH)
    with pytest.raises(ValueError):
        lz.inflate(raw, len(data), container="raw")                    # no BFINAL anywhere: neither shape
