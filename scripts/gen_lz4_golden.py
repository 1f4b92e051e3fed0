#!/usr/bin/env python3
"""Writes tests/golden/lz4_stock.json: what STOCK LZ4 writes for the inputs of tests/lz4_cases.golden_inputs(), as base64, with the
a SHA-256 prefix of each input, and how stock LZ4 judges one-byte mutations of some of its own blocks.
  blocks     raw blocks from pyarrow's "lz4_raw" codec (LZ4_compress_default)
  frames     frames from pyarrow's "lz4" codec and, where liblz4.so.1 loads through ctypes, from LZ4F_compressFrame with preferences
             for linked blocks, a content size, block checksums, a content checksum and a block maximum of 256 KiB
  mutations  (liblz4 only) per mutation of tests/lz4_cases.mutation_plan: LZ4_decompress_safe's return value with a capacity of
             the original size + MUTATION_ROOM, and the verdict, size and SHA-256 prefix that tests/lz4_cases.decode gives — the
             expectation the GPU decoder is held to; where stock accepts, the two must agree (tests/test_lz4_cpu.py)
The GPU tests read that file and never pyarrow or liblz4, which a GPU machine may not have; tests/test_lz4_cpu.py regenerates it
where both are installed and compares.  Run from the repository root:  python scripts/gen_lz4_golden.py"""
import base64
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def liblz4():
    try:
        return ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


# name -> (input, preferences): blockSizeID 4 = 64 KiB, 5 = 256 KiB; blockMode 0 = linked, 1 = independent
LZ4F = {"lz4f_linked": ("periodic_70000", dict(blockSizeID=4, blockMode=0)),
        "lz4f_content_size": ("chunk_offset_63", dict(blockSizeID=4, blockMode=1, contentSize=None)),
        "lz4f_block_checksum": ("chunk_offset_63", dict(blockSizeID=4, blockMode=1, blockChecksumFlag=1)),
        "lz4f_content_checksum": ("period3", dict(blockSizeID=4, blockMode=0, contentChecksumFlag=1)),
        "lz4f_256k": ("zeros", dict(blockSizeID=5, blockMode=1)),
        "lz4f_incompressible": ("noise_1000", dict(blockSizeID=4, blockMode=1))}


def lz4f_frame(L, data, prefs):
    p = Preferences()
    for k, v in prefs.items():
        setattr(p.frameInfo, k, len(data) if v is None else v)
    L.LZ4F_compressFrameBound.restype = ctypes.c_size_t
    L.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.POINTER(Preferences)]
    L.LZ4F_compressFrame.restype = ctypes.c_size_t
    L.LZ4F_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Preferences)]
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(p))
    buf = ctypes.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(buf, cap, data, len(data), ctypes.byref(p))
    assert not L.LZ4F_isError(ctypes.c_size_t(n)), n
    return buf.raw[:n]


def stock_block(L, stream, cap):
    """LZ4_decompress_safe -> (its return value, the bytes where it is >= 0)"""
    buf = ctypes.create_string_buffer(max(cap, 1))
    r = L.LZ4_decompress_safe(stream, buf, len(stream), cap)
    return r, buf.raw[:max(r, 0)]


def _entry(name, key, data, stream, writer):
    return {"name": name, "input": key, "writer": writer, "sha256": hashlib.sha256(data).hexdigest()[:16],
            "stream": base64.b64encode(stream).decode("ascii")}


def document(with_liblz4=True):
    import pyarrow as pa
    import lz4_cases as Z
    inputs = Z.golden_inputs()
    raw, fr = pa.Codec("lz4_raw"), pa.Codec("lz4")
    doc = {"format": "LZ4 raw blocks and frames, base64", "blocks": [], "frames": [], "mutations": []}
    for name, data in inputs.items():
        doc["blocks"].append(_entry(name, name, data, raw.compress(data, asbytes=True), "pyarrow.Codec('lz4_raw')"))
        doc["frames"].append(_entry(name, name, data, fr.compress(data, asbytes=True), "pyarrow.Codec('lz4')"))
    L = liblz4() if with_liblz4 else None
    if L is None:
        return doc
    for name, (key, prefs) in LZ4F.items():
        doc["frames"].append(_entry(name, key, inputs[key], lz4f_frame(L, inputs[key], prefs), "LZ4F_compressFrame"))
    blocks = {e["name"]: base64.b64decode(e["stream"]) for e in doc["blocks"]}
    for name in Z.MUTATED:
        cap = len(inputs[name]) + Z.MUTATION_ROOM
        for at, mask in Z.mutation_plan(name, blocks[name]):
            s = Z.mutate(blocks[name], at, mask)
            r, _ = stock_block(L, s, cap)
            out, verdict, n = Z.decode(s, "block", cap)
            doc["mutations"].append([name, at, mask, r, verdict, n, hashlib.sha256(out).hexdigest()[:16] if out is not None else None])
    return doc


def text(doc):
    """one line per stream; the mutations as rows [block, position, xor mask, stock's return value, verdict, out_bytes, SHA-256
    prefix of the expected bytes], eight to a line"""
    rows = [json.dumps(r, separators=(",", ":")) for r in doc["mutations"]]
    lines = ['{"format": %s,' % json.dumps(doc["format"])]
    for kind in ("blocks", "frames"):
        lines.append(' "%s": [' % kind)
        lines += ["  " + json.dumps(e) + "," for e in doc[kind][:-1]] + ["  " + json.dumps(doc[kind][-1]) + "],"]
    lines.append(' "mutations": [')
    lines += ["  " + ",".join(rows[k:k + 8]) + ("," if k + 8 < len(rows) else "") for k in range(0, len(rows), 8)]
    return "\n".join(lines + [" ]}"]) + "\n"


if __name__ == "__main__":
    import lz4_cases as Z
    out = text(document())
    with open(Z.GOLDEN, "w") as f:
        f.write(out)
    d = json.loads(out)
    print(f"{Z.GOLDEN}: {len(out)} bytes, {len(d['blocks'])} blocks, {len(d['frames'])} frames, {len(d['mutations'])} mutations")
