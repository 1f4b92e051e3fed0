#!/usr/bin/env python3
"""ORACLE — TEST INFRASTRUCTURE ONLY.

tests/golden/defz.json: fixtures for deflate "mode Z" (oracle/orc_defz.c).

The bytes are the ORACLE's output, committed so that a change of the format shows up as a diff.  Before anything is
written, the token streams that are coded are checked against the ones tests/golden/kat_small.json and
enwik_like_300k.json pin to the real reference, and every stream must inflate back to its input through stock zlib.

    python oracle/gen_golden_defz.py
"""
import gzip
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import orc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CONTAINERS = ("raw", "zlib", "gzip")


def inflate(x, container):
    if container == "raw":
        return zlib.decompress(x, -15)
    if container == "zlib":
        return zlib.decompress(x)
    return gzip.decompress(x)


def build():
    """-> the fixture dict, or exits without one on any mismatch"""
    out = {}
    kat = json.load(open(os.path.join(GOLD, "kat_small.json")))
    small = {}
    for name, e in sorted(kat.items()):
        data = bytes.fromhex(e["input_hex"])
        tok, sizes = orc.deflate_stream(data, 65536, True)
        if tok.tobytes().hex() != e["deflate_fresh_hex"]:
            sys.exit(f"{name}: oracle tokens differ from the reference golden vector; not writing fixtures")
        x, bits = orc.defz_stream(data, 65536, "raw", tokens=(tok, sizes))
        if inflate(x, "raw") != data:
            sys.exit(f"{name}: the oracle's stream does not inflate; not writing fixtures")
        small[name] = {"raw_hex": x.hex(), "block_bits": bits}
    out["kat_small"] = small
    sample = np.fromfile(os.path.join(GOLD, "enwik_like_300k.bin"), dtype=np.uint8)
    g = json.load(open(os.path.join(GOLD, "enwik_like_300k.json")))["deflate_independent"]
    big = {}
    for block in (65536, 4096):
        tok, sizes = orc.deflate_stream(sample, block, True)
        if block == 65536 and hashlib.sha256(tok.tobytes()).hexdigest() != g["sha256"]:
            sys.exit("300k sample: oracle tokens differ from the reference golden vector; not writing fixtures")
        for c in CONTAINERS:
            x, bits = orc.defz_stream(sample, block, c, tokens=(tok, sizes))
            if inflate(x, c) != sample.tobytes():
                sys.exit(f"300k sample, block {block}, {c}: the oracle's stream does not inflate; not writing fixtures")
            big[f"{c}_{block}"] = {"bytes": len(x), "sha256": hashlib.sha256(x).hexdigest(),
                                   "block_bits_sha256": hashlib.sha256(np.asarray(bits, np.uint64).tobytes()).hexdigest()}
    out["enwik_like_300k"] = big
    return out


def main():
    out = build()
    json.dump(out, open(os.path.join(GOLD, "defz.json"), "w"), indent=1, sort_keys=True)
    print("wrote defz.json:", {k: v["bytes"] for k, v in out["enwik_like_300k"].items()})


if __name__ == "__main__":
    main()
