#!/usr/bin/env python3
"""Writes tests/golden/snappy_stock.json: what STOCK Snappy (pyarrow's "snappy" codec, which links google/snappy) writes for
the inputs of tests/snappy_cases.golden_inputs(), as base64, with the SHA-256 of each input.  The GPU tests read that file and
never pyarrow, which a GPU machine may not have; tests/test_snappy_cpu.py regenerates it where pyarrow is installed and
compares.  Run from the repository root:  python scripts/gen_snappy_golden.py"""
import base64
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def document():
    import pyarrow as pa
    import snappy_cases as S
    codec = pa.Codec("snappy")
    streams = [{"name": name, "bytes": len(data), "sha256": hashlib.sha256(data).hexdigest(),
                "stream": base64.b64encode(codec.compress(data, asbytes=True)).decode("ascii")}
               for name, data in S.golden_inputs().items()]
    return {"format": "raw snappy (snappy::Compress), base64", "writer": "pyarrow.Codec('snappy')", "streams": streams}


def text(doc):
    return json.dumps(doc, indent=1) + "\n"


if __name__ == "__main__":
    import snappy_cases as S
    out = text(document())
    with open(S.GOLDEN, "w") as f:
        f.write(out)
    print(f"{S.GOLDEN}: {len(out)} bytes, {len(json.loads(out)['streams'])} streams")
