"""A workspace layout is written once, as a sequence of mi_carver::take calls, and the byte count handed to mi_ws_reserve is
the end of that same sequence (data layout).  mi_ws_reserve allocates more than it is asked for, which would hide a
layout that overruns its own measure; the test build of the library (lib_test, -DMI_TEST_HOOKS) turns that slack into a guard:
mi_test_ws_guard fills everything behind the largest request with a pattern (arm) and looks for the first changed byte
(check).  Every entry point that uses the workspace runs twice in a fresh context — the first call grows the workspace, the
second runs over the armed guard — and must leave the guard whole and give the same output both times.  A case is one entry
point, so that the guard lies behind ITS request: what a decoder, a reader or a later step reads is made on another context.  Nothing is provoked:
a layout that overran would land in the slack.  The cases are in ws_guard_cases.py and run in one child process (a library is
chosen when a process starts)."""
import json
import os
import subprocess
import sys

import pytest

from compression_algorithms_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_LIB = os.path.join(_lib.LIB_DIR, "..", "lib_test", "libmi_codec.so")     # the core library built with -DMI_TEST_HOOKS (csrc/Makefile)

CASES = ([f + t for t in ("", "_batch2") for f in ("tokens", "h", "z_zlib", "bgzf", "lz77w14")] +
         ["deflate_batch", "wide_sliced", "wide_whole_block", "wide_one_block_redone", "find_all", "find_all32",
          "huffman_100000", "huffman_build_100000", "huffman_with_tree_100000", "huffman_0", "huffman_build_0",
          "huffman_with_tree_0", "fse", "compress_old", "decompress_whole", "decompress_z", "bgzf_index", "decompress_bgzf",
          "bgzf_read", "inflate_batch_ordered"])


@pytest.fixture(scope="module")
def results():
    if not os.path.exists(TEST_LIB):
        _lib.build()
    env = dict(os.environ, MI_CODEC_LIB=os.path.abspath(TEST_LIB), PYTHONPATH=ROOT)
    for k in ("MI_LZ_BATCH", "MI_LZW_SLICED", "MI_INFLATE_BATCH_ORDER"):      # the cases set their own
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ws_guard_cases.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("WS_GUARD ")][-1]
    return json.loads(line[len("WS_GUARD "):])


def test_every_case_ran(results):
    assert sorted(results) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_call_stays_inside_what_it_reserved(results, case):
    at, same = results[case]
    assert at == -1, f"{case}: the guard behind the reserved bytes was written at workspace offset {at}"
    assert same, f"{case}: two calls on one context gave different output"
