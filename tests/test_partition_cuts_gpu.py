"""The cut walk of the partition (lz2_partition_cuts in csrc/lz2_partition.hip): one 64-way probe and one window of
64 groups per cut, against the search it replaced and against the rule itself.

The test build of the library (lib_test, -DMI_TEST_HOOKS) keeps the earlier search behind MI_LZ_TEST_OLD_CUTS=1, read when a
context is created, and hands back what a context's last partition launch wrote (mi_test_partmap).  Every child process below
makes one context of each kind and encodes the same bytes on both: per block n, nparts, base, fallback, part_start / part_count /
part_lo up to nparts and all seven planes must be equal word for word.  For text, parts of 640 entries and the lz77 tables the
record is also held against the numpy restatement of the rule (tests/partition_rule.py) — the parts are pinned to the rule, not
only to the old code.  All three kernels run: k_lz2_partition_direct (aligned input), k_lz2_partition<false> (a view at +1 byte)
and k_lz2_partition<true> (the batched deflate)."""
import os
import subprocess
import sys
import textwrap

import pytest

from compression_algorithms_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_LIB = os.path.join(_lib.LIB_DIR, "..", "lib_test", "libmi_codec.so")

PRELUDE = """
    import ctypes as C
    import os, sys
    import numpy as np, torch
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import partition_rule as rule
    from compression_algorithms_amd import lz, synth
    from compression_algorithms_amd.context import Context

    PLANES, PLANE_DW, MAXPARTS = 7, 2048, 128
    META_DW = 8 + 3 * MAXPARTS                                  # Lz2BlockMeta (csrc/lz2.h)

    def contexts():
        assert "MI_LZ_TEST_OLD_CUTS" not in os.environ
        new = Context(0)
        os.environ["MI_LZ_TEST_OLD_CUTS"] = "1"                 # read when a context is created
        old = Context(0)
        del os.environ["MI_LZ_TEST_OLD_CUTS"]
        return new, old

    def partmap(ctx, max_blocks):
        f = ctx.L.mi_test_partmap
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        planes = np.zeros((max_blocks, PLANES, PLANE_DW), np.uint32)
        meta = np.zeros((max_blocks, META_DW), np.uint32)
        nb = f(ctx.h, planes.ctypes.data, meta.ctypes.data, max_blocks)
        assert nb >= 0, "no partition launch on this context, or a HIP error"
        return planes[:min(nb, max_blocks)], meta[:min(nb, max_blocks)]

    def same_maps(new, old, want_n, what):
        # what the two contexts' last partition launches wrote; returns the new context's records
        (pn, mn), (po, mo) = partmap(new, 8), partmap(old, 8)
        assert len(pn) == len(po) and len(pn) >= len(want_n), (what, len(pn), len(po))
        for b in range(len(pn)):
            if b < len(want_n):
                assert int(mn[b][0]) == want_n[b], (what, b, "n", int(mn[b][0]))
            assert np.array_equal(mn[b][:4], mo[b][:4]), (what, b, "n, nparts, base, fallback", mn[b][:4], mo[b][:4])
            k, fb = int(mn[b][1]), int(mn[b][3])
            for f, name in enumerate(("part_start", "part_count", "part_lo")):
                a = 8 + f * MAXPARTS
                assert np.array_equal(mn[b][a:a + k], mo[b][a:a + k]), (what, b, name)
            if not fb:                                           # (a block that falls back has no part map)
                bad = np.flatnonzero(pn[b].reshape(-1) != po[b].reshape(-1))
                assert bad.size == 0, (what, b, "plane dwords differ", bad[:8])
        return mn

    def is_the_rules(meta, r, what):
        k = int(meta[1])
        assert int(meta[3]) == r["fallback"] == 0, (what, "fallback")
        assert int(meta[0]) == r["n"] and k == r["nparts"] and int(meta[2]) == r["base"], (what, meta[:4], r["nparts"], r["base"])
        assert np.array_equal(meta[8 + MAXPARTS:8 + MAXPARTS + k], r["part_count"]), (what, "part_count")
        assert np.array_equal(meta[8 + 2 * MAXPARTS:8 + 2 * MAXPARTS + k], r["part_lo"]), (what, "part_lo")

    def text(n, seed):
        return synth.enwik_like(n, seed=seed).numpy()

    def aligned(x):
        d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        assert d.data_ptr() % 16 == 0
        return d

    def both(new, old, d, p):
        for ctx in (new, old):
            lz.compress(d, p, ctx); ctx.sync()
"""


def _child(body, **env_extra):
    if not os.path.exists(TEST_LIB):
        _lib.build()
    env = dict(os.environ, PYTHONPATH=ROOT, MI_CODEC_LIB=os.path.abspath(TEST_LIB), **env_extra)
    env.pop("MI_LZ_TEST_OLD_CUTS", None)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(PRELUDE) + textwrap.dedent(body)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


def test_both_searches_cut_the_same_parts_and_the_rules():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        full = text(65536, 12345)
        for n in (65536, 4099, 2048, 1):                                      # ~33 cuts; a few; one part; no walk
            both(new, old, aligned(full[:n]), p)
            m = same_maps(new, old, [n], n)
            is_the_rules(m[0], rule.parts(full[:n], 20, True), n)
            assert (int(m[0][1]) > 30) if n == 65536 else (int(m[0][1]) == 1) == (n <= 2048), (n, int(m[0][1]))
        for wbits in (14, 16):                                                # no ring (gstart 0); T = 2^22: every group in the span, the probe repeats
            both(new, old, aligned(full), lz.params("lz77", wbits))
            m = same_maps(new, old, [65536], ("lz77", wbits))
            is_the_rules(m[0], rule.parts(full, wbits + 6, False), ("lz77", wbits))
        seen = set()
        for kind in ("runs", "pages"):                                        # wide parts, and the exit to the fallback
            for seed in (1, 2):
                both(new, old, aligned(synth.family(kind, seed, 65536)), p)
                m = same_maps(new, old, [65536], (kind, seed))
                k = int(m[0][1])
                seen.add("fallback" if int(m[0][3]) else "wide" if (m[0][8 + MAXPARTS:8 + MAXPARTS + k] > 2048).any() else "plain")
        odd = aligned(text(65536 + 4099 + 1, 397))[1:]                        # a view at +1 byte: k_lz2_partition<false>
        assert odd.data_ptr() % 16 == 1
        both(new, old, odd, p)
        same_maps(new, old, [65536, 4099], "view at +1")
        items = [aligned(text(65536 + 777, 398)), aligned(text(4099, 396))]   # the batched deflate: k_lz2_partition<true>
        for ctx in (new, old):
            assert lz.deflate_batch(items, p, "raw", ctx=ctx).failed == 0
        m = same_maps(new, old, [65536, 777, 4099], "batch")
        is_the_rules(m[0], rule.parts(items[0][:65536].cpu().numpy(), 20, True), "batch, block 0")
        assert new.order_violations() == 0 and old.order_violations() == 0
        print("ok", sorted(seen))
    """)
    assert "ok" in out


def test_parts_of_640_entries():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        for n, seed in ((65536, 700), (65535, 701)):                         # ~100 cuts, most of their windows reach below the part's start
            data = text(n, seed)
            both(new, old, aligned(data), p)
            m = same_maps(new, old, [n], ("small parts", n))
            assert int(m[0][1]) > 64 and not int(m[0][3]), m[0][:4]
            is_the_rules(m[0], rule.parts(data, 20, True, cap=640), ("small parts", n))
        assert new.order_violations() == 0 and old.order_violations() == 0
        print("ok")
    """, MI_LZ_TEST_SMALL_PARTS="1")
    assert "ok" in out


def test_a_cut_whose_last_certified_group_lies_below_the_window():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        data = rule.block_with_distant_cut()
        r = rule.parts(data, 20, True)
        # the window is the 64 groups in front of an end that lies at or behind the boundary: from 65 groups on it cannot hold the cut
        far = [boundary - g for glo, boundary, g in r["cuts"]]
        assert not r["fallback"] and max(far) >= 80, ("the input no longer has a cut below the window", far)
        both(new, old, aligned(data), p)
        m = same_maps(new, old, [len(data)], "distant cut")
        is_the_rules(m[0], r, "distant cut")
        st = lz.compress(aligned(data), p, new); new.sync()
        assert np.array_equal(lz.decompress(st, new).cpu().numpy(), data)
        assert new.path_stats()["fallback_blocks"] == 0 and new.order_violations() == 0
        print("ok", max(far))
    """)
    assert "ok" in out
