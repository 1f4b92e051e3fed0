"""k_lz2_partition_direct — the partition of blocks that start on 16-byte boundaries of one buffer, block kept in registers,
two workgroups per CU (csrc/lz2_partition.hip) — against k_lz2_partition, which every other input still takes.

The test build of the library (lib_test, -DMI_TEST_HOOKS) sends aligned one-buffer input through the old kernel too when a
context is created under MI_LZ_TEST_OLD_PARTITION=1, and hands back what a context's last partition launch wrote
(mi_test_partmap).  Every child process below makes one context of each kind and encodes the same bytes on both: per block the
seven planes, n, nparts, base, fallback and part_start / part_count / part_lo up to nparts must be equal word for word.  (The
work list's order depends on atomics and is not compared.)  The families around it: blocks that fall back, a view one byte
into an allocation (the old kernel, in the shipped path too), and streams against the oracle's."""
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
    import os
    import numpy as np, torch
    from compression_algorithms_amd import lz, synth
    from compression_algorithms_amd.context import Context
    from oracle import orc

    PLANES, PLANE_DW, MAXPARTS = 7, 2048, 128
    META_DW = 8 + 3 * MAXPARTS                                  # Lz2BlockMeta (csrc/lz2.h)
    SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 67, 68, 127, 128, 129, 2048, 2049, 4096, 65535, 65536]
    LONG = 3 * 65536 + 100

    def contexts():
        assert "MI_LZ_TEST_OLD_PARTITION" not in os.environ
        new = Context(0)
        os.environ["MI_LZ_TEST_OLD_PARTITION"] = "1"            # read when a context is created
        old = Context(0)
        del os.environ["MI_LZ_TEST_OLD_PARTITION"]
        return new, old

    def partmap(ctx, max_blocks):
        f = ctx.L.mi_test_partmap
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        planes = np.zeros((max_blocks, PLANES, PLANE_DW), np.uint32)
        meta = np.zeros((max_blocks, META_DW), np.uint32)
        nb = f(ctx.h, planes.ctypes.data, meta.ctypes.data, max_blocks)
        assert 0 <= nb <= max_blocks, nb
        return planes[:nb], meta[:nb]

    def same_maps(new, old, want_n, what):
        # what the two contexts' last partition launches wrote; returns the blocks' (nparts, fallback)
        (pn, mn), (po, mo) = partmap(new, 8), partmap(old, 8)
        assert len(pn) == len(po) == len(want_n), (what, len(pn), len(po))
        res = []
        for b, n in enumerate(want_n):
            assert int(mn[b][0]) == int(mo[b][0]) == n, (what, b, "n")
            assert np.array_equal(mn[b][:4], mo[b][:4]), (what, b, "n, nparts, base, fallback", mn[b][:4], mo[b][:4])
            k, fb = int(mn[b][1]), int(mn[b][3])
            for f, name in enumerate(("part_start", "part_count", "part_lo")):
                a = 8 + f * MAXPARTS
                assert np.array_equal(mn[b][a:a + k], mo[b][a:a + k]), (what, b, name)
            if not fb:                                           # (a block that falls back has no part map)
                bad = np.flatnonzero(pn[b].reshape(-1) != po[b].reshape(-1))
                assert bad.size == 0, (what, b, "plane dwords differ", bad[:8])
                code = np.zeros(65536, np.uint32)
                bits = np.unpackbits(pn[b].view(np.uint8).reshape(PLANES, PLANE_DW * 4), axis=1, bitorder="little")
                for q in range(PLANES):
                    code |= bits[q].astype(np.uint32) << q
                assert np.all(code[n:] == 127) and np.all(code[:n] < k), (what, b, "codes")
            res.append((k, fb))
        return res

    def text(n, seed):
        return synth.enwik_like(n, seed=seed).numpy()

    def aligned(x):
        d = torch.from_numpy(x).cuda()
        assert d.data_ptr() % 16 == 0
        return d

    def blocks_of(n):
        return [min(65536, n - a) for a in range(0, n, 65536)]

    def oracle_records(data, block=65536):
        d = orc.Deflate(block)
        recs = []
        for at in range(0, len(data), block):
            d.fresh()
            recs.append(orc.defh_encode_block(d.block_encode(data[at:at + block])))
        return np.concatenate(recs)

    def streams_are_the_oracles(data, d, p, ctx, what):
        st = lz.compress(d, p, ctx); ctx.sync()
        assert np.array_equal(st.data[: st.nbytes].cpu().numpy(), orc.deflate_stream(data, p.block, True)[0]), (what, "tokens differ from the oracle's")
        assert np.array_equal(lz.decompress(st, ctx).cpu().numpy(), data), what
        h = lz.compress_h(d, p, ctx); ctx.sync()
        assert np.array_equal(np.frombuffer(h.tobytes(), np.uint8), oracle_records(data, p.block)), (what, "mode H records differ from the oracle's")
        assert np.array_equal(lz.decompress_h(h, ctx).cpu().numpy(), data), what
"""


def _child(body, **env_extra):
    if not os.path.exists(TEST_LIB):
        _lib.build()
    env = dict(os.environ, PYTHONPATH=ROOT, MI_CODEC_LIB=os.path.abspath(TEST_LIB), **env_extra)
    env.pop("MI_LZ_TEST_OLD_PARTITION", None)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(PRELUDE) + textwrap.dedent(body)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


def test_both_kernels_write_the_same_map_and_record():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        for i, n in enumerate(SIZES):
            d = aligned(text(n, 300 + i))
            for ctx in (new, old):
                lz.compress(d, p, ctx); ctx.sync()
            same_maps(new, old, [n], n)
        d = aligned(text(LONG, 399))
        for ctx in (new, old):
            lz.compress(d, p, ctx); ctx.sync()
        parts = same_maps(new, old, blocks_of(LONG), "long")
        assert min(k for k, fb in parts[:3]) > 8 and not any(fb for k, fb in parts), parts
        for flavour, wbits in (("deflate", None), ("lz77", 14), ("lz77", 16)):       # the table sizes, one full and one short block
            d = aligned(text(65536 + 777, 398))
            for ctx in (new, old):
                lz.compress(d, lz.params(flavour, wbits), ctx); ctx.sync()
            r = same_maps(new, old, [65536, 777], (flavour, wbits))
            assert not any(fb for k, fb in r), (flavour, wbits, r)
        for ctx in (new, old):
            assert ctx.order_violations() == 0
            assert ctx.path_stats()["fallback_blocks"] == 0, ctx.path_stats()
        print("ok", parts)
    """)
    assert "ok" in out


def test_both_kernels_with_parts_of_640_entries():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        for n, seed in ((65535, 701), (65536, 700)):
            data = text(n, seed)
            d = aligned(data)
            for ctx in (new, old):
                lz.compress(d, p, ctx); ctx.sync()
            (k, fb), = same_maps(new, old, [n], n)
            assert k > 64 and not fb, (n, k, fb)                             # the seventh plane tells parts apart
            streams_are_the_oracles(data, d, p, new, ("small parts", n))
        assert new.path_stats()["fallback_blocks"] == 0 and old.path_stats()["fallback_blocks"] == 0
        assert new.order_violations() == 0 and old.order_violations() == 0
        print("ok")
    """, MI_LZ_TEST_SMALL_PARTS="1")
    assert "ok" in out


def test_blocks_that_fall_back():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        for name, data in (("zeros", np.zeros(65536, np.uint8)), ("single_symbol", np.full(65536, 0x41, np.uint8))):
            d = aligned(data)
            for ctx in (new, old):
                lz.compress(d, p, ctx); ctx.sync()
            (k, fb), = same_maps(new, old, [65536], name)
            assert fb == 1, (name, "one cluster of 65 536 entries must go to the fallback", k, fb)
            streams_are_the_oracles(data, d, p, new, name)
        assert new.order_violations() == 0 and old.order_violations() == 0
        print("ok")
    """)
    assert "ok" in out


def test_view_one_byte_into_an_allocation_and_three_blocks():
    out = _child("""
        new, old = contexts()
        p = lz.params("deflate")
        data = text(LONG + 1, 397)
        d = aligned(data)
        odd = d[1:]                                                          # not 16-byte aligned: k_lz2_partition on every context
        assert odd.data_ptr() % 16 == 1
        streams_are_the_oracles(data[1:], odd, p, new, "view at +1")
        for ctx in (new, old):
            lz.compress(odd, p, ctx); ctx.sync()
        same_maps(new, old, blocks_of(LONG), "view at +1")
        whole = aligned(data[:LONG].copy())                                  # three full blocks and a short one through the new kernel
        streams_are_the_oracles(data[:LONG], whole, p, new, "three blocks")
        for ctx in (new, old):
            assert ctx.order_violations() == 0
            assert ctx.path_stats()["fallback_blocks"] == 0, ctx.path_stats()
        print("ok")
    """)
    assert "ok" in out
