"""k_lz2_prefix (lz2_find.hip): the insert-only prefix of every plain exported cluster of 128..1024 entries is
placed and answered in bulk, and k_lz2_rows / k_lz2_big start their replay behind it.  The streams must stay the oracle's with the
prefix on (default), off (MI_LZ_PREFIX=0) and on the wave replay alone (MI_LZ_ROWS=0: two wave classes instead of three), for
deflate (W = 32 KiB) and the shipped lz77 window (W = 16 KiB); the test build's counters (mi_test_prefix_stats) show that the
replays really started from a prefix; and the switch changes no byte.

Inputs (at most 8 blocks each): text, a ten-symbol alphabet, the "phrases" and "runs" families, a block of exactly 65 536 bytes
and one of 32 768 + 9 (clusters with a single retirement), and CRAFTED blocks: one word X at even spacing over random filler
plus about k / 12 foreign words whose homes lie 1..k / 2 buckets above X's, each inserted once per half of the block, sized so
that X's cluster has exactly k entries for k at every class edge (scripts/cluster_census.py checks that on the CPU first).
Reference behaviour emulated: algorithms/lz77/lz77.c:55-108, algorithms/deflate/lz77.c:77-174."""
import importlib.util
import os

import numpy as np
import pytest

from test_fallback_chain_gpu import ROOT, TEST_LIB, _child

pytestmark = pytest.mark.gpu

CRAFTED_K = (130, 255, 256, 300, 511, 512, 700, 1024)


def _census():
    spec = importlib.util.spec_from_file_location("cluster_census", os.path.join(ROOT, "scripts", "cluster_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def crafted_block(k, tbits=20):
    """65 536 bytes whose word X lives in a mixed, plain, non-quiet cluster of exactly k entries -> (block, that cluster).
    X stands k - 2 nf times at even spacing; nf = k / 12 foreign words with homes 1..k / 2 above X's stand once in each half of the
    block: all but one in a clump behind the half's second X (long runs of X follow), one where — as far as the spacing allows
    (k = 130, 300, 700, 1024) — it is the first entry of the 16-entry pass that holds `pre`.  Filler words that would fall into the cluster's buckets by chance are redrawn."""
    cen = _census()
    rng = np.random.default_rng(4000 + k)
    tmask = np.uint32((1 << tbits) - 1)
    while True:                                                    # X's cluster away from bucket 0 / T
        x = rng.integers(0, 1 << 32, size=1, dtype=np.uint64).astype(np.uint32)
        hx = int(cen.mix32(x)[0] & tmask)
        if 8192 < hx < (1 << tbits) - 8192:
            break
    nf = max(1, k // 12)
    pool = rng.integers(0, 1 << 32, size=1 << 22, dtype=np.uint64).astype(np.uint32)
    hp = (cen.mix32(pool) & tmask).astype(np.int64)
    foreign = pool[(hp > hx) & (hp <= hx + k // 2)][:nf]
    assert len(foreign) == nf, (k, len(foreign))
    blk = rng.integers(0, 256, size=65536, dtype=np.uint8)
    fixed = np.zeros(65536, bool)

    def put(at, w):
        for b in range(4):
            blk[at + b] = (int(w) >> (8 * b)) & 0xFF
        fixed[at:at + 4] = True

    nx = k - 2 * nf
    step = 65536 // nx
    xpos = 16 + step * np.arange(nx)
    for at in xpos:
        put(int(at), x[0])
    nxh = int(np.searchsorted(xpos, xpos[0] + 32768, side="right"))        # X inside the prefix (W = 32 KiB)
    pre = nxh + nf
    g0 = min(max((pre & ~15) - nf, nf + 2), nxh - 2)              # its foreign word is entry number g0 + nf: the first of pre's pass
    for j, w in enumerate(foreign):
        put(int(xpos[g0 if j == 0 else 1 + j]) + step // 2, w)
        put(int(xpos[nxh + 1 + j]) + step // 2, w)
    for _ in range(200):                                           # no other word in or next to the cluster's buckets
        h = (cen.mix32(cen.words_of(blk)) & tmask).astype(np.int64)
        bad = np.flatnonzero((h >= hx - 64) & (h <= hx + k + 64))
        bad = [q for q in bad if not fixed[q:q + 4].all()]
        if not bad:
            break
        for q in bad:
            free = [q + b for b in range(4) if q + b < 65536 and not fixed[q + b]]
            blk[free[0]] = rng.integers(0, 256)
    mine = [c for c in cen.block_clusters(blk, tbits, 15) if (c["word"] == x[0]).any()]
    assert len(mine) == 1
    c = mine[0]
    assert len(c["pos"]) == k and c["mixed"] and not c["quiet"] and not c["covers_zero"], (k, len(c["pos"]))
    assert c["pre"] == pre and (c["word"] != x[0]).sum() == 2 * nf, (k, c["pre"], pre)
    return blk, c


COMMON = """
    import sys, ctypes as C
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    from test_prefix_replay_gpu import crafted_block, CRAFTED_K

    def inputs(group):
        if group == "text":
            return [("text", synth.enwik_like(6 * 65536 - 777, seed=91).numpy())]
        if group == "low":
            rng = np.random.default_rng(5)
            return [("low", rng.choice(np.frombuffer(b"abcdefgh \\n", np.uint8), size=4 * 65536,
                                       p=[.3, .2, .1, .1, .05, .05, .05, .05, .05, .05]).astype(np.uint8))]
        if group == "families":
            return [(f, np.asarray(synth.family(f, 77, 4 * 65536))) for f in ("phrases", "runs")]
        if group == "edges":
            t = synth.enwik_like(2 * 65536, seed=92).numpy()
            return [("one block", t[:65536]), ("half a block + 9", t[65536:65536 + 32768 + 9])]
        assert group == "crafted"
        return [(f"k={k}", crafted_block(k)[0]) for k in CRAFTED_K]

    def check(ctx, name, data):
        for p in (lz.params("deflate"), lz.params("lz77", 14)):
            st = lz.compress(data, p, ctx)
            ctx.sync()
            assert oracle_equal(st, data, p), (name, "stream differs from the oracle")
            assert np.array_equal(lz.decompress(st, ctx).cpu().numpy(), data), name

    def prefix_stats(ctx):
        f = ctx.L.mi_test_prefix_stats
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        out = (C.c_uint64 * 2)()
        assert f(ctx.h, out, 1) == 1
        return int(out[0]), int(out[1])
"""

PARITY = COMMON + """
    ctx = Context(0)
    for name, data in inputs(GROUP):
        check(ctx, name, data)
    assert ctx.order_violations() == 0
    print("ok")
"""


@pytest.mark.parametrize("group", ["text", "low", "families", "edges", "crafted"])
@pytest.mark.parametrize("env", [{}, {"MI_LZ_PREFIX": "0"}, {"MI_LZ_ROWS": "0"}], ids=["default", "prefix_off", "rows_off"])
def test_streams_equal_the_oracle(env, group):
    assert "ok" in _child(PARITY.replace("GROUP", repr(group)), **env)


def test_replays_start_from_the_prefix():
    """test build: at least one cluster per block of text and of every crafted block starts from a precomputed prefix (the census
    gives 22 per block of text); with MI_LZ_PREFIX=0 nothing does"""
    out = _child(COMMON + """
    ctx = Context(0)
    p = lz.params("deflate")
    prefix_stats(ctx)
    (name, text), = inputs("text")
    lz.compress(text, p, ctx); ctx.sync()
    cl, en = prefix_stats(ctx)
    print("text", cl, en)
    assert cl >= 6 and en > 0, (cl, en)
    for name, data in inputs("crafted"):
        lz.compress(data, p, ctx); ctx.sync()
        cl, en = prefix_stats(ctx)
        print(name, cl, en)
        assert cl >= 1 and en > 0, (name, cl, en)
    os.environ["MI_LZ_PREFIX"] = "0"
    for name, data in [(name, text)] + inputs("crafted")[:2]:
        lz.compress(data, p, ctx); ctx.sync()
        assert prefix_stats(ctx) == (0, 0), name
    assert ctx.order_violations() == 0
    print("ok")
    """, MI_CODEC_LIB=os.path.abspath(TEST_LIB))
    assert "ok" in out


def test_the_switch_changes_no_byte():
    out = _child(COMMON + """
    ctx = Context(0)
    (name, text), = inputs("text")
    for p in (lz.params("deflate"), lz.params("lz77", 14)):
        os.environ.pop("MI_LZ_PREFIX", None)
        a = lz.compress(text, p, ctx); ctx.sync()
        os.environ["MI_LZ_PREFIX"] = "0"
        b = lz.compress(text, p, ctx); ctx.sync()
        assert a.nbytes == b.nbytes and torch.equal(a.data[: a.nbytes], b.data[: b.nbytes])
        assert torch.equal(a.block_bits, b.block_bits)
    print("ok")
    """)
    assert "ok" in out
