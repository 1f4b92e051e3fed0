"""CPU tests of the mode-Z oracle (oracle/orc_defz.c): the restatement of include/mi_codec.h ("mode Z") that the GPU
encoder is compared with byte for byte (tests/test_deflate_z_oracle_gpu.py).

They pin what a round trip cannot see: the block type is the shortest form (fixed included, ties in the contract's
order), the limiter keeps codes complete, monotone and near the optimal length-limited cost, the padding of a code with
fewer than two used symbols is zlib's, the tokens are mode T's with the clip, and the output is the committed fixture.
No GPU library is loaded."""
import gzip
import json
import os
import zlib

import numpy as np
import pytest

import defz_cases as D
import rfc1951_tokens as R
from oracle import orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HDR = {"raw": 0, "zlib": 2, "gzip": 10}
CASES = D.cases()


def _inflate(x, container):
    if container == "raw":
        return zlib.decompress(x, -15)
    if container == "zlib":
        return zlib.decompress(x)
    return gzip.decompress(x)


def _blocks(data, block):
    """-> [(byte tokens, block bytes)] of the oracle, fresh table per block"""
    tok, sizes = orc.deflate_stream(data, block, True)
    out, at = [], 0
    for b, s in enumerate(sizes):
        out.append((tok[at:at + int(s)], data[b * block:(b + 1) * block]))
        at += int(s)
    return out


def _tokens(tok):
    """byte tokens -> [(c,)] / [(L, d)]"""
    out, i = [], 0
    while i < len(tok):
        if tok[i] == 0:
            out.append((int(tok[i + 1]),)); i += 2
        else:
            out.append((int(tok[i + 3]), int(tok[i + 1]) | int(tok[i + 2]) << 8)); i += 4
    return out


def _clip(toks, data):
    pos = sum(1 if len(t) == 1 else t[0] for t in toks[:-1])
    t = toks[-1]
    if len(t) == 2 and pos + t[0] > len(data):
        L = len(data) - pos
        return toks[:-1] + ([(L, t[1])] if L >= 3 else [(c,) for c in data[pos:]])
    return toks


def _body_bits(rec):
    """bits of the record's DEFLATE blocks before the sync flush, read with the RFC reader"""
    st = R.read(rec, stop_at_end=False)
    assert st.blocks[-1].btype == 0 and not st.blocks[-1].tokens and rec[-4:] == b"\0\0\xff\xff"
    return st.blocks[-1].start_bit, st


# ---------------------------------------------------------------- streams
@pytest.mark.parametrize("block", D.BLOCKS)
def test_streams_inflate(block):
    for name, data in CASES.items():
        toks = orc.deflate_stream(data, block, True)
        nb = (len(data) + block - 1) // block
        for c in ("raw", "zlib", "gzip"):
            x, bits = orc.defz_stream(data, block, c, tokens=toks)
            assert _inflate(x, c) == data, (name, block, c)
            assert len(bits) == nb + 1 and bits[0] == 8 * HDR[c] and all(v % 8 == 0 for v in bits)
            assert x[bits[-1] // 8: bits[-1] // 8 + 2] == b"\x03\x00"
            assert len(x) == bits[-1] // 8 + 2 + {"raw": 0, "zlib": 4, "gzip": 8}[c]
            if c == "gzip":
                assert x[-8:] == (zlib.crc32(data).to_bytes(4, "little") + (len(data) % 2**32).to_bytes(4, "little"))
            if c == "zlib":
                assert x[:2] == b"\x78\x9c" and x[-4:] == zlib.adler32(data).to_bytes(4, "big")
            for b in range(0, nb, max(1, nb // 7)):                 # restart points
                d = zlib.decompressobj(-15)
                assert d.decompress(x[bits[b] // 8: bits[b + 1] // 8]) == data[b * block:(b + 1) * block], (name, block, b)


def test_checksums_are_zlibs():
    rng = np.random.default_rng(2)
    for n in (0, 1, 3, 5551, 5552, 5553, 65536, 300_001):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert orc.crc32(d) == zlib.crc32(d) and orc.adler32(d) == zlib.adler32(d)
    d = b"\xff" * 1_000_000                                          # Adler-32's sums at their largest
    assert orc.adler32(d) == zlib.adler32(d)


@pytest.mark.parametrize("block", (65536, 4096, 257))
def test_tokens_are_mode_t_clipped(block):
    """every record read back with the RFC reader gives the oracle's mode-T tokens of its block, with the clip"""
    for name, data in sorted(CASES.items()):
        data = data[:70_000] if block >= 4096 else data[:6000]
        for b, (tok, blk) in enumerate(_blocks(data, block)):
            rec, info = orc.defz_record(tok, blk)
            _, st = _body_bits(rec)
            assert st.data == blk
            want = _clip(_tokens(tok), blk)
            if info["type"] != 0:
                assert st.tokens == want, (name, block, b)
            clipped = want != _tokens(tok)
            assert bool(info["clip"]) == clipped


def test_clip_both_kinds():
    block = 4096
    data = D.clip_blocks(block)
    for b, (keep, (tok, blk)) in enumerate(zip((1, 2, 3, 4), _blocks(data, block))):
        rec, info = orc.defz_record(tok, blk)
        assert info["clip"] == keep and info["type"] == 2
        got = R.read(rec, stop_at_end=False).tokens
        assert got == _clip(_tokens(tok), blk)
        if keep < 3:
            assert got[-keep:] == [(c,) for c in blk[-keep:]]
        else:
            assert got[-1] == (keep, _tokens(tok)[-1][1])


# ---------------------------------------------------------------- the block type
def _forms(tok, blk):
    rec, info = orc.defz_record(tok, blk)
    forms = {}
    for t in (2, 1, 0):
        r, _ = orc.defz_record(tok, blk, force=t)
        d = zlib.decompressobj(-15)
        assert d.decompress(r) == bytes(blk), t
        forms[t] = (r, _body_bits(r)[0])
    return rec, info, forms


def _check_shortest(tok, blk):
    rec, info, forms = _forms(tok, blk)
    sizes = {2: forms[2][1], 1: forms[1][1], 0: forms[0][1]}
    assert (sizes[2], sizes[1], sizes[0]) == (info["dyn_bits"], info["fix_bits"], info["sto_bits"])
    best = min(sizes.values())
    assert info["type"] == max(t for t in sizes if sizes[t] == best)      # ties: dynamic > fixed > stored
    assert rec == forms[info["type"]][0]
    return info


def test_block_type_is_the_shortest_form():
    seen = {0: 0, 1: 0, 2: 0}
    for name in ("text1m", "zeros", "random", "period3", "period16385", "tail_zeros", "size1", "size2", "size3", "size5",
                 "size65537"):
        data = CASES[name]
        for block in (1000, 257):
            for tok, blk in _blocks(data[:3 * block + 17], block):
                seen[_check_shortest(tok, blk)["type"]] += 1
    rng = np.random.default_rng(5)
    for n in (6, 10, 20, 40, 80, 160):                                 # short blocks of few distinct symbols
        for k in (1, 2, 4, 16):
            blk = rng.integers(0, k, n, dtype=np.uint8) + 97
            for tok, b in _blocks(blk.tobytes(), 65536):
                seen[_check_shortest(tok, b)["type"]] += 1
    assert seen[1] > 0, "no block where fixed Huffman is the shortest"
    assert seen[0] > 0 and seen[2] > 0, seen


def _tie_fixed_stored():
    """a literal-only block of distinct bytes, 30 of them >= 144 (9-bit fixed codes), the rest < 144 (8 bits): fixed
    costs 3 + 8 n + 30 + 7 = 8 n + 40 bits, exactly the stored form.  The smallest such block where dynamic is longer."""
    rng = np.random.default_rng(1)
    hi = rng.permutation(np.arange(144, 256))[:30]
    for m in range(0, 144):
        blk = np.concatenate([hi, rng.permutation(np.arange(0, 144))[:m]]).astype(np.uint8)
        rng.shuffle(blk)
        (tok, b), = _blocks(blk.tobytes(), 65536)
        _, info = orc.defz_record(tok, b)
        if info["dyn_bits"] > info["fix_bits"]:
            return tok, b, info
    raise AssertionError("no block with dynamic above the fixed / stored tie")


def test_tie_fixed_and_stored_goes_to_fixed():
    tok, blk, info = _tie_fixed_stored()
    assert info["fix_bits"] == info["sto_bits"] == 8 * len(blk) + 40 and info["dyn_bits"] > info["fix_bits"]
    assert _check_shortest(tok, blk)["type"] == 1


# ---------------------------------------------------------------- code lengths
def _random_tallies(nsym, count, rng, skew):
    for _ in range(count):
        f = np.floor(2.0 ** rng.uniform(0, skew, nsym)).astype(np.uint32) * (rng.random(nsym) < rng.uniform(0.2, 1.0))
        yield f.astype(np.uint32)


def test_heap_without_limiter_is_mode_hs():
    rng = np.random.default_rng(7)
    n = 0
    for f in _random_tallies(286, 200, rng, 10):
        if np.count_nonzero(f) < 2:
            continue
        want = orc.defh_lengths(f)
        if want.max() > 15:
            continue
        got, fired = orc.defz_lengths(f, 15)
        assert not fired and np.array_equal(got, want)
        n += 1
    for k in range(8):                                                # real tallies
        data = np.frombuffer(D.text(65536, seed=k + 1), np.uint8)
        _, freq = orc.Deflate(65536).block_encode(data, want_freq=True)
        got, fired = orc.defz_lengths(freq, 15)
        assert not fired and np.array_equal(got, orc.defh_lengths(freq))
        n += 1
    assert n > 150


def _package_merge(freq, limit):
    """optimal length-limited code lengths (package-merge) over the nonzero frequencies -> cost sum f * len"""
    items = sorted((int(f), i) for i, f in enumerate(freq) if f)
    if len(items) < 2:
        return sum(f for f, _ in items)
    leaves = [(f, (i,)) for f, i in items]
    cur = list(leaves)
    for _ in range(limit - 1):
        pk = [(cur[j][0] + cur[j + 1][0], cur[j][1] + cur[j + 1][1]) for j in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda t: t[0])
    ln = {}
    for _, syms in cur[:2 * len(items) - 2]:
        for s in syms:
            ln[s] = ln.get(s, 0) + 1
    return sum(f * ln[i] for f, i in items)


def _fib_tally(nsym, k, rng):
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    f = np.zeros(nsym, np.uint32)
    f[rng.permutation(nsym)[:k]] = fib[:k]
    return f


# the largest (cost - optimum) / optimum of the limited code seen on the tallies below: 0.27 % at limit 15 (both
# alphabets), 11.0 % at limit 7 (extreme Fibonacci tallies); the bounds leave a little room
MAX_EXCESS = {15: 0.005, 7: 0.12}


@pytest.mark.parametrize("nsym,limit", [(286, 15), (30, 15), (19, 7)])
def test_limiter(nsym, limit):
    rng = np.random.default_rng(nsym * 100 + limit)
    tallies = list(_random_tallies(nsym, 150, rng, 24 if limit == 15 else 12))
    tallies += [_fib_tally(nsym, k, rng) for k in range(limit + 2, min(nsym, 28) + 1) for _ in range(3)]
    fired, worst = 0, 0.0
    for f in tallies:
        if np.count_nonzero(f) < 2:
            continue
        unl, _ = orc.defz_lengths(f, 40)
        got, fl = orc.defz_lengths(f, limit)
        assert fl == (unl.max() > limit)
        assert ((got > 0) == (f > 0)).all()
        assert got.max() <= limit
        num, den = R.kraft([int(v) for v in got])
        assert num == den, "incomplete or over-subscribed code"
        # lengths do not increase as the unlimited length goes down (order: unlimited length, then symbol)
        order = sorted((int(unl[s]), s) for s in range(nsym) if f[s])
        new = [int(got[s]) for _, s in order]
        assert new == sorted(new)
        cost = int((f.astype(np.int64) * got).sum())
        opt = _package_merge(f, limit)
        assert cost >= opt
        if fl:
            fired += 1
            worst = max(worst, (cost - opt) / opt)
        else:
            assert cost == int((f.astype(np.int64) * unl).sum())
    assert fired >= 20, fired
    assert worst <= MAX_EXCESS[limit], worst


def test_padding_rule():
    """fewer than two used symbols: two codes of length 1 as zlib's build_tree pads (none -> 0 and 1; s -> s and s + 1
    when s < 2, else s and 0)"""
    for nsym, limit in ((30, 15), (19, 7), (286, 15)):
        ln, fired = orc.defz_lengths(np.zeros(nsym, np.uint32), limit)
        assert not fired and ln.tolist() == [1, 1] + [0] * (nsym - 2)
        for s in (0, 1, 2, 5, nsym - 1):
            f = np.zeros(nsym, np.uint32)
            f[s] = 9
            ln, _ = orc.defz_lengths(f, limit)
            other = s + 1 if s < 2 else 0
            assert sorted(np.nonzero(ln)[0].tolist()) == sorted([s, other]) and ln[s] == 1 and ln[other] == 1


def _zlib_dynamic(data, strategy):
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
    st = R.read(co.compress(data) + co.flush())
    return [b for b in st.blocks if b.btype == 2]


def test_padding_against_zlib():
    # no distance used: zlib's Huffman-only strategy codes literals only
    text = D.text(20_000, seed=3)
    blocks = _zlib_dynamic(text, zlib.Z_HUFFMAN_ONLY)
    assert blocks
    want, _ = orc.defz_lengths(np.zeros(30, np.uint32), 15)
    for b in blocks:
        assert b.dist_lengths + [0] * (30 - len(b.dist_lengths)) == want.tolist()
    (tok, blk), = _blocks(D.skewed_block(), 65536)                    # the oracle's record of a literal-only block
    rec, info = orc.defz_record(tok, blk)
    st = R.read(rec, stop_at_end=False)
    assert info["type"] == 2 and all(len(t) == 1 for t in st.tokens) and st.blocks[0].dist_lengths == [1, 1]
    # only distance 1 (code 0) used: zlib's run-length strategy
    rng = np.random.default_rng(4)
    runs = np.repeat(rng.integers(0, 256, 4000, dtype=np.uint8), rng.integers(1, 9, 4000)).tobytes()
    blocks = _zlib_dynamic(runs, zlib.Z_RLE)
    assert blocks
    f = np.zeros(30, np.uint32)
    f[0] = 1
    want, _ = orc.defz_lengths(f, 15)
    for b in blocks:
        used = sum(1 for t in b.tokens if len(t) == 2)
        assert used and all(t[1] == 1 for t in b.tokens if len(t) == 2)
        assert b.dist_lengths + [0] * (30 - len(b.dist_lengths)) == want.tolist()


# ---------------------------------------------------------------- crafted limiter blocks
@pytest.mark.parametrize("name,flag", [("skewed", "lim_ll"), ("cl_limit", "lim_cl"), ("dist_limit", "lim_dc")])
def test_crafted_blocks_take_the_limiter(name, flag):
    data = {"skewed": D.skewed_block, "cl_limit": D.cl_limit_block, "dist_limit": D.dist_limit_block}[name]()
    (tok, blk), = _blocks(data, 65536)
    rec, info = orc.defz_record(tok, blk)
    assert info[flag] == 1 and info["type"] == 2, info
    st = R.read(rec, stop_at_end=False)
    k = st.blocks[0]
    lens = {"lim_ll": k.lit_lengths, "lim_dc": k.dist_lengths, "lim_cl": k.cl_lengths}[flag]
    assert max(lens) == (7 if flag == "lim_cl" else 15)
    for ls in (k.lit_lengths, k.dist_lengths, k.cl_lengths):
        num, den = R.kraft(ls)
        assert num == den
    assert st.data == blk and st.tokens == _clip(_tokens(tok), blk)


# ---------------------------------------------------------------- fixture
def test_fixture():
    """the oracle's output on the golden inputs is the committed tests/golden/defz.json"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_defz", os.path.join(os.path.dirname(GOLD), "..", "oracle",
                                                                                  "gen_golden_defz.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(GOLD, "defz.json")))
    assert gen.build() == want
