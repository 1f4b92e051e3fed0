"""What tests/stream_cases.py takes for granted, checked without a GPU: the poison really differs from the data where the
harness says it does, an encoder fed the poison writes another stream than for the data (so a fork that does not wait shows),
stock zlib refuses the zero poison in all three containers, the shapes take the paths they are named after, and the delay rule
is the one the GPU file documents."""
import gzip
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import stream_cases as sc

RECIPES = sorted({c[2] for c in sc.ENCODER_CASES})


@pytest.mark.parametrize("recipe", RECIPES, ids=lambda r: f"{r[0]}-{r[1]}")
def test_poison_differs_in_every_64_byte_line(recipe):
    data = sc.make(recipe)
    p = sc.data_poison(data)
    assert p.size == data.size and p.dtype == np.uint8
    pad = (-data.size) % 64
    diff = np.concatenate([p != data, np.zeros(pad, dtype=bool)]).reshape(-1, 64)
    assert diff.any(axis=1).all()
    assert np.array_equal(p, sc.data_poison(data)), "the poison is fixed"


@pytest.mark.parametrize("case", sc.ENCODER_CASES, ids=lambda c: c[0])
def test_the_oracle_tells_poison_from_data(case):
    """the stream (and with it every table entry behind the first, and the size) differs between data and poison: a call
    that read the poison cannot pass"""
    name, kind, recipe, block, wbits, container = case
    data = sc.make(recipe)
    want = sc.expected(kind, recipe, block, wbits, container)
    other = sc.expected_of(kind, sc.data_poison(data), block, wbits, container)
    main = {"FIND": "cand", "HUFF": "words", "FSE": "records", "CRC": "value", "ADLER": "value"}.get(kind, "out")
    assert want[main] != other[main], name
    if "bits" in want and kind != "HUFF" and kind != "OLD":
        assert want["bits"][0] == other["bits"][0] and want["bits"][1:] != other["bits"][1:], name
        assert all(a != b for a, b in zip(want["bits"][1:], other["bits"][1:])), name
    elif "bits" in want:
        assert want["bits"] != other["bits"], name
    if "nbytes" in want:
        assert want["nbytes"] != other["nbytes"], name


def test_expected_streams_are_what_stock_tools_read():
    for name, kind, recipe, block, wbits, container in sc.ENCODER_CASES:
        want, data = sc.expected(kind, recipe, block, wbits, container), sc.make(recipe).tobytes()
        if kind == "Z":
            assert zlib.decompress(want["out"], {"raw": -15, "zlib": 15, "gzip": 31}[container]) == data, name
            assert want["nbytes"] == len(want["out"]) and len(want["bits"]) == (len(data) + block - 1) // block + 1
        if kind == "BGZF":
            assert gzip.decompress(want["out"]) == data, name
            so, oo = B.walk(want["out"])
            assert [8 * v for v in so[:-1]] == want["bits"] and oo[-1] == len(data), name
        if kind in ("T", "L", "H"):
            assert len(want["bits"]) == (len(data) + block - 1) // block + 1 and want["bits"][0] == 0
            assert (want["bits"][-1] + 7) // 8 == len(want["out"]), name


@pytest.mark.parametrize("wbits", [-15, 15, 31])
@pytest.mark.parametrize("n", [2, 18, 28, 1000, 70_000])
def test_zlib_refuses_the_zero_poison(wbits, n):
    with pytest.raises(zlib.error):
        d = zlib.decompressobj(wbits)
        d.decompress(bytes(sc.zero_poison(bytes(n))))
        if not d.eof:
            raise zlib.error("the stream never ends")


def test_shapes_take_the_paths_they_are_named_after():
    blocks = lambda recipe, block: (recipe[1] + block - 1) // block
    assert blocks(sc.SOLO, 65536) == 4 and blocks(sc.SOLO_PAGES, 65536) == 4                                  # one batch without MI_LZ_BATCH
    assert blocks(sc.PIPE, 65536) == 14 and blocks(sc.PIPE_BGZF, 65280) == 14 and -(-14 // 3) == 5 > 3   # five batches, three sets
    assert blocks(sc.SHORT, 65536) == 3                                 # one batch of three: no pipeline
    assert blocks(sc.PAGES, 65536) == 64 and blocks(sc.FB_A, 65536) > 2 * 16 and blocks(sc.FB_B, 65536) > 2 * 16
    assert blocks(sc.WIDE, 262144) == 4
    assert len({c[0] for c in sc.ENCODER_CASES}) == len(sc.ENCODER_CASES)
    freq, stand_in = sc.fse_histograms()
    assert (freq != stand_in).any() and int(freq.sum()) == sc.WHOLE[1]


def test_delay_rule_and_chain():
    assert sc.delay_for(0.0) == 5.0 and sc.delay_for(0.001) == 5.0 and sc.delay_for(0.01) == 40.0 and sc.delay_for(1.0) == 250.0
    ran = []
    f = lambda rc: (lambda: ran.append(rc) or rc)
    assert sc.chain(f(0), f(0))() == 0 and ran == [0, 0]
    assert sc.chain(f(0), f(4), f(0))() == 4 and ran == [0, 0, 0, 4], "the chain stops at the first status that is not MI_OK"
