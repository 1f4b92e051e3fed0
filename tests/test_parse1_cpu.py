"""Mode Z's parse 1 on the CPU: the restated rule (tests/parse1_cases.py) gives valid, smaller streams; the public hook
(the sixth field of the parameters) exists and leaves the bounds alone; and the resource budget of the parse-1
instantiations of k_lz_parse_emit (compiled for gfx950, not run)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import dict_cases
import parse1_cases as P
from compression_algorithms_amd import _lib, lz
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compression_algorithms_amd", "csrc")
CASES = P.cases()
ZDICTS = (300, 40000)


@pytest.mark.parametrize("block", P.BLOCKS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_streams_inflate_and_matches_stay_inside(name, block):
    data = CASES[name]
    for a in range(0, len(data), block):
        blk = data[a:a + block]
        at = 0
        for p, ln, d in P.walk(blk):
            assert p == at and (ln == 0 or 3 <= ln <= 255) and p + max(ln, 1) <= len(blk) and (ln == 0 or 1 <= d <= p), (name, a, p, ln, d)
            at = p + max(ln, 1)
        assert at == len(blk)
    for c in P.CONTAINERS:
        out, bits = P.expected_z(data, block, c)
        assert P.inflate(out, c) == data, (name, c)
        assert len(bits) == (len(data) + block - 1) // block + 1
    if block in P.BGZF_BLOCKS:
        out, table = P.expected_bgzf(data, block)
        assert P.inflate(out, "gzip") == data


@pytest.mark.parametrize("block", (65536, 1000))
@pytest.mark.parametrize("dl", ZDICTS)
def test_expected_items_inflate_with_the_dictionary(dl, block):
    zd = dict_cases.dictionary(dl)
    for k, item in enumerate(P.batch_items() + [zd[-700:], dict_cases.text(50000)[300:300 + block + 17]]):
        for c in dict_cases.CONTAINERS:
            assert dict_cases.stock_inflate(P.expected_item(item, zd, block, c), c, zd) == item, (k, c)


def test_the_crafted_cases_are_what_they_claim():
    w = P.walk(P.chunk_offset_63())
    assert (P.MATCH_AT, 255, P.MATCH_AT) in w and P.MATCH_AT % 64 == 63
    e = P.ends_at_n()
    assert P.walk(e)[-1] == (len(e) - 100, 100, len(e) - 100)
    r = P.rising()
    l0, _ = P.len0(r)
    a = P.RISING_AT
    assert list(l0[a:a + 5]) == [4, 5, 8, 21, 20]
    assert [t[:2] for t in P.walk(r) if a <= t[0] <= a + 3] == [(a, 0), (a + 1, 0), (a + 2, 0), (a + 3, 21)]
    z = P.walk(bytes(70_000)[:65536])
    assert max(ln for _, ln, _ in z) == 255 and sum(max(ln, 1) for _, ln, _ in z) == 65536


@pytest.mark.parametrize("name", ("golden300k", "zeros", "mixed"))
def test_parse1_is_shorter_than_parse0(name):
    data = {"golden300k": P.golden_text(), "zeros": CASES["zeros"], "mixed": CASES["mixed"]}[name]
    lazy, greedy = P.expected_z(data, 65536, "zlib")[0], orc.defz_stream(data, 65536, "zlib")[0]
    print(f"{name}: {len(data)} bytes -> parse 0 {len(greedy)}, parse 1 {len(lazy)}")
    assert len(lazy) < len(greedy)


def test_params_carry_the_parse():
    assert lz.params("deflate", parse=1).parse == 1 and lz.params("deflate").parse == 0
    assert lz.params("deflate", block=4096, parse=1).block == 4096
    p = _lib.LzParams(15, 5, 20, 1, 65536)                                      # the five-positional form: parse 0
    assert p.parse == 0 and C.sizeof(_lib.LzParams) == 24


def test_bounds_do_not_depend_on_the_parse():
    L = _lib.lib()
    for block in P.BLOCKS:
        p0, p1 = lz.params("deflate", block=block), lz.params("deflate", block=block, parse=1)
        for n in (0, 1, block - 1, block, block + 1, 10 * block + 7, 10 ** 9):
            for c in (0, 1, 2):
                assert L.mi_deflate_z_bound_bytes(n, C.byref(p1), c) == L.mi_deflate_z_bound_bytes(n, C.byref(p0), c)
                assert L.mi_deflate_batch_bound_bytes(n, C.byref(p1), c) == L.mi_deflate_batch_bound_bytes(n, C.byref(p0), c)
            assert L.mi_bgzf_bound_bytes(n, C.byref(p1)) == L.mi_bgzf_bound_bytes(n, C.byref(p0))


# ---- resources of k_lz_parse_emit (in the manner of tests/test_find_budget.py) ----------------------------------------------------
def _hipcc():
    p = shutil.which("hipcc")
    if p:
        return p
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    return p if os.access(p, os.X_OK) else None


@pytest.fixture(scope="module")
def emit_usage(tmp_path_factory):
    """{(DESC, DICT, PARSE): resource remarks} of every k_lz_parse_emit instantiation"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("budget") / "lz_emit.o"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-ffp-contract=off",
           "--cuda-device-only", "-c", os.path.join(CSRC, "lz_emit.hip"), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    usage, fn = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            k = re.fullmatch(r"_Z15k_lz_parse_emitILb([01])ELb([01])ELi([01])EE.*", m.group(1))
            fn = tuple(int(v) for v in k.groups()) if k else None
            if fn is not None:
                usage[fn] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and fn is not None:
            usage[fn][m.group(1)] = int(m.group(2))
    assert sorted(usage) == [(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)], sorted(usage)
    for k in sorted(usage):
        print("k_lz_parse_emit<DESC, DICT, PARSE> =", k, usage[k])
    return usage


@pytest.mark.parametrize("inst", ((0, 0, 1), (1, 0, 1), (1, 1, 1)))
def test_parse1_instantiations_fit_and_do_not_spill(emit_usage, inst):
    u = emit_usage[inst]
    assert u["LDS Size"] <= 163840
    assert u["ScratchSize"] == 0
    assert u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0


@pytest.mark.parametrize("inst", ((0, 0, 0), (1, 0, 0), (1, 1, 0)))
def test_parse0_instantiations_keep_their_budget(emit_usage, inst):
    u = emit_usage[inst]
    assert u["LDS Size"] <= 163840
    assert u["ScratchSize"] == 0
