"""Mode Z's parse 1 on the GPU (mi_lz_params.parse = MI_PARSE_LAZY): every stream byte for byte what the CPU restatement of
the rule gives (tests/parse1_cases.py over the oracle's candidates and record writer), through mode Z, BGZF, the batched
deflate with and without a preset dictionary and the host forms; read back by stock zlib / gzip and by the library's own
inflaters; on a caller's stream with late input; over several pipeline batches; every refused combination; and parse 0
in the same process still the oracle's."""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch

import dict_cases
import parse1_cases as P
import stream_cases as sc
from compression_algorithms_amd import _lib, lz
from compression_algorithms_amd.context import default_context
from oracle import orc

pytestmark = pytest.mark.gpu

CASES = P.cases()
OK, ARG, CAPACITY = 0, 1, 4
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    return default_context()


def _p(block=65536, parse=1):
    return lz.params("deflate", block=block, parse=parse)


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


# ---- mode Z --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", P.BLOCKS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_compress_z_is_the_restated_rule(ctx, name, block):
    data = CASES[name]
    for c in P.CONTAINERS:
        want, wbits = P.expected_z(data, block, c)
        st = lz.compress_z(data, _p(block), c, ctx=ctx)
        got, gbits = st.tobytes(), [int(v) for v in st.block_bits.cpu()]
        assert got == want and gbits == wbits, (f"{name} block {block} {c}: {len(got)} vs {len(want)} bytes, first byte differing at "
                                               f"{_first_diff(got, want)}")
        assert P.inflate(got, c) == data
        assert lz.decompress_z(st, ctx=ctx).cpu().numpy().tobytes() == data
        assert lz.inflate(got, len(data), wbits, block, c, ctx=ctx).cpu().numpy().tobytes() == data


@pytest.mark.parametrize("name", ("text", "zeros", "mixed", "text_3", "zeros_1"))
def test_compress_z_host_form(ctx, name):
    data = CASES[name]
    for block, c in ((65536, "gzip"), (1000, "zlib")):
        got, bits = lz.compress_z_host(data, _p(block), c, ctx=ctx)
        assert (got, bits) == P.expected_z(data, block, c), (name, block, c)


# ---- BGZF ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", P.BGZF_BLOCKS)
@pytest.mark.parametrize("name", ("text", "zeros", "period3", "mixed", "chunk_offset_63", "rising", "text_1", "zeros_4"))
def test_compress_bgzf_is_the_restated_rule(ctx, name, block):
    data = CASES[name]
    want, wtable = P.expected_bgzf(data, block)
    st = lz.compress_bgzf(data, _p(block), ctx=ctx)
    got = st.tobytes()
    assert got == want and [int(v) for v in st.member_bits.cpu()] == wtable, (name, block, _first_diff(got, want))
    assert gzip.decompress(got) == data
    assert lz.decompress_bgzf(got, ctx=ctx).cpu().numpy().tobytes() == data
    so, oo = lz.bgzf_index(got, ctx=ctx)
    nb = (len(data) + block - 1) // block
    assert [int(v) * 8 for v in so.cpu()][: nb + 1] == wtable and int(oo.cpu()[-1]) == len(data)
    host, htable = lz.compress_bgzf_host(data, _p(block), ctx=ctx)
    assert host == want and htable == wtable


# ---- the batched deflate ---------------------------------------------------------------------------------------------------------------
def _packed(items, lead=3):
    """one buffer with `lead` bytes in front and the items back to back (no alignment), and its offsets"""
    buf = bytes(lead) + b"".join(items)
    offs = np.concatenate([[lead], lead + np.cumsum([len(x) for x in items])]).tolist()
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8), offs


@pytest.mark.parametrize("container", P.CONTAINERS)
@pytest.mark.parametrize("block", (65536, 1000))
def test_deflate_batch_items_are_compress_z(ctx, block, container):
    items = P.batch_items() + [CASES["zeros"][:65536 + 5], CASES["text"][:2 * 65536 + 1]] * (block == 65536)
    p = _p(block)
    d = lz.deflate_batch(items, p, container, ctx=ctx).raise_for_status()
    got = [o.cpu().numpy().tobytes() for o in d.outputs]
    for k, (x, g) in enumerate(zip(items, got)):
        assert g == P.expected_z(x, block, container)[0], (k, len(x))
        assert g == lz.compress_z(x, p, container, ctx=ctx).tobytes(), k
        assert P.inflate(g, container) == x
    buf, offs = _packed(items)
    d2 = lz.deflate_batch((buf.to(ctx.device), offs), p, container, ctx=ctx).raise_for_status()
    assert [o.cpu().numpy().tobytes() for o in d2.outputs] == got
    host, st = lz.deflate_batch_host(items, p, container, ctx=ctx)
    assert st == [OK] * len(items) and host == got


@pytest.mark.parametrize("container", dict_cases.CONTAINERS)
@pytest.mark.parametrize("block,dl", ((65536, 300), (65536, 40000), (1000, 300), (1000, 40000)))
def test_deflate_batch_with_a_dictionary(ctx, block, dl, container):
    zd = dict_cases.dictionary(dl)
    items = P.batch_items() + [zd[-700:], dict_cases.text(50000)[300:300 + block + 17]]
    p = _p(block)
    buf, offs = _packed(items, lead=5)
    d = lz.deflate_batch((buf.to(ctx.device), offs), p, container, ctx=ctx, zdict=zd).raise_for_status()
    got = [o.cpu().numpy().tobytes() for o in d.outputs]
    for k, (x, g) in enumerate(zip(items, got)):
        want = P.expected_item(x, zd, block, container)
        assert g == want, (k, len(x), len(g), len(want), _first_diff(g, want))
        assert dict_cases.stock_inflate(g, container, zd) == x, k
    host, st = lz.deflate_batch_host(items, p, container, ctx=ctx, zdict=zd)
    assert st == [OK] * len(items) and host == got


@pytest.mark.parametrize("short", (1, 7))
def test_deflate_batch_capacity(ctx, short):
    """an item whose buffer is `short` bytes too small: MI_ERR_CAPACITY, the size it needs, and not a byte at or past its capacity"""
    block, container = 1000, "zlib"
    items = [CASES["mixed"][:3017], CASES["text"][:2500], bytes(1500), CASES["text"][5000:5100]]
    p, c = _p(block), lz.CONTAINERS[container]
    want = [P.expected_z(x, block, container)[0] for x in items]
    victim = 1
    caps = [lz.bound_bytes_z(len(x), p, c) for x in items]
    caps[victim] = len(want[victim]) - short
    stride = 8192
    dev = ctx.device
    d_in = torch.frombuffer(bytearray(b"".join(items)), dtype=torch.uint8).to(dev)
    d_out = torch.full((stride * len(items),), FILL, dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    at = np.concatenate([[0], np.cumsum([len(x) for x in items])])
    d_ptr, d_nb = i64([d_in.data_ptr() + int(a) for a in at[:-1]]), i64([len(x) for x in items])
    d_optr, d_cap = i64([d_out.data_ptr() + k * stride for k in range(len(items))]), i64(caps)
    nbytes = torch.full((len(items),), -1, dtype=torch.int64, device=dev)
    status = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
    failed = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = ctx.L.mi_deflate_batch_dev(ctx.h, C.byref(p), c, len(items), ptr(d_ptr), ptr(d_nb), sum((len(x) + block - 1) // block for x in items),
                                    ptr(d_optr), ptr(d_cap), ptr(nbytes), ptr(status), ptr(failed), ctx.stream_ptr())
    assert st == OK
    ctx.sync()
    out = d_out.cpu().numpy()
    assert [int(v) for v in status.cpu()] == [CAPACITY if k == victim else OK for k in range(len(items))] and int(failed.item()) == 1
    assert [int(v) for v in nbytes.cpu()] == [len(w) for w in want]
    for k, w in enumerate(want):
        cell = out[k * stride:(k + 1) * stride]
        if k == victim:
            assert bool((cell[caps[k]:] == FILL).all())
        else:
            assert cell[: len(w)].tobytes() == w and bool((cell[caps[k]:] == FILL).all())


# ---- stream order, pipeline batches ------------------------------------------------------------------------------------------------------
def test_late_input_on_a_callers_stream(ctx):
    """the late-input / early-poison harness of tests/stream_cases.py around one parse-1 mode-Z call on a non-blocking stream"""
    block, container = 65536, "zlib"
    data = np.frombuffer(CASES["text"][:3 * 65536 + 777], dtype=np.uint8)
    n, nblocks = data.size, 4
    p, cid = _p(block), lz.CONTAINERS[container]
    want, wbits = P.expected_z(data.tobytes(), block, container)
    case = sc.Case(ctx, "parse1-z-zlib")
    d_in = case.late(data, sc.data_poison(data))
    cap = (lz.bound_bytes_z(n, p, cid) + 3) & ~3
    out, bits, nb = case.out("out", cap), case.out("bits", 8 * (nblocks + 1), table=True), case.out("nbytes", 8, table=True)
    call = lambda: ctx.L.mi_deflate_z_encode_dev(ctx.h, C.byref(p), cid, sc.ptr(d_in), n, sc.ptr(out), cap, sc.ptr(bits), sc.ptr(nb),
                                                 ctx.stream_ptr())

    def check(got):
        assert sc._table(got["bits"], nblocks + 1) == wbits and sc._table(got["nbytes"], 1) == [len(want)]
        assert got["out"][: len(want)].tobytes() == want
    case.check = check
    sc.run(case, call, torch.cuda.Stream())


def test_several_pipeline_batches(ctx, monkeypatch):
    """about ten blocks, two per pipeline batch: the overlapped pipeline gives the bytes of the one-batch call"""
    block = 4096
    data = CASES["text"][:9 * block + 1234] + bytes(3000) + CASES["mixed"][:2000]
    p = _p(block)
    one = lz.compress_z(data, p, "gzip", ctx=ctx).tobytes()
    one_b = lz.compress_bgzf(data, p, ctx=ctx).tobytes()
    monkeypatch.setenv("MI_LZ_BATCH", "2")
    assert lz.compress_z(data, p, "gzip", ctx=ctx).tobytes() == one == P.expected_z(data, block, "gzip")[0]
    assert lz.compress_bgzf(data, p, ctx=ctx).tobytes() == one_b == P.expected_bgzf(data, block)[0]
    items = [data[:5 * block + 7], b"", data[3000:3100], data[7 * block:]]
    d = lz.deflate_batch(items, p, "raw", ctx=ctx).raise_for_status()
    assert [o.cpu().numpy().tobytes() for o in d.outputs] == [P.expected_z(x, block, "raw")[0] for x in items]


# ---- what is refused ---------------------------------------------------------------------------------------------------------------------
def test_refused_combinations(ctx):
    """MI_ERR_ARG before anything is queued, the outputs untouched: another parse value anywhere, and parse 1 on everything that
    keeps the reference's tokens"""
    L, h, dev, s = ctx.L, ctx.h, ctx.device, ctx.stream_ptr
    data = CASES["text"][:70000]
    n = len(data)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    out = torch.full((4 * n,), FILL, dtype=torch.uint8, device=dev)
    bits = torch.full((64,), -1, dtype=torch.int64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cap = out.numel()

    def mk(parse, flavour="deflate", block=65536, w=None, **fields):
        p = lz.params(flavour, w, block, parse=parse)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def z(p, c=2):
        return L.mi_deflate_z_encode_dev(h, C.byref(p), c, ptr(d_in), n, ptr(out), cap, ptr(bits), ptr(bits[32:]), s())

    def bgzf(p):
        return L.mi_bgzf_encode_dev(h, C.byref(p), ptr(d_in), n, ptr(out), cap, ptr(bits), ptr(bits[32:]), s())

    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    b_ptr, b_nb, b_optr, b_cap = i64([d_in.data_ptr()]), i64([n]), i64([out.data_ptr()]), i64([cap])
    b_st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    zd = torch.frombuffer(bytearray(dict_cases.dictionary(300)), dtype=torch.uint8).to(dev)

    def batch(p):
        return L.mi_deflate_batch_dev(h, C.byref(p), 1, 1, ptr(b_ptr), ptr(b_nb), 4, ptr(b_optr), ptr(b_cap), ptr(bits), ptr(b_st), ptr(b_st), s())

    def batch_dict(p):
        return L.mi_deflate_batch_dict_dev(h, C.byref(p), 1, 1, ptr(b_ptr), ptr(b_nb), 4, ptr(b_optr), ptr(b_cap), ptr(bits), ptr(b_st), ptr(b_st),
                                           ptr(zd), zd.numel(), s())

    def tokens(p):
        return L.mi_lz_encode_dev(h, C.byref(p), ptr(d_in), n, ptr(out), cap, ptr(bits), s())

    def mode_h(p):
        return L.mi_deflate_h_encode_dev(h, C.byref(p), ptr(d_in), n, ptr(out), cap, ptr(bits), s())

    def find(p):
        return L.mi_lz_find_all_dev(h, C.byref(p), ptr(d_in), n, ptr(out), s())

    def find32(p):
        return L.mi_lz_find_all32_dev(h, C.byref(p), ptr(d_in), n, ptr(out), s())

    refused = [
        ("z parse 2", z, mk(2)), ("z parse 0xFFFFFFFF", z, mk(0xFFFFFFFF)), ("bgzf parse 2", bgzf, mk(2, block=65280)),
        ("batch parse 2", batch, mk(2)), ("batch_dict parse 2", batch_dict, mk(2)),
        ("z parse 1 lbits 4", z, mk(1, lbits=4)), ("z parse 1 lbits 8", z, mk(1, lbits=8)), ("z parse 1 wbits 14", z, mk(1, wbits=14)),
        ("z parse 1 lz77", z, mk(1, "lz77", w=15)), ("z parse 1 block 65537", z, mk(1, block=65537)),
        ("bgzf parse 1 block 65536", bgzf, mk(1, block=65536)),
        ("tokens parse 1", tokens, mk(1)), ("tokens parse 2", tokens, mk(2)), ("lz77 parse 1", tokens, mk(1, "lz77", w=14)),
        ("lz77 256 KiB parse 1", tokens, mk(1, "lz77", block=262144, w=16)),
        ("mode H parse 1", mode_h, mk(1)), ("find_all parse 1", find, mk(1)), ("find_all32 parse 1", find32, mk(1, "lz77", block=262144, w=16)),
    ]
    for what, f, p in refused:
        assert f(p) == ARG, what
    # the host forms and the multi-device ones
    h_in = np.frombuffer(data, dtype=np.uint8)
    h_out = np.full(4 * n, FILL, dtype=np.uint8)
    h_bits = np.full(8, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    nb = C.c_uint64(77)
    assert L.mi_deflate_z_encode(h, C.byref(mk(2)), 2, hp(h_in), n, hp(h_out), h_out.size, hp(h_bits), C.byref(nb)) == ARG
    assert L.mi_bgzf_encode(h, C.byref(mk(2, block=65280)), hp(h_in), n, hp(h_out), h_out.size, hp(h_bits), C.byref(nb)) == ARG
    assert L.mi_lz_encode(h, C.byref(mk(1)), hp(h_in), n, hp(h_out), h_out.size, hp(h_bits)) == ARG
    assert L.mi_deflate_h_encode(h, C.byref(mk(1)), hp(h_in), n, hp(h_out), h_out.size, hp(h_bits)) == ARG
    with pytest.raises(_lib.MiError) as e:
        lz.deflate_batch_host([data[:100]], mk(2), "zlib", ctx=ctx)
    assert e.value.status == ARG
    with pytest.raises(_lib.MiError) as e:
        lz.deflate_batch_host([data[:100]], mk(2), "zlib", ctx=ctx, zdict=dict_cases.dictionary(300))
    assert e.value.status == ARG
    from compression_algorithms_amd.multi import Multi
    m = Multi([ctx.device.index or 0])
    try:
        ptrs = (C.c_void_p * 1)(C.c_void_p(d_in.data_ptr()))
        for mode in (0, 1):
            assert L.mi_lz_encode_multi_dev(m.h, C.byref(mk(1)), mode, ptrs, n, ptr(out), cap, ptr(bits)) == ARG
        assert L.mi_lz_encode_multi(m.h, C.byref(mk(1)), hp(h_in), n, hp(h_out), h_out.size, hp(h_bits)) == ARG
        assert L.mi_deflate_h_encode_multi(m.h, C.byref(mk(1)), hp(h_in), n, hp(h_out), h_out.size, hp(h_bits)) == ARG
    finally:
        m.close()
    ctx.sync()
    assert bool((out == FILL).all()) and bool((bits == -1).all()) and bool((b_st == -1).all())
    assert bool((h_out == FILL).all()) and bool((h_bits == 0xFFFFFFFFFFFFFFFF).all()) and nb.value == 77


# ---- parse 0 beside it ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_parse0_is_still_the_oracles(ctx, name):
    data = CASES[name]
    for block, c in ((65536, "gzip"), (1000, "raw")):
        lz.compress_z(data[:5000], _p(block, 1), c, ctx=ctx)                   # (a parse-1 call just before, on the same context)
        st = lz.compress_z(data, _p(block, 0), c, ctx=ctx)
        want, wbits = orc.defz_stream(data, block, c)
        assert st.tobytes() == bytes(want) and [int(v) for v in st.block_bits.cpu()] == wbits, (name, block, c)
    if len(data) > 1000:
        got = lz.compress_bgzf(data, _p(65280, 0), ctx=ctx).tobytes()
        import bgzf_cases
        assert got == bgzf_cases.expected_bgzf(data, 65280)[0]
