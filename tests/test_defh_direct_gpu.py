"""Mode H packs every record straight into the caller's stream: k_defh_lengths computes the record's size from the tally and
the code lengths (csrc/defh_size.h), the scan places the records, k_defh_encode writes each one at its final words — no slot,
no k_lz_concat.  Pinned here: stream and block table equal the oracle's (oracle/orc_defh.c per block, records concatenated)
where placement can go wrong — one block, a ragged last block, tiny inputs, batches that meet at a base that is not zero (with
and without the three-stream pipeline), one-leaf trees, blocks without a match — and nothing is written past the stream."""
import ctypes as C

import numpy as np
import pytest

from compression_algorithms_amd import synth

pytestmark = pytest.mark.gpu


def _oracle(data, block):
    from oracle import orc
    d = orc.Deflate(block)
    recs = []
    for at in range(0, len(data), block):
        d.fresh()
        recs.append(orc.defh_encode_block(d.block_encode(data[at:at + block])))
    return recs


def _check(data, block=65536):
    from compression_algorithms_amd import lz
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    st = lz.compress_h(data, lz.params("deflate", None, block))
    recs = _oracle(data, block)
    want_bits = np.concatenate([[0], np.cumsum([len(r) * 8 for r in recs])]).astype(np.int64)
    assert np.array_equal(st.block_bits.cpu().numpy(), want_bits), "block table"
    got = np.frombuffer(st.tobytes(), dtype=np.uint8)
    want = np.concatenate(recs)
    assert len(got) == len(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"mode H stream differs at byte {bad[:5]} of {len(want)}"
    assert np.array_equal(lz.decompress_h(st).cpu().numpy(), data)
    return st


def test_one_block():
    _check(synth.enwik_like(65536, seed=41).numpy())


def test_ragged_last_block():
    _check(synth.enwik_like(5 * 65536 + 12345, seed=42).numpy())


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_tiny(n):
    _check(synth.adversarial("random", n))
    _check(synth.enwik_like(n, seed=43).numpy())


@pytest.mark.parametrize("overlap", [True, False])
def test_batches_meet_at_a_nonzero_base(monkeypatch, overlap):
    """five batches of up to 5 blocks: every batch after the first starts where the one before ended"""
    monkeypatch.setenv("MI_LZ_BATCH", "5")
    if not overlap:
        monkeypatch.setenv("MI_LZ_NO_OVERLAP", "1")
    _check(synth.enwik_like(23 * 65536 + 77, seed=44).numpy())


def test_many_small_blocks_in_batches(monkeypatch):
    """small blocks, batches of 100: 313 records in four batches"""
    monkeypatch.setenv("MI_LZ_BATCH", "100")
    _check(synth.enwik_like(313 * 1024 - 5, seed=45).numpy(), 1024)


@pytest.mark.parametrize("kind", [k for k in synth.FAMILIES if k != "text"])
def test_families(kind):
    _check(synth.family(kind, 46, 6 * 65536 + 999))


@pytest.mark.parametrize("kind,n", [("zeros", 3 * 65536 + 17), ("single", 2 * 65536), ("random", 3 * 65536 + 1),
                                    ("random_nonzero", 65536)])
def test_one_leaf_and_no_matches(kind, n):
    """zeros / one symbol: a one-leaf tree (len = 1) beside the match symbols; random: no matches, no extra bits"""
    _check(synth.adversarial(kind, n))


@pytest.mark.parametrize("kind,n,block", [("text", 4 * 65536 + 333, 65536), ("random", 65536, 1024), ("zeros", 70000, 65536),
                                          ("random", 5, 65536)])
def test_nothing_is_written_past_the_stream(kind, n, block):
    """a buffer of exactly the bound + the 64 bytes of slack the Python layer adds, filled with a pattern: every byte from
    the stream's end on still holds it"""
    import torch
    from compression_algorithms_amd import lz, _lib
    from compression_algorithms_amd.context import as_device_bytes, default_context
    ctx = default_context()
    data = synth.enwik_like(n, seed=47).numpy() if kind == "text" else np.frombuffer(synth.adversarial(kind, n), dtype=np.uint8)
    p = lz.params("deflate", None, block)
    d_in = as_device_bytes(data, ctx.device)
    nblocks = (n + block - 1) // block
    cap = int(ctx.L.mi_deflate_h_bound_bytes(n, C.byref(p))) + 64
    pattern = ((np.arange(cap, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)
    out = torch.from_numpy(pattern.copy()).to(ctx.device)
    assert out.data_ptr() % 4 == 0
    bits = torch.zeros(nblocks + 1, dtype=torch.int64, device=ctx.device)
    st = ctx.L.mi_deflate_h_encode_dev(ctx.h, C.byref(p), C.c_void_p(d_in.data_ptr()), n, C.c_void_p(out.data_ptr()), cap,
                                       C.c_void_p(bits.data_ptr()), ctx.stream_ptr())
    _lib.check(st, "mi_deflate_h_encode_dev")
    ctx.sync()
    nbytes = int(bits[-1]) // 8
    got = out.cpu().numpy()
    want = np.concatenate(_oracle(data, block))
    assert nbytes == len(want) and nbytes <= cap - 64
    assert np.array_equal(got[:nbytes], want)
    assert np.array_equal(got[nbytes:], pattern[nbytes:]), "bytes past the stream were written"
