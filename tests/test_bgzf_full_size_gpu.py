"""BGZF at full size: the 10^9 bytes of the bench input (the generator and digest of test_full_size_gpu.py) encoded,
indexed and inflated on the GPU; the whole stream through gzip.decompress on the host; a seeded sample of 256 members
against the CPU oracle."""
import gzip

import numpy as np
import pytest
import torch

import bgzf_cases as B
from compression_algorithms_amd import lz, synth

pytestmark = pytest.mark.gpu

N9 = 1_000_000_000
SEED = 12345
DIGEST_1E9 = "fc5b7c102ca0b71b"
BLOCK = B.BGZF_BLOCK


def test_1e9_bgzf():
    x = synth.enwik_like(N9, seed=SEED, device="cuda")
    host = x.cpu().numpy()
    assert synth.digest(host) == DIGEST_1E9
    s = lz.compress_bgzf(x)
    nbytes = s.nbytes
    nblocks = (N9 + BLOCK - 1) // BLOCK
    bits = s.member_bits.cpu().numpy()
    assert len(bits) == nblocks + 1 and bits[0] == 0 and int(bits[-1]) // 8 == nbytes - 28
    # index and inflate on the GPU, from the bytes alone
    stream = s.data[:nbytes]
    idx = lz.bgzf_index(stream)
    so, oo = (t.cpu().numpy() for t in idx)
    assert idx.members == nblocks + 1 and int(so[-1]) == nbytes and int(oo[-1]) == N9
    assert np.array_equal(so[:-1] * 8, bits)
    assert np.array_equal(oo[:-1], np.minimum(np.arange(nblocks + 1, dtype=np.int64) * BLOCK, N9))
    for verify in (True, False):
        y = lz.decompress_bgzf(stream, members=idx, verify=verify)
        assert y.numel() == N9 and torch.equal(y, x)
        del y
    y = lz.decompress_bgzf(stream)
    assert torch.equal(y, x)
    del y
    # the whole stream on the host
    got = stream.cpu().numpy()
    assert got[-28:].tobytes() == B.EOF
    back = gzip.decompress(got.tobytes())
    assert len(back) == N9 and np.array_equal(np.frombuffer(back, dtype=np.uint8), host)
    del back
    # a seeded sample of 256 members, byte for byte
    rng = np.random.default_rng(20261017)
    sample = sorted({0, nblocks - 1} | set(int(b) for b in rng.choice(np.arange(1, nblocks - 1), 254, replace=False)))
    bad = []
    for b in sample:
        want, _ = B.expected_bgzf(host[b * BLOCK:(b + 1) * BLOCK].tobytes(), BLOCK)
        if got[so[b]:so[b + 1]].tobytes() != want[:-28]:
            bad.append(b)
    assert len(sample) == 256 and not bad, f"{len(bad)} members differ, first {bad[:8]}"
