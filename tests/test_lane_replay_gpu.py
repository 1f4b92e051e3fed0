"""The lane replay of the exported clusters of 8..127 entries (k_lz2_lane_count / k_lz2_lane_place sort them by size into one
list, k_lz2_lanes replays them: lz2_find.hip) against the oracle: at the default LDS budget per wave, at half of it
(MI_LZ_LANES_KIB=4) and with a one-batch call's stage B on one stream (MI_LZ_B_SPLIT=0), the same inputs each time.  Inputs
with many clusters at every size from 8 to 127: text, phrases and a low-entropy family; deflate (W = 32 KiB, the bucket-0 / T
cluster stops the probe) and the shipped lz77 window (W = 16 KiB); a batch of one block and one of nine; an input without any
lane-class cluster (random bytes: every launch of the chain is empty).
k_lz2_lanes checks that every cluster a wave takes has the wave's size (the list is sorted) and counts an order violation
otherwise."""
import pytest

from test_fallback_chain_gpu import _child

pytestmark = pytest.mark.gpu

BODY = """
    ctx = Context(0)
    rng = np.random.default_rng(11)
    inputs = [("text9", synth.family("text", 3, 9 * 65536 - 301)), ("text1", synth.family("text", 4, 65536)),
              ("phrases", synth.family("phrases", 5, 9 * 65536)), ("lowent", synth.family("lowent", 6, 3 * 65536 + 17)),
              ("random", rng.integers(0, 256, 2 * 65536, dtype=np.uint8))]
    for name, data in inputs:
        for p in (lz.params("deflate"), lz.params("lz77", 14)):
            st = lz.compress(data, p, ctx)
            ctx.sync()
            assert oracle_equal(st, data, p), (name, "stream differs from the oracle")
            assert np.array_equal(lz.decompress(st, ctx).cpu().numpy(), data)
    assert ctx.order_violations() == 0
    print("ok")
"""


@pytest.mark.parametrize("env", [{}, {"MI_LZ_LANES_KIB": "4"}, {"MI_LZ_B_SPLIT": "0"}])
def test_lane_replay_equals_the_oracle(env):
    assert "ok" in _child(BODY, **env)
