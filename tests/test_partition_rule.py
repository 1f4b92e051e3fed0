"""The numpy restatement of the partition's rule (tests/partition_rule.py) against what the rule promises: the parts cover
[0, T) in order, their counts sum to n, no part is above its cap, every cut lies on a certified group and is the last one that
fits.  CPU only; tests/test_partition_cuts_gpu.py holds the device's parts against the same restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_rule as rule

from compression_algorithms_amd import synth


@pytest.fixture(scope="module")
def text():
    return synth.enwik_like(2 * 65536, seed=12345).numpy()


def test_mix32_and_its_inverse():
    w = np.array([0, 1, 0x61626364, 0xFFFFFFFF, 0xDEADBEEF], np.uint32)
    for x, h in zip(w, rule.mix32(w)):
        assert rule.unmix32(int(h)) == int(x)


@pytest.mark.parametrize("tbits,deflate,cap", [(20, True, 2048), (20, True, 640), (20, False, 2048), (22, False, 2048)])
def test_parts_of_text_keep_the_rules_promises(text, tbits, deflate, cap):
    for b in range(2):
        r = rule.parts(text[65536 * b:65536 * (b + 1)], tbits, deflate, cap)
        rule.self_check(r, tbits)
        assert deflate or r["base"] == 0
        assert r["nparts"] >= 65536 // cap, r["nparts"]                    # ~33 parts of 2 048 entries, ~100 of 640
        assert max(rule.lookback(r)) < 48                                  # text: the window of 64 groups always holds the cut


@pytest.mark.parametrize("n", [4099, 2048, 1])
def test_short_blocks(text, n):
    r = rule.parts(text[:n], 20, True)
    rule.self_check(r, 20)
    # at most 2 048 entries: one part, no cut.  One entry more than two parts' worth: cuts, and more than two parts (so few
    # entries are spread thin, and a part of this table also stays within 2^16 homes)
    assert (r["nparts"] == 1) == (n <= 2048) and r["nparts"] <= 17


def test_one_symbol_has_no_certified_cut():
    assert rule.parts(np.zeros(65536, np.uint8), 20, True)["fallback"] == 1
    assert rule.parts(np.zeros(65536, np.uint8), 20, False)["fallback"] == 1


def test_the_constructed_block_has_a_cut_far_below_its_boundary():
    r = rule.parts(rule.block_with_distant_cut(), 20, True)
    rule.self_check(r, 20)
    assert max(boundary - g for glo, boundary, g in r["cuts"]) >= 80
