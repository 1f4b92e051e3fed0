"""BGZF byte ranges without a device: the numpy model of the plan against brute force over the walker's members, the pure
torch helpers (piece counts, virtual offsets), the host-side bound on the pieces, and the exported names."""
import pytest
import torch

import bgzf_range_cases as R
from compression_algorithms_amd import _lib, lz


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (stream, data) in R.streams().items():
        so, oo = R.walk(stream)
        out[name] = (stream, data, so, oo, R.ranges_for(stream, name))
    return out


def test_case_set_is_what_the_issue_lists(cases):
    _, _, _, oo, r = cases["S2"]
    assert [b - a for a, b in zip(oo, oo[1:])] == [1, 0, 7, 300, 0, 0, 65280, 0]
    assert (0, 2) in r and (7, 2) in r and (307, 2) in r                  # across the empty members, single and doubled
    assert (0, 9) in r                                                    # member 0's last byte through member 3's first
    assert (oo[-1] - 1, 10) in r and (oo[-1], 3) in r and (oo[-1] + 5, 3) in r
    assert (40_001, 19_998) in cases["S3"][4]
    for name, (_, data, _, _, r) in cases.items():
        assert (0, len(data)) in r and (0, 0) in r, name
        assert any(r.count(x) >= 2 for x in r), name


def test_plan_model_equals_brute_force(cases):
    for name, (_, _, _, oo, r) in cases.items():
        model, brute = R.plan_model(oo, r), R.plan_brute(oo, r)
        assert model == brute, name
        for (a, n), pieces in zip(r, model):
            assert sum(p[1] == "edge" for p in pieces) <= 2, (name, a, n)
            assert all(p[1] == "interior" for p in pieces[1:-1]), (name, a, n)
            assert sum(hi - lo for _, _, lo, hi in pieces) == max(min(a + n, oo[-1]) - a, 0) if n else not pieces, (name, a, n)
        counts = lz.bgzf_piece_counts(torch.tensor(oo), r)
        assert [int(v) for v in counts] == [len(p) for p in brute], name


def test_max_pieces_bounds_the_exact_count(cases):
    L = _lib.lib()
    for name, (_, _, _, oo, r) in cases.items():
        exact = sum(len(p) for p in R.plan_brute(oo, r))
        smallest = min(b - a for a, b in zip(oo, oo[1:]) if b > a)
        total_len = sum(n for _, n in r)
        for mmb in {smallest, max(smallest // 2, 1), 1}:                 # every bound the caller can truthfully give
            assert L.mi_bgzf_read_max_pieces(len(r), total_len, mmb) >= exact, (name, mmb)
            assert lz.bgzf_read_max_pieces(len(r), total_len, mmb) == len(r) + total_len // mmb + len(r)
        # range by range, too: a bound that only holds in the sum would hide a range it fails
        for (a, n), pieces in zip(r, R.plan_brute(oo, r)):
            assert L.mi_bgzf_read_max_pieces(1, n, smallest) >= len(pieces), (name, a, n)
    assert L.mi_bgzf_read_max_pieces(3, 1000, 0) == 3 + 1000 + 3         # (0 is read as 1)


def test_voffset_to_offset():
    #            member:  0    1 (empty)  2     3
    so, oo = [0, 100, 128, 1000, 1028], [0, 50, 50, 650, 650]
    idx = (torch.tensor(so), torch.tensor(oo))
    v = [(0 << 16) | 0, (0 << 16) | 49, (0 << 16) | 50, (100 << 16) | 0, (128 << 16) | 599, (128 << 16) | 600, (1000 << 16) | 0]
    assert [int(x) for x in lz.bgzf_voffset_to_offset(idx, v)] == [0, 49, 50, 50, 649, 650, 650]
    assert lz.bgzf_voffset_to_offset(idx, []).numel() == 0
    with pytest.raises(ValueError, match="not the start of a member"):
        lz.bgzf_voffset_to_offset(idx, [(101 << 16) | 0])
    with pytest.raises(ValueError, match="not the start of a member"):
        lz.bgzf_voffset_to_offset(idx, [(1028 << 16) | 0])              # the end of the stream starts no member
    with pytest.raises(ValueError, match="exceeds"):
        lz.bgzf_voffset_to_offset(idx, [(0 << 16) | 51])
    with pytest.raises(ValueError, match="exceeds"):
        lz.bgzf_voffset_to_offset(idx, [(100 << 16) | 1])


def test_voffset_to_offset_on_a_real_index(cases):
    _, _, so, oo, _ = cases["S2"]
    idx = (torch.tensor(so), torch.tensor(oo))
    v = [(so[m] << 16) | ((oo[m + 1] - oo[m]) // 2) for m in range(len(so) - 1) if oo[m + 1] - oo[m] < 65536]
    want = [oo[m] + (oo[m + 1] - oo[m]) // 2 for m in range(len(so) - 1) if oo[m + 1] - oo[m] < 65536]
    assert [int(x) for x in lz.bgzf_voffset_to_offset(idx, v)] == want


def test_names_are_exported():
    L = _lib.lib()
    for name in ("mi_bgzf_read_max_pieces", "mi_bgzf_read_ranges_dev", "mi_bgzf_read_ranges"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("bgzf_read", "bgzf_read_host", "bgzf_voffset_to_offset", "bgzf_read_max_pieces", "bgzf_piece_counts"):
        assert callable(getattr(lz, name)), name
