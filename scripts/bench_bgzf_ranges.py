"""Byte-range reads from BGZF: 10^4 ranges of 1 to 200 KiB over a 10^9-byte stream (bench.py's corpus as this library's
BGZF), warm, HIP events, the median of alternating runs in one process.

  ranges     lz.bgzf_read: one call for all ranges (the index made once, outside the timing; max_pieces from
             mi_bgzf_read_max_pieces, so the call reads nothing back)
  by_member  what a caller did before: per range the member lookup on the host (the index copied down once, outside the
             timing), lz.decompress_bgzf(first=, count=) for the members that hold the range, and a slice

Both are checked against slices of the corpus before anything is timed.  The baseline runs over a sample of the ranges
(--baseline-ranges) and is scaled to all of them: ten thousand synchronising calls take minutes.  One JSON line.

    python scripts/bench_bgzf_ranges.py [--bytes 1000000000] [--ranges 10000] [--repeats 5]
"""
import argparse
import bisect
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compression_algorithms_amd import lz, synth  # noqa: E402


def timed(f, repeats):
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return sorted(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=12345)            # bench.py's corpus
    ap.add_argument("--ranges", type=int, default=10_000)
    ap.add_argument("--baseline-ranges", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = lz.default_context()
    x = synth.enwik_like(a.bytes, seed=a.seed, device=dev)
    n = x.numel()
    s = lz.compress_bgzf(x)
    stream = s.data[: s.nbytes].clone()
    del s
    idx = lz.bgzf_index(stream)
    rng = np.random.default_rng(1)
    lens = rng.integers(1, 200 * 1024 + 1, a.ranges)
    offs = rng.integers(0, n - 200 * 1024, a.ranges)
    r = torch.from_numpy(np.stack([offs, lens], 1).astype(np.int64)).to(dev)
    total_len = int(lens.sum())
    bound = lz.bgzf_read_max_pieces(a.ranges, total_len, lz.BGZF_BLOCK)
    at = torch.from_numpy((np.cumsum(lens) - lens).astype(np.int64)).to(dev)
    out = torch.empty(total_len, dtype=torch.uint8, device=dev)

    def ranges():
        return lz.bgzf_read(stream, r, members=idx, max_pieces=bound, out=out, out_offsets=at)

    res = ranges()
    assert res.failed == 0 and torch.equal(res[2].cpu(), torch.from_numpy(lens.astype(np.int64)))
    for i in rng.integers(0, a.ranges, 50):
        o, ln, p = int(offs[i]), int(lens[i]), int(at[i])
        assert torch.equal(out[p:p + ln], x[o:o + ln]), i

    oo = [int(v) for v in idx[1].cpu()]                            # the host's copy of the index, for the lookups

    def one(o, ln):
        first = bisect.bisect_right(oo, o) - 1
        last = bisect.bisect_left(oo, o + ln)                       # members [first, last) hold the range
        y = lz.decompress_bgzf(stream, members=idx, first=first, count=last - first)
        return y[o - oo[first]: o - oo[first] + ln]

    nb = min(a.baseline_ranges, a.ranges)

    def by_member():
        for i in range(nb):
            one(int(offs[i]), int(lens[i]))

    for i in range(min(nb, 20)):
        assert torch.equal(one(int(offs[i]), int(lens[i])), x[int(offs[i]): int(offs[i]) + int(lens[i])]), i
    tr, tb = timed(ranges, a.repeats), timed(by_member, max(a.repeats // 2, 1))
    med_r, med_b = tr[len(tr) // 2], tb[len(tb) // 2] * a.ranges / nb
    out_json = dict(
        ranges=dict(ms_median=round(med_r, 3), ms_min=round(tr[0], 3), ms_max=round(tr[-1], 3), gbps_out=round(total_len / med_r / 1e6, 3),
                    max_pieces=bound, exact_pieces=int(lz.bgzf_piece_counts(idx[1], r).sum())),
        by_member=dict(ms_median_scaled=round(med_b, 3), sampled_ranges=nb, gbps_out=round(total_len / med_b / 1e6, 3)),
        by_member_over_ranges=round(med_b / med_r, 2), n_ranges=a.ranges, bytes_out=total_len, members=idx.members,
        device=torch.cuda.get_device_name(0), bytes=n, repeats=a.repeats)
    print(json.dumps(out_json))


if __name__ == "__main__":
    main()
