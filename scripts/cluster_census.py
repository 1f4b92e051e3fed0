#!/usr/bin/env python3
"""Census of a block's hash-table clusters, numpy only: the reasoning behind k_lz2_prefix.

A block's entries are its positions; an entry's home is mix32(le32 word at the position) & (T - 1); a cluster is a maximal run
of buckets that first fit WITHOUT retirement occupies (linear table: deflate's ring cut at bucket T is ignored).  For every
cluster: its entries in time order, whether more than one word lives in it (mixed), whether anything is ever retired (not
quiet: the last position exceeds the first + W), the share of its most frequent word, and its insert-only PREFIX — the entries
with position <= pos[0] + W, before which nothing is retired — with the steps a bulk placement of that prefix takes when a run of
consecutive entries with the same home is one step (at most `cap` entries per step).

    python scripts/cluster_census.py [--blocks 12] [--seed 12345] [--tbits 20] [--wbits 15]

prints the table of DESIGN.md 4.8 for blocks of synth.enwik_like.  tests/test_prefix_replay_gpu.py uses block_clusters() to
check its crafted blocks before the GPU sees them."""
import argparse
import os
import sys

import numpy as np

BLOCK = 65536
TAIL = 8


def mix32(w):
    """the reference hash (algorithms/lz77/lz77.c:13-41) over a uint32 array"""
    w = np.asarray(w, dtype=np.uint32)
    with np.errstate(over="ignore"):
        k = w * np.uint32(0xCC9E2D51)
        k = (k << np.uint32(15)) | (k >> np.uint32(17))
        k = k * np.uint32(0x1B873593)
        h = (k << np.uint32(13)) | (k >> np.uint32(19))
        h = h * np.uint32(5) + np.uint32(0xE6546B64)
        h ^= h >> np.uint32(16)
        h = h * np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h = h * np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def words_of(block):
    """le32 word at every position of the block (zeros behind its end, as the reference reads them)"""
    b = np.concatenate([np.asarray(block, dtype=np.uint8), np.zeros(TAIL, np.uint8)]).astype(np.uint32)
    n = len(block)
    return b[0:n] | (b[1:n + 1] << 8) | (b[2:n + 2] << 16) | (b[3:n + 3] << 24)


def block_clusters(block, tbits=20, wbits=15, min_size=8):
    """list of dicts, one per cluster of at least min_size entries: pos (time order), home (relative to the cluster's first
    bucket), word, mixed, quiet, dominant (share of the most frequent word), pre"""
    words = words_of(block)
    home = (mix32(words) & np.uint32((1 << tbits) - 1)).astype(np.int64)
    order = np.argsort(home, kind="stable")                      # by home, time order inside a home
    hs = home[order]
    # parking: a cluster ends where the next home lies beyond the buckets filled so far
    n = len(hs)
    head = np.zeros(n, bool)
    end = -1
    ends = np.empty(n, np.int64)
    for i in range(n):                                           # (65 536 steps: a second per block)
        if hs[i] > end:
            head[i] = True
            end = hs[i] + 1
        else:
            end += 1
        ends[i] = end
    starts = np.flatnonzero(head)
    out = []
    W = 1 << wbits
    for a, b in zip(starts, np.append(starts[1:], n)):
        if b - a < min_size:
            continue
        pos = np.sort(order[a:b])
        w = words[pos]
        h = home[pos] - hs[a]
        _, counts = np.unique(w, return_counts=True)
        out.append(dict(pos=pos, home=h, word=w, mixed=len(counts) > 1, quiet=pos[-1] <= pos[0] + W,
                        dominant=counts.max() / len(pos), pre=int(np.searchsorted(pos, pos[0] + W, side="right")),
                        covers_zero=bool(hs[a] == 0 or ends[b - 1] >= (1 << tbits))))
    return out


def prefix_steps(c, cap):
    """steps of a bulk placement of the cluster's prefix: one per run of consecutive entries with equal home, cap entries at most"""
    h = c["home"][: c["pre"]]
    if len(h) == 0:
        return 0
    cut = np.flatnonzero(np.diff(h) != 0) + 1
    runs = np.diff(np.concatenate([[0], cut, [len(h)]]))
    return int(np.sum((runs + cap - 1) // cap))


def census(blocks, tbits, wbits):
    classes = [(8, 127), (128, 511), (512, 1024)]
    acc = {c: dict(entries=0, clusters=0, dom=0.0, pre=0, steps16=0, steps64=0) for c in classes}
    total = 0
    for blk in blocks:
        total += len(blk)
        for c in block_clusters(blk, tbits, wbits):
            if not c["mixed"] or c["quiet"]:
                continue
            n = len(c["pos"])
            for cl in classes:
                if cl[0] <= n <= cl[1]:
                    a = acc[cl]
                    a["entries"] += n; a["clusters"] += 1; a["dom"] += c["dominant"] * n; a["pre"] += c["pre"]
                    a["steps16"] += prefix_steps(c, 16); a["steps64"] += prefix_steps(c, 64)
    return acc, total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--tbits", type=int, default=20)
    ap.add_argument("--wbits", type=int, default=15)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from compression_algorithms_amd import synth
    data = synth.enwik_like(a.blocks * BLOCK, seed=a.seed).numpy()
    acc, total = census([data[i * BLOCK:(i + 1) * BLOCK] for i in range(a.blocks)], a.tbits, a.wbits)
    print(f"{a.blocks} blocks of enwik_like(seed={a.seed}), T = 2^{a.tbits}, W = 2^{a.wbits}; mixed, non-quiet clusters")
    print("| size | share of entries | clusters per block | dominant word | prefix share | entries per prefix step (<= 16) | (<= 64) | prefix steps per block (<= 64) |")
    print("|---|---|---|---|---|---|---|---|")
    for (lo, hi), v in acc.items():
        if not v["entries"]:
            print(f"| {lo}..{hi} | 0 | 0 | - | - | - | - | - |")
            continue
        print(f"| {lo}..{hi} | {100 * v['entries'] / total:.2f} % | {v['clusters'] / a.blocks:.2f} | {100 * v['dom'] / v['entries']:.1f} % | "
              f"{100 * v['pre'] / v['entries']:.0f} % | {v['pre'] / max(v['steps16'], 1):.1f} | {v['pre'] / max(v['steps64'], 1):.1f} | {v['steps64'] / a.blocks:.0f} |")


if __name__ == "__main__":
    main()
