#!/usr/bin/env python3
"""Line-count model of the lookupN(3) trips (CPU only, numpy): distinct 128-B lines the 64 lanes
of one wave instruction touch, per key, for the lean kernel's arrival order and for
k_lookupn_sorted's tiles ordered by h >> 20.

The L1 merges the lanes of one instruction that fall into the same 128-B line, so the L1 -> L2
read requests per key are about (distinct lines per 64 consecutive tile slots) / 64, summed over
the index load (an 8-B group record) and the window load (16 B at 3 x position, which may cross
a line), plus 0.28 for the key stream (36 B a key in 128-B lines).

Without a ring the model takes M uniform tokens (the window at 3 floor(h M / 2^32)); with
--servers N (the oracle builds the C2-style ring) or --tokens FILE (a .npy of the ring's sorted
uint32 tokens, e.g. HashRing.dump()[0]) it takes the real bucket starts of the compact layout.

  python3 tools/model_sorted_lines.py                  # uniform, M = 999,892
  python3 tools/model_sorted_lines.py --servers 10000  # the C2 ring through the oracle
"""
import argparse
import os
import sys

import numpy as np

KEY_STREAM = 0.28  # 36 B a key / 128 B a line
SHAPES = [(2048, False), (2048, True), (4096, True), (8192, True)]


def lines_per_key(line_sets, tile, ordered, sort_key):
    """line_sets: list of (n,) int64 arrays of line ids per key (a key's lines: all arrays at its
    index; equal entries count once). Returns distinct lines per key over waves of 64 slots."""
    n = len(sort_key) // tile * tile
    total = 0
    for t0 in range(0, n, tile):
        sl = slice(t0, t0 + tile)
        order = np.argsort(sort_key[sl], kind="stable") if ordered else np.arange(tile)
        # lane tid takes slots tid + k THREADS: one instruction = 64 consecutive slots
        cols = [a[sl][order].reshape(-1, 64) for a in line_sets]
        rows = np.sort(np.concatenate(cols, axis=1), axis=1)
        total += int((np.diff(rows, axis=1) != 0).sum()) + rows.shape[0]
    return total / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--tokens-uniform", type=int, default=999_892, help="M of the uniform approximation")
    ap.add_argument("--servers", type=int, default=0, help="build the ring of N C2 servers x 100 points with the oracle")
    ap.add_argument("--tokens", default=None, help=".npy of the ring's sorted uint32 tokens")
    ap.add_argument("--bin-shift", type=int, default=20, help="the sort's bin is h >> this")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    rng = np.random.default_rng(args.seed)
    tok = None
    if args.tokens:
        tok = np.sort(np.load(args.tokens).astype(np.uint64))
    elif args.servers:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
        import pyoracle
        if not os.path.exists(pyoracle._LIB_PATH):
            pyoracle.build()
        ring = pyoracle.Ring(100)
        ring.add_remove([pyoracle.c2_addr(i) for i in range(args.servers)])
        tok = ring.dump()[0].astype(np.uint64)
    if tok is not None:
        # the real key stream's hashes are uniform too; what the ring changes is where windows start
        h = rng.integers(0, 1 << 32, size=args.keys, dtype=np.uint64)
        M = len(tok)
        cb = max(3, int(np.floor(np.log2(M))))
        # window 1 starts within an entry or two of the key's position (hints): take the position
        pos = np.searchsorted(tok, h, side="left").astype(np.int64)
        group = (h >> np.uint64(32 - cb + 3)).astype(np.int64)
        src = "ring of %d tokens (cb %d)" % (M, cb)
    else:
        h = rng.integers(0, 1 << 32, size=args.keys, dtype=np.uint64)
        M = args.tokens_uniform
        cb = int(np.floor(np.log2(M)))
        pos = ((h * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
        group = (h >> np.uint64(32 - cb + 3)).astype(np.int64)
        src = "uniform, M = %d (cb %d)" % (M, cb)
    idx_line = (group * 8) >> 7
    w0 = (3 * pos) >> 7
    w1 = (3 * pos + 15) >> 7  # the window's last byte: another line when it crosses
    sort_key = (h >> np.uint64(args.bin_shift)).astype(np.int64)

    print("model: %s, %d keys, bin = h >> %d (%d index lines)" % (src, args.keys, args.bin_shift, int(idx_line.max()) + 1))
    print("| tile (keys), order | index lines / key | window lines / key | total / key |")
    print("|---|---|---|---|")
    for tile, ordered in SHAPES:
        il = lines_per_key([idx_line], tile, ordered, sort_key)
        wl = lines_per_key([w0, w1], tile, ordered, sort_key)
        print("| %d, %s | %.3f | %.3f | %.2f |" % (tile, "ordered by h >> %d" % args.bin_shift if ordered else "arrival order",
                                               il, wl, il + wl + KEY_STREAM))


if __name__ == "__main__":
    main()
