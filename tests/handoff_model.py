"""The numpy model of the hand-off plan (rp_ring_handoff*), written from the semantics in
include/ringpop_amd.h. A helper of the hand-off tests, not a test.

Inputs: the two [n, W] lookupN row arrays of the keys (B under the snapshot, A under the ring now,
NIL padded), the in-ring mask per server id (ring membership now), only_src and cap.
"""
import numpy as np

NIL = 0xFFFFFFFF


def sources(B, in_ring):
    """src(i): the first entry of B[i], in slot order, whose server is in the ring now; NIL if none."""
    B = np.asarray(B, dtype=np.uint32)
    in_ring = np.asarray(in_ring, dtype=bool)
    n, w = B.shape
    live = np.zeros((n, w), dtype=bool)
    ok = (B != NIL) & (B < len(in_ring))
    live[ok] = in_ring[B[ok]]
    first = live.argmax(axis=1)
    src = B[np.arange(n), first] if n else np.empty(0, dtype=np.uint32)
    return np.where(live.any(axis=1), src, np.uint32(NIL)).astype(np.uint32)


def gained(B, A):
    """[n, W] bool: A[i, q] is non-null and occurs nowhere in B[i]."""
    B = np.asarray(B, dtype=np.uint32)
    A = np.asarray(A, dtype=np.uint32)
    held = (A[:, :, None] == B[:, None, :]).any(axis=2)
    return (A != NIL) & ~held


def record_stream(B, A, in_ring, only_src=NIL):
    """(key, dst, src, slot) of every record, in (key index, slot) order."""
    A = np.asarray(A, dtype=np.uint32)
    g = gained(B, A)
    src = sources(B, in_ring)
    if only_src != NIL:
        g &= (src == np.uint32(only_src))[:, None]
    key, slot = np.nonzero(g)  # row-major: (key, slot) order
    return key.astype(np.uint32), A[key, slot], src[key], slot.astype(np.uint8)


def plan(B, A, in_ring, only_src=NIL, cap=None):
    """(dests, group_off, key_idx, src, slot, count): the first T = min(count, cap) records of the
    stream grouped by destination id (ascending), (key, slot) order kept inside a group."""
    key, dst, src, slot = record_stream(B, A, in_ring, only_src)
    count = len(key)
    t = count if cap is None else min(count, int(cap))
    key, dst, src, slot = key[:t], dst[:t], src[:t], slot[:t]
    order = np.argsort(dst, kind="stable")
    dests, heads = np.unique(dst[order], return_index=True)
    group_off = np.append(heads, t).astype(np.uint32)
    return dests.astype(np.uint32), group_off, key[order], src[order], slot[order], count
