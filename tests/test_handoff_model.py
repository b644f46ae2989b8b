"""CPU tests of the hand-off plan's numpy model (tests/handoff_model.py) against the CPU oracle: a
store simulation shows that the plan the model derives from the oracle's lookupN rows is a correct
hand-off, and the record counts of the shapes the GPU tests use are pinned.

The store model: every server in a key's lookupN row holds the key. After applying every transfer
that has a source, every server of the row now holds every key that had a surviving holder.
"""
import functools

import numpy as np
import pytest

import handoff_model as hm

NIL = hm.NIL
NKEYS = 50_000


def names_for(orc, servers, add, rem):
    initial = [orc.c2_addr(i) for i in range(servers)]
    added = [orc.c2_addr(servers + j) for j in range(add)]
    removed = [initial[(j * 7 + 1) % servers] for j in range(rem)]
    return initial, added, removed


@functools.lru_cache(maxsize=None)
def case(servers, add, rem, nrep):
    """(B, A, in_ring) in the oracle's id space for 50,000 UUID keys (seed 42)."""
    import pyoracle as orc
    initial, added, removed = names_for(orc, servers, add, rem)
    ob, oa = orc.Ring(100), orc.Ring(100)
    ob.add_remove(initial, None)
    oa.add_remove(initial, None)
    oa.add_remove(added, removed)
    keys = orc.uuid_keys(42, 0, NKEYS)
    B, _ = ob.lookupn_keys(keys, nrep)
    A, _ = oa.lookupn_keys(keys, nrep)
    now = set(initial + added) - set(removed)
    in_ring = np.array([oa.name(i) in now for i in range(servers + add)], dtype=bool)
    for x in (B, A, in_ring):
        x.setflags(write=False)
    return B, A, in_ring


SHAPES = [(1, 1, 0), (2, 1, 0), (3, 0, 1), (64, 1, 1), (64, 0, 32), (1000, 10, 10)]


@pytest.mark.parametrize("nrep", [-2, 0, 1, 3, 8])
@pytest.mark.parametrize("servers,add,rem", SHAPES)
def test_store_simulation(orc, servers, add, rem, nrep):
    B, A, in_ring = case(servers, add, rem, nrep)
    nid = len(in_ring)
    dests, goff, kidx, src, slot, count = hm.plan(B, A, in_ring)
    assert count == len(kidx) == goff[-1]
    # store_before[s] = the keys with s in B
    held = np.zeros((NKEYS, nid), dtype=bool)
    for q in range(B.shape[1]):
        ok = B[:, q] != NIL
        held[np.flatnonzero(ok), B[ok, q]] = True
    for s in range(nid):
        assert np.array_equal(np.flatnonzero(held[:, s]), np.flatnonzero((B == s).any(axis=1)))
    dst = np.repeat(dests, np.diff(goff))
    assert (np.diff(dests.astype(np.int64)) > 0).all()
    for g in range(len(dests)):  # strictly ascending key indices inside a group
        assert (np.diff(kidx[goff[g]:goff[g + 1]].astype(np.int64)) > 0).all()
    # no transfer goes to a prior holder; each destination is in the key's row now, at its slot
    assert not held[kidx, dst].any()
    assert np.array_equal(A[kidx, slot], dst)
    # each source is in the ring now and held the key
    has = src != NIL
    assert in_ring[src[has]].all() and held[kidx[has], src[has]].all()
    # apply every transfer that has a source
    after = held.copy()
    after[kidx[has], dst[has]] = True
    src_of_key = hm.sources(B, in_ring)
    served = src_of_key != NIL
    for q in range(A.shape[1]):
        ok = served & (A[:, q] != NIL)
        assert after[np.flatnonzero(ok), A[ok, q]].all()
    # orphans: the keys with no live server in B (they need every server of A from elsewhere)
    live = np.zeros(B.shape, dtype=bool)
    live[B != NIL] = in_ring[B[B != NIL]]
    assert (~served).sum() == (~live.any(axis=1)).sum()
    assert set(np.unique(kidx[~has])) <= set(np.flatnonzero(~served))
    # the filtered plans over all live servers, plus the orphans, partition the stream
    total = (src == NIL).sum()
    for s in np.flatnonzero(in_ring):
        total += hm.plan(B, A, in_ring, only_src=s)[5]
    assert total == count


def stats(servers, add, rem, nrep):
    B, A, in_ring = case(servers, add, rem, nrep)
    dests, goff, kidx, src, slot, count = hm.plan(B, A, in_ring)
    moved = int((B != A).any(axis=1).sum())
    keys_with = len(np.unique(kidx))
    orphans = int((hm.sources(B, in_ring) == NIL).sum())
    per_key = int(np.bincount(kidx).max()) if count else 0
    return {"moved": moved, "transfers": count, "keys": keys_with, "dests": len(dests), "orphans": orphans,
            "max_per_key": per_key}


def test_pinned_counts(orc):
    """The figures the GPU parity tests assert as sanity of their own expectations."""
    s = stats(64, 1, 1, 3)
    assert (s["moved"], s["transfers"], s["dests"], s["orphans"]) == (4537, 4537, 61, 0)
    s = stats(64, 1, 1, 1)
    assert (s["transfers"], s["orphans"]) == (1460, 693)
    s = stats(64, 0, 32, 3)
    assert (s["transfers"], s["moved"], s["max_per_key"], s["orphans"]) == (75199, 44392, 3, 5757)
    s = stats(64, 0, 32, 8)
    assert (s["transfers"], s["max_per_key"]) == (200711, 8)
    for nrep in (3, 8):
        s = stats(3, 0, 1, nrep)
        assert (s["moved"], s["transfers"]) == (NKEYS, 0)  # rows only shrink
    s = stats(1000, 10, 10, 3)
    assert (s["transfers"], s["keys"], s["dests"]) == (2901, 2880, 609)


def test_cap_cuts_the_stream_not_the_groups(orc):
    B, A, in_ring = case(64, 0, 32, 3)
    key, dst, src, slot = hm.record_stream(B, A, in_ring)
    full = len(key)
    for cap in (0, 1, full - 1, full, full + 7):
        dests, goff, kidx, s, q, count = hm.plan(B, A, in_ring, cap=cap)
        t = min(cap, full)
        assert count == full and goff[-1] == t and len(kidx) == t
        # the same multiset of records as the first t of the stream
        got = sorted(zip(kidx.tolist(), np.repeat(dests, np.diff(goff)).tolist(), s.tolist(), q.tolist()))
        want = sorted(zip(key[:t].tolist(), dst[:t].tolist(), src[:t].tolist(), slot[:t].tolist()))
        assert got == want
