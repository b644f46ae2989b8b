"""GPU parity tests of the moved-ranges calls through the C ABI (rp_ring_moved_ranges*,
rp_ring_snap_moved_ranges*, rp_ring_snap_dump): which hash intervals changed hands between a ring
snapshot and the ring now, without any key.

Oracle: the same add / remove sequence replayed on oracle/liboracle.so. lookupN depends on the hash
only through "the first token >= h", so oracle_ranges() asks the oracle for the lookupN row of
every value of the sorted union of both token sets (2^32-1 appended) under both rings, drops the
equal pairs and joins neighbours that touch and carry the same pair. Everything is compared bit
for bit: lo, hi, both row arrays, the run count and the moved hash count.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_ring_moved_gpu import GRID, names_for, to_gpu_ids

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
TOP = 0xFFFFFFFF
SENT = 0x5A5A5A5A
NREPS = [-2, 0, 1, 3, 8]
# union sizes around the wave (64), the kernels' tile (256 merged elements a workgroup) and
# multiples of it; 4097 = 17 tiles
UNION_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4097]


# ---------------------------------------------------------------------------- the expectation
def oracle_ranges(ob, oa, nrep):
    """The moved ranges between the oracle rings ob and oa, in the oracle's ids:
    {lo, hi, before, after (uint32 arrays), moved (hash values), differing (intervals of the union
    whose rows differ, before joining), union (its size)}."""
    w = max(nrep, 1)
    u = np.union1d(np.union1d(ob.dump()[0], oa.dump()[0]), np.array([TOP], dtype=np.uint32)).astype(np.int64)
    los, his, rbs, ras = [], [], [], []
    differing = 0
    prev = -1
    for h in u:
        b, a = ob.lookupn_hash(int(h), nrep), oa.lookupn_hash(int(h), nrep)
        lo, prev = prev + 1, int(h)
        if a == b:
            continue
        differing += 1
        b, a = b + [NIL] * (w - len(b)), a + [NIL] * (w - len(a))
        if his and his[-1] + 1 == lo and rbs[-1] == b and ras[-1] == a:
            his[-1] = int(h)
            continue
        los.append(lo)
        his.append(int(h))
        rbs.append(b)
        ras.append(a)
    arr = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
    return {"lo": arr(los), "hi": arr(his), "before": arr(rbs).reshape(-1, w), "after": arr(ras).reshape(-1, w),
            "moved": sum(h - l + 1 for l, h in zip(los, his)), "differing": differing, "union": len(u)}


@functools.lru_cache(maxsize=None)
def oracle_pair(servers, add, rem, points=100):
    """The oracle rings before and after +add / -rem on `servers` servers (shared, never changed)."""
    import pyoracle
    initial, added, removed = names_for(pyoracle, max(servers, 1), add, rem)
    initial = initial[:servers]
    ob, oa = pyoracle.Ring(points), pyoracle.Ring(points)
    if initial:
        ob.add_remove(initial, None)
        oa.add_remove(initial, None)
    if added or removed:
        oa.add_remove(added, removed)
    return ob, oa


@functools.lru_cache(maxsize=None)
def want_ranges(servers, add, rem, nrep, points=100):
    ob, oa = oracle_pair(servers, add, rem, points)
    w = oracle_ranges(ob, oa, nrep)
    for k in ("lo", "hi", "before", "after"):
        w[k].setflags(write=False)
    return w


def device_pair(gpu, orc, servers, add, rem, points=100):
    """Device ring + snapshot of `servers` servers, then +add / -rem."""
    initial, added, removed = names_for(orc, max(servers, 1), add, rem)
    initial = initial[:servers]
    ring = gpu.HashRing({"replicaPoints": points})
    if initial:
        ring.addRemoveServers(initial, None)
    snap = ring.snapshot()
    if added or removed:
        ring.addRemoveServers(added, removed)
    return ring, snap


def invariants(lo, hi, br, ar, moved_hashes):
    """What every result satisfies, whatever the rings."""
    lo64, hi64 = lo.astype(np.int64), hi.astype(np.int64)
    assert (lo64 <= hi64).all()
    assert (hi64[:-1] < lo64[1:]).all()  # ascending and disjoint
    touch = hi64[:-1] + 1 == lo64[1:]
    same = (br[:-1] == br[1:]).all(axis=1) & (ar[:-1] == ar[1:]).all(axis=1)
    assert not (touch & same).any()  # maximal runs
    assert (br != ar).any(axis=1).all()
    assert int((hi64 - lo64 + 1).sum()) == moved_hashes


def moved_hashes_call(gpu, ring, snap, hs, nrep):
    """rp_ring_moved_hashes over the hashes hs: (idx, before rows, after rows)."""
    hs = np.ascontiguousarray(hs, dtype=np.uint32)
    w = max(nrep, 1)
    idx = np.empty(len(hs), dtype=np.uint32)
    br = np.empty((len(hs), w), dtype=np.uint32)
    ar = np.empty((len(hs), w), dtype=np.uint32)
    c = ctypes.c_uint32()
    gpu.check(gpu.lib().rp_ring_moved_hashes(ring._h, snap._h, hs.ctypes.data, len(hs), nrep, len(hs),
                                             idx.ctypes.data, br.ctypes.data, ar.ctypes.data, ctypes.byref(c)))
    return idx[:c.value], br[:c.value], ar[:c.value]


def point_probes(gpu, ring, snap, got, nrep, seed=7):
    """The existing per-key call agrees: a hash has moved exactly when it lies inside a range, and
    its rows are that range's rows."""
    lo, hi, br, ar = got
    lo64, hi64 = lo.astype(np.int64), hi.astype(np.int64)
    edges = np.concatenate([lo64, hi64, lo64 - 1, hi64 + 1])
    edges = edges[(edges >= 0) & (edges <= TOP)]
    rnd = np.random.default_rng(seed).integers(0, 1 << 32, 4096, dtype=np.int64)
    hs = np.concatenate([edges, rnd])
    j = np.searchsorted(lo64, hs, side="right") - 1  # the last range that starts at or below h
    inside = (j >= 0) & (hs <= hi64[np.maximum(j, 0)]) if len(lo) else np.zeros(len(hs), dtype=bool)
    idx, pb, pa = moved_hashes_call(gpu, ring, snap, hs, nrep)
    assert np.array_equal(idx, np.flatnonzero(inside))
    assert np.array_equal(pb, br[j[inside]]) and np.array_equal(pa, ar[j[inside]])


def assert_ranges(gpu, ring, snap, got, counts, want, oa, nnames, nrep):
    lo, hi, br, ar = got
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32
    assert counts == (len(want["lo"]), want["moved"]), (counts, len(want["lo"]), want["moved"])
    assert np.array_equal(lo, want["lo"]) and np.array_equal(hi, want["hi"])
    assert np.array_equal(br, to_gpu_ids(ring, oa, want["before"], nnames))
    assert np.array_equal(ar, to_gpu_ids(ring, oa, want["after"], nnames))
    invariants(lo, hi, br, ar, counts[1])
    point_probes(gpu, ring, snap, got, nrep)


def ranges_of(ring, snap, nrep, cap=None):
    got = ring.moved_range_ids(snap, nrep, cap)
    return got, (ring.moved_range_count, ring.moved_hash_count)


# ---------------------------------------------------------------------------- 1. parity grid
@pytest.mark.parametrize("nrep", NREPS)
@pytest.mark.parametrize("servers,add,rem", GRID)
def test_parity_grid(gpu, orc, servers, add, rem, nrep):
    ring, snap = device_pair(gpu, orc, servers, add, rem)
    ob, oa = oracle_pair(servers, add, rem)
    want = want_ranges(servers, add, rem, nrep)
    got, counts = ranges_of(ring, snap, nrep)
    assert_ranges(gpu, ring, snap, got, counts, want, oa, servers + add, nrep)
    if servers >= 64:  # the expectation itself is a partial, non-trivial set
        assert 0 < counts[0] < want["union"]
    if (servers, add, rem) in ((1, 1, 0), (64, 1, 1), (1000, 10, 10)):  # joining is exercised
        assert counts[0] < want["differing"]
    # the figures the oracle alone gave when the call was specified
    known = {(64, 1, 1, 3): (571, 582), (1000, 10, 10, 3): (5909, 5916), (1, 1, 0, 1): (53, 100),
             (1, 1, 0, 3): (107, 201)}
    if (servers, add, rem, nrep) in known:
        assert (counts[0], want["differing"]) == known[(servers, add, rem, nrep)]
    if (servers, add, rem, nrep) == (1, 1, 0, 3):  # the list length changes: every hash moves
        assert counts[1] == 1 << 32
    if (servers, add, rem, nrep) == (1000, 10, 10, 3):
        assert want["union"] == 101_001 and round(counts[1] / 2.0 ** 32, 3) == 0.059
    snap.close()
    ring.close()


# ---------------------------------------------------------------------------- 2. tile edges
def edge_case(gpu, orc, union, nrep):
    """One replica point a server, so the union has servers + added + 1 values."""
    servers, add = max(union - 2, 0), 1 if union >= 2 else 0
    rem = 1 if servers else 0
    ring, snap = device_pair(gpu, orc, servers, add, rem, points=1)
    ob, oa = oracle_pair(servers, add, rem, 1)
    want = want_ranges(servers, add, rem, nrep, 1)
    assert want["union"] == union  # (no two of these servers share a token, none is 2^32-1)
    got, counts = ranges_of(ring, snap, nrep)
    assert_ranges(gpu, ring, snap, got, counts, want, oa, servers + add, nrep)
    if union > 2:
        assert counts[0] > 0
    snap.close()
    ring.close()


@pytest.mark.parametrize("nrep", [1, 3])
@pytest.mark.parametrize("union", UNION_SIZES)
def test_tile_edges(gpu, orc, union, nrep):
    edge_case(gpu, orc, union, nrep)


@pytest.mark.parametrize("tile,scan", [(64, 8), (1, 1024), (255, 1), (256, 2)])
def test_small_tiles_and_scan_passes(gpu, orc, monkeypatch, tile, scan):
    """RP_RANGES_TILE / RP_RANGES_SCAN shrink the tile and the scan pass: many tiles, partly filled
    workgroups, and a tile-total scan of several passes with a carry (with the defaults that takes
    more than 262,144 merged elements)."""
    monkeypatch.setenv("RP_RANGES_TILE", str(tile))
    monkeypatch.setenv("RP_RANGES_SCAN", str(scan))
    for union in (513, 4097):
        edge_case(gpu, orc, union, 3)
    ring, snap = device_pair(gpu, orc, 64, 1, 1)
    want = want_ranges(64, 1, 1, 3)
    got, counts = ranges_of(ring, snap, 3)
    assert_ranges(gpu, ring, snap, got, counts, want, oracle_pair(64, 1, 1)[1], 65, 3)


# ---------------------------------------------------------------------------- 5. share identity
@pytest.mark.parametrize("servers,add,rem", [(3, 0, 1), (64, 1, 1), (1000, 10, 10)])
def test_share_identity(gpu, orc, servers, add, rem):
    """n = 1: what a server's hash-space share gained is what flowed in minus what flowed out."""
    ring, snap = device_pair(gpu, orc, servers, add, rem)
    (lo, hi, br, ar), counts = ranges_of(ring, snap, 1)
    bound = ring.id_bound()
    size = hi.astype(np.int64) - lo.astype(np.int64) + 1
    flow = np.zeros(bound + 1, dtype=np.int64)  # (slot `bound`: no owner)
    np.add.at(flow, np.where(ar[:, 0] == NIL, bound, ar[:, 0]), size)
    np.subtract.at(flow, np.where(br[:, 0] == NIL, bound, br[:, 0]), size)
    delta = ring.owner_share_ids().astype(np.int64) - snap.owner_share_ids(bound).astype(np.int64)
    assert np.array_equal(delta, flow[:bound]) and flow[bound] == 0
    share = ring.movedShare(snap)
    assert sum(share.values()) == ring.moved_hash_count == counts[1] > 0
    assert all(a != b for a, b in share)


# ---------------------------------------------------------------------------- 6. custom tokens
def custom_case(gpu, orc, before, steps):
    """Rings of four caller-chosen tokens a server. before: {name: [4 tokens]}; steps: a list of
    (added {name: [4 tokens]}, removed [names]) applied after the snapshot. Returns the device ring,
    its snapshot, both oracle rings and the names in interning order."""
    table = {}

    def learn(d):
        for s, toks in d.items():
            assert len(toks) == 4
            for i, t in enumerate(toks):
                table[s + str(i)] = t

    learn(before)
    for added, _ in steps:
        learn(added)
    ring = gpu.HashRing({"replicaPoints": 4, "hashFunc": lambda s: table[s]})
    ob, oa = orc.Ring(4), orc.Ring(4)
    names = list(before)
    tk = lambda d, ns: np.array([t for s in ns for t in d[s]], dtype=np.uint32)  # noqa: E731
    if names:
        ring.addRemoveServers(names, None)
        ob.add_remove(names, None, add_tokens=tk(before, names))
        oa.add_remove(names, None, add_tokens=tk(before, names))
    snap = ring.snapshot()
    known = dict(before)
    for added, removed in steps:
        ring.addRemoveServers(list(added) or None, removed or None)
        known.update(added)
        oa.add_remove(list(added), removed, add_tokens=tk(added, list(added)) if added else None,
                      rem_tokens=tk(known, removed) if removed else None)
        names += [s for s in added if s not in names]
    assert np.array_equal(ring.dump()[0], oa.dump()[0]) and np.array_equal(snap.dump()[0], ob.dump()[0])
    return ring, snap, ob, oa, names


A4, B4 = [10, 20, 30, 40], [15, 17, 35, 45]
CUSTOM = {
    "zero_after": ({"a": A4, "b": B4}, [({"c": [0, 22, 33, 44]}, [])]),
    "zero_before": ({"a": [0, 20, 30, 40], "b": B4}, [({}, ["a"])]),
    "zero_both": ({"a": [0, 20, 30, 40], "b": B4}, [({"c": [5, 22, 33, 44]}, [])]),
    "top_present": ({"a": [10, 20, 30, TOP], "b": B4}, [({"c": [5, 22, 33, 44]}, [])]),
    "top_added": ({"a": A4, "b": B4}, [({"c": [5, 22, 33, TOP]}, [])]),
    "top_removed": ({"a": [10, 20, 30, TOP], "b": B4}, [({}, ["a"])]),
    "top_absent": ({"a": A4, "b": B4}, [({"c": [5, 22, 33, 44]}, [])]),
    "neighbours": ({"a": [10, 100, 300, 400], "b": [15, 101, 350, 450]}, [({"c": [99, 102, 301, 449]}, ["b"])]),
    "replace": ({"a": A4, "b": B4}, [({}, ["b"]), ({"d": B4}, [])]),
}


@pytest.mark.parametrize("nrep", [-1, 0, 1, 3])
@pytest.mark.parametrize("case", sorted(CUSTOM))
def test_custom_tokens(gpu, orc, case, nrep):
    before, steps = CUSTOM[case]
    ring, snap, ob, oa, names = custom_case(gpu, orc, before, steps)
    want = oracle_ranges(ob, oa, nrep)
    got, counts = ranges_of(ring, snap, nrep)
    assert_ranges(gpu, ring, snap, got, counts, want, oa, len(names), nrep)
    lo, hi, br, ar = got
    assert counts[0] > 0
    if case == "top_absent":
        last = int(ring.dump()[0].max())
        if nrep <= 0:  # above the last token both rows are empty: never moved
            assert int(hi.max()) <= last
        else:  # the top interval wraps to the smallest token, which is the new server's
            assert int(hi[-1]) == TOP and int(lo[-1]) == last + 1 and int(lo[0]) == 0
            assert ar[-1, 0] == ring.server_id("c") == ar[0, 0]
    if case == "replace":  # the union is unchanged and every interval of the old server moves
        assert np.array_equal(ring.dump()[0], snap.dump()[0])
        b, d = ring.server_id("b"), ring.server_id("d")
        if nrep == 1:  # (10, 15] and (15, 17] carry the same pair and are joined
            assert lo.tolist() == [11, 31, 41] and hi.tolist() == [17, 35, 45]
            assert (br[:, 0] == b).all() and (ar[:, 0] == d).all()
        if nrep <= 0:
            assert lo.tolist() == [11, 31, 41] and hi.tolist() == [17, 35, 45]
        if nrep == 3:  # every row holds both servers, so every hash moves
            assert counts[1] == 1 << 32


# ---------------------------------------------------------------------------- 7. empty / equal
@pytest.mark.parametrize("nrep", [0, 1, 3])
def test_empty_and_equal_sides(gpu, orc, nrep):
    names = [orc.c2_addr(i) for i in range(5)]
    ring = gpu.HashRing()
    empty = ring.snapshot()
    none, full = orc.Ring(100), orc.Ring(100)
    full.add_remove(names, None)
    got, counts = ranges_of(ring, empty, nrep)  # both empty
    assert counts == (0, 0) and all(len(x) == 0 for x in got)
    ring.addRemoveServers(names, None)
    got, counts = ranges_of(ring, empty, nrep)  # before empty: joined by the rows now
    assert_ranges(gpu, ring, empty, got, counts, oracle_ranges(none, full, nrep), full, 5, nrep)
    assert (got[2] == NIL).all() and 0 < counts[0] < 501
    if nrep >= 1:
        assert counts[1] == 1 << 32 and int(got[0][0]) == 0 and int(got[1][-1]) == TOP
    snap = ring.snapshot()
    got, counts = ranges_of(ring, snap, nrep)  # unchanged
    assert counts == (0, 0) and all(len(x) == 0 for x in got)
    ring.addRemoveServers(None, names)
    got, counts = ranges_of(ring, snap, nrep)  # now empty: the symmetric case
    assert_ranges(gpu, ring, snap, got, counts, oracle_ranges(full, none, nrep), full, 5, nrep)
    assert (got[3] == NIL).all()
    if nrep >= 1:
        assert counts[1] == 1 << 32
    got, counts = ranges_of(ring, empty, nrep)  # both empty again
    assert counts == (0, 0)


# ---------------------------------------------------------------------------- device helpers
def ranges_dev(call, nrep, cap, alloc, rows=True, arrays=True, **kw):
    """A _dev form over sentinel-filled device outputs of `alloc` entries: call(nrep, cap, lo, hi,
    before, after, count, moved_hashes, **kw) with data pointers."""
    w = max(nrep, 1)
    fill = lambda *shape: torch.full(shape, SENT, dtype=torch.int64, device="cuda").to(torch.int32)  # noqa: E731
    lo, hi = fill(max(alloc, 1)), fill(max(alloc, 1))
    br, ar = fill(max(alloc, 1), w), fill(max(alloc, 1), w)
    cnt = fill(1)
    mh = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    call(nrep, cap, lo.data_ptr() if arrays else None, hi.data_ptr() if arrays else None,
         br.data_ptr() if rows and arrays else None, ar.data_ptr() if rows and arrays else None, cnt.data_ptr(),
         mh.data_ptr(), **kw)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return int(u(cnt)[0]), int(mh.cpu().numpy().view(np.uint64)[0]), u(lo), u(hi), u(br), u(ar)


# ---------------------------------------------------------------------------- 8. cap
def test_cap_bounds_every_write(gpu, orc):
    ring, snap = device_pair(gpu, orc, 64, 1, 1)
    nrep = 3
    (lo, hi, br, ar), (total, moved) = ranges_of(ring, snap, nrep)
    assert total == 571
    call = functools.partial(ring.moved_ranges_dev, snap)
    full = ranges_dev(call, nrep, total + 8, total + 8)
    assert full[:2] == (total, moved)
    for got, want in zip(full[2:], (lo, hi, br, ar)):
        assert np.array_equal(got[:total], want) and (got[total:] == SENT).all()
    for cap in (0, 1, 37, total - 1):
        c = ranges_dev(call, nrep, cap, total + 8)
        assert c[:2] == (total, moved)  # counted in full
        for got, want in zip(c[2:], (lo, hi, br, ar)):
            assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == SENT).all()
    c = ranges_dev(call, nrep, 0, 4, arrays=False)  # cap = 0 with NULL arrays
    assert c[:2] == (total, moved)
    c = ranges_dev(call, nrep, total, total + 8, rows=False)  # no row buffers
    assert c[:2] == (total, moved) and np.array_equal(c[2][:total], lo) and np.array_equal(c[3][:total], hi)
    assert (c[4] == SENT).all() and (c[5] == SENT).all()
    # the host form: a cap below the count, cap = 0 with NULL arrays, and no row buffers
    (l2, h2, b2, a2), counts = ranges_of(ring, snap, nrep, cap=37)
    assert counts == (total, moved) and len(l2) == 37
    assert np.array_equal(l2, lo[:37]) and np.array_equal(h2, hi[:37])
    assert np.array_equal(b2, br[:37]) and np.array_equal(a2, ar[:37])
    cnt, mh = ctypes.c_uint32(), ctypes.c_uint64()
    L = gpu.lib()
    gpu.check(L.rp_ring_moved_ranges(ring._h, snap._h, nrep, 0, None, None, None, None, ctypes.byref(cnt),
                                     ctypes.byref(mh)))
    assert (cnt.value, mh.value) == (total, moved)
    hl = np.full(total + 4, SENT, dtype=np.uint32)
    hh = hl.copy()
    gpu.check(L.rp_ring_moved_ranges(ring._h, snap._h, nrep, 100, hl.ctypes.data, hh.ctypes.data, None, None,
                                     ctypes.byref(cnt), ctypes.byref(mh)))
    assert (cnt.value, mh.value) == (total, moved)
    assert np.array_equal(hl[:100], lo[:100]) and (hl[100:] == SENT).all()
    assert np.array_equal(hh[:100], hi[:100]) and (hh[100:] == SENT).all()


# ---------------------------------------------------------------------------- 9. snapshots
def test_between_two_snapshots(gpu, orc):
    names = [orc.c2_addr(i) for i in range(80)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names[:64], None)
    snap_a = ring.snapshot()
    dump_a = [x.copy() for x in ring.dump()]
    ring.addRemoveServers(names[64:66], names[3:5])
    snap_b = ring.snapshot()
    dump_b = [x.copy() for x in ring.dump()]
    for nrep in (1, 3):
        want, counts = ranges_of(ring, snap_a, nrep)
        assert counts[0] > 0
        got = snap_a.moved_range_ids(snap_b, nrep)
        assert (snap_a.moved_range_count, snap_a.moved_hash_count) == counts
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    want3 = [x.copy() for x in ranges_of(ring, snap_a, 3)[0]]
    ring.addRemoveServers(names[66:80], names[10:20])  # the ring moves on: the snapshots do not
    assert all(np.array_equal(g, w) for g, w in zip(snap_a.moved_range_ids(snap_b, 3), want3))
    assert len(ring.moved_range_ids(snap_b, 3)[0]) > 0
    ring.close()  # and they outlive the ring
    assert all(np.array_equal(g, w) for g, w in zip(snap_a.moved_range_ids(snap_b, 3), want3))
    assert all(len(x) == 0 for x in snap_b.moved_range_ids(snap_b, 3))
    for snap, dump in ((snap_a, dump_a), (snap_b, dump_b)):
        t, o = snap.dump()
        assert np.array_equal(t, dump[0]) and np.array_equal(o, dump[1])
    # the device form between two snapshots, with a cap
    total = len(want3[0])
    c = ranges_dev(functools.partial(snap_a.moved_ranges_dev, snap_b), 3, 50, total + 8)
    assert c[0] == total and np.array_equal(c[2][:50], want3[0][:50]) and (c[2][50:] == SENT).all()
    assert np.array_equal(c[5][:50], want3[3][:50]) and (c[5][50:] == SENT).all()
    assert snap_a.close() == 0 and snap_b.close() == 0


# ---------------------------------------------------------------------------- 10. device form
def test_device_form_on_a_side_stream(gpu, orc):
    ring, snap = device_pair(gpu, orc, 1000, 10, 10)
    (lo, hi, br, ar), (total, moved) = ranges_of(ring, snap, 3)
    assert total == 5909
    side = torch.cuda.Stream()
    call = functools.partial(ring.moved_ranges_dev, snap)
    for kw in ({}, {"stream": side.cuda_stream}, {}):
        c = ranges_dev(call, 3, total + 8, total + 8, **kw)
        assert c[:2] == (total, moved)
        for got, want in zip(c[2:], (lo, hi, br, ar)):
            assert np.array_equal(got[:total], want) and (got[total:] == SENT).all()


# ---------------------------------------------------------------------------- 11. errors, names
def test_argument_errors(gpu, orc):
    ring, snap = device_pair(gpu, orc, 3, 1, 0)
    L = gpu.lib()
    call = functools.partial(ring.moved_ranges_dev, snap)
    with pytest.raises(gpu.RingpopAmdError, match="nrep"):
        ranges_dev(call, 9, 16, 16)
    lo = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    rows = torch.full((16, 9), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    mh = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    rc = L.rp_ring_moved_ranges_dev(ring._h, snap._h, 9, 16, lo.data_ptr(), lo.data_ptr(), rows.data_ptr(),
                                    rows.data_ptr(), cnt.data_ptr(), mh.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"nrep" in L.rp_last_error()
    assert (lo == 7).all() and (rows == 7).all() and (cnt == 7).all() and (mh == 7).all()  # nothing written
    c, m = ctypes.c_uint32(7), ctypes.c_uint64(7)
    hl = np.full(16, 7, dtype=np.uint32)
    for fn, a, b in ((L.rp_ring_moved_ranges, ring._h, snap._h), (L.rp_ring_snap_moved_ranges, snap._h, snap._h)):
        assert fn(a, b, 9, 16, hl.ctypes.data, hl.ctypes.data, None, None, ctypes.byref(c), ctypes.byref(m)) == -1
        assert b"nrep" in L.rp_last_error()
        assert fn(a, None, 3, 16, hl.ctypes.data, hl.ctypes.data, None, None, ctypes.byref(c), ctypes.byref(m)) == -1
        assert b"snapshot" in L.rp_last_error()
    assert L.rp_ring_moved_ranges(ring._h, snap._h, 3, 16, None, None, None, None, ctypes.byref(c),
                                  ctypes.byref(m)) == -1  # a cap without range buffers
    assert (c.value, m.value) == (7, 7) and (hl == 7).all()
    with pytest.raises(gpu.RingpopAmdError):
        ring.moved_range_ids(snap, 9)
    assert L.rp_ring_snap_dump(None, None, None, 0) == -1


def test_moved_ranges_names(gpu, orc):
    """The string-level API: (lo, hi, [names before], [names now])."""
    ring, snap = device_pair(gpu, orc, 64, 1, 1)
    ob, oa = oracle_pair(64, 1, 1)
    want = want_ranges(64, 1, 1, 3)
    names = lambda o, row: [o.name(int(x)) for x in row if x != NIL]  # noqa: E731
    assert ring.movedRanges(snap, 3) == [(int(l), int(h), names(oa, b), names(oa, a)) for l, h, b, a in
                                         zip(want["lo"], want["hi"], want["before"], want["after"])]
    w1 = want_ranges(64, 1, 1, 1)
    share = {}
    for l, h, b, a in zip(w1["lo"], w1["hi"], w1["before"][:, 0], w1["after"][:, 0]):
        k = (oa.name(int(b)), oa.name(int(a)))
        share[k] = share.get(k, 0) + int(h) - int(l) + 1
    assert ring.movedShare(snap) == share


def test_beside_the_lookup_service(gpu, orc):
    ring, snap = device_pair(gpu, orc, 64, 1, 1)
    ring.service(50)
    try:
        key = "some-key"
        first = ring.lookupN(key, 3)  # (starts the resident service)
        got, counts = ranges_of(ring, snap, 3)
        assert counts[0] == 571 and np.array_equal(got[0], want_ranges(64, 1, 1, 3)["lo"])
        assert ring.lookupN(key, 3) == first
    finally:
        ring.service(0)
