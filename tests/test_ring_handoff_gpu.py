"""GPU parity tests of the hand-off plan through the C ABI (rp_ring_handoff*): which keys to send
to whom after a ring change, grouped by destination.

Oracle: the same add / remove sequence replayed on oracle/liboracle.so; its lookupN rows before and
after; the numpy model of the semantics (tests/handoff_model.py, itself pinned by a store
simulation in tests/test_handoff_model.py). Bit-exact: all five arrays and the count.
"""
import ctypes

import numpy as np
import pytest

import handoff_model as hm
import ring_key_forms as kf
from test_ring_moved_gpu import SENT, _keys, changed_pair, dev_keys, names_for, oracle_rows, to_gpu_ids

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
KEY_COUNTS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2055, 50_000]
GRID = [(1, 1, 0), (2, 1, 0), (3, 0, 1), (64, 1, 1), (64, 0, 32), (1000, 10, 10)]
NAMES = ("dests", "group_off", "key_idx", "src", "slot")


def in_ring_mask(ring):
    m = np.zeros(ring.id_bound(), dtype=bool)
    m[ring.server_ids()] = True
    return m


def assert_plan(got, count, want):
    """got: the five arrays; want: the model's (five arrays, count)."""
    assert count == want[5], (count, want[5])
    for name, g, w in zip(NAMES, got, want[:5]):
        assert g.dtype == w.dtype, (name, g.dtype, w.dtype)
        assert np.array_equal(g, w), (name, len(g), len(w))


# ---------------------------------------------------------------------------- 1. parity grid
@pytest.mark.parametrize("nrep", [-2, 0, 1, 3, 8])
@pytest.mark.parametrize("servers,add,rem", GRID)
def test_parity_grid(gpu, orc, servers, add, rem, nrep):
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, servers, add, rem)
    keys = _keys(max(KEY_COUNTS))
    wb, wa = oracle_rows(ring, ob, oa, keys, nrep, nnames)
    mask = in_ring_mask(ring)
    for n in KEY_COUNTS:
        want = hm.plan(wb[:n], wa[:n], mask)
        assert_plan(ring.handoff_ids(keys[:n], snap, nrep), ring.handoff_count, want)
    # the expectations themselves (tests/test_handoff_model.py pins the same figures on the CPU)
    dests, goff, kidx, src, slot, count = want
    moved = int((wb != wa).any(axis=1).sum())
    orphans = int((hm.sources(wb, mask) == NIL).sum())
    if (servers, add, rem) == (64, 1, 1) and nrep == 3:
        assert (moved, count, len(dests), orphans) == (4537, 4537, 61, 0)
    if (servers, add, rem) == (64, 1, 1) and nrep == 1:
        assert (count, orphans) == (1460, 693)
    if (servers, add, rem) == (64, 0, 32) and nrep == 3:
        assert (count, moved, int(np.bincount(kidx).max()), orphans) == (75199, 44392, 3, 5757)
    if (servers, add, rem) == (64, 0, 32) and nrep == 8:
        assert (count, int(np.bincount(kidx).max())) == (200711, 8)
    if (servers, add, rem) == (3, 0, 1) and nrep in (3, 8):
        assert (moved, count) == (50_000, 0)  # rows only shrink: moved, and nothing to send
    if (servers, add, rem) == (1000, 10, 10) and nrep == 3:
        assert (count, len(np.unique(kidx)), len(dests)) == (2901, 2880, 609)
    snap.close()
    ring.close()


# ---------------------------------------------------------------------------- 2. only_src
def test_only_src(gpu, orc):
    servers, add, rem, nrep, n = 64, 1, 32, 3, 10_000
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, servers, add, rem)
    initial, added, removed = names_for(orc, servers, add, rem)
    keys = _keys(n)
    wb, wa = oracle_rows(ring, ob, oa, keys, nrep, nnames)
    mask = in_ring_mask(ring)
    full = hm.plan(wb, wa, mask)
    assert_plan(ring.handoff_ids(keys, snap, nrep), ring.handoff_count, full)
    survivor = next(s for s in initial if s not in removed)
    # a survivor, a removed server, and one that never held anything (it joined after the snapshot)
    sizes = []
    for name in (survivor, removed[0], added[0]):
        sid = ring.server_id(name)
        want = hm.plan(wb, wa, mask, only_src=sid)
        got = ring.handoff_ids(keys, snap, nrep, only_src=sid)
        assert_plan(got, ring.handoff_count, want)
        assert (got[3] == sid).all()
        sizes.append(ring.handoff_count)
    assert sizes[0] > 0 and sizes[1] == 0 and sizes[2] == 0
    # the filtered plans over all live servers, plus the orphans, partition the unfiltered stream
    seen = [(int(k), int(q)) for k, q, s in zip(full[2], full[4], full[3]) if s == NIL]
    assert len(seen) > 0
    for sid in ring.server_ids():
        d, go, k, s, q = ring.handoff_ids(keys, snap, nrep, only_src=int(sid))
        assert_plan((d, go, k, s, q), ring.handoff_count, hm.plan(wb, wa, mask, only_src=int(sid)))
        seen += list(zip(k.tolist(), q.tolist()))
    assert len(seen) == full[5] and sorted(seen) == sorted(zip(full[2].tolist(), full[4].tolist()))
    # the name-level form of one node's share
    plan = ring.handoffPlan([bytes(k).decode() for k in keys[:2055]], snap, nrep, whoami=survivor)
    assert plan and all(s == survivor for recs in plan.values() for _, s in recs)
    assert ring.handoffPlan(["a"], snap, nrep, whoami="10.9.9.9:1") == {}  # never interned


# ---------------------------------------------------------------------------- device helpers
def u32(t):
    return t.cpu().numpy().view(np.uint32)


def handoff_dev(ring, snap, keys_ptr, n, nrep, cap, alloc, only_src=NIL, opt=True, **kw):
    """rp_ring_handoff_dev over sentinel-filled outputs: `alloc` record entries, id_bound + 8
    destination entries. Returns (count, ndest, dests, group_off, key_idx, src, slot) in full."""
    nd = ring.id_bound() + 8
    full = lambda k: torch.full((k,), SENT, dtype=torch.int64, device="cuda").to(torch.int32)  # noqa: E731
    dests, goff, kidx, src = full(nd), full(nd + 1), full(max(alloc, 1)), full(max(alloc, 1))
    slot = torch.full((max(alloc, 1),), 0x5A, dtype=torch.uint8, device="cuda")
    ndest, cnt = full(1), full(1)
    ring.handoff_dev(snap, keys_ptr, n, nrep, cap, dests.data_ptr(), goff.data_ptr(), kidx.data_ptr(),
                     src.data_ptr() if opt else None, slot.data_ptr() if opt else None, ndest.data_ptr(),
                     cnt.data_ptr(), only_src=only_src, **kw)
    torch.cuda.synchronize()
    return int(u32(cnt)[0]), int(u32(ndest)[0]), u32(dests), u32(goff), u32(kidx), u32(src), slot.cpu().numpy()


def handoff_hashes(gpu, ring, snap, hashes, nrep, cap, alloc, only_src=NIL):
    """rp_ring_handoff_hashes over sentinel-filled host outputs, shaped as handoff_dev's result."""
    nd = ring.id_bound() + 8
    full = lambda k: np.full(k, SENT, dtype=np.uint32)  # noqa: E731
    dests, goff, kidx, src = full(nd), full(nd + 1), full(max(alloc, 1)), full(max(alloc, 1))
    slot = np.full(max(alloc, 1), 0x5A, dtype=np.uint8)
    ndest, cnt = ctypes.c_uint32(SENT), ctypes.c_uint32(SENT)
    h = np.ascontiguousarray(hashes, dtype=np.uint32)
    gpu.check(gpu.lib().rp_ring_handoff_hashes(ring._h, snap._h, h.ctypes.data, len(h), nrep, only_src, cap,
                                               dests.ctypes.data, goff.ctypes.data, kidx.ctypes.data, src.ctypes.data,
                                               slot.ctypes.data, ctypes.byref(ndest), ctypes.byref(cnt)))
    return cnt.value, ndest.value, dests, goff, kidx, src, slot


def assert_dev(res, want, cap, id_bound):
    """The device result equals the model's plan and nothing at or past the stated capacities
    (dests: min(cap, id bound), group_off: one more, key_idx / src / slot: cap) is touched."""
    count, ndest, dests, goff, kidx, src, slot = res
    wd, wg, wk, ws, wq, wcount = want
    t = min(wcount, cap)
    assert count == wcount and ndest == len(wd) and len(wk) == t
    assert np.array_equal(dests[:ndest], wd) and np.array_equal(goff[:ndest + 1], wg)
    assert np.array_equal(kidx[:t], wk) and np.array_equal(src[:t], ws) and np.array_equal(slot[:t], wq)
    dcap = min(cap, id_bound)
    assert (dests[dcap:] == SENT).all() and (goff[dcap + 1:] == SENT).all()
    assert (kidx[cap:] == SENT).all() and (src[cap:] == SENT).all() and (slot[cap:] == 0x5A).all()


# ---------------------------------------------------------------------------- 3. cap
def test_cap_bounds_every_write(gpu, orc):
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, 64, 0, 32)
    n, nrep = 10_000, 3
    wb, wa = oracle_rows(ring, ob, oa, _keys(n), nrep, nnames)
    mask = in_ring_mask(ring)
    key, dst, src, slot = hm.record_stream(wb, wa, mask)
    total = len(key)
    assert total > n  # several records a key
    # a cap that cuts inside one key's records: just after the first record of a key with more
    inside = int(np.flatnonzero(key[1:] == key[:-1])[0]) + 1
    assert key[inside - 1] == key[inside]
    keys = dev_keys(gpu, n)
    bound = ring.id_bound()
    for cap in (0, 1, total - 1, total, total + 7, inside):
        res = handoff_dev(ring, snap, keys.data_ptr(), n, nrep, cap, total + 16)
        assert_dev(res, hm.plan(wb, wa, mask, cap=cap), cap, bound)
    # cap = 0 with no arrays at all: the counts only
    cnt = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    ring.handoff_dev(snap, keys.data_ptr(), n, nrep, 0, None, None, None, None, None, cnt[1:].data_ptr(),
                     cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt.tolist() == [total, 0]
    # no src / slot buffers
    res = handoff_dev(ring, snap, keys.data_ptr(), n, nrep, total, total + 16, opt=False)
    want = hm.plan(wb, wa, mask)
    assert res[0] == total and np.array_equal(res[4][:total], want[2]) and np.array_equal(res[2][:res[1]], want[0])
    assert (res[5] == SENT).all() and (res[6] == 0x5A).all()
    # the host form below the count
    for cap in (1, inside, total - 1):
        assert_plan(ring.handoff_ids(_keys(n), snap, nrep, cap=cap), ring.handoff_count,
                    hm.plan(wb, wa, mask, cap=cap))


# ---------------------------------------------------------------------------- 4. empty sides
def test_empty_sides_and_no_keys(gpu, orc):
    keys = _keys(513)
    names = [orc.c2_addr(i) for i in range(5)]
    for nrep in (1, 3):
        w = max(nrep, 1)
        ring = gpu.HashRing()
        empty = ring.snapshot()
        d, go, k, s, q = ring.handoff_ids(keys, empty, nrep)  # both empty
        assert len(d) == 0 and go.tolist() == [0] and len(k) == 0 and ring.handoff_count == 0
        ring.addRemoveServers(names, None)
        oracle = orc.Ring(100)
        oracle.add_remove(names, None)
        rows = to_gpu_ids(ring, oracle, oracle.lookupn_keys(keys, nrep)[0], 5)
        none = np.full((513, w), NIL, dtype=np.uint32)
        mask = in_ring_mask(ring)
        want = hm.plan(none, rows, mask)  # before empty: every key yields its whole row, no source
        assert want[5] == 513 * min(w, 5)
        got = ring.handoff_ids(keys, empty, nrep)
        assert_plan(got, ring.handoff_count, want)
        assert (got[3] == NIL).all()
        full = ring.snapshot()
        d, go, k, s, q = ring.handoff_ids(keys[:0], full, nrep)  # no keys
        assert len(d) == 0 and go.tolist() == [0] and len(k) == 0 and ring.handoff_count == 0
        d, go, k, s, q = ring.handoff_ids(keys, full, nrep)  # no change
        assert len(d) == 0 and go.tolist() == [0] and len(k) == 0 and ring.handoff_count == 0
        ring.addRemoveServers(None, names)
        d, go, k, s, q = ring.handoff_ids(keys, full, nrep)  # ring now empty: nothing is gained
        assert len(d) == 0 and go.tolist() == [0] and len(k) == 0 and ring.handoff_count == 0
        # the device form writes ndest = 0 and group_off[0] = 0 in these cases too
        dk = dev_keys(gpu, 513)
        res = handoff_dev(ring, full, dk.data_ptr(), 513, nrep, 100, 100)
        assert res[0] == 0 and res[1] == 0 and res[3][0] == 0 and (res[4] == SENT).all()
        res = handoff_dev(ring, full, dk.data_ptr(), 0, nrep, 100, 100)
        assert res[0] == 0 and res[1] == 0 and res[3][0] == 0


# ---------------------------------------------------------------------------- 5. key forms
def queued_change(gpu, orc, servers=64, add=1, rem=32):
    """changed_pair, with one more ring change made just before the caller's device call (on the
    ring's own stream; the call runs on another)."""
    initial, added, removed = names_for(orc, servers, add, rem)
    ring = gpu.HashRing()
    ring.addRemoveServers(initial, None)
    snap = ring.snapshot()
    ob, oa = orc.Ring(100), orc.Ring(100)
    ob.add_remove(initial, None)
    oa.add_remove(initial, None)
    oa.add_remove(added, removed)
    return ring, snap, ob, oa, servers + add, (added, removed)


@pytest.mark.parametrize("nrep", [1, 3, 8])
def test_key_forms_on_a_side_stream(gpu, orc, nrep):
    n = 2055
    side = torch.cuda.Stream()
    kw = {"stream": side.cuda_stream}
    for form in kf.FORMS:
        ring, snap, ob, oa, nnames, change = queued_change(gpu, orc)
        ptr, extra, keep = kf.device_side(form, n)
        wb, wa = kf.oracle_rows(ob, form, n, nrep), kf.oracle_rows(oa, form, n, nrep)
        torch.cuda.synchronize()
        ring.addRemoveServers(*change)  # queued just before the call on the other stream
        wb, wa = to_gpu_ids(ring, oa, wb, nnames), to_gpu_ids(ring, oa, wa, nnames)
        mask = in_ring_mask(ring)
        want = hm.plan(wb, wa, mask)
        assert want[5] > 0, form
        cap = want[5] + 9
        if form == "hashes":  # (the host entry point: the ring's own stream)
            res = handoff_hashes(gpu, ring, snap, keep, nrep, cap, cap + 8)
        else:
            res = handoff_dev(ring, snap, ptr, n, nrep, cap, cap + 8, **extra, **kw)
        assert_dev(res, want, cap, ring.id_bound())
        snap.close()
        ring.close()


def test_caller_hashes_with_forced_collisions(gpu, orc):
    """options.hashFunc with hash % 2000 (as the ring goldens do): tokens collide, first insert
    wins, rows can change order only. The host hashes form."""
    def hf(s):
        return orc.hash32(s) % 2000

    servers, nkeys = 50, 3000
    names = [orc.c2_addr(i) for i in range(servers)]
    extra = [orc.c2_addr(servers + i) for i in range(2)]
    gone = names[3:5]
    tk = lambda ns: np.array([hf(s + str(i)) for s in ns for i in range(100)], dtype=np.uint32)  # noqa: E731
    skeys = ["key-%d" % i for i in range(nkeys)]
    for nrep in (1, 3, 8):
        ring = gpu.HashRing({"hashFunc": hf})
        ring.addRemoveServers(names, None)
        snap = ring.snapshot()
        ring.addRemoveServers(extra, gone)
        ob, oa = orc.Ring(100), orc.Ring(100)
        ob.add_remove(names, None, add_tokens=tk(names))
        oa.add_remove(names, None, add_tokens=tk(names))
        oa.add_remove(extra, gone, add_tokens=tk(extra), rem_tokens=tk(gone))
        w = max(nrep, 1)
        wb = np.full((nkeys, w), NIL, dtype=np.uint32)
        wa = wb.copy()
        for i, k in enumerate(skeys):
            b, a = ob.lookupn_hash(hf(k), nrep), oa.lookupn_hash(hf(k), nrep)
            wb[i, :len(b)] = b
            wa[i, :len(a)] = a
        wb, wa = to_gpu_ids(ring, oa, wb, servers + 2), to_gpu_ids(ring, oa, wa, servers + 2)
        want = hm.plan(wb, wa, in_ring_mask(ring))
        assert 0 < want[5]
        assert_plan(ring.handoff_ids(skeys, snap, nrep), ring.handoff_count, want)


# ---------------------------------------------------------------------------- 6. names
def test_handoff_plan_names(gpu, orc):
    """The string-level API against a plan built from lookupn_hash per key."""
    ring, snap, ob, oa, _ = changed_pair(gpu, orc, 64, 1, 1)
    initial, added, removed = names_for(orc, 64, 1, 1)
    now = set(initial + added) - set(removed)
    skeys = [bytes(k).decode() for k in _keys(2055)]
    by_dest = {}
    for k in skeys:
        h = orc.hash32(k)
        b = [ob.name(x) for x in ob.lookupn_hash(h, 3)]
        a = [oa.name(x) for x in oa.lookupn_hash(h, 3)]
        src = next((s for s in b if s in now), None)
        for d in a:
            if d not in b:
                by_dest.setdefault(d, []).append((k, src))
    want = {d: by_dest[d] for d in sorted(by_dest, key=ring.server_id)}
    assert 0 < sum(map(len, want.values())) < len(skeys)
    got = ring.handoffPlan(skeys, snap, 3)
    assert list(got) == list(want) and got == want


# ---------------------------------------------------------------------------- 7. arguments
def test_argument_errors(gpu, orc):
    ring, snap, _, _, _ = changed_pair(gpu, orc, 3, 1, 0)
    L = gpu.lib()
    n = 300
    keys = dev_keys(gpu, n)
    mk = lambda k: torch.full((k,), 7, dtype=torch.int32, device="cuda")  # noqa: E731
    dests, goff, kidx, src, cnt = mk(16), mk(17), mk(n * 9), mk(n * 9), mk(2)
    slot = torch.full((n * 9,), 7, dtype=torch.uint8, device="cuda")

    def call(ringh, snaph, nrep, only_src, nkeys=n):
        rc = L.rp_ring_handoff_dev(ringh, snaph, keys.data_ptr(), None, 36, nkeys, nrep, only_src, n,
                                   dests.data_ptr(), goff.data_ptr(), kidx.data_ptr(), src.data_ptr(),
                                   slot.data_ptr(), cnt[1:].data_ptr(), cnt.data_ptr(), None)
        torch.cuda.synchronize()
        for t in (dests, goff, kidx, src, cnt, slot):
            assert (t == 7).all()  # nothing written
        return rc, L.rp_last_error()

    rc, err = call(ring._h, snap._h, 9, NIL)
    assert rc == -1 and b"nrep" in err
    rc, err = call(ring._h, None, 3, NIL)
    assert rc == -1 and b"snapshot" in err
    rc, err = call(None, snap._h, 3, NIL)
    assert rc == -1 and b"ring" in err
    rc, err = call(ring._h, snap._h, 3, ring.id_bound())
    assert rc == -1 and b"only_src" in err
    rc, err = call(ring._h, snap._h, 3, NIL, nkeys=(1 << 32) // 3 + 1)  # n * W >= 2^32
    assert rc == -1 and b"2^32" in err
    c, nd = ctypes.c_uint32(7), ctypes.c_uint32(7)
    k = np.ascontiguousarray(_keys(n))
    h = np.full(n * 9, 7, dtype=np.uint32)
    hs = np.full(n * 9, 7, dtype=np.uint8)
    args = (h.ctypes.data, h.ctypes.data, h.ctypes.data, h.ctypes.data, hs.ctypes.data, ctypes.byref(nd),
            ctypes.byref(c))
    assert L.rp_ring_handoff(ring._h, snap._h, k.ctypes.data, None, 36, n, 9, NIL, n, *args) == -1
    assert L.rp_ring_handoff(ring._h, None, k.ctypes.data, None, 36, n, 3, NIL, n, *args) == -1
    assert L.rp_ring_handoff(ring._h, snap._h, k.ctypes.data, None, 36, n, 3, ring.id_bound() + 5, n, *args) == -1
    assert L.rp_ring_handoff_hashes(ring._h, None, h.ctypes.data, n, 3, NIL, n, *args) == -1
    assert L.rp_ring_handoff_hashes(ring._h, snap._h, h.ctypes.data, n, 9, NIL, n, *args) == -1
    assert c.value == 7 and nd.value == 7 and (h == 7).all() and (hs == 7).all()
    with pytest.raises(gpu.RingpopAmdError):
        ring.handoff_ids(_keys(10), snap, 9)
