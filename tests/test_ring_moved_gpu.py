"""GPU parity tests of ring snapshots and the fused moved-keys call through the C ABI
(rp_ring_snapshot, rp_ring_snap_*, rp_ring_moved_keys*): which keys changed hands between a
snapshot and the ring now, for hand-off after ringChanged (lib/ring/index.js:87-93).

Oracle: the same add / remove sequence replayed on oracle/liboracle.so (pinned against the
reference's ring goldens in tests/test_oracle.py); lookupN rows before and after; a key has moved
iff its two rows differ. Bit-exact: the moved indices equal np.flatnonzero(rows differ) (so they
are ascending and complete) and both row arrays equal the oracle's rows at those indices.
"""
import ctypes
import functools

import numpy as np
import pytest

import ring_key_forms as kf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
SENT = 0x5A5A5A5A
# wave / workgroup / 512-key streamer edges, and the moved-keys kernels' own tiles (256 generic,
# 512 for rows of 5-8 owners, 1024 for rows of up to 4) +- 1
KEY_COUNTS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2055, 50_000]
GRID = [(1, 1, 0), (2, 1, 0), (3, 0, 1), (64, 1, 1), (1000, 10, 10)]


@functools.lru_cache(maxsize=None)
def _keys(n):
    import pyoracle
    k = pyoracle.uuid_keys(42, 0, n)
    k.setflags(write=False)
    return k


def names_for(orc, servers, add, rem):
    """(initial, added, removed): removed are spread over the initial servers."""
    initial = [orc.c2_addr(i) for i in range(servers)]
    added = [orc.c2_addr(servers + j) for j in range(add)]
    removed = [initial[(j * 7 + 1) % servers] for j in range(rem)]
    return initial, added, removed


def to_gpu_ids(ring, oracle, rows, nnames):
    """Oracle rows with the oracle's interned ids replaced by the device ring's."""
    lut = np.array([ring.server_id(oracle.name(i)) for i in range(nnames)] + [NIL], dtype=np.uint32)
    return lut[np.where(rows == NIL, nnames, rows)]


def changed_pair(gpu, orc, servers, add, rem):
    """Device ring + snapshot of `servers` servers, then +add / -rem; the oracle twin before and
    after. Returns (ring, snap, oracle_before, oracle_after, number of names)."""
    initial, added, removed = names_for(orc, servers, add, rem)
    ring = gpu.HashRing()
    ring.addRemoveServers(initial, None)
    snap = ring.snapshot()
    ring.addRemoveServers(added, removed)
    ob, oa = orc.Ring(100), orc.Ring(100)
    ob.add_remove(initial, None)
    oa.add_remove(initial, None)
    oa.add_remove(added, removed)
    return ring, snap, ob, oa, servers + add


def oracle_rows(ring, ob, oa, keys, nrep, nnames):
    wb, _ = ob.lookupn_keys(keys, nrep)
    wa, _ = oa.lookupn_keys(keys, nrep)
    # (oa interned every name ob did, in the same order)
    return to_gpu_ids(ring, oa, wb, nnames), to_gpu_ids(ring, oa, wa, nnames)


def assert_moved(got, wb, wa, n):
    idx, br, ar = got
    want = np.flatnonzero((wb[:n] != wa[:n]).any(axis=1))
    assert idx.dtype == np.uint32 and np.array_equal(idx, want), (len(idx), len(want))
    assert np.array_equal(br, wb[want])
    assert np.array_equal(ar, wa[want])
    return len(want)


# ---------------------------------------------------------------------------- 1. parity grid
@pytest.mark.parametrize("nrep", [-2, 0, 1, 3, 8])
@pytest.mark.parametrize("servers,add,rem", GRID)
def test_parity_grid(gpu, orc, servers, add, rem, nrep):
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, servers, add, rem)
    keys = _keys(max(KEY_COUNTS))
    wb, wa = oracle_rows(ring, ob, oa, keys, nrep, nnames)
    moved = {}
    for n in KEY_COUNTS:
        moved[n] = assert_moved(ring.moved_ids(keys[:n], snap, nrep), wb, wa, n)
        assert ring.moved_count == moved[n]
    if servers >= 64:  # the expectation itself is a partial, non-trivial set
        assert 0 < moved[50_000] < 50_000 // 2
    if (servers, nrep) in ((2, 3), (3, 3)):  # the list length changes: every key moved
        assert moved[513] == 513
    snap.close()
    ring.close()


def test_moved_keys_names(gpu, orc):
    """The string-level API: (key, [names before], [names now]) in input order."""
    ring, snap, ob, oa, _ = changed_pair(gpu, orc, 64, 1, 1)
    skeys = [bytes(k).decode() for k in _keys(2055)]
    want = []
    for k in skeys:
        h = orc.hash32(k)
        b = [ob.name(x) for x in ob.lookupn_hash(h, 3)]
        a = [oa.name(x) for x in oa.lookupn_hash(h, 3)]
        if a != b:
            want.append((k, b, a))
    assert 0 < len(want) < len(skeys)
    assert ring.movedKeys(skeys, snap, 3) == want


# ---------------------------------------------------------------------------- 2. empty sides
def test_empty_sides(gpu, orc):
    keys = _keys(513)
    names = [orc.c2_addr(i) for i in range(5)]
    for nrep in (1, 3):
        w = max(nrep, 1)
        ring = gpu.HashRing()
        empty = ring.snapshot()
        assert empty.info() == {"tokens": 0, "servers": 0, "checksum": None}
        idx, br, ar = ring.moved_ids(keys, empty, nrep)  # both empty
        assert len(idx) == 0 and ring.moved_count == 0
        ring.addRemoveServers(names, None)
        oracle = orc.Ring(100)
        oracle.add_remove(names, None)
        rows = to_gpu_ids(ring, oracle, oracle.lookupn_keys(keys, nrep)[0], 5)
        idx, br, ar = ring.moved_ids(keys, empty, nrep)  # before empty: every key moved
        assert np.array_equal(idx, np.arange(513, dtype=np.uint32))
        assert (br == NIL).all() and br.shape == (513, w)
        assert np.array_equal(ar, rows)
        full = ring.snapshot()
        ring.addRemoveServers(None, names)
        idx, br, ar = ring.moved_ids(keys, full, nrep)  # now empty: the symmetric case
        assert np.array_equal(idx, np.arange(513, dtype=np.uint32))
        assert np.array_equal(br, rows)
        assert (ar == NIL).all() and ar.shape == (513, w)
        idx, _, _ = ring.moved_ids(keys[:0], full, nrep)  # no keys
        assert len(idx) == 0 and ring.moved_count == 0
        idx, _, _ = ring.moved_ids(keys, empty, nrep)  # both empty again
        assert len(idx) == 0 and ring.moved_count == 0


# ---------------------------------------------------------------------------- 3. no change
def test_no_change(gpu, orc):
    keys = _keys(2055)
    names = [orc.c2_addr(i) for i in range(64)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names, None)
    snap = ring.snapshot()
    for nrep in (1, 3, 8):
        assert len(ring.moved_ids(keys, snap, nrep)[0]) == 0 and ring.moved_count == 0
    extra = [orc.c2_addr(64 + i) for i in range(3)]
    ring.addRemoveServers(extra, None)
    assert len(ring.moved_ids(keys, snap, 3)[0]) > 0
    ring.addRemoveServers(None, extra)  # the same tokens again, the ids are stable
    for nrep in (-2, 1, 3, 8):
        assert len(ring.moved_ids(keys, snap, nrep)[0]) == 0 and ring.moved_count == 0


# ---------------------------------------------------------------------------- device helpers
def dev_keys(gpu, n, lead=0):
    """n device UUID keys at byte offset `lead` of a fresh buffer."""
    buf = torch.zeros(n * 36 + 16, dtype=torch.uint8, device="cuda")
    if lead == 0:
        gpu.gen_uuid_keys_dev(42, 0, n, buf.data_ptr())
    else:
        buf[lead:lead + n * 36] = torch.from_numpy(np.array(_keys(n)).reshape(-1)).cuda()
    return buf


def moved_dev(ring, snap, keys_ptr, n, nrep, cap, alloc, rows=True, **kw):
    """rp_ring_moved_keys_dev over sentinel-filled outputs of `alloc` entries."""
    w = max(nrep, 1)
    idx = torch.full((max(alloc, 1),), SENT, dtype=torch.int64, device="cuda").to(torch.int32)
    br = torch.full((max(alloc, 1), w), SENT, dtype=torch.int64, device="cuda").to(torch.int32)
    ar = br.clone()
    cnt = torch.full((1,), SENT, dtype=torch.int64, device="cuda").to(torch.int32)
    ring.moved_dev(snap, keys_ptr, n, nrep, cap, idx.data_ptr(), br.data_ptr() if rows else None,
                   ar.data_ptr() if rows else None, cnt.data_ptr(), **kw)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return int(u(cnt)[0]), u(idx), u(br), u(ar)


# ---------------------------------------------------------------------------- 4. cap
def test_cap_bounds_every_write(gpu, orc):
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, 64, 1, 1)
    n, nrep = 10_000, 3
    wb, wa = oracle_rows(ring, ob, oa, _keys(n), nrep, nnames)
    want = np.flatnonzero((wb != wa).any(axis=1))
    total = len(want)
    assert total > 40
    keys = dev_keys(gpu, n)
    cnt, idx, br, ar = moved_dev(ring, snap, keys.data_ptr(), n, nrep, n, n)  # uncapped
    assert cnt == total
    assert np.array_equal(idx[:total], want) and (idx[total:] == SENT).all()
    assert np.array_equal(br[:total], wb[want]) and (br[total:] == SENT).all()
    assert np.array_equal(ar[:total], wa[want]) and (ar[total:] == SENT).all()
    for cap in (0, 1, 37, total - 1):
        c2, i2, b2, a2 = moved_dev(ring, snap, keys.data_ptr(), n, nrep, cap, total + 8)
        assert c2 == total  # counted in full
        assert np.array_equal(i2[:cap], idx[:cap]) and (i2[cap:] == SENT).all()
        assert np.array_equal(b2[:cap], br[:cap]) and (b2[cap:] == SENT).all()
        assert np.array_equal(a2[:cap], ar[:cap]) and (a2[cap:] == SENT).all()
    # no row buffers at all
    c3, i3, b3, a3 = moved_dev(ring, snap, keys.data_ptr(), n, nrep, n, n, rows=False)
    assert c3 == total and np.array_equal(i3[:total], want) and (i3[total:] == SENT).all()
    assert (b3 == SENT).all() and (a3 == SENT).all()
    # the host form: cap below the count, and no row buffers
    i4, b4, a4 = ring.moved_ids(_keys(n), snap, nrep, cap=37)
    assert ring.moved_count == total and np.array_equal(i4, want[:37])
    assert np.array_equal(b4, wb[want[:37]]) and np.array_equal(a4, wa[want[:37]])
    c = ctypes.c_uint32()
    hidx = np.full(total, SENT, dtype=np.uint32)
    k = np.ascontiguousarray(_keys(n))
    gpu.check(gpu.lib().rp_ring_moved_keys(ring._h, snap._h, k.ctypes.data, None, 36, n, nrep, total,
                                           hidx.ctypes.data, None, None, ctypes.byref(c)))
    assert c.value == total and np.array_equal(hidx, want)


# ---------------------------------------------------------------------------- 5. generic path
def test_generic_variable_length_keys(gpu, orc):
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, 64, 1, 1)
    skeys = ["k%d" % i * (1 + i % 7) for i in range(2055)] + ["", "x" * 200]
    for nrep in (1, 3, 8):
        w = max(nrep, 1)
        wb = np.full((len(skeys), w), NIL, dtype=np.uint32)
        wa = wb.copy()
        for i, k in enumerate(skeys):
            h = orc.hash32(k)
            b, a = ob.lookupn_hash(h, nrep), oa.lookupn_hash(h, nrep)
            wb[i, :len(b)] = b
            wa[i, :len(a)] = a
        wb, wa = to_gpu_ids(ring, oa, wb, nnames), to_gpu_ids(ring, oa, wa, nnames)
        m = assert_moved(ring.moved_ids(skeys, snap, nrep), wb, wa, len(skeys))
        assert 0 < m < len(skeys)


@pytest.mark.parametrize("n", [255, 257, 2055])
def test_generic_unaligned_base(gpu, orc, n):
    """36-byte stride, the base offset by one byte: the per-thread byte path."""
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, 64, 1, 1)
    wb, wa = oracle_rows(ring, ob, oa, _keys(n), 3, nnames)
    want = np.flatnonzero((wb != wa).any(axis=1))
    buf = dev_keys(gpu, n, lead=1)
    cnt, idx, br, ar = moved_dev(ring, snap, buf.data_ptr() + 1, n, 3, n, n)
    assert cnt == len(want) and np.array_equal(idx[:cnt], want)
    assert np.array_equal(br[:cnt], wb[want]) and np.array_equal(ar[:cnt], wa[want])
    # and at a 4-byte (not 16-byte) aligned base: the fixed-stride kernel's dword staging
    buf4 = dev_keys(gpu, n, lead=4)
    cnt, idx, br, ar = moved_dev(ring, snap, buf4.data_ptr() + 4, n, 3, n, n)
    assert cnt == len(want) and np.array_equal(idx[:cnt], want)
    assert np.array_equal(br[:cnt], wb[want]) and np.array_equal(ar[:cnt], wa[want])


@pytest.mark.parametrize("form", kf.FORMS)
@pytest.mark.parametrize("nrep", [1, 3, 8])
def test_key_forms(gpu, orc, nrep, form):
    """Every key form through every kernel shape (rows of 1, up to 4, up to 8 owners). 2,055 keys:
    two full 1,024-key tiles + 7 and four full 512-key tiles + 7, so a launch has full tiles and a
    partial last one."""
    n = 2055
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, 64, 1, 1)
    wb = to_gpu_ids(ring, oa, kf.oracle_rows(ob, form, n, nrep), nnames)
    wa = to_gpu_ids(ring, oa, kf.oracle_rows(oa, form, n, nrep), nnames)
    ptr, extra, keep = kf.device_side(form, n)
    if form == "hashes":  # (only the host entry point takes them)
        w = max(nrep, 1)
        idx = np.full(n, SENT, dtype=np.uint32)
        br, ar = np.full((n, w), SENT, dtype=np.uint32), np.full((n, w), SENT, dtype=np.uint32)
        c = ctypes.c_uint32(SENT)
        gpu.check(gpu.lib().rp_ring_moved_hashes(ring._h, snap._h, keep.ctypes.data, n, nrep, n, idx.ctypes.data,
                                                 br.ctypes.data, ar.ctypes.data, ctypes.byref(c)))
        cnt = c.value
    else:
        cnt, idx, br, ar = moved_dev(ring, snap, ptr, n, nrep, n, n, **extra)
    assert 0 < cnt < n
    assert (idx[cnt:] == SENT).all() and (br[cnt:] == SENT).all() and (ar[cnt:] == SENT).all()
    assert assert_moved((idx[:cnt], br[:cnt], ar[:cnt]), wb, wa, n) == cnt
    snap.close()
    ring.close()


def hash_func_case(gpu, orc, hf, servers, nkeys, nrep):
    names = [orc.c2_addr(i) for i in range(servers)]
    extra = [orc.c2_addr(servers + i) for i in range(2)]
    gone = names[3:5]
    tk = lambda ns: np.array([hf(s + str(i)) for s in ns for i in range(100)], dtype=np.uint32)  # noqa: E731
    ring = gpu.HashRing({"hashFunc": hf})
    ring.addRemoveServers(names, None)
    snap = ring.snapshot()
    ring.addRemoveServers(extra, gone)
    ob, oa = orc.Ring(100), orc.Ring(100)
    ob.add_remove(names, None, add_tokens=tk(names))
    oa.add_remove(names, None, add_tokens=tk(names))
    oa.add_remove(extra, gone, add_tokens=tk(extra), rem_tokens=tk(gone))
    skeys = ["key-%d" % i for i in range(nkeys)]
    w = max(nrep, 1)
    wb = np.full((nkeys, w), NIL, dtype=np.uint32)
    wa = wb.copy()
    for i, k in enumerate(skeys):
        b, a = ob.lookupn_hash(hf(k), nrep), oa.lookupn_hash(hf(k), nrep)
        wb[i, :len(b)] = b
        wa[i, :len(a)] = a
    wb, wa = to_gpu_ids(ring, oa, wb, servers + 2), to_gpu_ids(ring, oa, wa, servers + 2)
    return ring, assert_moved(ring.moved_ids(skeys, snap, nrep), wb, wa, nkeys)


def test_hash_func_uses_the_hashes_form(gpu, orc):
    """options.hashFunc (lib/ring/index.js:29): the caller's key hashes drive the diff."""
    def hf(s):
        return orc.hash32(s[::-1])

    for nrep in (1, 3):
        _, m = hash_func_case(gpu, orc, hf, 50, 3000, nrep)
        assert 0 < m < 3000


def test_forced_token_collisions(gpu, orc):
    """A hashFunc mapping the replica strings onto 1,024 values, all in one bucket of the top
    token bits: tokens collide (first insert wins) and no compact layout can be built."""
    def hf(s):
        return orc.hash32(s) & 0x3FF

    for nrep in (1, 3):
        ring, m = hash_func_case(gpu, orc, hf, 50, 3000, nrep)
        assert ring.size <= 1024
        assert 0 < m <= 3000


# ---------------------------------------------------------------------------- 6. lifetime
def test_snapshot_outlives_ring_changes_and_the_ring(gpu, orc):
    names = [orc.c2_addr(i) for i in range(1000)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names[:3], None)
    want_info = {"tokens": ring.size, "servers": ring.getServerCount(), "checksum": ring.checksum}
    snap = ring.snapshot()
    ob, oa = orc.Ring(100), orc.Ring(100)
    ob.add_remove(names[:3], None)
    oa.add_remove(names[:3], None)
    for lo, hi in ((3, 10), (10, 64), (64, 300), (300, 1000)):  # layouts switch, buffers regrow
        ring.addRemoveServers(names[lo:hi], None)
        oa.add_remove(names[lo:hi], None)
    assert snap.info() == want_info and ring.size > 90_000
    n = 2055
    wb, wa = oracle_rows(ring, ob, oa, _keys(n), 3, 1000)
    keys = dev_keys(gpu, n)
    rows = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    cnts = torch.empty(n, dtype=torch.uint8, device="cuda")
    snap.lookupn_dev(keys.data_ptr(), n, 3, rows.data_ptr(), cnts.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), wb)
    assert (cnts.cpu().numpy() == 3).all()
    assert_moved(ring.moved_ids(_keys(n), snap, 3), wb, wa, n)
    # the ring goes first
    h, ring._h = ring._h, None
    assert gpu.lib().rp_ring_destroy(h) == 0
    snap.lookupn_dev(keys.data_ptr(), n, 3, rows.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), wb)
    assert snap.close() == 0


# ---------------------------------------------------------------------------- 7. at size
def test_device_form_at_size(gpu, orc):
    """The C2 ring (10k servers) -10 / +10, 2^20 device keys, n = 3: the fused list equals the two
    device lookups (each pinned by the lookup parity tests) compared in torch; on the null stream
    and on a side stream."""
    names = [orc.c2_addr(i) for i in range(10_010)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names[:10_000], None)
    snap = ring.snapshot()
    ring.addRemoveServers(names[10_000:], names[100:1100:100])
    n = 1 << 20
    keys = dev_keys(gpu, n)
    now = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    was = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    ring.lookupn_dev(keys.data_ptr(), n, 3, now.data_ptr())
    snap.lookupn_dev(keys.data_ptr(), n, 3, was.data_ptr())
    torch.cuda.synchronize()
    want = torch.nonzero((now != was).any(dim=1)).flatten()
    total = int(want.numel())
    assert 1000 < total < n // 50  # sparse, not empty (the oracle: 423 of 2^16 on this shape)
    want_idx = want.cpu().numpy().astype(np.uint32)
    want_b = was[want].cpu().numpy().view(np.uint32)
    want_a = now[want].cpu().numpy().view(np.uint32)
    side = torch.cuda.Stream()
    for stream in (None, side):
        kw = {} if stream is None else {"stream": stream.cuda_stream}
        cnt, idx, br, ar = moved_dev(ring, snap, keys.data_ptr(), n, 3, total + 64, total + 64, **kw)
        assert cnt == total
        assert np.array_equal(idx[:total], want_idx) and (idx[total:] == SENT).all()
        assert np.array_equal(br[:total], want_b) and np.array_equal(ar[:total], want_a)


# ---------------------------------------------------------------------------- 8. arguments
def test_argument_errors(gpu, orc):
    ring, snap, _, _, _ = changed_pair(gpu, orc, 3, 1, 0)
    L = gpu.lib()
    n = 300
    keys = dev_keys(gpu, n)
    idx = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    rows = torch.full((n, 9), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rc = L.rp_ring_moved_keys_dev(ring._h, snap._h, keys.data_ptr(), None, 36, n, 9, n, idx.data_ptr(),
                                  rows.data_ptr(), rows.data_ptr(), cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"nrep" in L.rp_last_error()
    assert (idx == 7).all() and (rows == 7).all() and (cnt == 7).all()  # nothing written
    rc = L.rp_ring_moved_keys_dev(ring._h, None, keys.data_ptr(), None, 36, n, 3, n, idx.data_ptr(), None, None,
                                  cnt.data_ptr(), None)
    assert rc == -1 and b"snapshot" in L.rp_last_error()
    c = ctypes.c_uint32(7)
    k = np.ascontiguousarray(_keys(n))
    hidx = np.full(n, 7, dtype=np.uint32)
    assert L.rp_ring_moved_keys(ring._h, snap._h, k.ctypes.data, None, 36, n, 9, n, hidx.ctypes.data, None, None,
                                ctypes.byref(c)) == -1
    assert L.rp_ring_moved_keys(ring._h, None, k.ctypes.data, None, 36, n, 3, n, hidx.ctypes.data, None, None,
                                ctypes.byref(c)) == -1
    assert L.rp_ring_moved_hashes(ring._h, None, hidx.ctypes.data, n, 3, n, hidx.ctypes.data, None, None,
                                  ctypes.byref(c)) == -1
    assert c.value == 7 and (hidx == 7).all()
    with pytest.raises(gpu.RingpopAmdError):
        ring.moved_ids(_keys(10), snap, 9)
    assert L.rp_ring_snapshot(ring._h, None) == -1
    assert L.rp_ring_snap_info(None, None, None, None, None) == -1
    assert L.rp_ring_snap_destroy(None) == 0


# ---------------------------------------------------------------------------- 9. service
def test_moved_keys_beside_the_lookup_service(gpu, orc):
    ring, snap, ob, oa, nnames = changed_pair(gpu, orc, 64, 1, 1)
    ring.service(50)
    try:
        key = bytes(_keys(1)[0]).decode()
        want1 = [oa.name(x) for x in oa.lookupn_hash(orc.hash32(key), 3)]
        assert ring.lookupN(key, 3) == want1  # (starts the resident service)
        wb, wa = oracle_rows(ring, ob, oa, _keys(2055), 3, nnames)
        assert_moved(ring.moved_ids(_keys(2055), snap, 3), wb, wa, 2055)
        assert ring.lookupN(key, 3) == want1
        assert ring.lookup(key) == want1[0]
    finally:
        ring.service(0)
