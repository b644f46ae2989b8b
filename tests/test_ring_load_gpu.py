"""GPU parity tests of the owner load and the hash-space share through the C ABI
(rp_ring_id_bound, rp_ring_owner_load*, rp_ring_snap_owner_load_dev, rp_ring_owner_share,
rp_ring_snap_owner_share): how many keys each server carries in each lookupN slot, and how many
of the 2^32 hash values it owns.

Oracle: the same add / remove sequence replayed on oracle/liboracle.so (pinned against the
reference's ring goldens in tests/test_oracle.py); its lookupN rows, ids mapped to the device
ring's, counted per slot with np.bincount. Every comparison is an exact integer equality.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
SENT = 0x5A5A5A5A5A5A5A5A
KEY_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 2055, 50_000]


@functools.lru_cache(maxsize=None)
def _keys(n):
    import pyoracle
    k = pyoracle.uuid_keys(42, 0, n)
    k.setflags(write=False)
    return k


def to_gpu_ids(ring, oracle, rows, nnames):
    """Oracle rows with the oracle's interned ids replaced by the device ring's."""
    lut = np.array([ring.server_id(oracle.name(i)) for i in range(nnames)] + [NIL], dtype=np.uint32)
    return lut[np.where(rows == NIL, nnames, rows)]


def want_load(rows, id_bound):
    """[id_bound, W] per-slot bincount of rows [n, W] (NIL padding not counted)."""
    w = rows.shape[1]
    out = np.zeros((id_bound, w), dtype=np.uint64)
    for q in range(w):
        col = rows[:, q]
        out[:, q] = np.bincount(col[col != NIL], minlength=id_bound)
    return out


def pair(gpu, orc, servers):
    """A device ring and its oracle twin with `servers` servers."""
    names = [orc.c2_addr(i) for i in range(servers)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names, None)
    oracle = orc.Ring(100)
    oracle.add_remove(names, None)
    return ring, oracle


def oracle_load(ring, oracle, keys, nrep, nnames, id_bound=None):
    rows = to_gpu_ids(ring, oracle, oracle.lookupn_keys(keys, nrep)[0], nnames)
    return want_load(rows, ring.id_bound() if id_bound is None else id_bound)


def dev_keys(gpu, n, lead=0):
    """n device UUID keys at byte offset `lead` of a fresh buffer."""
    buf = torch.zeros(n * 36 + 16, dtype=torch.uint8, device="cuda")
    if n:
        buf[lead:lead + n * 36] = torch.from_numpy(np.array(_keys(n)).reshape(-1)).cuda()
    return buf


def sent_buf(entries):
    out = torch.full((max(entries, 1),), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (filled before a call on any other stream may write it)
    return out


def u64(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def load_dev(h, keys_ptr, n, nrep, id_cap, out=None, accumulate=False, **kw):
    """owner_load_dev of a ring or a snapshot into `out` (default: a sentinel-filled buffer);
    the [id_cap, W] counters."""
    w = max(nrep, 1)
    if out is None:
        out = sent_buf(id_cap * w)
    h.owner_load_dev(keys_ptr, n, nrep, out.data_ptr(), id_cap, accumulate=accumulate, **kw)
    return u64(out)[:id_cap * w].reshape(id_cap, w)


# ---------------------------------------------------------------------------- 1. parity grid
@pytest.mark.parametrize("nrep", [-2, 0, 1, 3, 5])
@pytest.mark.parametrize("servers", [1, 2, 3, 64, 1000])
def test_parity_grid(gpu, orc, servers, nrep):
    """Every shape here keeps several copies of its bin window (64 copies at 1-3 servers, 8 and 4
    at 1000 servers x 3 and x 5); test_one_copy_at_the_default_window covers the plain path."""
    ring, oracle = pair(gpu, orc, servers)
    assert ring.id_bound() == servers
    keys = _keys(max(KEY_COUNTS))
    rows = to_gpu_ids(ring, oracle, oracle.lookupn_keys(keys, nrep)[0], servers)
    w = max(nrep, 1)
    for n in KEY_COUNTS:
        got = ring.owner_load_ids(keys[:n], nrep)
        assert got.dtype == np.uint64 and got.shape == (servers, w)
        assert np.array_equal(got, want_load(rows[:n], servers)), n
        filled = min(w, servers)
        if nrep >= 1:  # every key has an owner in every slot the ring can fill
            assert (got[:, :filled].sum(axis=0) == n).all()
        else:  # lookupN's single step does not wrap: a key above the last token has no owner
            assert int(got[:, 0].sum()) == int((rows[:n, 0] != NIL).sum()) <= n
        assert (got[:, filled:] == 0).all()
    ring.close()


# ---------------------------------------------------------------------------- 2. windows
def test_bin_windows(gpu, orc, monkeypatch):
    """900 flat bins in one window, in 4 windows of 256 and in 900 windows of 1."""
    ring, oracle = pair(gpu, orc, 300)
    keys = _keys(50_000)
    want = oracle_load(ring, oracle, keys, 3, 300)
    one = ring.owner_load_ids(keys, 3)
    assert np.array_equal(one, want)
    monkeypatch.setenv("RP_LOAD_BINS", "256")
    assert np.array_equal(ring.owner_load_ids(keys, 3), one)
    monkeypatch.setenv("RP_LOAD_BINS", "1")
    got = ring.owner_load_ids(keys[:2055], 3)
    assert np.array_equal(got, oracle_load(ring, oracle, keys[:2055], 3, 300))
    monkeypatch.delenv("RP_LOAD_BINS")
    assert np.array_equal(ring.owner_load_ids(keys[:2055], 3), got)


# ---------------------------------------------------------------------------- 2b. the streaming loop
@pytest.mark.parametrize("nrep", [3, 5])
@pytest.mark.parametrize("servers", [3, 300])
def test_small_grid_reaches_the_unrolled_loop(gpu, orc, monkeypatch, servers, nrep):
    """The default grid covers these inputs in one grid-stride step, so the loop that keeps four
    16-B loads in flight a thread (and the single-load loop after it) would run at most once.
    RP_LOAD_GRID = 1 and 2 make one and two workgroups stream all the rows: 50,000 keys are
    37,500 / 62,500 vectors against a stride of 1,024 / 2,048, and 49,999 keys leave a tail of
    1 / 3 slots (nslots % 4 != 0); with 256-bin windows every window re-reads the rows through
    the same loops."""
    ring, oracle = pair(gpu, orc, servers)
    keys = _keys(50_000)
    rows = to_gpu_ids(ring, oracle, oracle.lookupn_keys(keys, nrep)[0], servers)
    for n in (50_000, 49_999):
        want = want_load(rows[:n], servers)
        assert (n * nrep) % 4 == (0 if n == 50_000 else (1 if nrep == 3 else 3))
        for grid in ("1", "2"):
            monkeypatch.setenv("RP_LOAD_GRID", grid)
            assert np.array_equal(ring.owner_load_ids(keys[:n], nrep), want), (n, grid)
        if servers == 300:  # 900 / 1500 bins: 4 / 6 windows, each one copy of 256 bins or fewer
            monkeypatch.setenv("RP_LOAD_BINS", "256")
            assert np.array_equal(ring.owner_load_ids(keys[:n], nrep), want), (n, "windows")
            monkeypatch.delenv("RP_LOAD_BINS")
        monkeypatch.delenv("RP_LOAD_GRID")
    ring.close()


def test_one_copy_at_the_default_window(gpu, orc, monkeypatch):
    """id_cap 6000 x 3 = 18,000 bins: more than half the default window, so one copy (no
    replication) without any knob; also through the streaming loop."""
    ring, oracle = pair(gpu, orc, 64)
    n = 50_000
    want = np.zeros((6000, 3), dtype=np.uint64)
    want[:64] = oracle_load(ring, oracle, _keys(n), 3, 64)
    buf = dev_keys(gpu, n)
    assert np.array_equal(load_dev(ring, buf.data_ptr(), n, 3, 6000), want)
    monkeypatch.setenv("RP_LOAD_GRID", "1")
    assert np.array_equal(load_dev(ring, buf.data_ptr(), n, 3, 6000), want)


# ---------------------------------------------------------------------------- 3. chunks
def test_chunks(gpu, orc, monkeypatch):
    ring, oracle = pair(gpu, orc, 300)
    counts = (999, 1000, 1001, 2500)
    base = {n: ring.owner_load_ids(_keys(2500)[:n], 3) for n in counts}
    for n in counts:
        assert np.array_equal(base[n], oracle_load(ring, oracle, _keys(2500)[:n], 3, 300))
    monkeypatch.setenv("RP_LOAD_CHUNK", "1000")
    for n in counts:
        assert np.array_equal(ring.owner_load_ids(_keys(2500)[:n], 3), base[n]), n
    # the device form, and variable-length keys (the offsets advance with the chunks)
    buf = dev_keys(gpu, 2500)
    assert np.array_equal(load_dev(ring, buf.data_ptr(), 2500, 3, 300), base[2500])
    skeys = ["k%d" % i * (1 + i % 7) for i in range(2500)]
    chunked = ring.owner_load_ids(skeys, 3)
    monkeypatch.setenv("RP_LOAD_BINS", "256")  # several chunks x several windows
    assert np.array_equal(ring.owner_load_ids(_keys(2500), 3), base[2500])
    monkeypatch.delenv("RP_LOAD_BINS")
    monkeypatch.delenv("RP_LOAD_CHUNK")
    assert np.array_equal(ring.owner_load_ids(skeys, 3), chunked)
    assert chunked[:, 0].sum() == 2500


# ---------------------------------------------------------------------------- 4. sparse ids
def test_sparse_ids_and_id_cap(gpu, orc):
    names = [orc.c2_addr(i) for i in range(23)]
    ring = gpu.HashRing()
    oracle = orc.Ring(100)
    for add, rem in ((names[:20], None), (None, names[3:8]), (names[20:], None)):
        ring.addRemoveServers(add, rem)
        oracle.add_remove(add, rem)
    assert ring.id_bound() == 23 and ring.getServerCount() == 18
    n = 2055
    want = oracle_load(ring, oracle, _keys(n), 3, 23)
    got = ring.owner_load_ids(_keys(n), 3)
    assert np.array_equal(got, want)
    gone = [ring.server_id(s) for s in names[3:8]]
    assert (got[gone] == 0).all() and (got[:, 0] > 0).sum() == 18
    # id_cap below the bound: RP_EINVAL, nothing written (device and host forms)
    buf = dev_keys(gpu, n)
    out = sent_buf(23 * 3)
    with pytest.raises(gpu.RingpopAmdError, match="id_cap"):
        ring.owner_load_dev(buf.data_ptr(), n, 3, out.data_ptr(), 22)
    assert (u64(out) == SENT).all()
    L = gpu.lib()
    host = np.full(23 * 3, SENT, dtype=np.uint64)
    k = np.ascontiguousarray(_keys(n))
    assert L.rp_ring_owner_load(ring._h, k.ctypes.data, None, 36, n, 3, 22, host.ctypes.data) == -1
    assert b"id_cap" in L.rp_last_error() and (host == SENT).all()
    assert L.rp_ring_owner_share(ring._h, 22, host.ctypes.data) == -1 and (host == SENT).all()
    # id_cap above the bound: the extra entries are zero
    big = load_dev(ring, buf.data_ptr(), n, 3, 40)
    assert np.array_equal(big[:23], want) and (big[23:] == 0).all()
    assert L.rp_ring_owner_load(ring._h, k.ctypes.data, None, 36, n, 3, 23, host.ctypes.data) == 0
    assert np.array_equal(host.reshape(23, 3), want)


# ---------------------------------------------------------------------------- 5. accumulate
def test_accumulate(gpu, orc):
    ring, oracle = pair(gpu, orc, 64)
    n, half = 2055, 1000
    want = oracle_load(ring, oracle, _keys(n), 3, 64)
    buf = dev_keys(gpu, n)
    out = sent_buf(64 * 3)
    zero = load_dev(ring, buf.data_ptr(), 0, 3, 64, out=out)  # accumulate = 0 over nothing: cleared
    assert (zero == 0).all()
    first = load_dev(ring, buf.data_ptr(), half, 3, 64, out=out, accumulate=True).copy()
    assert np.array_equal(first, oracle_load(ring, oracle, _keys(n)[:half], 3, 64))
    both = load_dev(ring, buf.data_ptr() + half * 36, n - half, 3, 64, out=out, accumulate=True)
    assert np.array_equal(both, want)
    # accumulate = 0 overwrites whatever the buffer holds
    assert np.array_equal(load_dev(ring, buf.data_ptr(), n, 3, 64), want)
    assert np.array_equal(load_dev(ring, buf.data_ptr(), n, 3, 64, out=out), want)


# ---------------------------------------------------------------------------- 6. key forms
def test_key_forms(gpu, orc):
    ring, oracle = pair(gpu, orc, 64)
    n = 2055
    want = oracle_load(ring, oracle, _keys(n), 3, 64)
    # variable-length keys through offsets
    skeys = ["k%d" % i * (1 + i % 7) for i in range(n)] + ["", "x" * 200]
    rows = np.full((len(skeys), 3), NIL, dtype=np.uint32)
    for i, k in enumerate(skeys):
        rows[i] = oracle.lookupn_hash(orc.hash32(k), 3)
    assert np.array_equal(ring.owner_load_ids(skeys, 3), want_load(to_gpu_ids(ring, oracle, rows, 64), 64))
    # stride 40: the 36 key bytes and 4 more
    k40 = np.zeros((n, 40), dtype=np.uint8)
    k40[:, :36] = _keys(n)
    k40[:, 36:] = np.frombuffer(b"-pad", dtype=np.uint8)
    rows = np.array([oracle.lookupn_hash(orc.hash32(bytes(r)), 3) for r in k40], dtype=np.uint32)
    want40 = want_load(to_gpu_ids(ring, oracle, rows, 64), 64)
    assert np.array_equal(ring.owner_load_ids(k40, 3), want40)
    d40 = torch.from_numpy(k40).cuda()
    assert np.array_equal(load_dev(ring, d40.data_ptr(), n, 3, 64, stride=40), want40)
    # a base that is 4-byte but not 16-byte aligned, and the aligned one
    buf4 = dev_keys(gpu, n, lead=4)
    assert np.array_equal(load_dev(ring, buf4.data_ptr() + 4, n, 3, 64), want)
    assert np.array_equal(load_dev(ring, dev_keys(gpu, n).data_ptr(), n, 3, 64), want)
    # a caller hashFunc's hashes
    hs = np.array([orc.hash32(bytes(k)[::-1]) for k in _keys(n)], dtype=np.uint32)
    rows = np.array([oracle.lookupn_hash(int(h), 3) for h in hs], dtype=np.uint32)
    assert np.array_equal(ring.owner_load_hashes(hs, 3), want_load(to_gpu_ids(ring, oracle, rows, 64), 64))


# ---------------------------------------------------------------------------- 7. empty ring
def test_empty_ring_and_no_keys(gpu, orc):
    ring = gpu.HashRing()
    assert ring.id_bound() == 0
    assert ring.owner_load_ids(_keys(65), 3).shape == (0, 3)
    assert ring.owner_share_ids().shape == (0,)
    assert ring.ownerLoad([], 3) == {} and ring.ownerShare() == {}
    buf = dev_keys(gpu, 65)
    out = sent_buf(8 * 3)
    ring.owner_load_dev(buf.data_ptr(), 65, 3, None, 0)  # id_cap = 0 is accepted, nothing to write
    assert (load_dev(ring, buf.data_ptr(), 65, 3, 8, out=out) == 0).all()
    names = [orc.c2_addr(i) for i in range(5)]
    ring.addRemoveServers(names, None)
    assert (ring.owner_load_ids(_keys(65)[:0], 3) == 0).all()
    assert (load_dev(ring, buf.data_ptr(), 0, 3, 5) == 0).all()
    ring.addRemoveServers(None, names)  # empty again, 5 ids interned
    assert ring.id_bound() == 5
    assert (ring.owner_load_ids(_keys(65), 3) == 0).all()
    assert (ring.owner_share_ids() == 0).all() and ring.owner_share_ids().shape == (5,)


# ---------------------------------------------------------------------------- 8. snapshot
def test_snapshot_load(gpu, orc):
    names = [orc.c2_addr(i) for i in range(74)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names[:64], None)
    snap = ring.snapshot()
    assert snap.id_bound() == 64
    share_before = ring.owner_share_ids()
    ring.addRemoveServers(names[64:], names[5:55:5])
    ob, oa = orc.Ring(100), orc.Ring(100)
    ob.add_remove(names[:64], None)
    oa.add_remove(names[:64], None)
    oa.add_remove(names[64:], names[5:55:5])
    n = 2055
    keys = _keys(n)
    # (oa interned every name ob did, in the same order)
    before = want_load(to_gpu_ids(ring, oa, ob.lookupn_keys(keys, 3)[0], 74), 74)
    after = want_load(to_gpu_ids(ring, oa, oa.lookupn_keys(keys, 3)[0], 74), 74)
    assert not np.array_equal(before, after)
    buf = dev_keys(gpu, n)
    assert np.array_equal(load_dev(snap, buf.data_ptr(), n, 3, 74), before)
    assert np.array_equal(load_dev(snap, buf.data_ptr(), n, 3, 64), before[:64])  # the bound at snapshot time
    assert np.array_equal(ring.owner_load_ids(keys, 3), after)
    out = sent_buf(63 * 3)
    with pytest.raises(gpu.RingpopAmdError, match="id_cap"):
        snap.owner_load_dev(buf.data_ptr(), n, 3, out.data_ptr(), 63)
    assert (u64(out) == SENT).all()
    # share: the snapshot keeps the share before the change
    assert np.array_equal(snap.owner_share_ids(), share_before)
    assert not np.array_equal(ring.owner_share_ids()[:64], share_before)
    # variable-length keys and accumulate under the snapshot
    half = 1000
    out = sent_buf(74 * 3)
    load_dev(snap, buf.data_ptr(), half, 3, 74, out=out)
    assert np.array_equal(load_dev(snap, buf.data_ptr() + half * 36, n - half, 3, 74, out=out, accumulate=True),
                          before)
    # the ring goes first
    h, ring._h = ring._h, None
    assert gpu.lib().rp_ring_destroy(h) == 0
    assert np.array_equal(load_dev(snap, buf.data_ptr(), n, 3, 74), before)
    assert np.array_equal(snap.owner_share_ids(), share_before)
    assert snap.close() == 0


# ---------------------------------------------------------------------------- 9. a foreign stream
def test_side_stream_after_a_ring_change(gpu, orc):
    names = [orc.c2_addr(i) for i in range(1010)]
    ring = gpu.HashRing()
    oracle = orc.Ring(100)
    ring.addRemoveServers(names[:1000], None)
    oracle.add_remove(names[:1000], None)
    n = 50_000
    buf = dev_keys(gpu, n)
    out = sent_buf(1010 * 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ring.addRemoveServers(names[1000:], names[100:1000:100])
    oracle.add_remove(names[1000:], names[100:1000:100])
    ring.owner_load_dev(buf.data_ptr(), n, 3, out.data_ptr(), 1010, stream=side.cuda_stream)
    side.synchronize()
    want = oracle_load(ring, oracle, _keys(n), 3, 1010)
    assert np.array_equal(u64(out).reshape(1010, 3), want)
    # back on the null stream, then the side stream again: the scratch is ordered across streams
    assert np.array_equal(load_dev(ring, buf.data_ptr(), n, 3, 1010), want)
    assert np.array_equal(load_dev(ring, buf.data_ptr(), n, 3, 1010, stream=side.cuda_stream), want)


# ---------------------------------------------------------------------------- 10. share
def want_share(ring):
    """The numpy restatement from the sorted (token, owner) arrays."""
    tok, own = ring.dump()
    out = np.zeros(ring.id_bound(), dtype=np.uint64)
    if len(tok):
        t = tok.astype(np.int64)
        d = np.empty(len(t), dtype=np.int64)
        d[1:] = t[1:] - t[:-1]
        d[0] = t[0] + (1 << 32) - t[-1]
        np.add.at(out, own, d.astype(np.uint64))
    return out


@pytest.mark.parametrize("servers,points", [(1, 1), (3, 100), (1000, 100)])
def test_share(gpu, orc, servers, points):
    ring = gpu.HashRing({"replicaPoints": points})
    ring.addRemoveServers([orc.c2_addr(i) for i in range(servers)], None)
    got = ring.owner_share_ids()
    assert got.dtype == np.uint64 and got.shape == (servers,)
    assert np.array_equal(got, want_share(ring))
    assert int(got.sum()) == 1 << 32
    if servers == 1:  # one token owns every hash value
        assert ring.size == 1 and int(got[0]) == 1 << 32
    if servers == 1000:  # even to within a factor of two of 2^32 / 1000 on this ring
        assert got.min() > 0


def test_share_with_edge_tokens(gpu, orc):
    """Caller tokens at 0 and at 2^32 - 1: the wrap term is 1 for token 0."""
    fixed = {"a0": 0, "b0": 0xFFFFFFFF}

    def hf(s):
        return fixed.get(s, orc.hash32(s))

    ring = gpu.HashRing({"replicaPoints": 2, "hashFunc": hf})
    ring.addRemoveServers(["a", "b", "c"], None)
    tok, _ = ring.dump()
    assert tok[0] == 0 and tok[-1] == 0xFFFFFFFF and len(tok) == 6
    got = ring.owner_share_ids()
    assert np.array_equal(got, want_share(ring)) and int(got.sum()) == 1 << 32
    snap = ring.snapshot()
    ring.addRemoveServers(["d"], ["a"])
    assert np.array_equal(snap.owner_share_ids(), got)
    now = ring.owner_share_ids()
    assert np.array_equal(now, want_share(ring)) and int(now.sum()) == 1 << 32 and now[ring.server_id("a")] == 0


# ---------------------------------------------------------------------------- 11. names
def test_names(gpu, orc):
    names = [orc.c2_addr(i) for i in range(20)]
    ring = gpu.HashRing()
    ring.addRemoveServers(names, None)
    ring.addRemoveServers(None, names[3:8])
    skeys = [bytes(k).decode() for k in _keys(2055)]
    load = ring.owner_load_ids(skeys, 3)
    share = ring.owner_share_ids()
    got = ring.ownerLoad(skeys, 3)
    assert list(got) == list(ring.servers) and len(got) == 15
    assert got == {s: [int(x) for x in load[ring.server_id(s)]] for s in ring.servers}
    assert sum(v[0] for v in got.values()) == 2055
    sh = ring.ownerShare()
    assert list(sh) == list(ring.servers)
    assert sh == {s: int(share[ring.server_id(s)]) for s in ring.servers} and sum(sh.values()) == 1 << 32


# ---------------------------------------------------------------------------- arguments
def test_argument_errors(gpu, orc):
    ring, _ = pair(gpu, orc, 3)
    L = gpu.lib()
    out = sent_buf(9)
    assert L.rp_ring_owner_load_dev(ring._h, None, None, 36, 10, 3, 3, 0, out.data_ptr(), None) == -1
    assert b"null key buffer" in L.rp_last_error()
    buf = dev_keys(gpu, 10)
    assert L.rp_ring_owner_load_dev(ring._h, buf.data_ptr(), None, 36, 10, 3, 3, 0, None, None) == -1
    assert L.rp_ring_snap_owner_load_dev(None, buf.data_ptr(), None, 36, 10, 3, 3, 0, out.data_ptr(), None) == -1
    assert b"snapshot" in L.rp_last_error()
    assert L.rp_ring_snap_owner_share(None, 3, None) == -1
    assert L.rp_ring_id_bound(ring._h, None) == -1
    assert (u64(out) == SENT).all()
    v = ctypes.c_uint32()
    assert L.rp_ring_id_bound(ring._h, ctypes.byref(v)) == 0 and v.value == 3
