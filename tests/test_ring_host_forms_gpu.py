"""GPU characterisation of the ring's three C-ABI forms: for lookup / lookupN, grouping, moved keys,
the hand-off plan, owner load and routing agreement, the host form over key bytes, the host form
over caller hashes and the _dev form over device buffers give identical results on the same ring
and snapshot. Every output array and count is compared, bit-exact; there is no oracle here, the
forms are pinned against each other (the parity tests of each operation hold them to the oracle).

Rings: 5 servers x 3 points and 40 servers x 100 points, each with a snapshot taken before two
servers were removed and one was added. Key sources: fixed 36-byte keys (stride 36), the same bytes
through offsets, variable keys of 1 to 70 bytes (offsets), and hash32 of either as caller hashes;
within one key set all sources must agree. Key counts sit where the host path changes course: 0,
1, 64 (the small path's last count), 65, 64 keys of 60 bytes (over the small path's 3,072 bytes)
and 1,100 (past 4 x 256: the tiled path and a partial tile). Grouping and routing agreement are
lookup-only (no replica count). The lookup service stays off.

The argument errors are rejected on the host; their texts are the ones the C ABI has carried since
each entry point was added.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
SENT = 0x5A5A5A5A
RINGS = {"5x3": (5, 3), "40x100": (40, 100)}
KEY_SETS = ["0", "1", "64", "65", "64x60", "1100"]


# ---------------------------------------------------------------------------- rings and keys
class Pair:
    """A ring of `servers` servers now, and the snapshot from before two left and one joined."""

    def __init__(self, gpu, servers, points):
        names = ["10.30.%d.%d:%d" % (i // 200, i % 200, 3000 + i % 7) for i in range(servers + 2)]
        self.ring = gpu.HashRing({"replicaPoints": points})
        self.ring.addRemoveServers(names[:servers + 1], None)
        self.snap = self.ring.snapshot()
        self.ring.addRemoveServers([names[servers + 1]], [names[1], names[servers // 2 + 1]])
        assert self.ring.getServerCount() == servers and self.snap.info()["servers"] == servers + 1
        self.h, self.s, self.idb = self.ring._h, self.snap._h, self.ring.id_bound()
        self.servers = servers


@pytest.fixture(scope="module")
def pairs(gpu):
    out = {k: Pair(gpu, *v) for k, v in RINGS.items()}
    yield out
    for p in out.values():
        p.snap.close()
        p.ring.close()


class Src:
    """One key source: bytes with a stride or offsets, or hashes; on the host or on the device."""

    def __init__(self, label, n, blob=None, off=None, stride=0, hashes=None, dev=False):
        self.label, self.n, self.stride, self.dev = label, n, stride, dev
        if dev:  # (the byte buffer keeps a 16-byte tail, as the ring's own staging buffer does)
            blob = None if blob is None else torch.from_numpy(np.concatenate([blob, np.zeros(16, np.uint8)])).cuda()
            off = None if off is None else torch.from_numpy(off.view(np.int64)).cuda()
            hashes = None if hashes is None else torch.from_numpy(hashes.view(np.int32).copy()).cuda()
        self.blob, self.off, self.hashes = blob, off, hashes

    @staticmethod
    def _p(a):
        return None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)

    @property
    def kargs(self):
        return self._p(self.blob), self._p(self.off), self.stride

    @property
    def hptr(self):
        return self._p(self.hashes)


def _hashes(gpu, blob, off):
    b = blob.tobytes()
    return np.array([gpu.hash32(b[off[i]:off[i + 1]]) for i in range(len(off) - 1)], dtype=np.uint32)


@pytest.fixture(scope="module")
def key_sets(gpu):
    """{name: [groups]}; a group is a list of sources over the same keys, which must all agree."""
    rng = np.random.default_rng(20240611)
    out = {}
    for name in KEY_SETS:
        n, width = (int(name.split("x")[0]), int(name.split("x")[1])) if "x" in name else (int(name), 36)
        fixed = rng.integers(33, 127, size=(n, width), dtype=np.uint8)
        foff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(width))
        fblob = np.concatenate([fixed.reshape(-1), np.zeros(1, np.uint8)])  # (never an empty buffer)
        fh = _hashes(gpu, fblob, foff)
        groups = [[Src("stride", n, fblob, None, width), Src("offsets", n, fblob, foff, 0),
                   Src("hashes", n, hashes=fh), Src("dev stride", n, fblob, None, width, dev=True),
                   Src("dev offsets", n, fblob, foff, 0, dev=True), Src("dev hashes", n, hashes=fh, dev=True)]]
        if width == 36:  # variable keys of 1 to 70 bytes
            lens = rng.integers(1, 71, size=n)
            if n >= 2:
                lens[0], lens[-1] = 1, 70
            voff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            vblob = rng.integers(33, 127, size=int(voff[-1]) + 1, dtype=np.uint8)
            vh = _hashes(gpu, vblob, voff)
            groups.append([Src("var offsets", n, vblob, voff, 0), Src("var hashes", n, hashes=vh),
                           Src("var dev offsets", n, vblob, voff, 0, dev=True)])
        out[name] = groups
    yield out
    out.clear()  # (the device copies go with the module)


def host(count, dtype=np.uint32):
    fill = {np.uint32: SENT, np.uint8: 0x5A, np.uint64: 0x5A5A5A5A5A5A5A5A}[dtype]
    return np.full(max(int(count), 1), fill, dtype=dtype)


def dev(count, dtype=np.uint32):
    return torch.from_numpy(host(count, dtype).view({np.uint32: np.int32, np.uint8: np.uint8,
                                                     np.uint64: np.int64}[dtype])).cuda()


def buf(src, count, dtype=np.uint32):
    return dev(count, dtype) if src.dev else host(count, dtype)


def ptr(a):
    return None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def val(a, dtype=np.uint32):
    if isinstance(a, torch.Tensor):
        torch.cuda.synchronize()
        return a.cpu().numpy().view(dtype)
    return a


def ok(L, rc):
    assert rc == 0, L.rp_last_error()


def agree(results, what):
    """results: [(label, tuple of arrays / ints)]; every one equals the first."""
    l0, r0 = results[0]
    for label, r in results[1:]:
        assert len(r) == len(r0), (what, label)
        for i, (a, b) in enumerate(zip(r0, r)):
            assert np.array_equal(a, b), (what, l0, label, i)


# ---------------------------------------------------------------------------- the operations
def run_lookupn(L, p, src, nrep, counts=True):
    w = max(nrep, 1)
    out, cnt = buf(src, src.n * w), (buf(src, src.n, np.uint8) if counts else None)
    if src.hashes is not None:
        fn = L.rp_ring_lookupn_hashes_dev if src.dev else L.rp_ring_lookupn_hashes
        ok(L, fn(p.h, src.hptr, src.n, nrep, ptr(out), ptr(cnt), *([None] if src.dev else [])))
    else:
        fn = L.rp_ring_lookupn_dev if src.dev else L.rp_ring_lookupn
        ok(L, fn(p.h, *src.kargs, src.n, nrep, ptr(out), ptr(cnt), *([None] if src.dev else [])))
    res = (val(out)[:src.n * w],)
    return res + ((val(cnt, np.uint8)[:src.n],) if counts else ())


def run_lookup(L, p, src):
    out = buf(src, src.n)
    if src.hashes is not None and src.dev:  # (no rp_ring_lookup_hashes_dev: the one-step walk by its other name)
        ok(L, L.rp_ring_lookupn_hashes_dev(p.h, src.hptr, src.n, 1, ptr(out), None, None))
    elif src.hashes is not None:
        ok(L, L.rp_ring_lookup_hashes(p.h, src.hptr, src.n, ptr(out)))
    elif src.dev:
        ok(L, L.rp_ring_lookup_dev(p.h, *src.kargs, src.n, ptr(out), None))
    else:
        ok(L, L.rp_ring_lookup(p.h, *src.kargs, src.n, ptr(out)))
    return (val(out)[:src.n],)


def run_group(L, p, src, self_id):
    n = src.n
    dests, goff, perm, nd = buf(src, n), buf(src, n + 1), buf(src, n), buf(src, 1)
    outs = (ptr(dests), ptr(goff), ptr(perm), ptr(nd))
    if src.dev:
        if src.hashes is not None:
            return None  # (grouping has no device form over hashes)
        ok(L, L.rp_ring_group_keys_dev(p.h, *src.kargs, n, self_id, *outs, None))
    elif src.hashes is not None:
        ok(L, L.rp_ring_group_hashes(p.h, src.hptr, n, self_id, *outs))
    else:
        ok(L, L.rp_ring_group_keys(p.h, *src.kargs, n, self_id, *outs))
    g = int(val(nd)[0])
    assert g <= min(n, p.servers + 1)
    return g, val(dests)[:g], val(goff)[:g + 1], val(perm)[:n]


def run_moved(L, p, src, nrep, cap, rows=True):
    w, n = max(nrep, 1), src.n
    idx, cnt = buf(src, cap), buf(src, 1)
    br, ar = (buf(src, cap * w), buf(src, cap * w)) if rows else (None, None)
    outs = (cap, ptr(idx), ptr(br), ptr(ar), ptr(cnt))
    if src.dev:
        if src.hashes is not None:
            return None
        ok(L, L.rp_ring_moved_keys_dev(p.h, p.s, *src.kargs, n, nrep, *outs, None))
    elif src.hashes is not None:
        ok(L, L.rp_ring_moved_hashes(p.h, p.s, src.hptr, n, nrep, *outs))
    else:
        ok(L, L.rp_ring_moved_keys(p.h, p.s, *src.kargs, n, nrep, *outs))
    count = int(val(cnt)[0])
    m = min(count, cap)
    res = (count, val(idx)[:m])
    return res + ((val(br)[:m * w], val(ar)[:m * w]) if rows else ())


def run_handoff(L, p, src, nrep, cap, only_src=NIL, opt=True):
    n = src.n
    dests, goff = buf(src, p.idb + 8), buf(src, p.idb + 9)
    kidx, nd, cnt = buf(src, cap), buf(src, 1), buf(src, 1)
    sr, sl = (buf(src, cap), buf(src, cap, np.uint8)) if opt else (None, None)
    outs = (only_src, cap, ptr(dests), ptr(goff), ptr(kidx), ptr(sr), ptr(sl), ptr(nd), ptr(cnt))
    if src.dev:
        if src.hashes is not None:
            return None
        ok(L, L.rp_ring_handoff_dev(p.h, p.s, *src.kargs, n, nrep, *outs, None))
    elif src.hashes is not None:
        ok(L, L.rp_ring_handoff_hashes(p.h, p.s, src.hptr, n, nrep, *outs))
    else:
        ok(L, L.rp_ring_handoff(p.h, p.s, *src.kargs, n, nrep, *outs))
    count, g = int(val(cnt)[0]), int(val(nd)[0])
    t = min(count, cap)
    res = (count, g, val(dests)[:g], val(goff)[:g + 1], val(kidx)[:t])
    return res + ((val(sr)[:t], val(sl, np.uint8)[:t]) if opt else ())


def run_load(L, p, src, nrep, id_cap):
    w = max(nrep, 1)
    load = buf(src, id_cap * w, np.uint64)
    if src.dev:
        if src.hashes is not None:
            return None
        ok(L, L.rp_ring_owner_load_dev(p.h, *src.kargs, src.n, nrep, id_cap, 0, ptr(load), None))
    elif src.hashes is not None:
        ok(L, L.rp_ring_owner_load_hashes(p.h, src.hptr, src.n, nrep, id_cap, ptr(load)))
    else:
        ok(L, L.rp_ring_owner_load(p.h, *src.kargs, src.n, nrep, id_cap, ptr(load)))
    return (val(load, np.uint64)[:id_cap * w],)


def run_route(L, p, src, allowed, truth, opt=True):
    n, (nv, rs) = src.n, allowed.shape
    up = (lambda a: None if a is None else torch.from_numpy(a).cuda()) if src.dev else (lambda a: a)
    rows, tr = up(allowed), up(truth)
    # (not accumulating: the counters are set, whatever they held)
    wrong, lost = buf(src, nv, np.uint64), buf(src, nv, np.uint64)
    kw, to, ow = (buf(src, n), buf(src, n), buf(src, n * nv)) if opt else (None, None, None)
    keys = (None, None, 0, src.hptr) if src.hashes is not None else src.kargs + (None,)
    fn = L.rp_ring_route_views_dev if src.dev else L.rp_ring_route_views
    ok(L, fn(p.h, *keys, n, ptr(rows), rs, 1, nv, None, p.idb, ptr(tr), None, 0, ptr(wrong), ptr(lost), ptr(kw),
             ptr(to), ptr(ow), *([None] if src.dev else [])))
    res = (val(wrong, np.uint64)[:nv], val(lost, np.uint64)[:nv])
    return res + ((val(kw)[:n], val(to)[:n], val(ow)[:n * nv]) if opt else ())


def each_group(key_sets, fn):
    for name in KEY_SETS:
        for group in key_sets[name]:
            res = [(s.label, fn(s)) for s in group]
            res = [(l, r) for l, r in res if r is not None]
            assert len(res) >= 3, name  # host keys, host hashes and a device form at the least
            agree(res, name)


# ---------------------------------------------------------------------------- 1. the six operations
@pytest.mark.parametrize("which", list(RINGS))
def test_lookup_forms_agree(gpu, pairs, key_sets, which):
    L, p = gpu.lib(), pairs[which]
    each_group(key_sets, lambda s: run_lookup(L, p, s))
    for nrep in (0, 1, 3, 6, p.servers + 2):  # (the last: more replicas than servers, before and now)
        each_group(key_sets, lambda s: run_lookupn(L, p, s, nrep))
    each_group(key_sets, lambda s: run_lookupn(L, p, s, 3, counts=False))
    # a full row on the big ring, a short one where nrep exceeds the servers
    rows, cnt = run_lookupn(L, p, key_sets["1100"][0][0], p.servers + 2)
    assert (cnt == p.servers).all() and (rows.reshape(1100, -1)[:, p.servers:] == NIL).all()


@pytest.mark.parametrize("which", list(RINGS))
def test_group_forms_agree(gpu, pairs, key_sets, which):
    L, p = gpu.lib(), pairs[which]
    for self_id in (NIL, 0):
        each_group(key_sets, lambda s: run_group(L, p, s, self_id))
    g, dests, goff, perm = run_group(L, p, key_sets["1100"][0][0], NIL)
    assert len(set(dests)) == g <= p.servers and goff[g] == 1100 and sorted(perm) == list(range(1100))


@pytest.mark.parametrize("which", list(RINGS))
def test_moved_forms_agree(gpu, pairs, key_sets, which):
    L, p = gpu.lib(), pairs[which]
    for nrep in (1, 3, 8) + ((p.servers + 2,) if p.servers + 2 <= 8 else ()):
        for name in KEY_SETS:
            for group in key_sets[name]:
                n = group[0].n
                count = run_moved(L, p, group[0], nrep, n)[0]
                caps = [n] + ([count // 2] if count >= 2 else []) + [0]  # all, a cut list, the count only
                for cap in caps:
                    res = [(s.label, run_moved(L, p, s, nrep, cap)) for s in group]
                    res = [(l, r) for l, r in res if r is not None]
                    assert len(res) >= 3 and res[0][1][0] == count and len(res[0][1][1]) == min(count, cap)
                    agree(res, (name, nrep, cap))
                if name == "1100":
                    assert 2 <= count <= n
    each_group(key_sets, lambda s: run_moved(L, p, s, 3, s.n, rows=False))


@pytest.mark.parametrize("which", list(RINGS))
def test_handoff_forms_agree(gpu, pairs, key_sets, which):
    L, p = gpu.lib(), pairs[which]
    for nrep in (1, 3, 8) + ((p.servers + 2,) if p.servers + 2 <= 8 else ()):
        w = max(nrep, 1)
        for name in KEY_SETS:
            for group in key_sets[name]:
                n = group[0].n
                count = run_handoff(L, p, group[0], nrep, n * w)[0]
                caps = [n * w] + ([count // 2] if count >= 2 else []) + [0]
                for cap in caps:
                    res = [(s.label, run_handoff(L, p, s, nrep, cap)) for s in group]
                    res = [(l, r) for l, r in res if r is not None]
                    assert len(res) >= 3 and res[0][1][0] == count and len(res[0][1][4]) == min(count, cap)
                    agree(res, (name, nrep, cap))
                if name == "1100":
                    assert 2 <= count
    each_group(key_sets, lambda s: run_handoff(L, p, s, 3, s.n * 3, opt=False))
    only = int(p.ring.server_ids()[0])  # what one surviving server has to send
    each_group(key_sets, lambda s: run_handoff(L, p, s, 3, s.n * 3, only_src=only))


@pytest.mark.parametrize("which", list(RINGS))
def test_owner_load_forms_agree(gpu, pairs, key_sets, which):
    L, p = gpu.lib(), pairs[which]
    for nrep in (1, 3, 6, p.servers + 2):
        each_group(key_sets, lambda s: run_load(L, p, s, nrep, p.idb))
    each_group(key_sets, lambda s: run_load(L, p, s, 3, p.idb + 5))  # a roomier id_cap
    load = run_load(L, p, key_sets["1100"][0][0], 3, p.idb)[0].reshape(p.idb, 3)
    assert (load.sum(axis=0) == 1100).all()  # every key has three owners on either ring


@pytest.mark.parametrize("which", list(RINGS))
def test_route_forms_agree(gpu, pairs, key_sets, which):
    L, p = gpu.lib(), pairs[which]
    live = p.ring.server_ids()
    allowed = np.zeros((4, p.idb), dtype=np.uint8)
    allowed[0] = 1                                  # every server
    allowed[1, live[::2]] = 1                       # every other server
    allowed[2, live[0]] = 1                         # one server
    truth = np.ones(p.idb, dtype=np.uint8)          # view 3 allows nobody
    truth[live[1]] = 0
    for tr in (None, truth):
        each_group(key_sets, lambda s: run_route(L, p, s, allowed, tr))
    each_group(key_sets, lambda s: run_route(L, p, s, allowed, truth, opt=False))
    wrong, lost, kw, to, ow = run_route(L, p, key_sets["1100"][0][0], allowed, None)
    assert wrong[0] == 0 and wrong[3] == 1100 and 0 < wrong[1] < 1100 and (ow.reshape(1100, 4)[:, 3] == NIL).all()


def test_snapshot_forms_follow_the_ring(gpu, pairs, key_sets):
    """The snapshot forms share the replica-count rule: a snapshot of the ring as it is answers
    lookupN and owner load as the ring does, and the moved ranges agree between host and device."""
    L = gpu.lib()
    for p in pairs.values():
        now = p.ring.snapshot()
        for nrep in (0, 1, 3, p.servers + 2):
            w = max(nrep, 1)
            for name in ("65", "1100"):
                src = key_sets[name][0][3]
                assert src.label == "dev stride"
                want = run_lookupn(L, p, src, nrep)
                out, cnt = dev(src.n * w), dev(src.n, np.uint8)
                ok(L, L.rp_ring_snap_lookupn_dev(now._h, *src.kargs, src.n, nrep, ptr(out), ptr(cnt), None))
                agree([("ring", want), ("snap", (val(out)[:src.n * w], val(cnt, np.uint8)[:src.n]))], (name, nrep))
                load = dev(p.idb * w, np.uint64)
                ok(L, L.rp_ring_snap_owner_load_dev(now._h, *src.kargs, src.n, nrep, p.idb, 0, ptr(load), None))
                agree([("ring", run_load(L, p, src, nrep, p.idb)), ("snap", (val(load, np.uint64)[:p.idb * w],))],
                      (name, nrep))
        now.close()
        for nrep in (1, 3, 8):
            w = max(nrep, 1)
            cap = p.snap.info()["tokens"] + p.ring.size + 1
            res = []
            for on_dev in (False, True):
                mk = dev if on_dev else host
                lo, hi, br, ar, cnt, mh = mk(cap), mk(cap), mk(cap * w), mk(cap * w), mk(1), mk(1, np.uint64)
                fn = L.rp_ring_moved_ranges_dev if on_dev else L.rp_ring_moved_ranges
                ok(L, fn(p.h, p.s, nrep, cap, ptr(lo), ptr(hi), ptr(br), ptr(ar), ptr(cnt), ptr(mh),
                         *([None] if on_dev else [])))
                c = int(val(cnt)[0])
                res.append((str(on_dev), (c, int(val(mh, np.uint64)[0]), val(lo)[:c], val(hi)[:c], val(br)[:c * w],
                                          val(ar)[:c * w])))
            assert res[0][1][0] > 0
            agree(res, nrep)


# ---------------------------------------------------------------------------- 2. the Python binding
def test_python_hashfunc_ring_agrees(gpu, pairs, key_sets):
    """A ring whose hashFunc is hash32 takes the hashes entry points and answers as the default ring
    does over the same keys, through every batch method."""
    def twin(hash_func):
        opts = {"replicaPoints": 3}
        if hash_func:
            opts["hashFunc"] = hash_func
        ring = gpu.HashRing(opts)
        names = ["10.30.0.%d:3000" % i for i in range(8)]
        ring.addRemoveServers(names[:6], None)
        snap = ring.snapshot()
        ring.addRemoveServers(names[6:], names[1:3])
        return ring, snap
    (a, sa), (b, sb) = twin(None), twin(lambda k: gpu.hash32(k))
    assert all(np.array_equal(u, v) for u, v in zip(a.dump(), b.dump()))
    src = key_sets["65"][1][0]
    blob = src.blob.tobytes()
    var = [blob[src.off[i]:src.off[i + 1]].decode() for i in range(src.n)]
    fixed = key_sets["65"][0][0].blob[:65 * 36].reshape(65, 36)
    allowed = np.ones((2, a.id_bound()), dtype=np.uint8)
    allowed[1, ::2] = 0
    for keys in (var, fixed, var[:1], []):
        eq = lambda x, y: all(np.array_equal(u, v) and u.dtype == v.dtype and u.shape == v.shape  # noqa: E731
                              for u, v in zip(x, y)) and len(x) == len(y)
        assert eq((a.lookup_ids(keys),), (b.lookup_ids(keys),))
        assert eq(a.lookupn_ids(keys, 3), b.lookupn_ids(keys, 3))
        assert eq(a.group_ids(keys), b.group_ids(keys))
        assert eq(a.moved_ids(keys, sa, 3), b.moved_ids(keys, sb, 3)) and a.moved_count == b.moved_count
        assert eq(a.moved_ids(keys, sa, 3, cap=2), b.moved_ids(keys, sb, 3, cap=2)) and a.moved_count == b.moved_count
        assert eq(a.handoff_ids(keys, sa, 3), b.handoff_ids(keys, sb, 3)) and a.handoff_count == b.handoff_count
        assert eq((a.owner_load_ids(keys, 3),), (b.owner_load_ids(keys, 3),))
        ra, rb = a.route_view_ids(keys, allowed, owners=True), b.route_view_ids(keys, allowed, owners=True)
        assert sorted(ra) == sorted(rb) and eq([ra[k] for k in sorted(ra)], [rb[k] for k in sorted(rb)])
    assert a.moved_count == 0 and len(a.lookupn_ids(var, 3)[0]) == 65 and a.lookupn_ids(var, 3)[0].shape == (65, 3)
    for x in (sa, sb, a, b):
        x.close()


# ---------------------------------------------------------------------------- 3. argument errors
M_NREP = " nrep is at most 8 (the rows are compared in registers)"
M_IDCAP = " id_cap is below the ring's id bound (rp_ring_id_bound)"
M_ONE = "route_views: exactly one of the key buffer and the hash buffer"


def test_argument_errors_are_einval_with_their_text(gpu, pairs):
    """Rejected on the host, before any device work: the status and the text of every entry point."""
    L, p = gpu.lib(), pairs["5x3"]
    n = 3
    keys = np.full((n, 36), 65, dtype=np.uint8)
    off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(36))
    hs = np.arange(n, dtype=np.uint32)
    K, O, H = keys.ctypes.data, off.ctypes.data, hs.ctypes.data
    o = [host(64) for _ in range(8)]
    a, b, c, d, e, f, g, x = (v.ctypes.data for v in o)
    load = host(64 * 9, np.uint64)
    ld = load.ctypes.data
    rows = np.ones((1, p.idb), dtype=np.uint8)
    R = rows.ctypes.data
    h, s, idb = p.h, p.s, p.idb

    def route(kp, op, stride, hp, id_cap=idb):
        return L.rp_ring_route_views(h, kp, op, stride, hp, n, R, idb, 1, 1, None, id_cap, None, None, 0, ld, ld,
                                     a, b, c)
    cases = [
        # a null key buffer, null offsets with stride 0, a null hash buffer
        ("lookup: null buffer", lambda: L.rp_ring_lookup(h, None, None, 36, n, a)),
        ("lookup: null buffer", lambda: L.rp_ring_lookup(h, K, None, 0, n, a)),
        ("lookup: null buffer", lambda: L.rp_ring_lookup(h, K, None, 36, n, None)),
        ("lookupn: null buffer", lambda: L.rp_ring_lookupn(h, None, O, 0, n, 3, a, b)),
        ("lookupn: null buffer", lambda: L.rp_ring_lookupn(h, K, None, 0, n, 3, a, b)),
        ("lookupn: null buffer", lambda: L.rp_ring_lookupn(h, K, O, 0, n, 3, None, b)),
        ("lookup_hashes: null buffer", lambda: L.rp_ring_lookup_hashes(h, None, n, a)),
        ("lookup_hashes: null buffer", lambda: L.rp_ring_lookup_hashes(h, H, n, None)),
        ("lookupn_hashes: null buffer", lambda: L.rp_ring_lookupn_hashes(h, None, n, 3, a, b)),
        ("lookupn_hashes: null buffer", lambda: L.rp_ring_lookupn_hashes(h, H, n, 3, None, b)),
        ("group_keys: null key buffer", lambda: L.rp_ring_group_keys(h, None, None, 36, n, NIL, a, b, c, d)),
        ("group_keys: null key buffer", lambda: L.rp_ring_group_keys(h, K, None, 0, n, NIL, a, b, c, d)),
        ("group_hashes: null hash buffer", lambda: L.rp_ring_group_hashes(h, None, n, NIL, a, b, c, d)),
        ("moved_keys: null key buffer", lambda: L.rp_ring_moved_keys(h, s, None, None, 36, n, 3, n, a, b, c, d)),
        ("moved_keys: null key buffer", lambda: L.rp_ring_moved_keys(h, s, K, None, 0, n, 3, n, a, b, c, d)),
        ("moved_hashes: null hash buffer", lambda: L.rp_ring_moved_hashes(h, s, None, n, 3, n, a, b, c, d)),
        ("handoff: null key buffer",
         lambda: L.rp_ring_handoff(h, s, None, None, 36, n, 3, NIL, 9, a, b, c, d, e, f, g)),
        ("handoff: null key buffer", lambda: L.rp_ring_handoff(h, s, K, None, 0, n, 3, NIL, 9, a, b, c, d, e, f, g)),
        ("handoff_hashes: null hash buffer",
         lambda: L.rp_ring_handoff_hashes(h, s, None, n, 3, NIL, 9, a, b, c, d, e, f, g)),
        ("owner_load: null key buffer", lambda: L.rp_ring_owner_load(h, None, None, 36, n, 3, idb, ld)),
        ("owner_load: null key buffer", lambda: L.rp_ring_owner_load(h, K, None, 0, n, 3, idb, ld)),
        ("owner_load_hashes: null hash buffer", lambda: L.rp_ring_owner_load_hashes(h, None, n, 3, idb, ld)),
        (M_ONE, lambda: route(None, None, 36, None)),
        (M_ONE, lambda: route(K, None, 36, H)),
        ("route_views: null key offsets", lambda: route(K, None, 0, None)),
        # nrep = 9
        ("moved_keys:" + M_NREP, lambda: L.rp_ring_moved_keys(h, s, K, None, 36, n, 9, n, a, b, c, d)),
        ("moved_keys:" + M_NREP, lambda: L.rp_ring_moved_hashes(h, s, H, n, 9, n, a, b, c, d)),
        ("handoff:" + M_NREP, lambda: L.rp_ring_handoff(h, s, K, None, 36, n, 9, NIL, 9, a, b, c, d, e, f, g)),
        ("handoff:" + M_NREP, lambda: L.rp_ring_handoff_hashes(h, s, H, n, 9, NIL, 9, a, b, c, d, e, f, g)),
        # an id_cap below the id bound
        ("owner_load:" + M_IDCAP, lambda: L.rp_ring_owner_load(h, K, None, 36, n, 3, idb - 1, ld)),
        ("owner_load:" + M_IDCAP, lambda: L.rp_ring_owner_load_hashes(h, H, n, 3, idb - 1, ld)),
        ("route_views:" + M_IDCAP, lambda: route(K, None, 36, None, id_cap=idb - 1)),
        # null outputs
        ("group_keys: null output buffer", lambda: L.rp_ring_group_keys(h, K, None, 36, n, NIL, None, b, c, d)),
        ("group_keys: null output buffer", lambda: L.rp_ring_group_hashes(h, H, n, NIL, a, b, c, None)),
        ("moved_keys: null count", lambda: L.rp_ring_moved_keys(h, s, K, None, 36, n, 3, n, a, b, c, None)),
        ("moved_keys: null index buffer", lambda: L.rp_ring_moved_hashes(h, s, H, n, 3, n, None, b, c, d)),
        ("handoff: null count", lambda: L.rp_ring_handoff(h, s, K, None, 36, n, 3, NIL, 9, a, b, c, d, e, None, g)),
        ("handoff: only_src is not a server id of this ring",
         lambda: L.rp_ring_handoff_hashes(h, s, H, n, 3, idb, 9, a, b, c, d, e, f, g)),
        ("handoff: null output buffer",
         lambda: L.rp_ring_handoff(h, s, K, None, 36, n, 3, NIL, 9, None, b, c, d, e, f, g)),
        ("owner_load: null load buffer", lambda: L.rp_ring_owner_load(h, K, None, 36, n, 3, idb, None)),
        # where two checks fail, the one that came first
        ("moved_keys: null key buffer", lambda: L.rp_ring_moved_keys(h, s, None, None, 36, n, 9, n, a, b, c, None)),
        ("moved_hashes: null hash buffer", lambda: L.rp_ring_moved_hashes(h, s, None, n, 9, n, a, b, c, None)),
        ("handoff: null key buffer",
         lambda: L.rp_ring_handoff(h, s, None, None, 36, n, 9, NIL, 9, a, b, c, d, e, None, None)),
        ("handoff: null count", lambda: L.rp_ring_handoff(h, s, K, None, 36, n, 9, NIL, 9, a, b, c, d, e, None, None)),
        ("moved_keys: null count", lambda: L.rp_ring_moved_keys(h, s, K, None, 36, n, 9, n, a, b, c, None)),
        ("group_keys: null key buffer", lambda: L.rp_ring_group_keys(h, None, None, 36, n, NIL, None, b, c, d)),
        ("owner_load: null key buffer", lambda: L.rp_ring_owner_load(h, None, None, 36, n, 3, idb - 1, None)),
        ("owner_load:" + M_IDCAP, lambda: L.rp_ring_owner_load(h, K, None, 36, n, 3, idb - 1, None)),
        ("route_views:" + M_IDCAP, lambda: route(None, None, 36, None, id_cap=idb - 1)),
        ("null ring handle", lambda: L.rp_ring_moved_keys(None, None, None, None, 36, n, 9, n, a, b, c, d)),
        ("null snapshot handle", lambda: L.rp_ring_handoff(h, None, None, None, 36, n, 9, NIL, 9, a, b, c, d, e, f, g)),
    ]
    for i, (text, call) in enumerate(cases):
        assert call() == -1, (i, text)  # RP_EINVAL
        assert L.rp_last_error().decode() == text, (i, text)
    # n == 0 asks for no key buffer at all
    nd = ctypes.c_uint32(7)
    ok(L, L.rp_ring_lookup(h, None, None, 0, 0, None))
    ok(L, L.rp_ring_lookupn_hashes(h, None, 0, 3, None, None))
    ok(L, L.rp_ring_group_keys(h, None, None, 0, 0, NIL, a, b, c, ctypes.addressof(nd)))
    ok(L, L.rp_ring_moved_hashes(h, s, None, 0, 3, 4, None, None, None, ctypes.addressof(nd)))
    ok(L, L.rp_ring_owner_load(h, None, None, 0, 0, 3, idb, ld))
    assert nd.value == 0 and (load[:idb * 3] == 0).all() and load[idb * 3] == 0x5A5A5A5A5A5A5A5A
    # and the ring answers as before
    out = host(n)
    ok(L, L.rp_ring_lookup(h, K, None, 36, n, out.ctypes.data))
    assert (out[:n] < idb).all() and len(set(out[:n])) == 1
