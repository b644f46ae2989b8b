"""GPU tests of the routing-agreement entry points (rp_ring_route_views*): every key's owner under
many views of one ring at once, and the per-view / per-key disagreement counts.

Reference: tests/routing_model.py (numpy; pinned against the oracle ring by
tests/test_route_model.py). Results are integers; every comparison is exact, on all five outputs.
"""
import functools
import zlib

import numpy as np
import pytest

import routing_model as rm
from test_ring_moved_gpu import _keys

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
S = 70
OUT = ("wrong", "lost", "key_wrong", "truth_owner", "owners")


@functools.lru_cache(maxsize=None)
def _hashes(n):
    import pyoracle
    h = np.array([pyoracle.hash32(bytes(k)) for k in _keys(n)], dtype=np.uint32)
    h.setflags(write=False)
    return h


@pytest.fixture(scope="module")
def base(gpu, orc):
    ring = gpu.HashRing()
    ring.addRemoveServers([orc.c2_addr(i) for i in range(S)], None)
    tok, own = ring.dump()
    assert len(tok) == S * 100 == len(np.unique(tok))  # no token collision: the model is `lookup`
    yield ring, tok, own
    ring.close()


def views_for(nv, ids, seed, own):
    """allowed[nv][ids] at density 0.9 with the special views last (the truth alone below four views): everybody,
    nobody, exactly one server, the truth itself; a truth at density 0.8; active partly zero."""
    rng = np.random.default_rng(seed)
    allowed = rng.random((nv, ids)) < 0.9
    truth = rng.random(ids) < 0.8
    special = [np.ones(ids, dtype=bool), np.zeros(ids, dtype=bool), np.zeros(ids, dtype=bool), truth]
    special[2][int(own[len(own) // 3])] = True
    at = [nv - 1 - i for i in range(4)] if nv >= 4 else [0]  # the last views: the partial last word
    for v, row in zip(at, [special[3]] if nv < 4 else special):
        allowed[v] = row
    active = rng.random(nv) < 0.7
    active[at[-1]] = True  # the truth as a view
    return allowed, truth, active, at


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def alloc(n, nv):
    """Sentinel-filled device outputs for n keys and nv views."""
    return {"wrong": torch.full((max(nv, 1),), 77, dtype=torch.int64, device="cuda"),
            "lost": torch.full((max(nv, 1),), 77, dtype=torch.int64, device="cuda"),
            "key_wrong": torch.full((max(n, 1),), 77, dtype=torch.int32, device="cuda"),
            "truth_owner": torch.full((max(n, 1),), 77, dtype=torch.int32, device="cuda"),
            "owners": torch.full((max(n * nv, 1),), 77, dtype=torch.int32, device="cuda")}


def route_dev(ring, n, allowed, keys=None, hashes=None, truth=None, active=None, col=None, id_cap=None, bit=1,
              accumulate=False, into=None, owners=True, **kw):
    """rp_ring_route_views_dev over sentinel-filled device outputs; keys / hashes are device tensors."""
    nv, rs = allowed.shape
    rows = dev(allowed.astype(np.uint8) * bit, np.uint8)
    tr, ac, cl = dev(None if truth is None else truth.astype(np.uint8) * bit, np.uint8), dev(active, np.uint8), \
        dev(col, np.uint32)
    if into is None:
        into = alloc(n, nv)
    ring.route_views_dev(n, ptr(rows), rs, nv, keys_ptr=ptr(keys) if not isinstance(keys, int) else keys,
                         hashes_ptr=ptr(hashes), bit=bit, col_ptr=ptr(cl), id_cap=id_cap, truth_ptr=ptr(tr),
                         active_ptr=ptr(ac), accumulate=accumulate, wrong_ptr=ptr(into["wrong"]),
                         lost_ptr=ptr(into["lost"]), key_wrong_ptr=ptr(into["key_wrong"]),
                         truth_owner_ptr=ptr(into["truth_owner"]),
                         owners_ptr=ptr(into["owners"]) if owners else None, **kw)
    torch.cuda.synchronize()
    return into


def host(into, n, nv):
    return {"wrong": into["wrong"].cpu().numpy().view(np.uint64)[:nv],
            "lost": into["lost"].cpu().numpy().view(np.uint64)[:nv],
            "key_wrong": into["key_wrong"].cpu().numpy().view(np.uint32)[:n],
            "truth_owner": into["truth_owner"].cpu().numpy().view(np.uint32)[:n],
            "owners": into["owners"].cpu().numpy().view(np.uint32)[:n * nv].reshape(n, nv)}


def assert_same(got, want, names=OUT):
    for k in names:
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero((got[k] != want[k]).reshape(-1))[:8])


def assert_sane(res, truth_view=None):
    assert (res["lost"] <= res["wrong"]).all()
    if truth_view is not None:
        assert res["wrong"][truth_view] == 0 and res["lost"][truth_view] == 0


# ---------------------------------------------------------------------------- 1. view counts
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 130])
def test_view_counts(base, nv):
    ring, tok, own = base
    n = 700
    hs = _hashes(n)
    keys = dev(np.array(_keys(n)).reshape(-1), np.uint8)
    ids = ring.id_bound()
    allowed, truth, active, at = views_for(nv, ids, nv, own)
    for tr, ac in ((truth, active), (None, None), (truth, None)):
        want = rm.route(tok, own, hs, allowed, tr, ac)
        got = host(route_dev(ring, n, allowed, keys=keys, truth=tr, active=ac), n, nv)
        assert_same(got, want)
        assert_sane(got, at[-1] if tr is not None else None)
    want = rm.route(tok, own, hs, allowed, truth, active)
    assert (want["wrong"][~active] == 0).all()
    if nv >= 4:
        assert want["wrong"].sum() > 0 and want["lost"].sum() > 0
        everybody, nobody, one = at[0], at[1], at[2]
        assert (want["owners"][:, nobody] == NIL).all() and want["lost"][nobody] == 0
        assert len(np.unique(want["owners"][:, one])) == 1  # long walks, and wraps past the last token
        assert (want["owners"][:, at[3]] == want["truth_owner"]).all() and everybody == nv - 1
    # without the owners output the other four are the same (inactive views are then not walked)
    got = host(route_dev(ring, n, allowed, keys=keys, truth=truth, active=active, owners=False), n, nv)
    assert_same(got, want, OUT[:4])
    assert (got["owners"] == 77).all()
    # another bit of the row bytes (the simulator's rows carry theirs at 0x80)
    got = host(route_dev(ring, n, allowed, keys=keys, truth=truth, active=active, bit=0x80), n, nv)
    assert_same(got, want)


# ---------------------------------------------------------------------------- 2. hashes
def test_hashes_form(base):
    ring, tok, own = base
    rng = np.random.default_rng(11)
    hs = np.concatenate([rm.edge_hashes(tok), rng.integers(0, 1 << 32, 600, dtype=np.uint64).astype(np.uint32)])
    nv, ids = 65, ring.id_bound()
    allowed, truth, active, _ = views_for(nv, ids, 5, own)
    want = rm.route(tok, own, hs, allowed, truth, active)
    got = host(route_dev(ring, len(hs), allowed, hashes=dev(hs, np.uint32), truth=truth, active=active), len(hs), nv)
    assert_same(got, want)
    assert_same(ring.route_view_hashes(hs, allowed, truth, active, owners=True), want)
    # the hashes at both ends of the ring: the first token's owner before it and past the last
    full = rm.route(tok, own, hs[:6], np.ones((1, ids), dtype=bool))["owners"][:, 0]
    assert full.tolist() == [own[0], own[0], own[1], own[-1], own[0], own[0]]


# ---------------------------------------------------------------------------- 3. key forms
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2055])
def test_key_forms(gpu, base, n):
    ring, tok, own = base
    nv, ids = 65, ring.id_bound()
    allowed, truth, active, _ = views_for(nv, ids, 9, own)
    hs = _hashes(max(n, 1))[:n]
    want = rm.route(tok, own, hs, allowed, truth, active)
    flat = np.array(_keys(max(n, 1))).reshape(-1)[:n * 36]
    # stride 36 from a 16-byte aligned base, and from a base 4 bytes past one
    for lead in (0, 4):
        buf = torch.zeros(n * 36 + 32, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[lead:lead + n * 36] = torch.from_numpy(flat.copy()).cuda()
        got = host(route_dev(ring, n, allowed, keys=buf.data_ptr() + lead, truth=truth, active=active), n, nv)
        assert_same(got, want)
    # stride 36 from an odd base (the generic path)
    buf = torch.zeros(n * 36 + 32, dtype=torch.uint8, device="cuda")
    buf[1:1 + n * 36] = torch.from_numpy(flat.copy()).cuda()
    assert_same(host(route_dev(ring, n, allowed, keys=buf.data_ptr() + 1, truth=truth, active=active), n, nv), want)
    # offsets with variable lengths (through the host form)
    skeys = ["k%d-%s" % (i, "x" * (i % 41)) for i in range(n)]
    import pyoracle
    vh = np.array([pyoracle.hash32(k) for k in skeys], dtype=np.uint32)
    vwant = rm.route(tok, own, vh, allowed, truth, active)
    assert_same(ring.route_view_ids(skeys, allowed, truth, active, owners=True), vwant)
    # ... and through the device form
    blob, off, stride, k = ring._key_pack(skeys)
    assert stride == 0 and k == n
    doff = dev(off.view(np.int64), np.int64)
    got = host(route_dev(ring, n, allowed, keys=dev(blob, np.uint8), truth=truth, active=active, stride=0,
                         off_ptr=doff.data_ptr()), n, nv)
    assert_same(got, vwant)
    # the host form on 36-byte rows
    assert_same(ring.route_view_ids(np.array(_keys(max(n, 1)))[:n], allowed, truth, active, owners=True), want)


def test_hash_func_ring(gpu, orc):
    fn = lambda s: zlib.crc32(s.encode() if isinstance(s, str) else bytes(s))  # noqa: E731
    ring = gpu.HashRing({"hashFunc": fn})
    ring.addRemoveServers([orc.c2_addr(i) for i in range(S)], None)
    tok, own = ring.dump()
    assert len(np.unique(tok)) == len(tok) == S * 100
    skeys = ["key-%d" % i for i in range(513)]
    hs = np.array([fn(k) for k in skeys], dtype=np.uint32)
    allowed, truth, active, _ = views_for(65, ring.id_bound(), 13, own)
    want = rm.route(tok, own, hs, allowed, truth, active)
    assert_same(ring.route_view_ids(skeys, allowed, truth, active, owners=True), want)
    ring.close()


# ---------------------------------------------------------------------------- 4. sparse ids
def test_sparse_ids_and_column_map(gpu, orc):
    ring = gpu.HashRing()
    names = [orc.c2_addr(i) for i in range(90)]
    ring.addRemoveServers(names[:50], None)
    ring.addRemoveServers(None, names[5:45:3])
    ring.addRemoveServers(names[50:], None)
    tok, own = ring.dump()
    ids = ring.id_bound()
    live = np.zeros(ids, dtype=bool)
    live[ring.server_ids()] = True
    assert ids == 90 and 0 < (~live).sum() and len(tok) == int(live.sum()) * 100 == len(np.unique(tok))
    n, nv = 600, 65
    hs = _hashes(n)
    keys = dev(np.array(_keys(n)).reshape(-1), np.uint8)
    # the identity map: rows indexed by id, holes included (a hole's byte is never looked at)
    allowed, truth, active, _ = views_for(nv, ids, 21, own)
    want = rm.route(tok, own, hs, allowed & live, truth & live, active)
    assert_same(host(route_dev(ring, n, allowed, keys=keys, truth=truth, active=active), n, nv), want)
    # a column map: a permutation into wider rows, one live server with no column
    rng = np.random.default_rng(23)
    cols = 101
    col = rng.permutation(cols)[:ids + 3].astype(np.uint32)  # id_cap = ids + 3 entries
    nocol = int(own[7])
    col[nocol] = NIL
    rows = rng.random((nv, cols)) < 0.9
    trow = rng.random(cols) < 0.8
    by = rm.by_id(rows, col, ids) & live
    tby = rm.by_id(trow, col, ids)[0] & live
    assert not by[:, nocol].any() and not tby[nocol]
    want = rm.route(tok, own, hs, by, tby, active)
    assert (want["owners"] != nocol).all() and (want["truth_owner"] != nocol).all()
    got = host(route_dev(ring, n, rows, keys=keys, truth=trow, active=active, col=col, id_cap=ids + 3), n, nv)
    assert_same(got, want)
    assert_same(ring.route_view_ids(np.array(_keys(n)), rows, trow, active, col=col, owners=True), want)
    # an id_cap below the bound is refused, with nothing written
    with pytest.raises(gpu.RingpopAmdError, match="id_cap"):
        route_dev(ring, n, rows, keys=keys, col=col, id_cap=ids - 1)
    ring.close()


# ---------------------------------------------------------------------------- 5. view blocks
def test_view_blocks(base, monkeypatch):
    ring, tok, own = base
    n, nv = 700, 130
    hs = _hashes(n)
    keys = dev(np.array(_keys(n)).reshape(-1), np.uint8)
    allowed, truth, active, _ = views_for(nv, ring.id_bound(), 31, own)
    want = rm.route(tok, own, hs, allowed, truth, active)
    one = host(route_dev(ring, n, allowed, keys=keys, truth=truth, active=active), n, nv)
    monkeypatch.setenv("RP_ROUTE_VBLOCK", "64")  # three blocks of views, the last one partial
    three = host(route_dev(ring, n, allowed, keys=keys, truth=truth, active=active), n, nv)
    monkeypatch.setenv("RP_ROUTE_VBLOCK", "128")  # two blocks: a full one and a two-view one
    two = host(route_dev(ring, n, allowed, keys=keys, truth=truth, active=active), n, nv)
    for got in (one, three, two):
        assert_same(got, want)


# ---------------------------------------------------------------------------- 6. accumulate
def test_accumulate_and_empty(base):
    ring, tok, own = base
    n, nv, cut = 700, 65, 257
    hs = _hashes(n)
    flat = torch.from_numpy(np.array(_keys(n)).reshape(-1)).cuda()
    allowed, truth, active, _ = views_for(nv, ring.id_bound(), 41, own)
    want = rm.route(tok, own, hs, allowed, truth, active)
    whole = host(route_dev(ring, n, allowed, keys=flat, truth=truth, active=active), n, nv)
    assert_same(whole, want)
    a = route_dev(ring, cut, allowed, keys=flat, truth=truth, active=active)
    first = host(a, cut, nv)
    assert_same(first, rm.route(tok, own, hs[:cut], allowed, truth, active))
    b = route_dev(ring, n - cut, allowed, keys=flat.data_ptr() + cut * 36, truth=truth, active=active,
                  accumulate=True, into={**alloc(n - cut, nv), "wrong": a["wrong"], "lost": a["lost"]})
    second = host(b, n - cut, nv)
    assert np.array_equal(second["wrong"], want["wrong"]) and np.array_equal(second["lost"], want["lost"])
    assert np.array_equal(second["key_wrong"], want["key_wrong"][cut:])
    assert np.array_equal(second["owners"], want["owners"][cut:])
    # inactive views are left alone under accumulate, and set to 0 otherwise
    assert (first["wrong"][~active] == 0).all()
    pre = alloc(n, nv)
    pre["wrong"][:] = 5
    pre["lost"][:] = 3
    acc = host(route_dev(ring, n, allowed, keys=flat, truth=truth, active=active, accumulate=True, into=pre), n, nv)
    assert np.array_equal(acc["wrong"], want["wrong"] + 5) and np.array_equal(acc["lost"], want["lost"] + 3)
    # empty inputs are results, not errors
    e = host(route_dev(ring, 0, allowed, keys=None, truth=truth, active=active), 0, nv)
    assert (e["wrong"] == 0).all() and (e["lost"] == 0).all()
    none = np.zeros((0, ring.id_bound()), dtype=bool)
    z = host(route_dev(ring, n, none, keys=flat, truth=truth), n, 0)
    assert np.array_equal(z["truth_owner"], want["truth_owner"]) and (z["key_wrong"] == 0).all()
    r0 = ring.route_view_ids([], allowed, truth, active, owners=True)
    assert r0["owners"].shape == (0, nv) and (r0["wrong"] == 0).all()


def test_empty_ring(gpu):
    ring = gpu.HashRing()
    res = ring.route_view_ids(np.array(_keys(65)), np.ones((3, 1), dtype=bool), owners=True)
    assert (res["owners"] == NIL).all() and (res["truth_owner"] == NIL).all()
    assert (res["wrong"] == 0).all() and (res["lost"] == 0).all() and (res["key_wrong"] == 0).all()
    ring.close()


# ---------------------------------------------------------------------------- 7. names
def test_route_views_names(base, orc):
    ring, tok, own = base
    names = [orc.c2_addr(i) for i in range(S)]
    skeys = [bytes(k).decode() for k in _keys(300)]
    rng = np.random.default_rng(51)
    views = [[s for s in names if rng.random() < 0.9] for _ in range(5)] + [[], names[3:4], names + ["10.9.9.9:1"]]
    truth = [s for s in names if rng.random() < 0.8]
    ids = ring.id_bound()

    def row(ns):
        r = np.zeros(ids, dtype=bool)
        r[np.array([ring.server_id(s) for s in ns if ring.server_id(s) != NIL], dtype=np.int64)] = True
        return r
    allowed = np.stack([row(v) for v in views])
    want = rm.route(tok, own, _hashes(300), allowed, row(truth))
    got = ring.routeViews(skeys, views, truth)
    nm = lambda i: None if i == NIL else ring.name(int(i))  # noqa: E731
    assert got["owners"] == [[nm(i) for i in r] for r in want["owners"]]
    assert got["truth"] == [nm(i) for i in want["truth_owner"]]
    assert got["wrong"] == want["wrong"].tolist() and got["lost"] == want["lost"].tolist()
    assert all(o is None for r in got["owners"] for o in r[5:6]) and {r[6] for r in got["owners"]} == {names[3]}
    # truth None: every server; the last view holds them all
    got = ring.routeViews(skeys, views)
    assert got["wrong"][7] == 0 and got["lost"] == [0] * 8 and [r[7] for r in got["owners"]] == got["truth"]
