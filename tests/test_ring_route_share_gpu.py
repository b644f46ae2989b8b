"""GPU tests of the key-free routing-agreement entry points (rp_ring_route_share*): on how many of
the 2^32 hash values every view of a ring disagrees with the truth, and per token position how
many views do.

Reference: tests/route_share_model.py (routing_model.route at hashes = tok, weighted by the
interval lengths; pinned on the CPU by tests/test_route_share_model.py). Results are integers;
every comparison is exact, on all three outputs, over sentinel-filled buffers.
"""
import numpy as np
import pytest

import route_share_model as sm
import routing_model as rm
from test_ring_route_gpu import S, dev, ptr, views_for

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
OUT = ("wrong", "lost", "pos_wrong")
PAD = 5  # sentinel entries past V and past M that no call may touch
FULL = 1 << 32


@pytest.fixture(scope="module")
def base(gpu, orc):
    ring = gpu.HashRing()
    ring.addRemoveServers([orc.c2_addr(i) for i in range(S)], None)
    tok, own = ring.dump()
    assert len(tok) == S * 100 == len(np.unique(tok))
    yield ring, tok, own
    ring.close()


def alloc(m, nv):
    return {"wrong": torch.full((nv + PAD,), 77, dtype=torch.int64, device="cuda"),
            "lost": torch.full((nv + PAD,), 77, dtype=torch.int64, device="cuda"),
            "pos_wrong": torch.full((m + PAD,), 77, dtype=torch.int32, device="cuda")}


def share_dev(ring, allowed, truth=None, active=None, col=None, id_cap=None, bit=1, accumulate=False, into=None,
              pos=True, pos_cap=None, stream=None, wrong=True, lost=True):
    """rp_ring_route_share_dev over sentinel-filled device outputs."""
    nv, rs = allowed.shape
    m = ring.size
    rows = dev(allowed.astype(np.uint8) * bit, np.uint8)
    tr, ac, cl = dev(None if truth is None else truth.astype(np.uint8) * bit, np.uint8), dev(active, np.uint8), \
        dev(col, np.uint32)
    if into is None:
        into = alloc(m, nv)
    ring.route_share_dev(ptr(rows), rs, nv, bit=bit, col_ptr=ptr(cl), id_cap=id_cap, truth_ptr=ptr(tr),
                         active_ptr=ptr(ac), accumulate=accumulate, wrong_ptr=ptr(into["wrong"]) if wrong else None,
                         lost_ptr=ptr(into["lost"]) if lost else None,
                         pos_wrong_ptr=ptr(into["pos_wrong"]) if pos else None,
                         pos_cap=m if pos_cap is None else pos_cap, stream=stream)
    torch.cuda.synchronize()
    return into


def host(into, m, nv):
    """The outputs; the sentinels past them are checked on the way."""
    w, lo, p = (into[k].cpu().numpy() for k in OUT)
    assert (w[nv:] == 77).all() and (lo[nv:] == 77).all() and (p[m:] == 77).all()
    return {"wrong": w.view(np.uint64)[:nv], "lost": lo.view(np.uint64)[:nv], "pos_wrong": p.view(np.uint32)[:m]}


def untouched(into):
    return all(bool((into[k] == 77).all()) for k in OUT)


def assert_same(got, want, names=OUT):
    for k in names:
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8])


def assert_sane(res, truth_view=None):
    assert (res["lost"] <= res["wrong"]).all() and (res["wrong"] <= FULL).all()
    if truth_view is not None:
        assert res["wrong"][truth_view] == 0 and res["lost"][truth_view] == 0


# ---------------------------------------------------------------------------- 1. view counts
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 130])
def test_view_counts(base, nv):
    ring, tok, own = base
    m, ids = len(tok), ring.id_bound()
    allowed, truth, active, at = views_for(nv, ids, nv, own)
    for tr, ac in ((truth, active), (None, None), (truth, None)):
        want = sm.share(tok, own, allowed, tr, ac)
        got = host(share_dev(ring, allowed, truth=tr, active=ac), m, nv)
        assert_same(got, want)
        assert_sane(got, at[-1] if tr is not None else None)
    want = sm.share(tok, own, allowed, truth, active)
    assert (want["wrong"][~active] == 0).all()
    if nv >= 4:
        assert want["wrong"].sum() > 0 and want["lost"].sum() > 0 and want["pos_wrong"].max() > 0
    # every output alone: the others stay as they were
    for only in OUT:
        into = share_dev(ring, allowed, truth=truth, active=active, wrong=only == "wrong", lost=only == "lost",
                         pos=only == "pos_wrong")
        assert all(bool((into[k] == 77).all()) for k in OUT if k != only), only
        raw, n = into[only].cpu().numpy(), len(want[only])
        assert np.array_equal(raw[:n].view(want[only].dtype), want[only]) and (raw[n:] == 77).all(), only


# ---------------------------------------------------------------------------- 2. chunk sizes
@pytest.mark.parametrize("chunk", [1, 64, 100, 4096, 7000, 10 ** 6])
def test_chunk_sizes(base, monkeypatch, chunk):
    """One position a chunk, chunks that do not divide M, one chunk; a truth with exactly one server
    (its 100 tokens leave gaps far longer than 64 positions: carries cross several chunks and the
    wrap) and a dense one."""
    ring, tok, own = base
    m, nv, ids = len(tok), 130, ring.id_bound()
    allowed, dense, active, at = views_for(nv, ids, 61, own)
    sparse = np.zeros(ids, dtype=bool)
    sparse[int(own[m // 2])] = True
    gaps = np.diff(np.flatnonzero(sparse[own]))
    assert sparse[own].sum() == 100 and gaps.max() > 64
    monkeypatch.setenv("RP_SHARE_CHUNK", str(chunk))
    for tr in (sparse, dense):
        want = sm.share(tok, own, allowed, tr, active)
        got = host(share_dev(ring, allowed, truth=tr, active=active), m, nv)
        assert_same(got, want)
        assert_sane(got)
        got = host(share_dev(ring, allowed, truth=tr, active=active, pos=False), m, nv)
        assert_same(got, want, OUT[:2])
    assert want["wrong"][at[-1]] == 0  # the dense truth is views_for's: its own view agrees


# ---------------------------------------------------------------------------- 3. identities
def test_identities_with_owner_share(base):
    ring, tok, own = base
    m, ids = len(tok), ring.id_bound()
    shares = ring.owner_share_ids()
    assert int(shares.sum()) == FULL
    xs = [int(own[0]), int(own[m - 1]), int(own[m // 2]), 3]
    but = np.ones((len(xs), ids), dtype=bool)
    for v, x in enumerate(xs):
        but[v, x] = False
    # truth NULL, views allowing all but X: X's share goes elsewhere, to servers that exist
    got = host(share_dev(ring, but), m, len(xs))
    assert got["wrong"].tolist() == [int(shares[x]) for x in xs] and got["lost"].tolist() == [0] * len(xs)
    # truth = all but X, a view allowing all: X's share is sent to a server that is gone;
    # the truth as a view agrees everywhere
    for v, x in enumerate(xs):
        views = np.stack([np.ones(ids, dtype=bool), but[v]])
        got = host(share_dev(ring, views, truth=but[v]), m, 2)
        assert got["wrong"].tolist() == [int(shares[x]), 0] and got["lost"].tolist() == [int(shares[x]), 0]
        assert int(sm.lengths(tok)[got["pos_wrong"] > 0].sum()) == int(shares[x])
        assert np.array_equal(got["pos_wrong"] > 0, own == x)


# ---------------------------------------------------------------------------- 4. against the key path
def test_against_route_views_at_the_tokens(base):
    """rp_ring_route_views_dev at hashes = tok gives every interval's owners; weighted by the
    interval lengths on the host they are wrong / lost, and its key_wrong is pos_wrong."""
    ring, tok, own = base
    m, nv, ids = len(tok), 130, ring.id_bound()
    allowed, truth, active, _ = views_for(nv, ids, 71, own)
    rows, tr, ac = dev(allowed.astype(np.uint8), np.uint8), dev(truth.astype(np.uint8), np.uint8), dev(active, np.uint8)
    hashes = dev(tok, np.uint32)
    kw = torch.full((m,), 77, dtype=torch.int32, device="cuda")
    to = torch.full((m,), 77, dtype=torch.int32, device="cuda")
    ow = torch.full((m * nv,), 77, dtype=torch.int32, device="cuda")
    ring.route_views_dev(m, ptr(rows), ids, nv, hashes_ptr=ptr(hashes), truth_ptr=ptr(tr), active_ptr=ptr(ac),
                         key_wrong_ptr=ptr(kw), truth_owner_ptr=ptr(to), owners_ptr=ptr(ow))
    torch.cuda.synchronize()
    owners = ow.cpu().numpy().view(np.uint32).reshape(m, nv)
    t = to.cpu().numpy().view(np.uint32)
    ln = sm.lengths(tok)
    act = active.astype(bool)
    diff = (owners != t[:, None]) & act[None, :]
    real = owners != NIL
    gone = np.zeros_like(diff)
    gone[real] = ~truth[owners[real]]
    gone &= act[None, :]
    got = host(share_dev(ring, allowed, truth=truth, active=active), m, nv)
    assert np.array_equal(got["wrong"], (diff * ln[:, None]).sum(axis=0, dtype=np.uint64))
    assert np.array_equal(got["lost"], (gone * ln[:, None]).sum(axis=0, dtype=np.uint64))
    assert np.array_equal(got["pos_wrong"], kw.cpu().numpy().view(np.uint32))
    assert got["wrong"].sum() > 0 and got["lost"].sum() > 0


# ---------------------------------------------------------------------------- 5. degenerate rings and views
def test_empty_ring(gpu):
    ring = gpu.HashRing()
    into = share_dev(ring, np.ones((3, 1), dtype=bool), pos_cap=PAD)
    got = host(into, 0, 3)
    assert got["wrong"].tolist() == [0, 0, 0] and got["lost"].tolist() == [0, 0, 0]
    assert bool((into["pos_wrong"] == 77).all())  # nothing is written to pos_wrong
    res = ring.route_share_ids(np.ones((3, 1), dtype=bool))
    assert res["wrong"].tolist() == [0, 0, 0] and res["lost"].tolist() == [0, 0, 0] and len(res["pos_wrong"]) == 0
    assert ring.routeShare([["10.0.0.1:1"], []]) == {"wrong": [0, 0], "lost": [0, 0], "disputed": 0}
    ring.close()


def test_one_token_ring(gpu, orc):
    ring = gpu.HashRing({"replicaPoints": 1})
    ring.addRemoveServers([orc.c2_addr(0)], None)
    tok, own = ring.dump()
    assert len(tok) == 1 and sm.lengths(tok).tolist() == [FULL]
    ids = ring.id_bound()
    views = np.array([[True] * ids, [False] * ids], dtype=bool)
    # truth NULL: the only server; the view without it answers null everywhere
    got = host(share_dev(ring, views), 1, 2)
    assert got["wrong"].tolist() == [0, FULL] and got["lost"].tolist() == [0, 0] and got["pos_wrong"].tolist() == [1]
    assert_same(got, sm.share(tok, own, views))
    # a truth without it: the view that still has it loses every hash
    got = host(share_dev(ring, views, truth=np.zeros(ids, dtype=bool)), 1, 2)
    assert got["wrong"].tolist() == [FULL, 0] and got["lost"].tolist() == [FULL, 0]
    assert got["pos_wrong"].tolist() == [1]
    ring.close()


def test_degenerate_views(base):
    ring, tok, own = base
    m, ids = len(tok), ring.id_bound()
    allowed, _, active, at = views_for(65, ids, 81, own)
    # a truth that allows nobody: wrong and lost on all 2^32 hashes iff the view allows anybody
    nobody = np.zeros(ids, dtype=bool)
    got = host(share_dev(ring, allowed, truth=nobody), m, 65)
    assert_same(got, sm.share(tok, own, allowed, nobody))
    assert got["wrong"].tolist() == [FULL * int(a) for a in allowed.any(axis=1)]
    assert np.array_equal(got["lost"], got["wrong"]) and got["wrong"][at[1]] == 0
    assert (got["pos_wrong"] == int(allowed.any(axis=1).sum())).all()
    # n_views = 0: pos_wrong is set to zero, nothing else is touched
    none = np.zeros((0, ids), dtype=bool)
    into = share_dev(ring, none)
    z = host(into, m, 0)
    assert (z["pos_wrong"] == 0).all()
    r0 = ring.route_share_ids(none)
    assert len(r0["wrong"]) == 0 and len(r0["lost"]) == 0 and (r0["pos_wrong"] == 0).all()
    # a view of ids without tokens only (id_cap past the bound: ids the ring never interned)
    wide = np.zeros((2, ids + 7), dtype=bool)
    wide[0, ids:] = True
    wide[1, :] = True
    col = np.arange(ids + 7, dtype=np.uint32)
    got = host(share_dev(ring, wide, col=col, id_cap=ids + 7), m, 2)
    assert got["wrong"].tolist() == [FULL, 0] and got["lost"].tolist() == [0, 0]
    assert (got["pos_wrong"] == 1).all()


# ---------------------------------------------------------------------------- 6. plumbing
def test_column_map_and_bit(gpu, orc):
    ring = gpu.HashRing()
    names = [orc.c2_addr(i) for i in range(90)]
    ring.addRemoveServers(names[:50], None)
    ring.addRemoveServers(None, names[5:45:3])
    ring.addRemoveServers(names[50:], None)
    tok, own = ring.dump()
    m, ids = len(tok), ring.id_bound()
    live = np.zeros(ids, dtype=bool)
    live[ring.server_ids()] = True
    assert ids == 90 and 0 < (~live).sum() and m == int(live.sum()) * 100 == len(np.unique(tok))
    nv = 65
    allowed, truth, active, _ = views_for(nv, ids, 21, own)
    # the identity map: rows indexed by id, holes included
    want = sm.share(tok, own, allowed & live, truth & live, active)
    assert_same(host(share_dev(ring, allowed, truth=truth, active=active), m, nv), want)
    # a permutation into wider rows, one live server without a column and one with a column past row_stride
    rng = np.random.default_rng(23)
    cols = 101
    col = rng.permutation(cols)[:ids + 3].astype(np.uint32)  # id_cap = ids + 3 entries
    nocol, past = int(own[7]), int(own[m // 2])
    assert nocol != past
    col[nocol] = NIL
    col[past] = cols + 4
    rows = rng.random((nv, cols)) < 0.9
    trow = rng.random(cols) < 0.8
    by = rm.by_id(rows, col, ids) & live
    tby = rm.by_id(trow, col, ids)[0] & live
    assert not by[:, [nocol, past]].any() and not tby[nocol] and not tby[past]
    want = sm.share(tok, own, by, tby, active)
    for bit in (1, 0x40):
        got = host(share_dev(ring, rows, truth=trow, active=active, col=col, id_cap=ids + 3, bit=bit), m, nv)
        assert_same(got, want)
    # the host form equals the device form
    assert_same(ring.route_share_ids(rows, trow, active, col=col), want)
    res = ring.route_share_ids(rows, trow, active, col=col, pos=False)
    assert sorted(res) == ["lost", "wrong"]
    assert_same(res, want, OUT[:2])
    ring.close()


def test_accumulate(base):
    ring, tok, own = base
    m, nv, ids = len(tok), 65, ring.id_bound()
    allowed, truth, active, _ = views_for(nv, ids, 41, own)
    allowed2, truth2, _, _ = views_for(nv, ids, 43, own)
    a = sm.share(tok, own, allowed, truth, active)
    b = sm.share(tok, own, allowed2, truth2, active)
    assert (~active).any() and a["wrong"].sum() > 0
    into = share_dev(ring, allowed, truth=truth, active=active)
    assert_same(host(into, m, nv), a)
    into["wrong"][:nv] += 5  # inactive views hold 5 / 3 now: left alone under accumulate
    into["lost"][:nv] += 3
    got = host(share_dev(ring, allowed2, truth=truth2, active=active, accumulate=True, into=into), m, nv)
    assert np.array_equal(got["wrong"], a["wrong"] + b["wrong"] + 5)
    assert np.array_equal(got["lost"], a["lost"] + b["lost"] + 3)
    assert np.array_equal(got["pos_wrong"], b["pos_wrong"])  # set, not added
    assert (got["wrong"][~active] == 5).all() and (got["lost"][~active] == 3).all()
    # without accumulate the same buffers are set again
    assert_same(host(share_dev(ring, allowed, truth=truth, active=active, into=into), m, nv), a)


def test_caller_stream_after_a_ring_change(gpu, orc):
    ring = gpu.HashRing()
    names = [orc.c2_addr(i) for i in range(40)]
    ring.addRemoveServers(names[:30], None)
    st = torch.cuda.Stream()
    ids0 = ring.id_bound()
    share_dev(ring, np.ones((3, ids0), dtype=bool), stream=st.cuda_stream)  # the scratch was last used on st
    ring.addRemoveServers(names[30:], names[:4])  # rebuilt on the ring's own stream
    tok, own = ring.dump()
    m, ids = len(tok), ring.id_bound()
    allowed, truth, active, _ = views_for(65, ids, 91, own)
    live = np.zeros(ids, dtype=bool)
    live[ring.server_ids()] = True
    want = sm.share(tok, own, allowed & live, truth & live, active)
    assert_same(host(share_dev(ring, allowed, truth=truth, active=active, stream=st.cuda_stream), m, 65), want)
    assert_same(host(share_dev(ring, allowed, truth=truth, active=active), m, 65), want)  # and the ring's own
    ring.close()


def test_names(base, orc):
    ring, tok, own = base
    names = [orc.c2_addr(i) for i in range(S)]
    rng = np.random.default_rng(51)
    views = [[s for s in names if rng.random() < 0.9] for _ in range(5)] + [[], names[3:4], names + ["10.9.9.9:1"]]
    truth = [s for s in names if rng.random() < 0.8]
    ids = ring.id_bound()

    def row(ns):
        r = np.zeros(ids, dtype=bool)
        r[np.array([ring.server_id(s) for s in ns if ring.server_id(s) != NIL], dtype=np.int64)] = True
        return r
    want = sm.share(tok, own, np.stack([row(v) for v in views]), row(truth))
    got = ring.routeShare(views, truth)
    assert got == {"wrong": want["wrong"].tolist(), "lost": want["lost"].tolist(),
                   "disputed": sm.disputed(tok, want["pos_wrong"])}
    assert all(type(x) is int for x in got["wrong"] + got["lost"] + [got["disputed"]])
    assert got["wrong"][5] == FULL and got["lost"][5] == 0 and got["disputed"] == FULL
    # truth None: every server; the last view holds them all
    got = ring.routeShare(views)
    assert got["wrong"][7] == 0 and got["lost"] == [0] * 8 and 0 < got["disputed"] <= FULL
    assert ring.routeShare([]) == {"wrong": [], "lost": [], "disputed": 0}


def test_einval_writes_nothing(base, gpu):
    ring, tok, own = base
    m, ids = len(tok), ring.id_bound()
    allowed = np.ones((3, ids), dtype=bool)
    cases = [("bit", dict(bit=0)), ("id_cap", dict(id_cap=ids - 1)), ("pos_cap", dict(pos_cap=m - 1)),
             ("row_stride", dict(id_cap=ids + 1))]  # (no column map, and rows narrower than id_cap)
    for match, kw in cases:
        into = alloc(m, 3)
        with pytest.raises(gpu.RingpopAmdError, match=match):
            share_dev(ring, allowed, into=into, **kw)
        torch.cuda.synchronize()
        assert untouched(into), match
    # more views than route_views takes (no row is read before the refusal)
    into = alloc(m, 3)
    with pytest.raises(gpu.RingpopAmdError, match="views"):
        ring.route_share_dev(ptr(into["lost"]), ids, 65535 * 64 + 1, wrong_ptr=ptr(into["wrong"]),
                             pos_wrong_ptr=ptr(into["pos_wrong"]), pos_cap=m)
    torch.cuda.synchronize()
    assert untouched(into)
    # the host form refuses the same way
    L = gpu.lib()
    w = np.full(3, 77, dtype=np.uint64)
    p = np.full(m, 77, dtype=np.uint32)
    rows = np.ones((3, ids), dtype=np.uint8)
    for args in ((rows.ctypes.data, ids, 0, 3, None, ids), (rows.ctypes.data, ids, 1, 3, None, ids - 1),
                 (rows.ctypes.data, ids, 1, 3, None, ids + 1)):
        assert L.rp_ring_route_share(ring._h, *args, None, None, 0, w.ctypes.data, None, p.ctypes.data, m) == -1
        assert (w == 77).all() and (p == 77).all()
    assert L.rp_ring_route_share(ring._h, rows.ctypes.data, ids, 1, 3, None, ids, None, None, 0, w.ctypes.data, None,
                                 p.ctypes.data, m - 1) == -1
    assert (w == 77).all() and (p == 77).all()
    # pos_cap matters only with pos_wrong
    got = host(share_dev(ring, allowed, pos=False, pos_cap=0), m, 3)
    assert got["wrong"].tolist() == [0, 0, 0]
