"""CPU tests of tests/route_share_model.py, the model the GPU tests of rp_ring_route_share* compare
with. The model is routing_model.route at hashes = tok weighted by the interval lengths; here:
the lengths sum to 2^32, the owners are constant on every interval (which is what lets a token
stand for its interval), and the generate / propagate scan the kernels use, with its chunk
carries and the cyclic wrap value, gives the same numbers at every chunk size."""
import numpy as np
import pytest

import route_share_model as sm
import routing_model as rm

NIL = rm.NIL
# servers x replica points, views, truth density (None: no truth given), view density
SHAPES = [(7, 3, 3, 0.5, 0.6), (20, 4, 17, None, 0.9), (12, 5, 64, 0.0, 0.3), (5, 2, 65, 0.97, 0.99),
          (20, 4, 130, 0.2, 0.5), (7, 3, 9, None, 0.3), (70, 100, 130, 0.8, 0.9), (70, 100, 66, 0.03, 0.95)]


def make(orc, servers, points, nv, tdens, vdens, seed):
    ring = orc.Ring(points)
    ring.add_remove([orc.c2_addr(i) for i in range(servers)])
    tok, own = ring.dump()
    assert len(tok) == len(np.unique(tok)) > 0
    rng = np.random.default_rng(seed)
    allowed = rng.random((nv, servers)) < vdens
    truth = None if tdens is None else rng.random(servers) < tdens
    allowed[0] = False  # a view allowing nobody
    allowed[1] = False
    allowed[1][int(own[len(own) // 3])] = True  # a view with one server
    if truth is not None:
        allowed[2] = truth  # the truth itself as a view
    active = rng.random(nv) < 0.7
    active[:3] = True
    return tok, own, allowed, truth, active


@pytest.fixture(scope="module", params=range(len(SHAPES)), ids=["%dx%d-%dv" % s[:3] for s in SHAPES])
def case(request, orc):
    return make(orc, *SHAPES[request.param], seed=100 + request.param)


def test_lengths_sum_to_the_hash_space(case):
    tok = case[0]
    ln = sm.lengths(tok)
    assert ln.dtype == np.uint64 and int(ln.sum()) == 1 << 32 and (ln > 0).all()
    assert int(ln[0]) == int(tok[0]) + (1 << 32) - int(tok[-1])
    assert sm.lengths(np.array([12345], dtype=np.uint32)).tolist() == [1 << 32]  # a one-token ring
    assert len(sm.lengths(np.zeros(0, dtype=np.uint32))) == 0


def test_owners_are_constant_on_every_interval(case):
    """Both ends of every interval, the wrap pieces of interval 0 and random hashes inside give the
    owner that the token itself gives."""
    tok, own, allowed, truth, _ = case
    m = len(tok)
    rng = np.random.default_rng(1)
    first = (tok[:-1].astype(np.int64) + 1).astype(np.uint32)  # tok[i-1] + 1, the first hash of interval i > 0
    ln = sm.lengths(tok).astype(np.int64)
    inside = ((tok.astype(np.int64) - (rng.random(m) * ln).astype(np.int64)) % (1 << 32)).astype(np.uint32)
    edges = rm.edge_hashes(tok)  # 0, tok[0], tok[0]+1, tok[M-1], tok[M-1]+1, 2^32-1
    edge_pos = [0, 0, 1 % m, m - 1, 0, 0]
    rows = list(allowed[:8]) + [np.ones(allowed.shape[1], dtype=bool)] + ([] if truth is None else [truth])
    for a in rows:
        at_tok = rm.view_owners(tok, own, tok, a)
        assert np.array_equal(rm.view_owners(tok, own, first, a), at_tok[1:])
        assert np.array_equal(rm.view_owners(tok, own, inside, a), at_tok)
        assert rm.view_owners(tok, own, edges, a).tolist() == [int(at_tok[i]) for i in edge_pos]


@pytest.mark.parametrize("chunk", [1, 7, 64, None])
def test_the_scan_equals_the_model(case, chunk):
    tok, own, allowed, truth, active = case
    m = len(tok)
    for tr, ac in ((truth, active), (truth, None)):
        want = sm.share(tok, own, allowed, tr, ac)
        got = sm.scan(tok, own, allowed, tr, ac, chunk=m if chunk is None else chunk)
        for k in ("wrong", "lost", "pos_wrong"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        assert (want["lost"] <= want["wrong"]).all() and int(want["wrong"].max()) <= 1 << 32
        if tr is not None:
            assert want["wrong"][2] == 0 and want["lost"][2] == 0  # the truth as a view
        assert want["lost"][0] == 0  # the view allowing nobody sends nothing anywhere
        if ac is not None:
            assert (want["wrong"][~ac] == 0).all()
        assert sm.disputed(tok, want["pos_wrong"]) >= int(want["wrong"].max())


def test_a_truth_that_allows_nobody(orc):
    tok, own, allowed, _, _ = make(orc, 7, 3, 5, None, 0.6, seed=9)
    nobody = np.zeros(7, dtype=bool)
    for chunk in (1, 4, len(tok)):
        got = sm.scan(tok, own, allowed, nobody, None, chunk=chunk)
        want = sm.share(tok, own, allowed, nobody, None)
        anybody = allowed.any(axis=1)
        assert got["wrong"].tolist() == want["wrong"].tolist() == [(1 << 32) * int(a) for a in anybody]
        assert got["lost"].tolist() == want["lost"].tolist() == got["wrong"].tolist()
        assert np.array_equal(got["pos_wrong"], want["pos_wrong"])


def test_an_empty_ring():
    e32 = np.zeros(0, dtype=np.uint32)
    for f in (sm.share, sm.scan):
        r = f(e32, e32, np.ones((3, 1), dtype=bool))
        assert r["wrong"].tolist() == [0, 0, 0] and r["lost"].tolist() == [0, 0, 0] and len(r["pos_wrong"]) == 0
