"""CPU tests that pin tests/routing_model.py (the model the GPU routing tests compare with) against
the oracle ring, not against the code under test: a view's owners are `lookup` on the oracle ring
after add_remove(remove=the masked-out names), at allowed densities 0.9 / 0.5 / 0.02, on random
hashes and the six hashes at the ring's ends. That identity needs a base ring without token
collisions, which is asserted. The walk of the header (first allowed owner from the key's position,
cyclically) is checked against the same model, and the counts against their definitions."""
import numpy as np
import pytest

import routing_model as rm

NIL = rm.NIL
S = 70


@pytest.fixture(scope="module")
def base(orc):
    names = [orc.c2_addr(i) for i in range(S)]
    ring = orc.Ring(100)
    ring.add_remove(names)
    tok, own = ring.dump()
    rng = np.random.default_rng(7)
    hashes = np.concatenate([rm.edge_hashes(tok), rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)])
    return names, ring, tok, own, hashes


def test_no_token_collision(base, orc):
    names, ring, tok, own, _ = base
    assert ring.token_count() == S * 100 == len(np.unique(tok))
    big = orc.Ring(100)
    big.add_remove([orc.c2_addr(i) for i in range(300)])
    assert big.token_count() == 30_000


@pytest.mark.parametrize("density", [0.9, 0.5, 0.02])
def test_view_owners_are_the_oracle_ring_after_removal(base, orc, density):
    names, ring, tok, own, hashes = base
    rng = np.random.default_rng(int(density * 100))
    allowed = rng.random(S) < density
    if not allowed.any():
        allowed[int(rng.integers(S))] = True
    assert 0 < allowed.sum() < S
    sub = orc.Ring(100)
    sub.add_remove(names)
    sub.add_remove(remove=[n for n, a in zip(names, allowed) if not a])
    assert sub.server_count() == int(allowed.sum())
    want = [sub.name(sub.lookup_hash(int(h))) for h in hashes]
    by_ring_id = np.zeros(S, dtype=bool)
    for i in range(S):
        by_ring_id[i] = allowed[names.index(ring.name(i))]
    got = [ring.name(int(o)) for o in rm.view_owners(tok, own, hashes, by_ring_id)]
    assert got == want
    assert len(set(got[:6])) >= 1 and None not in got


def walk_owner(tok, own, h, allowed):
    """The header's definition, step by step."""
    m = len(tok)
    i = int(np.searchsorted(tok, h, "left"))
    if i == m:
        i = 0
    for s in range(m):
        o = int(own[(i + s) % m])
        if allowed[o]:
            return o
    return NIL


def test_the_walk_equals_the_filtered_ring(base):
    _, _, tok, own, hashes = base
    rng = np.random.default_rng(3)
    for density in (0.9, 0.5, 0.02, 0.0):
        allowed = rng.random(S) < density
        want = [walk_owner(tok, own, h, allowed) for h in hashes[:306]]
        assert rm.view_owners(tok, own, hashes[:306], allowed).tolist() == want
    one = np.zeros(S, dtype=bool)
    one[int(own[len(own) // 2])] = True  # long walks and the wrap
    assert rm.view_owners(tok, own, hashes, one).tolist() == [int(own[len(own) // 2])] * len(hashes)


def test_counts_follow_their_definitions(base):
    _, _, tok, own, hashes = base
    rng = np.random.default_rng(5)
    hs = hashes[:400]
    allowed = rng.random((9, S)) < 0.9
    allowed[3] = False
    truth = rng.random(S) < 0.8
    allowed[4] = truth
    active = np.ones(9, dtype=bool)
    active[[1, 6]] = False
    r = rm.route(tok, own, hs, allowed, truth, active)
    wrong = np.zeros(9, dtype=np.uint64)
    lost = np.zeros(9, dtype=np.uint64)
    kw = np.zeros(len(hs), dtype=np.uint32)
    for k, h in enumerate(hs):
        t = walk_owner(tok, own, h, truth)
        assert r["truth_owner"][k] == t
        for v in range(9):
            o = walk_owner(tok, own, h, allowed[v])
            assert r["owners"][k, v] == o
            if not active[v]:
                continue
            wrong[v] += o != t
            kw[k] += o != t
            lost[v] += o != NIL and not truth[o]
    assert np.array_equal(r["wrong"], wrong) and np.array_equal(r["lost"], lost)
    assert np.array_equal(r["key_wrong"], kw)
    assert (r["lost"] <= r["wrong"]).all() and r["wrong"][4] == 0 and r["wrong"][1] == 0
    assert r["wrong"][3] == len(hs) and r["lost"][3] == 0 and r["lost"].sum() > 0
    # truth None: every server of the ring
    r2 = rm.route(tok, own, hs, allowed)
    assert np.array_equal(r2["truth_owner"], rm.view_owners(tok, own, hs, np.ones(S, dtype=bool)))
    assert r2["lost"].sum() == 0


def test_by_id_applies_the_column_map():
    rows = np.array([[1, 0, 1, 0], [0, 0x80, 0, 0]], dtype=np.uint8)
    col = np.array([2, NIL, 1, 0, 7], dtype=np.uint32)
    got = rm.by_id(rows, col, 5)
    assert got.tolist() == [[True, False, False, True, False], [False, False, True, False, False]]
    assert rm.by_id(rows, None, 4).tolist() == (rows != 0).tolist()
