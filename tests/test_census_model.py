"""CPU tests of the census model (tests/census_model.py) and of census_reduce, the host's
combination of shard censuses: pure numpy, no device."""
import numpy as np
import pytest

import census_model as cm

A, S, F, L = 0, 1, 2, 3


def hand_case():
    st = np.array([[A, S, A], [A, F, A], [A, A, L]], dtype=np.uint8)
    inc = np.array([[10, 20, 30], [10, 21, 30], [11, 20, 31]], dtype=np.int64)
    ring = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=bool)
    return st, inc, ring


def test_hand_written_three_nodes():
    """Three nodes, three members; row v is node v's view:

        node 0: (alive 10) (suspect 20) (alive 30)   ring 1 1 1
        node 1: (alive 10) (faulty  21) (alive 30)   ring 1 0 1
        node 2: (alive 11) (alive   20) (leave 31)   ring 1 1 0

    Everybody observing: member 0 is alive in 3 views; member 1 is alive, suspect and faulty in one
    each; member 2 is alive in 2 and leave in 1. The newest incarnations are 11, 21, 31, each held
    by one node (2, 1, 2). Node 0 is behind on all three members, node 1 on members 0 and 2, node 2
    on member 1.
    Nodes 0 and 1 observing: the maxima are 10, 21, 30; both hold 10 and 30, node 1 alone 21, and
    only node 0 is behind (on member 1). Against the global maxima instead, the two hold only 21
    between them (node 1), node 0 is behind on 3 members, node 1 on 2."""
    st, inc, ring = hand_case()
    c = cm.census(st, inc, ring, [True] * 3)
    assert c["observers"] == 3
    assert c["status"].tolist() == [[3, 0, 0, 0], [1, 1, 1, 0], [2, 0, 0, 1]]
    assert c["in_ring"].tolist() == [3, 2, 2]
    assert c["max_inc"].tolist() == [11, 21, 31]
    assert c["at_max"].tolist() == [1, 1, 1]
    assert c["behind"].tolist() == [3, 2, 1]
    c = cm.census(st, inc, ring, [True, True, False])
    assert c["observers"] == 2
    assert c["status"].tolist() == [[2, 0, 0, 0], [0, 1, 1, 0], [2, 0, 0, 0]]
    assert c["in_ring"].tolist() == [2, 1, 2]
    assert c["max_inc"].tolist() == [10, 21, 30]
    assert c["at_max"].tolist() == [2, 1, 2]
    assert c["behind"].tolist() == [1, 0, 0]
    c = cm.census(st, inc, ring, [True, True, False], ref=[11, 21, 31])
    assert c["max_inc"].tolist() == [10, 21, 30]
    assert c["at_max"].tolist() == [0, 1, 0]
    assert c["behind"].tolist() == [3, 2, 0]
    c = cm.census(st, inc, ring, [False] * 3)
    assert c["observers"] == 0 and not c["status"].any() and not c["in_ring"].any() and not c["at_max"].any()
    assert (c["max_inc"] == cm.INT64_MIN).all() and not c["behind"].any()
    for k, dt in (("status", np.uint32), ("in_ring", np.uint32), ("max_inc", np.int64), ("at_max", np.uint32),
                  ("behind", np.uint32)):
        assert c[k].dtype == dt, k


def random_stack(rng, nl, n):
    st = rng.integers(0, 4, size=(nl, n)).astype(np.uint8)
    inc = rng.integers(-3, 4, size=(nl, n)).astype(np.int64) + 1434401518824
    ring = rng.integers(0, 2, size=(nl, n)).astype(bool)
    obs = rng.integers(0, 4, size=nl) != 0
    return st, inc, ring, obs


@pytest.mark.parametrize("bounds", [[0, 5, 13], [0, 4, 4, 13], [0, 0, 6, 13], [0, 13, 13]])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reduce_of_parts_against_the_global_max_is_the_whole(rpa, seed, bounds):
    rng = np.random.default_rng(seed)
    st, inc, ring, obs = random_stack(rng, 13, 9)
    if seed == 3:
        obs[bounds[0]:bounds[1]] = False  # a part without observers
    whole = cm.census(st, inc, ring, obs)
    cut = list(zip(bounds[:-1], bounds[1:]))
    first = [cm.census(st[a:b], inc[a:b], ring[a:b], obs[a:b]) for a, b in cut]
    ref = np.max([p["max_inc"] for p in first], axis=0)
    assert np.array_equal(ref, whole["max_inc"])
    parts = [cm.census(st[a:b], inc[a:b], ring[a:b], obs[a:b], ref=ref) for a, b in cut]
    assert cm.same(rpa.census_reduce(parts), whole) is None
    # the first phase's parts carry what they were asked for only
    only = rpa.census_reduce([{"observers": p["observers"], "max_inc": p["max_inc"]} for p in first])
    assert sorted(only) == ["max_inc", "observers"] and np.array_equal(only["max_inc"], whole["max_inc"])


def test_parts_without_a_common_reference_do_not_add_up(rpa):
    """Two shards of one node each; node 1 holds a newer incarnation of member 0. Each shard's own
    maximum is its only node's incarnation, so each reports its node at the maximum and nobody
    behind: the sum says 2 nodes hold the newest incarnation where 1 does."""
    st = np.zeros((2, 2), dtype=np.uint8)
    inc = np.array([[5, 9], [7, 9]], dtype=np.int64)
    ring = np.ones((2, 2), dtype=bool)
    obs = np.array([True, True])
    whole = cm.census(st, inc, ring, obs)
    assert whole["at_max"].tolist() == [1, 2] and whole["behind"].tolist() == [1, 0]
    own = [cm.census(st[i:i + 1], inc[i:i + 1], ring[i:i + 1], obs[i:i + 1]) for i in range(2)]
    bad = rpa.census_reduce(own)
    assert bad["at_max"].tolist() == [2, 2] and bad["behind"].tolist() == [0, 0]
    assert cm.same(bad, whole) == "at_max"
    ref = np.max([p["max_inc"] for p in own], axis=0)
    good = rpa.census_reduce([cm.census(st[i:i + 1], inc[i:i + 1], ring[i:i + 1], obs[i:i + 1], ref=ref)
                              for i in range(2)])
    assert cm.same(good, whole) is None
