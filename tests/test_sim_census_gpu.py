"""GPU tests of the simulator's census (rp_sim_census): every member's status,
ring and incarnation counts over all views, from the deviation bitmaps. Reference:
tests/census_model.py over view(v) / ring_members(v) of every node, so a row that changed without
its deviation bit shows as a wrong count. Exact comparisons."""
import ctypes

import numpy as np
import pytest

import census_model as cm
from test_sim_gpu import synth
from test_sim_route_gpu import LEAVE, LIMIT, NOW0, SUSP, scenario, up_after

pytestmark = pytest.mark.gpu


def cluster(n):
    S = synth()
    return [S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], np.zeros(n, dtype=np.uint8)


def stack(sim, n):
    """Every node's view, stacked: st, inc, ring [n, n]."""
    st = np.empty((n, n), dtype=np.uint8)
    inc = np.empty((n, n), dtype=np.int64)
    ring = np.empty((n, n), dtype=bool)
    for v in range(n):
        st[v], inc[v] = sim.view(v)
        ring[v] = sim.ring_members(v)
    return st, inc, ring


def check(got, want, what):
    bad = cm.same(got, want)
    assert bad is None, (what, bad, got[bad] if bad != "observers" else got["observers"],
                         want[bad] if bad != "observers" else want["observers"])
    n_obs = got["observers"]
    assert (got["status"].sum(axis=1) == n_obs).all() and (got["at_max"] <= n_obs).all(), what


@pytest.mark.parametrize("n", [30, 65])
def test_census_every_round_of_a_scenario(gpu, n):
    names, inc0, dead = cluster(n)
    assert sorted(names) != names or n <= 10  # address rank != member id
    ev = scenario(n)
    kw = dict(seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev)
    g = gpu.GossipSim(names, inc0, dead, **kw)
    sharded = []
    if n == 30:
        sharded = [gpu.ShardedGossipSim(names, inc0, dead, 2, **kw),
                   gpu.ShardedGossipSim(names, inc0, dead, 3, bounds=np.array([0, 11, 11, n], dtype=np.uint32), **kw)]
        assert sharded[1].shards[1].NL == 0
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    third[n - 1] = True  # killed at round 2 and never back: its view is kept
    done = None
    for r in range(LIMIT):
        g.step()
        for s in sharded:
            s.step()
        st, inc, ring = stack(g, n)
        up = up_after(n, ev, g.round)
        serving = up & (st[np.arange(n), np.arange(n)] != LEAVE)
        for what, obs in (("default", None), ("third", third), ("serving", serving)):
            want = cm.census(st, inc, ring, up if obs is None else obs)
            got = g.census(obs)
            check(got, want, (r, what))
            for s in sharded:
                check(s.census(obs), got, (r, what, "shards", s.G))
        if r > max(e[0] for e in ev) and g.converged():
            done = r
            assert (got["at_max"] == got["observers"]).all() and not got["behind"].any()
            assert got["observers"] == n - 2  # one node stays down, one has left
            break
    assert done is not None and done > 16, done
    for s in sharded:
        s.close()
    g.close()


def test_census_two_column_tiles_and_ragged_slabs(gpu, monkeypatch):
    """n = 530: 17 bitmap words a row, so two column tiles, the second one word wide, whose last
    word holds 18 ranks; slabs of 7 rows are no multiple of the 16 rows a step and do not divide
    the nodes, slabs of 64 give several whole ones."""
    n = 530
    S = synth()
    names, inc0, dead = cluster(n)
    killed = np.nonzero(S.kill_set(n, n // 20))[0]
    assert len(killed) == 26
    ev = [(1, "kill", int(v)) for v in killed] + [(8, "join", int(killed[3]))]
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev)
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    third[killed[0]] = True
    seen_deviation = False
    for rnd in (2, 6, 14):
        g.step(rnd - g.round)
        assert g.round == rnd
        st, inc, ring = stack(g, n)
        up = up_after(n, ev, rnd)
        wants = {"default": cm.census(st, inc, ring, up), "third": cm.census(st, inc, ring, third)}
        seen_deviation |= bool((wants["default"]["status"][:, 0] != wants["default"]["observers"]).any())
        for rows in (None, "7", "64"):
            if rows is None:
                monkeypatch.delenv("RP_CENSUS_ROWS", raising=False)
            else:
                monkeypatch.setenv("RP_CENSUS_ROWS", rows)
            check(g.census(), wants["default"], (rnd, rows, "default"))
            check(g.census(third), wants["third"], (rnd, rows, "third"))
    assert seen_deviation
    g.close()


def test_census_of_a_fresh_simulator(gpu):
    n = 33
    names, inc0, dead = cluster(n)
    dead[4] = 1
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0)
    c = g.census()
    assert c["observers"] == n - 1
    assert (c["status"][:, 0] == n - 1).all() and not c["status"][:, 1:].any()
    assert (c["in_ring"] == n - 1).all() and (c["at_max"] == n - 1).all() and not c["behind"].any()
    assert np.array_equal(c["max_inc"], inc0) and c["max_inc"].dtype == np.int64
    st, inc, ring = stack(g, n)
    check(c, cm.census(st, inc, ring, dead == 0), "round 0")
    z = g.census(np.zeros(n, dtype=bool))
    check(z, cm.census(st, inc, ring, np.zeros(n, dtype=bool)), "nobody observes")
    assert z["observers"] == 0 and (z["max_inc"] == cm.INT64_MIN).all()
    assert not z["status"].any() and not z["in_ring"].any() and not z["at_max"].any() and not z["behind"].any()
    # every output is optional in the C ABI
    n_obs = ctypes.c_uint32(77)
    gpu.check(gpu.lib().rp_sim_census(g._h, None, None, ctypes.byref(n_obs), None, None, None, None, None))
    assert n_obs.value == n - 1
    only = g.census(want=("in_ring",))
    assert sorted(only) == ["in_ring", "observers"] and (only["in_ring"] == n - 1).all()
    g.close()


def test_census_against_a_given_reference(gpu):
    n = 30
    names, inc0, dead = cluster(n)
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=scenario(n))
    # (a suspicion keeps the member's incarnation: nobody is behind before the revived node of
    # round 12 refutes its own with a newer one, which then takes some rounds to reach everybody)
    g.step(12)
    c = g.census()
    while not c["behind"].any() and g.round < 20:
        g.step()
        c = g.census()
    assert c["behind"].any() and (c["at_max"] < c["observers"]).any()
    check(g.census(max_ref=c["max_inc"]), c, "its own maximum")
    up = up_after(n, scenario(n), g.round)
    ahead = g.census(max_ref=c["max_inc"] + 1)
    assert not ahead["at_max"].any()
    assert np.array_equal(ahead["behind"], np.where(up, n, 0)) and ahead["behind"].dtype == np.uint32
    for k in ("status", "in_ring", "max_inc"):
        assert np.array_equal(ahead[k], c[k]), k
    st, inc, ring = stack(g, n)
    check(ahead, cm.census(st, inc, ring, up, ref=c["max_inc"] + 1), "one ahead")
    g.close()


def test_census_follows_the_queued_rounds(gpu):
    n = 30
    names, inc0, dead = cluster(n)
    kw = dict(seed=7, suspicion_rounds=SUSP, now0=NOW0, events=[(1, "kill", 5), (1, "kill", 17)])
    a = gpu.GossipSim(names, inc0, dead, **kw)
    b = gpu.GossipSim(names, inc0, dead, **kw)
    a.step_async(3)
    got = a.census()
    b.step(3)
    want = b.census()
    check(got, want, "after step_async(3)")
    assert (want["status"][:, 0] != want["observers"]).any()
    a.sync()
    a.close()
    b.close()


def test_census_errors(gpu):
    n = 30
    names, inc0, dead = cluster(n)
    g = gpu.GossipSim(names, inc0, dead)
    with pytest.raises(ValueError):
        g.census(np.ones(n - 1, dtype=bool))
    with pytest.raises(ValueError):
        g.census(max_ref=np.zeros(n + 1, dtype=np.int64))
    g.close()
    L = gpu.lib()
    two = gpu.ShardedGossipSim(names, inc0, dead, 2)
    sh = two.shards[0]
    with pytest.raises(ValueError):
        sh.census(np.ones(sh.NL, dtype=bool))  # observe is global, by node id
    assert sh.census()["observers"] == sh.NL  # a round boundary
    n_obs = ctypes.c_uint32()
    for k in range(gpu.SIM_STAGES):  # one round by hand, as ShardedGossipSim.step runs it
        for s in two.shards:
            s.stage(k)
        if k == gpu.SIM_STAGES - 1:
            break
        for s in two.shards:  # inside a round
            rc = L.rp_sim_census(s._h, None, None, ctypes.byref(n_obs), None, None, None, None, None)
            assert rc == -1 and b"round boundary" in L.rp_last_error(), k
        with pytest.raises(gpu.RingpopAmdError):
            sh.census()
        gpu.check(L.rp_sim_exchange_local(two._arr, two.G))
    assert two.round == 1 and two.census()["observers"] == n  # the next boundary
    two.close()
