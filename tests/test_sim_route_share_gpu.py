"""GPU tests of the simulator's key-free routing agreement (rp_sim_routing_share): every node's ring
membership as a view of one base ring, in misrouted hash values (of 2^32) per node, every few
rounds of the scenario of tests/test_sim_route_gpu.py (three kills, a leave, a revival, a join)
until the CPU oracle simulator reports convergence; unsharded, and on 2 and 3 shards with an empty
one. Reference: tests/route_share_model.py over ring_members(v) of every node and the default
truth, both rebuilt here from the scenario and the views. Exact comparisons."""
import numpy as np
import pytest

import route_share_model as sm
from test_sim_route_gpu import LIMIT, NOW0, SUSP, default_truth, make, scenario

pytestmark = pytest.mark.gpu

EVERY = 3
FULL = 1 << 32


def model(sim, ring, col, n, truth):
    tok, own = ring.dump()
    ids = ring.id_bound()
    allowed = np.zeros((n, ids), dtype=bool)
    for v in range(n):
        allowed[v, col] = sim.ring_members(v)
    tr = np.zeros(ids, dtype=bool)
    tr[col] = truth
    return sm.share(tok, own, allowed, tr, truth)


@pytest.mark.parametrize("n", [30, 65])
def test_routing_share_until_the_oracle_converges(gpu, orc, n):
    names, inc0, dead, ring, col = make(gpu, orc, n)
    ev = scenario(n)
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev)
    o = orc.Sim(names, inc0, dead, seed=7, susp_rounds=SUSP, now0=NOW0, events=ev)
    sharded = []
    if n == 30:
        sharded = [gpu.ShardedGossipSim(names, inc0, dead, 2, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev),
                   gpu.ShardedGossipSim(names, inc0, dead, 3, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev,
                                        bounds=np.array([0, 11, 11, n], dtype=np.uint32))]
        assert sharded[1].shards[1].NL == 0
    last_event = max(e[0] for e in ev)
    done = lost_after_kills = got = None
    for r in range(LIMIT):
        g.step()
        o.step()
        for s in sharded:
            s.step()
        stop = r > last_event and o.converged()
        if not (stop or r == 2 or r % EVERY == 0):
            continue
        assert np.array_equal(g.checksums(), o.checksums()), r
        truth = default_truth(g, n, ev)
        want = model(g, ring, col, n, truth)
        got = g.routingShare(ring)
        for k in ("wrong", "lost", "pos_wrong"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (r, k)
        assert (got["lost"] <= got["wrong"]).all() and (got["wrong"] <= FULL).all()
        assert (got["wrong"][~truth] == 0).all()
        # an explicit truth equal to the default
        again = g.routingShare(ring, truth=truth)
        assert all(np.array_equal(again[k], got[k]) for k in got), r
        for s in sharded:
            sg = s.routingShare(ring)
            assert all(np.array_equal(sg[k], got[k]) and sg[k].dtype == got[k].dtype for k in got), r
        if r == 2:  # the round whose events killed three nodes
            lost_after_kills = int(got["lost"].sum())
        if stop:
            done = r
            break
    assert lost_after_kills is not None and lost_after_kills > 0  # hash values sent to servers that are gone
    assert done is not None and done > 16, done  # past the last event
    assert g.converged()
    assert got["wrong"].sum() == 0 and got["lost"].sum() == 0 and got["pos_wrong"].sum() == 0
    for s in sharded:
        s.close()
    g.close()
    ring.close()


def test_sharded_handle_needs_the_truth_and_a_round_boundary(gpu, orc):
    n = 30
    names, inc0, dead, ring, _ = make(gpu, orc, n)
    L = gpu.lib()
    m = ring.size
    sh = gpu.SimShard(names, inc0, dead, 2, 0)
    w = np.full(sh.NL, 77, dtype=np.uint64)
    p = np.full(m, 77, dtype=np.uint32)
    rc = L.rp_sim_routing_share(sh._h, ring._h, None, w.ctypes.data, None, p.ctypes.data, m)
    assert rc == -1 and b"truth" in L.rp_last_error()
    truth = np.ones(n, dtype=np.uint8)
    rc = L.rp_sim_routing_share(sh._h, ring._h, truth.ctypes.data, w.ctypes.data, None, p.ctypes.data, m - 1)
    assert rc == -1 and b"pos_cap" in L.rp_last_error()
    assert (w == 77).all() and (p == 77).all()
    res = sh.routing_share(ring, truth)
    assert (res["wrong"] == 0).all() and (res["pos_wrong"] == 0).all()  # every view starts with everybody in the ring
    assert len(res["wrong"]) == sh.NL and len(res["pos_wrong"]) == m
    sh.stage(0)  # inside a round
    rc = L.rp_sim_routing_share(sh._h, ring._h, truth.ctypes.data, w.ctypes.data, None, p.ctypes.data, m)
    assert rc == -1 and b"round boundary" in L.rp_last_error()
    g = gpu.GossipSim(names, inc0, dead)
    rc = L.rp_sim_routing_share(g._h, None, None, None, None, None, 0)
    assert rc == -1 and b"ring" in L.rp_last_error()
    assert (w == 77).all() and (p == 77).all()
    sh.close()
    g.close()
    ring.close()
