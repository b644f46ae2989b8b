"""GPU tests of the simulator's routing agreement (rp_sim_ring_members, rp_sim_routing*): every
node's ring membership as a view of one base ring, in misrouted requests per node, every round of
a scenario with kills, a leave, a revival and a join, until the CPU oracle simulator reports
convergence. Reference: tests/routing_model.py over ring_members(v) of every node and the default
truth, both rebuilt here from the scenario and the views. Exact comparisons."""
import ctypes

import numpy as np
import pytest

import routing_model as rm
from test_ring_moved_gpu import _keys
from test_ring_route_gpu import _hashes
from test_sim_gpu import synth

pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
NOW0 = 1434401518824 + 10 ** 9
SUSP = 6
NKEYS = 512
LIMIT = 120
ALIVE, SUSPECT, FAULTY, LEAVE = 0, 1, 2, 3


def scenario(n):
    """Three kills at round 2, one leave, one revival, one join (a killed node's fresh process)."""
    a, b, c, d = 1, n // 2, n - 1, 3
    return [(2, "kill", a), (2, "kill", b), (2, "kill", c), (4, "leave", d), (12, "revive", a), (16, "join", b)]


def up_after(n, events, rnd):
    """Which nodes are up once the events of rounds below rnd have run."""
    up = np.ones(n, dtype=bool)
    for r, k, v in events:
        if r < rnd:
            up[v] = k != "kill"
    for r, k, v in events:  # (a leave does not take a node down)
        if r < rnd and k == "leave":
            up[v] = up[v]
    return up


def make(gpu, orc, n):
    S = synth()
    names = [S.c2_addr(i) for i in range(n)]
    inc0 = S.c3_members(n)[2]
    dead = np.zeros(n, dtype=np.uint8)
    ring = gpu.HashRing()
    ring.addRemoveServers(names, None)
    assert ring.size == n * 100  # no token collision: the model is `lookup` on each node's ring
    col = np.array([ring.server_id(s) for s in names], dtype=np.int64)  # member -> ring id
    return names, inc0, dead, ring, col


def model(sim, ring, col, n, hs, truth):
    tok, own = ring.dump()
    ids = ring.id_bound()
    allowed = np.zeros((n, ids), dtype=bool)
    for v in range(n):
        allowed[v, col] = sim.ring_members(v)
    tr = np.zeros(ids, dtype=bool)
    tr[col] = truth
    return rm.route(tok, own, hs, allowed, tr, truth)


def default_truth(sim, n, events):
    up = up_after(n, events, sim.round)
    own = np.array([sim.view(v)[0][v] for v in range(n)])
    return up & (own != LEAVE)


@pytest.mark.parametrize("n", [30, 65])
def test_routing_every_round_until_the_oracle_converges(gpu, orc, n):
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
    keys = np.array(_keys(NKEYS))
    hs = _hashes(NKEYS)
    done = None
    lost_after_kills = None
    for r in range(LIMIT):
        g.step()
        o.step()
        assert np.array_equal(g.checksums(), o.checksums()), r
        truth = default_truth(g, n, ev)
        want = model(g, ring, col, n, hs, truth)
        got = g.routing(ring, keys)
        for k in ("wrong", "lost", "key_wrong", "truth_owner"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (r, k)
        assert (got["lost"] <= got["wrong"]).all() and (got["wrong"][~truth] == 0).all()
        # an explicit truth equal to the default, and the caller-hash form
        again = g.routing(ring, keys, truth=truth)
        assert all(np.array_equal(again[k], got[k]) for k in got), r
        # ring membership against the status view
        for v in range(n):
            st = g.view(v)[0]
            ir = g.ring_members(v)
            assert ir[st == ALIVE].all() and not ir[(st == FAULTY) | (st == LEAVE)].any(), (r, v)
        for s in sharded:
            s.step()
            assert np.array_equal(s.default_truth(), truth), r
            sg = s.routing(ring, keys)
            assert all(np.array_equal(sg[k], got[k]) and sg[k].dtype == got[k].dtype for k in got), r
            assert np.array_equal(s.ring_members(n - 1), g.ring_members(n - 1))
        if r == 2:  # the round whose events killed three nodes
            lost_after_kills = int(got["lost"].sum())
        # the oracle says when to stop, once the whole scenario has run (an untouched cluster is
        # converged from round 0 on)
        if r > max(e[0] for e in ev) and o.converged():
            done = r
            break
    assert lost_after_kills is not None and lost_after_kills > 0  # requests went to servers that are gone
    assert done is not None and done > 16, done  # past the last event
    assert g.converged()
    assert got["wrong"].sum() == 0 and got["key_wrong"].sum() == 0
    assert truth.sum() == n - 2  # one node stays down, one has left
    for s in sharded:
        s.close()
    g.close()
    ring.close()


def test_routing_hashes_and_a_ring_that_lacks_members(gpu, orc):
    n = 30
    names, inc0, dead, _, _ = make(gpu, orc, n)
    ev = scenario(n)
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev)
    g.step(5)
    # a ring without member 5 and with a server that is no member, ids not in member order
    ring = gpu.HashRing()
    ring.addRemoveServers(["10.7.7.7:7"] + names[::-1], None)
    ring.addRemoveServers(None, [names[5]])
    tok, own = ring.dump()
    ids = ring.id_bound()
    truth = default_truth(g, n, ev)
    allowed = np.zeros((n, ids), dtype=bool)
    tr = np.zeros(ids, dtype=bool)
    for a, s in enumerate(names):
        i = ring.server_id(s)
        allowed[:, i] = [g.ring_members(v)[a] for v in range(n)]
        tr[i] = truth[a]
    hs = np.concatenate([rm.edge_hashes(tok), _hashes(NKEYS)])
    want = rm.route(tok, own, hs, allowed, tr, truth)
    assert (want["owners"] != ring.server_id("10.7.7.7:7")).all()
    L = gpu.lib()
    out = {"wrong": np.zeros(n, dtype=np.uint64), "lost": np.zeros(n, dtype=np.uint64),
           "key_wrong": np.zeros(len(hs), dtype=np.uint32), "truth_owner": np.zeros(len(hs), dtype=np.uint32)}
    gpu.check(L.rp_sim_routing_hashes(g._h, ring._h, hs.ctypes.data, len(hs), None, *(out[k].ctypes.data for k in out)))
    for k in out:
        assert np.array_equal(out[k], want[k]), k
    # after queued rounds the call follows them on the simulator's stream
    g.step_async(2)
    got = g.routing(ring, np.array(_keys(NKEYS)))
    g.sync()
    truth = default_truth(g, n, ev)
    for a, s in enumerate(names):
        allowed[:, ring.server_id(s)] = [g.ring_members(v)[a] for v in range(n)]
        tr[ring.server_id(s)] = truth[a]
    want = rm.route(tok, own, _hashes(NKEYS), allowed, tr, truth)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    g.close()
    ring.close()


def test_sharded_handle_needs_the_truth_and_a_ring_on_its_device(gpu, orc):
    n = 30
    names, inc0, dead, ring, _ = make(gpu, orc, n)
    L = gpu.lib()
    sh = gpu.SimShard(names, inc0, dead, 2, 0)
    keys = np.array(_keys(64))
    w = np.zeros(sh.NL, dtype=np.uint64)
    rc = L.rp_sim_routing(sh._h, ring._h, keys.ctypes.data, None, 36, 64, None, w.ctypes.data, None, None, None)
    assert rc == -1 and b"truth" in L.rp_last_error()
    truth = np.ones(n, dtype=np.uint8)
    gpu.check(L.rp_sim_routing(sh._h, ring._h, keys.ctypes.data, None, 36, 64, truth.ctypes.data, w.ctypes.data, None,
                               None, None))
    assert (w == 0).all()  # every view starts with everybody in the ring
    sh.stage(0)  # inside a round
    rc = L.rp_sim_routing(sh._h, ring._h, keys.ctypes.data, None, 36, 64, truth.ctypes.data, w.ctypes.data, None,
                          None, None)
    assert rc == -1 and b"round boundary" in L.rp_last_error()
    g = gpu.GossipSim(names, inc0, dead)
    rc = L.rp_sim_routing(g._h, None, keys.ctypes.data, None, 36, 64, None, None, None, None, None)
    assert rc == -1 and b"ring" in L.rp_last_error()
    sh.close()
    g.close()
    ring.close()


def test_ring_on_another_device_is_refused(gpu, orc):
    if gpu.device_count() < 2:
        pytest.skip("needs a second device")
    n = 30
    names, inc0, dead, ring, _ = make(gpu, orc, n)
    other = gpu.HashRing(device=1)
    other.addRemoveServers(names, None)
    g = gpu.GossipSim(names, inc0, dead)
    with pytest.raises(gpu.RingpopAmdError, match="another device"):
        g.routing(other, np.array(_keys(64)))
    assert g.routing(ring, np.array(_keys(64)))["wrong"].sum() == 0
    g.close()
    other.close()
    ring.close()
