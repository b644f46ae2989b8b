"""GPU parity of the gossip simulator under network partitions: "side" and "heal" events, sides()
and side_summary(). Every case of tests/golden/sim_net_golden.json (the reference modules, 2..17
nodes) unsharded and through the sharded path; at wave and workgroup boundaries (63..257 nodes) each
side of a three-way split against the CPU oracle's run of the equivalent kill scenario; the per-side
summary against a numpy model over the views. Bit-exact."""
import random

import numpy as np
import pytest

import sim_net_cases as net
import sim_tiny_cases
from test_sim_gpu import STAT, _golden_sim, synth
from test_sim_tiny_gpu import _shapes

pytestmark = pytest.mark.gpu

NET = net.load()


def _replay(case, sim, names):
    """Checksums, maxPiggybackCount and sides() after every round; the full syncs and the recorded
    views at the end."""
    for r, want in enumerate(case["checksums"]):
        sim.step()
        assert sim.checksums().tolist() == want, (case["name"], r)
        assert sim.piggyback().tolist() == case["maxPiggyback"][r], (case["name"], r)
        assert sim.sides().tolist() == case["sides"][r], (case["name"], r)
    assert sim.stats()["fullsyncs"] == case["fullSyncs"], case["name"]
    for v, view in zip(case["views"], case["finalViews"]):
        st, inc = sim.view(v)
        got = {names[i]: (int(st[i]), int(inc[i])) for i in range(case["n"])}
        assert got == {a: (STAT[s], i) for a, s, i in view}, (case["name"], v)
    sim.close()


def _sharded(gpu, case, bounds):
    S = synth()
    n = case["n"]
    names = [S.c2_addr(i) for i in range(n)]
    sim = gpu.ShardedGossipSim(names, S.c3_members(n)[2], np.array(case["dead"], dtype=np.uint8), len(bounds) - 1,
                               seed=case["seed"], suspicion_rounds=case["suspRounds"], now0=case["now0"],
                               events=case["events"], bounds=np.array(bounds, dtype=np.uint32))
    return names, sim


@pytest.mark.parametrize("case_name", list(NET))
def test_net_sim_matches_reference_goldens(gpu, case_name):
    """(a) Every golden case on one handle."""
    case = NET[case_name]
    names, sim = _golden_sim(gpu, case)
    _replay(case, sim, names)


SHARDED = [(name, shape) for name, c in NET.items() for shape in _shapes(c["n"])]


@pytest.mark.parametrize("case_name,shape", SHARDED)
def test_net_sharded_sim_matches_reference_goldens(gpu, case_name, shape):
    """(b) Every golden case through the sharded path: 2 and 3 shards, empty shards first, in the
    middle and last, one node per shard."""
    case = NET[case_name]
    names, sim = _sharded(gpu, case, _shapes(case["n"])[shape])
    _replay(case, sim, names)


def test_cuts_coincide_with_shard_bounds_and_cross_them():
    """The placements (b) promises do occur: a round whose every shard lies on one side while the
    cluster is cut (the cut runs along shard bounds), and a shard holding nodes of two sides."""
    seen = set()
    for name, shape in SHARDED:
        case = NET[name]
        bounds = _shapes(case["n"])[shape]
        for row in {tuple(r) for r in case["sides"]}:
            if len(set(row)) < 2:
                continue
            per_shard = [set(row[bounds[g]:bounds[g + 1]]) for g in range(len(bounds) - 1)]
            if shape != "g=n":
                seen.add("along" if all(len(s) <= 1 for s in per_shard) else "across")
    assert seen == {"along", "across"}


# ---- (c) each side of a three-way split against the oracle's kill scenario

_BOUNDARY = {}


def _boundary(orc, n):
    """Random kills, revives, leaves and joins in rounds 0..29 with a three-way split (node v on
    side v % 3) at round 5, and the oracle's checksums of each side's nodes after each of 40 rounds
    (its run of sim_net_cases.kill_equivalent). Once per process."""
    if n not in _BOUNDARY:
        S = synth()
        rng = random.Random(4000 + n)
        dead, events = sim_tiny_cases.random_dead_events(rng, n, 0.1, 30)
        at = next((i for i, e in enumerate(events) if e[0] >= 5), len(events))
        events = events[:at] + net.split(5, {v: v % 3 for v in range(n) if v % 3}) + events[at:]
        names = [S.c2_addr(i) for i in range(n)]
        inc0 = S.c3_members(n)[2]
        dead = np.array(dead, dtype=np.uint8)
        want = np.zeros((40, n), dtype=np.uint32)
        for s in range(3):
            o = orc.Sim(names, inc0, dead, seed=4000 + n, susp_rounds=3, now0=1434401518824 + 10 ** 9,
                        events=net.kill_equivalent(n, events, s))
            for r in range(40):
                o.step()
                want[r, s::3] = o.checksums()[s::3]
        _BOUNDARY[n] = (names, inc0, dead, events, want)
    return _BOUNDARY[n]


@pytest.mark.parametrize("sharded", [False, True], ids=["one", "g3"])
@pytest.mark.parametrize("n", [63, 64, 65, 129, 257])
def test_sides_of_a_split_vs_oracle_at_wave_boundaries(gpu, orc, n, sharded):
    """Around one, two and four waves, unsharded and in three shards of 1, n-2 and 1 nodes: every
    node's checksum after each of 40 rounds equals the oracle's for its side, where everyone outside
    the side was killed at the split instead."""
    names, inc0, dead, events, want = _boundary(orc, n)
    kw = dict(seed=4000 + n, suspicion_rounds=3, events=events)
    if sharded:
        g = gpu.ShardedGossipSim(names, inc0, dead, 3, bounds=np.array([0, 1, n - 1, n], dtype=np.uint32), **kw)
    else:
        g = gpu.GossipSim(names, inc0, dead, **kw)
    for r in range(40):
        g.step()
        assert np.array_equal(g.checksums(), want[r]), "round %d" % r
    assert g.sides().tolist() == [v % 3 for v in range(n)]
    g.close()


# ---- (d) side_summary

SUMMARY_CASES = ["n6-two", "n9-three-healed", "n6-side-all-down", "n6-side-all-down-revive", "n8-join-leave-healed",
                 "net-rand06-n15"]


def _observers(case):
    """[rounds] bool[n]: the nodes convergence compares after each round: up and not left (a leave
    counts when the node is up; a join starts a fresh process)."""
    up = [not d for d in case["dead"]]
    left = [False] * case["n"]
    out = []
    for r in range(case["rounds"]):
        for e in case["events"]:
            if e[0] != r:
                continue
            kind, v = e[1], e[2]
            if kind in ("kill", "revive"):
                up[v] = kind == "revive"
            elif kind == "leave" and up[v]:
                left[v] = True
            elif kind == "join":
                up[v], left[v] = True, False
        out.append((np.array(up), np.array(up) & ~np.array(left)))
    return out


def _summary_model(n, side, up, obs, cks, views):
    side = np.array(side)
    res = {"nodes": np.zeros(256, dtype=np.uint32), "ck_min": np.full(256, 0xFFFFFFFF, dtype=np.uint32),
           "ck_max": np.zeros(256, dtype=np.uint32), "cross_pingable": np.zeros(256, dtype=np.uint64)}
    for v in np.flatnonzero(obs):
        s = side[v]
        res["nodes"][s] += 1
        res["ck_min"][s] = min(res["ck_min"][s], cks[v])
        res["ck_max"][s] = max(res["ck_max"][s], cks[v])
        away = ~up | (side != s)
        res["cross_pingable"][s] += np.uint64(np.count_nonzero((views[v] <= STAT["suspect"]) & away))
    res["settled"] = (res["ck_min"] == res["ck_max"]) & (res["cross_pingable"] == 0)
    return res


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


@pytest.mark.parametrize("case_name", SUMMARY_CASES)
def test_side_summary_matches_model(gpu, case_name):
    """side_summary() after every round, on one handle and reduced over 3 shards and over a shape
    with empty shards, against a numpy model over view(v), the golden sides and the up / left sets;
    the cases see a settled side, an unsettled one, a side with no observer and the sides merged
    again."""
    case = NET[case_name]
    n = case["n"]
    _, one = _golden_sim(gpu, case)
    sharded = [_sharded(gpu, case, _shapes(n)[shape])[1] for shape in ("g3", "empty")]
    seen = set()
    for r, (up, obs) in enumerate(_observers(case)):
        one.step()
        views = [one.view(v)[0] for v in range(n)]
        want = _summary_model(n, case["sides"][r], up, obs, one.checksums(), views)
        got = one.side_summary()
        assert _same(got, want), (case_name, r)
        for sim in sharded:
            sim.step()
            assert _same(sim.side_summary(), want), (case_name, r)
        for s in range(256):
            if want["nodes"][s]:
                seen.add("settled" if want["settled"][s] else "unsettled")
            elif s in case["sides"][r]:
                seen.add("nobody observes")
    # every side is unsettled while it still pings across the cut; the structured cases also run
    # long enough for a side to hold everyone else faulty (the random one starts with nodes down
    # and keeps changing)
    assert {"unsettled"} | ({"settled"} if case["family"] == "structured" else set()) <= seen
    if case_name == "n6-side-all-down":
        assert "nobody observes" in seen
    for sim in [one] + sharded:
        sim.close()


def test_side_summary_mid_round_on_a_sharded_handle_raises(gpu):
    case = NET["n6-two"]
    _, sim = _sharded(gpu, case, _shapes(6)["g2"])
    sim.step(7)
    sim._joins()
    for k in range(gpu.SIM_STAGES):
        for s in sim.shards:
            s.stage(k)
        if k < gpu.SIM_STAGES - 1:
            with pytest.raises(gpu.RingpopAmdError, match="round boundary"):
                sim.shards[0].side_summary()
            gpu.check(gpu.lib().rp_sim_exchange_local(sim._arr, sim.G))
    assert sim.checksums().tolist() == case["checksums"][7]
    assert sim.side_summary()["nodes"][:2].tolist() == [3, 3]
    sim.close()


# ---- (e) validation

@pytest.mark.parametrize("G", [None, 2])
def test_bad_side_events_are_refused(gpu, G):
    """An event kind past "heal" and a side past 255 are refused at creation; a join whose side has
    no live node is refused by the step that reaches it, and the handle still closes."""
    S = synth()
    n = 4
    names = [S.c2_addr(i) for i in range(n)]
    args = (names, S.c3_members(n)[2], np.zeros(n, dtype=np.uint8))
    make = (lambda **kw: gpu.ShardedGossipSim(*args, G, **kw)) if G else (lambda **kw: gpu.GossipSim(*args, **kw))
    for events in ([(0, 6, 0)], [(1, "side", 2, 256)]):
        with pytest.raises(gpu.RingpopAmdError, match="bad event"):
            make(seed=5, suspicion_rounds=3, events=events)
    make(seed=5, suspicion_rounds=3, events=[(1, "side", 2, 255), (1, "heal", 3), (2, "kill", 1, 999)]).close()
    sim = make(seed=5, suspicion_rounds=3, events=[(1, "side", 3, 1), (2, "kill", 3), (3, "join", 3)])
    sim.step(3)
    with pytest.raises(gpu.RingpopAmdError, match="join"):
        sim.step()
    sim.close()
    assert all(s._h is None for s in (sim.shards if G else [sim]))


def test_routing_share_during_a_split_sharded_equals_unsharded(gpu):
    """What the INTEGRATION example does: routingShare() and side_summary() round by round through a
    split and its heal. The sharded simulator's default truth reads events with and without an
    argument, and its figures equal the unsharded handle's."""
    case = NET["n8-join-leave-healed"]
    n = case["n"]
    names, one = _golden_sim(gpu, case)
    _, sh = _sharded(gpu, case, _shapes(n)["g3"])
    ring = gpu.HashRing()
    ring.addRemoveServers(names)
    split_wrong = 0
    for r, (_, obs) in enumerate(_observers(case)):
        one.step()
        sh.step()
        assert sh.default_truth().tolist() == obs.tolist(), r
        a, b = one.routingShare(ring), sh.routingShare(ring)
        assert all(np.array_equal(a[k], b[k]) for k in ("wrong", "lost", "pos_wrong")), r
        if any(case["sides"][r]):
            split_wrong += int(a["wrong"].sum())
    assert split_wrong > 0  # the halves did route differently while cut
    one.close()
    sh.close()
    ring.close()
