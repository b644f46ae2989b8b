"""GPU parity of the gossip round simulator on tiny and degenerate clusters (2..17 nodes, shards
that own one node or none, everyone down or gone) against the reference goldens of
tests/golden/sim_tiny_golden.json, and at wave and workgroup boundaries (63..257 nodes) against
the CPU oracle. These sizes reach what the larger cases never do: a node with nobody to ping, a
ping-req with 0, 1 or 2 helpers, a join answered by 1 or 2 nodes, lane-pair checksum chains, the
D1 selection and the twin pass with fewer than 64 (or 0) local nodes. Bit-exact."""
import random

import numpy as np
import pytest

import golden_util as gu
import sim_tiny_cases
from test_sim_gpu import STAT, _golden_sim, synth

pytestmark = pytest.mark.gpu

TINY = {c["name"]: c for c in gu.load_sim("sim_tiny_golden.json")["cases"]}
STRUCTURED = [c for c in TINY.values() if c["family"] == "structured"]
_ORACLE = {}


def _oracle(orc, case):
    """The oracle's run of a golden case, once per process: converged() after every round and
    the final stats (the fixture holds neither)."""
    if case["name"] not in _ORACLE:
        S = synth()
        n = case["n"]
        sim = orc.Sim([S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], np.array(case["dead"], dtype=np.uint8),
                      seed=case["seed"], susp_rounds=case["suspRounds"], now0=case["now0"], events=case["events"])
        conv = []
        for want in case["checksums"]:
            sim.step()
            assert sim.checksums().tolist() == want  # (the CPU suite's check: the oracle is the golden)
            conv.append(sim.converged())
        _ORACLE[case["name"]] = {"converged": conv, "stats": sim.stats()}
    return _ORACLE[case["name"]]


def _check_all(orc, case, sim, names):
    """Checksums, maxPiggybackCount and converged() after every round; full syncs, stats and the
    recorded views at the end."""
    ora = _oracle(orc, case)
    for r, want in enumerate(case["checksums"]):
        sim.step()
        assert sim.checksums().tolist() == want, (case["name"], r)
        assert sim.piggyback().tolist() == case["maxPiggyback"][r], (case["name"], r)
        assert sim.converged() == ora["converged"][r], (case["name"], r)
    assert sim.stats()["fullsyncs"] == case["fullSyncs"], case["name"]
    assert sim.stats() == ora["stats"], case["name"]
    for v, view in zip(case["views"], case["finalViews"]):
        st, inc = sim.view(v)
        got = {names[i]: (int(st[i]), int(inc[i])) for i in range(case["n"])}
        assert got == {a: (STAT[s], i) for a, s, i in view}, (case["name"], v)
    sim.close()


@pytest.mark.parametrize("case_name", list(TINY))
def test_tiny_sim_matches_reference_goldens(gpu, orc, case_name):
    """(a) The default path on every tiny golden case."""
    case = TINY[case_name]
    names, sim = _golden_sim(gpu, case)
    _check_all(orc, case, sim, names)


KNOBS = {
    "opos0": {"RP_SIM_OPOS_BYTES": "0"},
    "xcap3": {"RP_SIM_D1_XCAP": "3"},
    "d1ck-pc": {"RP_SIM_D1_CK": "pc"},
    "d1ck-blockck": {"RP_SIM_D1_CK": "blockck"},
    "ck-pc": {"RP_SIM_CK": "pc"},
    "ck-lanes-p0": {"RP_SIM_CK": "lanes", "RP_SIM_PASS1": "0"},
    "ck-lanes-p1": {"RP_SIM_CK": "lanes", "RP_SIM_PASS1": "1"},
    "ck-pc3": {"RP_SIM_CK": "pc3"},
    "ck-pc32-p0": {"RP_SIM_CK": "pc32", "RP_SIM_PASS1": "0"},
    "ck-pc32-p1": {"RP_SIM_CK": "pc32", "RP_SIM_PASS1": "1"},
    "ck-pair": {"RP_SIM_CK": "pair"},
    "twins-verify": {"RP_SIM_TWINS": "1", "RP_SIM_TWIN_VERIFY": "1"},
    "early": {"RP_SIM_EARLY": "1"},
    "dlist1": {"RP_SIM_DLIST_BYTES": None},  # per case: 16 bytes a view = 1 piece
    "ck-lanes-sort0": {"RP_SIM_CK": "lanes", "RP_SIM_CK_SORT": "0"},
    "ck-lanes-sort1": {"RP_SIM_CK": "lanes", "RP_SIM_CK_SORT": "1"},
    "ck-pc-sortpc": {"RP_SIM_CK": "pc", "RP_SIM_CK_SORT_PC": "1"},
    "ck-pc32-twins-sortpc": {"RP_SIM_CK": "pc32", "RP_SIM_TWINS": "1", "RP_SIM_CK_SORT_PC": "1"},
    "d1-vpg16": {"RP_SIM_D1_VPG": "16"},
    "d1-blockck-flag": {"RP_SIM_D1_BLOCKCK": "1"},
}


@pytest.mark.parametrize("knob", list(KNOBS))
def test_tiny_sim_paths_match_reference_goldens(gpu, monkeypatch, knob):
    """(b) Every simulator path the larger tests name, on the structured families: the D1 scan
    and mixed selection, the three D1 checksum kernels, every refresh kernel with either pass 1,
    the twin pass with its fingerprints verified, the early refresh, and deviated-piece lists of
    one piece a view (the bitmap fallback), the refresh's list in list order, sorted by this
    round's shifts and sorted on the producer/consumer kernels, and the D1 senders' chains 16
    views a workgroup and inside D1. Checksums after every round and the full syncs.
    (A handle reads RP_SIM_D1_VPG with its other knobs. While the first simulator of a process
    fixed it for all later ones, "d1-vpg16" passed on k_ck_pair<6, 2, 8> whenever another test had
    run before it; it now runs k_ck_pair<6, 2, 16>.)"""
    for key, value in KNOBS[knob].items():
        if value is not None:
            monkeypatch.setenv(key, value)
    for case in STRUCTURED:
        if knob == "dlist1":
            monkeypatch.setenv("RP_SIM_DLIST_BYTES", str(16 * case["n"]))
        _, sim = _golden_sim(gpu, case)
        for r, want in enumerate(case["checksums"]):
            sim.step()
            assert sim.checksums().tolist() == want, (case["name"], r)
        assert sim.stats()["fullsyncs"] == case["fullSyncs"], case["name"]
        sim.close()


def _default_bounds(n, G):
    return [n * g // G for g in range(G + 1)]  # the C ABI's default partition


def _shapes(n):
    """Shard shapes for an n-node cluster: {id: bounds}."""
    a = max(1, 2 * n // 5)
    shapes = {"g2": _default_bounds(n, 2), "g3": _default_bounds(n, 3),
              "empty": [0, 0, a, a, n, n]}  # empty shards first, in the middle and last
    if n <= 8:
        shapes["g=n"] = list(range(n + 1))  # one node per shard
    if n == 2:
        shapes["g>n"] = _default_bounds(n, 3)
    if n == 3:
        shapes["g>n"] = _default_bounds(n, 8)
    return shapes


SHARDED = [(name, shape) for name, c in TINY.items() for shape in _shapes(c["n"])]


@pytest.mark.parametrize("case_name,shape", SHARDED)
def test_tiny_sharded_sim_matches_reference_goldens(gpu, orc, case_name, shape):
    """(c) Every tiny case through the sharded path: 2 and 3 shards, empty shards first, in the
    middle and last, one node per shard and more shards than nodes. With one node per shard the
    one- and two-responder families join with the joiner alone on its shard, every responder on
    another shard, and (empty shapes) a responder next to an empty shard."""
    case = TINY[case_name]
    bounds = _shapes(case["n"])[shape]
    S = synth()
    n = case["n"]
    names = [S.c2_addr(i) for i in range(n)]
    sim = gpu.ShardedGossipSim(names, S.c3_members(n)[2], np.array(case["dead"], dtype=np.uint8), len(bounds) - 1,
                               seed=case["seed"], suspicion_rounds=case["suspRounds"], now0=case["now0"],
                               events=case["events"], bounds=np.array(bounds, dtype=np.uint32))
    assert [s.NL for s in sim.shards] == [bounds[g + 1] - bounds[g] for g in range(len(bounds) - 1)]
    _check_all(orc, case, sim, names)


def test_tiny_join_shapes_are_covered():
    """The join placements (c) promises do occur in the cases above."""
    seen = set()
    for name, shape in SHARDED:
        case = TINY[name]
        if not ("one-responder" in name or "two-responders" in name):
            continue
        bounds = _shapes(case["n"])[shape]
        owner = lambda v: next(g for g in range(len(bounds) - 1) if bounds[g] <= v < bounds[g + 1])  # noqa: E731
        size = lambda g: bounds[g + 1] - bounds[g]  # noqa: E731
        up = [not d for d in case["dead"]]
        for _, kind, v in case["events"]:
            if kind == "kill":
                up[v] = False
            if kind != "join":
                continue
            resp = [u for u in range(case["n"]) if u != v and up[u]]
            assert 1 <= len(resp) <= 2
            up[v] = True
            if size(owner(v)) == 1:
                seen.add("joiner alone on its shard")
            if all(owner(u) != owner(v) for u in resp):
                seen.add("every responder on another shard")
            if any(size(g) == 0 for u in resp for g in (owner(u) - 1, owner(u) + 1) if 0 <= g < len(bounds) - 1):
                seen.add("a responder next to an empty shard")
    assert len(seen) == 3, seen


def _boundary_case(n):
    S = synth()
    rng = random.Random(2000 + n)
    dead, events = sim_tiny_cases.random_dead_events(rng, n, 0.1, 30)
    names = [S.c2_addr(i) for i in range(n)]
    return names, S.c3_members(n)[2], np.array(dead, dtype=np.uint8), events


@pytest.mark.parametrize("sharded", [False, True], ids=["one", "g3"])
@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_sim_wave_boundaries_vs_oracle(gpu, orc, n, sharded):
    """(d) Cluster sizes around one, two and four waves (and the 256-thread workgroups), with
    random kills, revives, leaves and joins in rounds 0..29, unsharded and in three shards of 1,
    n-2 and 1 nodes: checksums, piggyback counts and converged() after each of 40 rounds, then
    the stats and three views, against the oracle."""
    names, inc0, dead, events = _boundary_case(n)
    kw = dict(seed=2000 + n, suspicion_rounds=3, events=events)
    if sharded:
        g = gpu.ShardedGossipSim(names, inc0, dead, 3, bounds=np.array([0, 1, n - 1, n], dtype=np.uint32), **kw)
    else:
        g = gpu.GossipSim(names, inc0, dead, **kw)
    o = orc.Sim(names, inc0, dead, seed=2000 + n, susp_rounds=3, now0=1434401518824 + 10 ** 9, events=events)
    for r in range(40):
        g.step()
        o.step()
        assert np.array_equal(g.checksums(), o.checksums()), "round %d" % r
        assert np.array_equal(g.piggyback(), o.piggyback()), "round %d" % r
        assert g.converged() == o.converged(), "round %d" % r
    assert g.stats() == o.stats()
    for v in (0, n // 2, n - 1):
        gs, gi = g.view(v)
        os_, oi = o.view(v)
        assert np.array_equal(gs, os_) and np.array_equal(gi, oi), v
    g.close()


@pytest.mark.parametrize("G", [None, 2])
def test_join_nobody_can_answer_is_refused(gpu, G):
    """The model's rule in the reference harness, the oracle and here: a join needs a live node
    to answer it. The step that reaches such an event raises, unsharded and in two shards,
    whether the others were down from the start or killed; the handle still closes."""
    S = synth()
    for n, dead, events in [(2, [0, 1], [(3, "kill", 0), (4, "join", 1)]),
                            (3, [1, 1, 1], [(0, "join", 2)]),
                            (4, [0, 0, 0, 0], [(1, "kill", 1), (1, "kill", 2), (1, "kill", 3), (2, "join", 0)])]:
        names = [S.c2_addr(i) for i in range(n)]
        args = (names, S.c3_members(n)[2], np.array(dead, dtype=np.uint8))
        kw = dict(seed=5, suspicion_rounds=3, events=events)
        sim = gpu.ShardedGossipSim(*args, G, **kw) if G else gpu.GossipSim(*args, **kw)
        bad = max(e[0] for e in events)
        sim.step(bad)
        with pytest.raises(gpu.RingpopAmdError, match="join"):
            sim.step()
        sim.close()
        assert all(s._h is None for s in (sim.shards if G else [sim]))
