"""GPU tests of the simulator's ring membership bit (IN_RING of a status byte, read through
ring_members(v)) and of what is computed from it, against references that do not come from the
device: the reference modules' own rings (tests/golden/sim_ring_golden.json) at 2..65 nodes, and
beyond the fixture the CPU oracle, whose bit tests/test_oracle_sim_ring.py pins to that fixture.

The ring keeps a member that turns suspect as it was (createUpdatedHandlerForRing), so the bit is
history and not a function of the status. The fixture's flap family and four of its random cases,
and the flap scenario at every size below, hold suspect rows outside the ring; a bit derived from
the status fails on them.

(a) every fixture case on one handle; the cases with such rows and the join families through the
    sharded path (the join import); the same cases under every simulator knob
(b) 63..513 nodes (wave, bitmap-word and census-tile boundaries): views, ring rows and the census
    against the oracle's stacked rows
(c) the timeline at 129 and 513 nodes against the model fed from the oracle alone
(d) routing and routing share with allowed[v] = the reference's ring row
Exact comparisons throughout."""
import numpy as np
import pytest

import census_model as cm
import golden_util as gu
import route_share_model as sm
import routing_model as rm
import sim_ring_cases as ringc
import timeline_model as tm
from test_oracle_sim_ring import ORACLE_CASES, oracle_rows
from test_ring_moved_gpu import _keys
from test_ring_route_gpu import _hashes
from test_sim_gpu import _golden_sim, synth
from test_sim_net_gpu import _observers
from test_sim_tiny_gpu import KNOBS, _shapes

pytestmark = pytest.mark.gpu

RING = gu.load_sim_ring()
SUSPECT_OUT = ["rand10-n12", "rand13-n7", "rand24-n17", "rand31-n15"]  # tiny cases with a suspect row outside the ring
FLAPS = [name for name in RING if name.startswith("flap-")]
ALIVE, SUSPECT, FAULTY, LEAVE = range(4)


def ring_rows(sim, n):
    return np.stack([sim.ring_members(v) for v in range(n)]).astype(np.uint8)


def status_rows(sim, n):
    return np.stack([sim.view(v)[0] for v in range(n)])


# ---- (a) the fixture's cases

@pytest.mark.parametrize("case_name", list(RING))
def test_ring_members_match_reference(gpu, case_name):
    """One handle: after every round the checksums (they pin the status rows) and every node's ring
    row equal the reference's; no row is alive and outside the ring, or faulty / leave and in it."""
    case = RING[case_name]
    n = case["n"]
    _, sim = _golden_sim(gpu, case)
    for r in range(case["rounds"]):
        sim.step()
        assert sim.checksums().tolist() == case["checksums"][r], (case_name, r)
        want = case["rings"][r]
        assert np.array_equal(ring_rows(sim, n), want), (case_name, r)
        st = status_rows(sim, n)
        assert not np.any((st == ALIVE) & (want == 0)) and not np.any((st >= FAULTY) & (want == 1)), (case_name, r)
    sim.close()


JOIN_FAMILIES = [name for name in RING if RING[name]["source"] == "tiny" and
                 any(f in name for f in ("-one-responder", "-two-responders", "-same-round"))]
SHARDED = [(name, shape) for name in SUSPECT_OUT + FLAPS + JOIN_FAMILIES for shape in _shapes(RING[name]["n"])
           if shape in ("g2", "g3", "empty", "g=n")]


def _sharded(gpu, case, bounds):
    S = synth()
    n = case["n"]
    names = [S.c2_addr(i) for i in range(n)]
    return gpu.ShardedGossipSim(names, S.c3_members(n)[2], np.array(case["dead"], dtype=np.uint8), len(bounds) - 1,
                                seed=case["seed"], suspicion_rounds=case["suspRounds"], now0=case["now0"],
                                events=case["events"], bounds=np.array(bounds, dtype=np.uint32))


@pytest.mark.parametrize("case_name,shape", SHARDED)
def test_sharded_ring_members_match_reference(gpu, case_name, shape):
    """2 and 3 shards, empty shards and one node a shard: the join import across shards and a
    joiner alone on its shard keep the reference's ring rows."""
    case = RING[case_name]
    n = case["n"]
    sim = _sharded(gpu, case, _shapes(n)[shape])
    for r in range(case["rounds"]):
        sim.step()
        assert sim.checksums().tolist() == case["checksums"][r], (case_name, shape, r)
        assert np.array_equal(ring_rows(sim, n), case["rings"][r]), (case_name, shape, r)
    sim.close()


def test_sharded_cases_hold_the_join_shapes():
    assert len(JOIN_FAMILIES) == 14 and len(FLAPS) == 4
    assert any(shape == "g=n" and "responder" in name for name, shape in SHARDED)
    assert sum(shape == "empty" for _, shape in SHARDED) == len(SUSPECT_OUT + FLAPS + JOIN_FAMILIES)


@pytest.mark.parametrize("knob", list(KNOBS))
def test_ring_members_under_every_simulator_path(gpu, monkeypatch, knob):
    """Every path tests/test_sim_tiny_gpu.py names, on the cases with suspect rows outside the ring:
    the ring rows after every round."""
    for key, value in KNOBS[knob].items():
        if value is not None:
            monkeypatch.setenv(key, value)
    for name in SUSPECT_OUT + ["flap-n17"]:
        case = RING[name]
        n, R = case["n"], case["rounds"]
        if knob == "dlist1":
            monkeypatch.setenv("RP_SIM_DLIST_BYTES", str(16 * n))
        _, sim = _golden_sim(gpu, case)
        for r in range(R):  # (the rows a derived bit gets wrong last a suspicion period: every round, not three)
            sim.step()
            assert sim.checksums().tolist() == case["checksums"][r], (name, knob, r)
            assert np.array_equal(ring_rows(sim, n), case["rings"][r]), (name, knob, r)
        sim.close()


# ---- (b), (c) beyond the fixture: the flap scenario against the oracle

BOUNDARY_NS = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
_ORACLE = {}


def rounds_of(n):
    return 24 if n > 500 else 30


def checkpoints(n):
    """Round indices after which (b) compares: past the first kill, past the revival, past the
    second kill and its suspicions, and the last round."""
    return sorted({2, 15, 18, 20, 23, rounds_of(n) - 1})


def cluster(n):
    S = synth()
    return [S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], np.zeros(n, dtype=np.uint8), S.NOW0


def oracle_run(orc, n):
    """The oracle's run of the flap scenario with every eighth node flapping, once per process: the
    events, and per round the checksums, stats, status rows and ring rows (incarnation rows at the
    checkpoints). The second kill comes at the first of rounds 17..19 for which the ORACLE's run holds
    a suspect row outside the ring."""
    if n not in _ORACLE:
        names, inc0, dead, now0 = cluster(n)
        R = rounds_of(n)
        for kill2 in (17, 18, 19):
            events = ringc.flap_events(ringc.every_eighth(n), kill2)
            o = orc.Sim(names, inc0, dead, seed=ringc.SEED, susp_rounds=ringc.SUSP, now0=now0, events=events, threads=4)
            run = {"events": events, "ck": [], "stats": [], "st": np.zeros((R, n, n), dtype=np.uint8),
                   "ring": np.zeros((R, n, n), dtype=np.uint8), "inc": {}}
            for r in range(R):
                o.step()
                run["ck"].append(o.checksums())
                run["stats"].append(o.stats())
                views = [o.view(v) for v in range(n)]
                run["st"][r] = [st for st, _ in views]
                run["ring"][r] = [o.ring_members(v) for v in range(n)]
                if r in checkpoints(n):
                    run["inc"][r] = np.stack([inc for _, inc in views])
            run["suspect_out"] = int(np.count_nonzero((run["st"] == SUSPECT) & (run["ring"] == 0)))
            if run["suspect_out"]:
                break
        _ORACLE[n] = run
    return _ORACLE[n]


def up_after_round(n, events, r):
    up = np.ones(n, dtype=bool)
    for er, kind, v in events:
        if er <= r:
            up[v] = kind != "kill"
    return up


def check_census(got, want, what):
    bad = cm.same(got, want)
    assert bad is None, (what, bad)


@pytest.mark.parametrize("n", BOUNDARY_NS)
def test_views_rings_and_census_vs_oracle_at_boundaries(gpu, orc, monkeypatch, n):
    """Around one, two and four waves, a bitmap word and the census' column tile of 512 ranks (512:
    exactly one tile, 513: a second tile of one rank). At each checkpoint every node's view and ring
    row equal the oracle's, and census() over the nodes that are up, over every third node plus node
    1 (down at every checkpoint but 15) and against a reference one past its own maximum equal the
    model over the ORACLE's stacked rows. 65 and 513 repeat the census after round 20 in slabs of 1 and 7 rows; 65
    and 257 also run in three shards of 1, n-2 and 1 nodes."""
    run = oracle_run(orc, n)
    assert run["suspect_out"] > 0  # the oracle alone: the run holds a suspect row outside the ring
    assert np.any((run["st"][20] == SUSPECT) & (run["ring"][20] == 0))  # and so does the checkpoint after round 20
    names, inc0, dead, now0 = cluster(n)
    kw = dict(seed=ringc.SEED, suspicion_rounds=ringc.SUSP, now0=now0, events=run["events"])
    monkeypatch.delenv("RP_CENSUS_ROWS", raising=False)
    g = gpu.GossipSim(names, inc0, dead, **kw)
    sh = None
    if n in (65, 257):
        sh = gpu.ShardedGossipSim(names, inc0, dead, 3, bounds=np.array([0, 1, n - 1, n], dtype=np.uint32), **kw)
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    third[1] = True
    for r in checkpoints(n):
        g.step(r + 1 - g.round)
        assert np.array_equal(g.checksums(), run["ck"][r]), r
        st, inc, ring = run["st"][r], run["inc"][r], run["ring"][r]
        for v in range(n):
            gs, gi = g.view(v)
            assert np.array_equal(gs, st[v]) and np.array_equal(gi, inc[v]), (r, v)
        got_ring = ring_rows(g, n)
        assert np.array_equal(got_ring, ring), r
        up = up_after_round(n, run["events"], r)
        assert not up[1] or r == 15
        own = cm.census(st, inc, ring, up)
        wants = [("default", {}, own), ("third", {"observe": third}, cm.census(st, inc, ring, third)),
                 ("ahead", {"max_ref": own["max_inc"] + 1}, cm.census(st, inc, ring, up, ref=own["max_inc"] + 1))]
        for rows in (None, "1", "7") if r == 20 and n in (65, 513) else (None,):
            if rows is not None:
                monkeypatch.setenv("RP_CENSUS_ROWS", rows)
            for what, args, want in wants:
                check_census(g.census(**args), want, (r, what, rows))
            monkeypatch.delenv("RP_CENSUS_ROWS", raising=False)
        if sh is not None:
            sh.step(r + 1 - sh.round)
            check_census(sh.census(), own, (r, "three shards"))
            assert np.array_equal(ring_rows(sh, n), got_ring), (r, "three shards")
    g.close()
    if sh is not None:
        sh.close()


@pytest.mark.parametrize("n", [129, 513])
def test_timeline_vs_model_fed_from_the_oracle(gpu, orc, n):
    """All rounds queued at once and recorded on the device; the model is fed the oracle's
    checksums, stats, status rows and ring rows, so neither the census nor the device's rows are
    their own reference. Every field and first_seen."""
    run = oracle_run(orc, n)
    names, inc0, dead, now0 = cluster(n)
    R = rounds_of(n)
    g = gpu.GossipSim(names, inc0, dead, seed=ringc.SEED, suspicion_rounds=ringc.SUSP, now0=now0, events=run["events"])
    g.timeline_enable(R)
    g.step_async(R)
    got = g.timeline()
    g.close()
    model = tm.Timeline(n, dead, run["events"])
    for r in range(R):
        model.record(run["ck"][r], run["stats"][r], status_rows=run["st"][r], ring_rows=run["ring"][r])
    want = model.result()
    assert len(got["round"]) == R
    assert tm.same(got, want) is None, tm.same(got, want)
    # (the oracle's records count suspect rows outside the ring)
    assert (want["in_ring"] < want["pairs"][:, ALIVE] + want["pairs"][:, SUSPECT]).any()


# ---- (d) routing on the reference's ring bits

# (rand19-n2 and rand22-n3 are here for the view that allows nobody: a node that left and holds every
# other member faulty or gone; none of the other cases has one)
ROUTE_CASES = (["n2-all-leave", "n3-all-killed-midrun", "n4-onlyone", "rand19-n2", "rand22-n3"] + SUSPECT_OUT +
               ["flap-n33"])
NKEYS = 512


def route_inputs(orc, case):
    """Per round (allowed [n, n] = the reference's ring rows, truth [n] = up by the events and own
    status != leave in the oracle's view, status rows of the oracle): nothing from the device."""
    st, _ = oracle_rows(orc, case)
    n = case["n"]
    out = []
    for r, (up, _) in enumerate(_observers(case)):
        own = st[r][np.arange(n), np.arange(n)]
        out.append((case["rings"][r] != 0, up & (own != LEAVE), st[r]))
    return out


def test_route_cases_reach_the_edges(orc):
    """From the model inputs alone: a truth that allows nobody, a view that allows nobody, a view
    that differs from status <= suspect, and a two-node ring."""
    assert set(ROUTE_CASES) <= set(ORACLE_CASES)
    seen = set()
    for name in ROUTE_CASES:
        for allowed, truth, st in route_inputs(orc, RING[name]):
            seen |= {"no truth"} if not truth.any() else set()
            seen |= {"empty view"} if (~allowed.any(axis=1)).any() else set()
            seen |= {"not the status"} if (allowed != (st <= SUSPECT)).any() else set()
            seen |= {"two nodes"} if RING[name]["n"] == 2 else set()
    assert seen == {"no truth", "empty view", "not the status", "two nodes"}, seen


def _by_id(rows, col, ids):
    out = np.zeros(rows.shape[:-1] + (ids,), dtype=bool)
    out[..., col] = rows
    return out


@pytest.mark.parametrize("case_name", ROUTE_CASES)
def test_routing_on_the_reference_ring_rows(gpu, orc, case_name):
    """After every round: routing() over 512 keys, the caller-hash form over the ring's six edge
    hashes and those keys' hashes, and routingShare(), with the default truth, against the models
    over the reference's ring rows. flap-n33 also in two shards with the truth given."""
    case = RING[case_name]
    n = case["n"]
    names, g = _golden_sim(gpu, case)
    sh = _sharded(gpu, case, _shapes(n)["g2"]) if case_name == "flap-n33" else None
    ring = gpu.HashRing()
    ring.addRemoveServers(names, None)
    assert ring.size == n * 100  # no token collision: the model is `lookup` on each node's ring
    col = np.array([ring.server_id(s) for s in names], dtype=np.int64)
    tok, own = ring.dump()
    ids = ring.id_bound()
    keys = np.array(_keys(NKEYS))
    hs = _hashes(NKEYS)
    eh = np.concatenate([rm.edge_hashes(tok), hs])
    L = gpu.lib()
    for r, (allowed, truth, _) in enumerate(route_inputs(orc, case)):
        g.step()
        assert g.checksums().tolist() == case["checksums"][r], (case_name, r)
        al, tr = _by_id(allowed, col, ids), _by_id(truth, col, ids)
        want = rm.route(tok, own, hs, al, tr, truth)
        got = g.routing(ring, keys)
        for k in ("wrong", "lost", "key_wrong", "truth_owner"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (case_name, r, k)
        want_e = rm.route(tok, own, eh, al, tr, truth)
        out = {"wrong": np.zeros(n, dtype=np.uint64), "lost": np.zeros(n, dtype=np.uint64),
               "key_wrong": np.zeros(len(eh), dtype=np.uint32), "truth_owner": np.zeros(len(eh), dtype=np.uint32)}
        gpu.check(L.rp_sim_routing_hashes(g._h, ring._h, eh.ctypes.data, len(eh), None,
                                          *(out[k].ctypes.data for k in out)))
        for k in out:
            assert np.array_equal(out[k], want_e[k]), (case_name, r, k, "hashes")
        want_s = sm.share(tok, own, al, tr, truth)
        got_s = g.routingShare(ring)
        for k in ("wrong", "lost", "pos_wrong"):
            assert got_s[k].dtype == want_s[k].dtype and np.array_equal(got_s[k], want_s[k]), (case_name, r, k)
        if sh is not None:
            sh.step()
            sg, ss = sh.routing(ring, keys, truth=truth), sh.routingShare(ring, truth=truth)
            for k in ("wrong", "lost", "key_wrong", "truth_owner"):
                assert np.array_equal(sg[k], want[k]), (case_name, r, k, "two shards")
            for k in ("wrong", "lost", "pos_wrong"):
                assert np.array_equal(ss[k], want_s[k]), (case_name, r, k, "two shards")
    g.close()
    if sh is not None:
        sh.close()
    ring.close()
