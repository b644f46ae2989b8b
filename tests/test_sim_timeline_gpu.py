"""GPU tests of the simulator's timeline (rp_sim_timeline_enable / rp_sim_timeline_read, DESIGN
§4.4c): one record of cluster-wide aggregates per round, appended on the device. Reference:
tests/timeline_model.py fed from a twin handle stepped one round at a time (view(v),
ring_members(v), checksums(), stats(); from 129 nodes on the counts come from census(), which
test_sim_ring_gpu.py pins at 127..513 nodes against the CPU oracle's rows, where it also compares
the timeline at 129 and 513 nodes with the model fed from the oracle alone). Bit-exact throughout.

sim_tiny_golden.json has no one-node case (rp_sim_create refuses n < 2), so the smallest clusters
here are two of its two-node cases."""
import ctypes
import random

import numpy as np
import pytest

import golden_util as gu
import sim_net_cases as net
import sim_tiny_cases
import timeline_model as tm
from test_sim_gpu import _golden_sim, synth
from test_sim_tiny_gpu import _shapes

pytestmark = pytest.mark.gpu

TINY = {c["name"]: c for c in gu.load_sim("sim_tiny_golden.json")["cases"]}
NET = net.load()
GOLD = {c["name"]: c for c in gu.load("sim_golden.json")["cases"]}


def _random_case(n, rounds=40):
    rng = random.Random(3000 + n)
    dead, events = sim_tiny_cases.random_dead_events(rng, n, 0.1, 30)
    return {"name": "rand-n%d" % n, "n": n, "dead": dead, "events": events, "rounds": rounds, "seed": 3000 + n,
            "suspRounds": 3, "now0": 1434401518824 + 10 ** 9}


def _case(cid):
    if cid in TINY:
        return TINY[cid]
    if cid in NET:
        return NET[cid]
    n = int(cid.split("-")[0][1:])
    return _random_case(n, 24 if n > 500 else 40)


# case id -> RP_TIMELINE_ROWS
TWIN_CASES = {"n2-all-leave": None, "n2-killrevive": None,
              "n6-two": None, "n9-three-healed": None, "n6-side-all-down": None, "n8-join-leave-healed": None,
              "net-rand06-n15": None,
              "n33": None, "n63": None, "n64": None, "n65": None, "n129": None, "n257": None, "n513": None,
              "n65-rows1": "1", "n65-rows7": "7"}
_TWIN = {}


def _stack(sim, n, obs):
    st = np.zeros((n, n), dtype=np.uint8)
    ring = np.zeros((n, n), dtype=bool)
    for v in np.flatnonzero(obs):
        st[v] = sim.view(int(v))[0]
        ring[v] = sim.ring_members(int(v))
    return st, ring


def _model_run(sim, case, rounds, start=0):
    """The model's timeline of `rounds` rounds of a handle stepped one at a time."""
    n = case["n"]
    model = tm.Timeline(n, case["dead"], case["events"], start=start)
    for _ in range(rounds):
        sim.step()
        obs = model.observers()
        if n >= 129:
            c = sim.census(observe=obs, want=("status", "in_ring"))
            model.record(sim.checksums(), sim.stats(), counts=(c["status"], c["in_ring"]))
        else:
            st, ring = _stack(sim, n, obs)
            model.record(sim.checksums(), sim.stats(), status_rows=st, ring_rows=ring)
    return model


def _twin(gpu, cid):
    """(got, want) of a twin case, once per process: handle A records R rounds queued at once,
    handle B is stepped round by round into the model."""
    if cid not in _TWIN:
        case = _case(cid)
        rows = TWIN_CASES[cid]
        mp = pytest.MonkeyPatch()
        try:
            if rows is None:
                mp.delenv("RP_TIMELINE_ROWS", raising=False)
            else:
                mp.setenv("RP_TIMELINE_ROWS", rows)
            R = case["rounds"]
            _, a = _golden_sim(gpu, case)
            a.timeline_enable(R)
            a.step_async(R)
            got = a.timeline()
            a.close()
        finally:
            mp.undo()
        _, b = _golden_sim(gpu, case)
        want = _model_run(b, case, R).result()
        b.close()
        _TWIN[cid] = (got, want)
    return _TWIN[cid]


@pytest.mark.parametrize("cid", list(TWIN_CASES))
def test_timeline_equals_model_of_twin(gpu, cid):
    """(a) Every field of every record and first_seen."""
    got, want = _twin(gpu, cid)
    n = _case(cid)["n"]
    assert len(got["round"]) == _case(cid)["rounds"]
    assert tm.same(got, want) is None, (cid, tm.same(got, want))
    assert (got["pairs"].sum(axis=1) == got["observers"].astype(np.uint64) * np.uint64(n)).all()


def test_twin_cases_see_every_kind_of_record(gpu):
    """Across the cases of (a): unmet > 0, false_faulty > 0, a round nobody observes, a converged
    one, a ring short of members and every first_seen column."""
    seen = set()
    for cid in TWIN_CASES:
        got, _ = _twin(gpu, cid)
        n = _case(cid)["n"]
        seen |= {"unmet"} if got["unmet"].any() else set()
        seen |= {"false_faulty"} if got["false_faulty"].any() else set()
        seen |= {"nobody"} if (got["observers"] == 0).any() else set()
        seen |= {"converged"} if (got["converged"] & (got["observers"] > 0)).any() else set()
        seen |= {"ring"} if (got["in_ring"] < got["observers"].astype(np.uint64) * np.uint64(n)).any() else set()
        seen |= {"seen%d" % s for s in range(3) if (got["first_seen"][:, s] != gpu.SIM_NEVER).any()}
    assert seen == {"unmet", "false_faulty", "nobody", "converged", "ring", "seen0", "seen1", "seen2"}, seen


# ---- (b) recording does not perturb the run

PERTURB = [("tiny", "n6-killrevive"), ("tiny", "n8-same-round"), ("tiny", "n8-two-responders"),
           ("net", "n9-three-healed"), ("net", "n8-join-leave-healed"), ("net", "net-rand06-n15")] + \
          [("gold", name) for name in GOLD]


@pytest.mark.parametrize("family,name", PERTURB)
def test_recording_does_not_perturb_the_goldens(gpu, family, name):
    """With the timeline on, the golden checksums, maxPiggybackCount and full syncs round by round;
    and with all rounds queued at once, the final ones."""
    case = {"tiny": TINY, "net": NET, "gold": GOLD}[family][name]
    _, sim = _golden_sim(gpu, case)
    sim.timeline_enable(8)
    for r, want in enumerate(case["checksums"]):
        sim.step()
        assert sim.checksums().tolist() == want, (name, r)
        assert sim.piggyback().tolist() == case["maxPiggyback"][r], (name, r)
    assert sim.stats()["fullsyncs"] == case["fullSyncs"], name
    tl = sim.timeline()
    R = len(case["checksums"])
    assert tl["round"].tolist() == list(range(R - 8, R)) and int(tl["stats"][-1][2]) == case["fullSyncs"]
    sim.close()
    _, sim = _golden_sim(gpu, case)
    sim.timeline_enable(R)
    sim.step_async(R)
    assert sim.checksums().tolist() == case["checksums"][-1], name
    assert sim.piggyback().tolist() == case["maxPiggyback"][-1], name
    assert sim.stats()["fullsyncs"] == case["fullSyncs"], name
    sim.close()


def test_recorded_round_leaves_the_next_stage_0_nothing_to_hash(gpu):
    """The refresh at the end of a recorded round is the one the next round would have run: with no
    event to dirty a view in between, a run with the timeline on hashes exactly as many views as a
    run that is only stepped (its last round's views hashed by the checksums() call)."""
    S = synth()
    n, rounds = 130, 25
    names = [S.c2_addr(i) for i in range(n)]
    args = (names, S.c3_members(n)[2], S.kill_set(n, 4, 5))
    a = gpu.GossipSim(*args, seed=5, suspicion_rounds=3)
    b = gpu.GossipSim(*args, seed=5, suspicion_rounds=3)
    a.timeline_enable(rounds)
    a.step(rounds)
    b.step(rounds)
    cb = b.checksums()
    assert b.counters()["views_hashed"] > n  # the kills dirtied views
    assert a.counters() == b.counters()
    assert np.array_equal(a.checksums(), cb) and a.counters() == b.counters()  # nothing was left dirty
    a.close()
    b.close()


# ---- (c) the ring of records

def test_ring_keeps_the_last_records(gpu):
    case = _case("n33")
    _, small = _golden_sim(gpu, case)
    _, big = _golden_sim(gpu, case)
    small.timeline_enable(4)
    big.timeline_enable(16)
    small.step_async(11)
    big.step_async(11)
    a, b = small.timeline(), big.timeline()
    assert b["round"].tolist() == list(range(11)) and a["round"].tolist() == [7, 8, 9, 10]
    for k in tm.FIELDS + ("converged",):
        assert np.array_equal(a[k], b[k][7:]) and a[k].dtype == b[k].dtype, k
    assert np.array_equal(a["first_seen"], b["first_seen"]) and (b["first_seen"] != gpu.SIM_NEVER).any()
    assert (b["first_seen"][b["first_seen"] != gpu.SIM_NEVER] < 7).any()  # older than the kept records
    two = small.timeline(last=2)
    assert two["round"].tolist() == [9, 10] and tm.same(two, big.timeline(last=2)) is None
    # the C ABI: n, first_round, nullable first_seen
    recs = np.zeros(2, dtype=gpu._TL_REC)
    n, first = ctypes.c_uint32(), ctypes.c_uint64()
    gpu.check(gpu.lib().rp_sim_timeline_read(small._h, recs.ctypes.data, 2, ctypes.byref(n), ctypes.byref(first), None))
    assert (n.value, first.value) == (2, 9) and recs["round"].tolist() == [9, 10]
    assert not recs["tail"].any() and not recs["reserved"].any()
    small.close()
    big.close()


# ---- (d) enabling again, turning off, never enabled

def test_enable_again_mid_run_and_off(gpu):
    case = _case("n33")
    n = case["n"]
    _, sim = _golden_sim(gpu, case)
    _, twin = _golden_sim(gpu, case)
    sim.timeline_enable(8)
    sim.step(5)
    before = sim.timeline()
    assert before["round"].tolist() == list(range(5)) and (before["first_seen"] != gpu.SIM_NEVER).any()
    sim.timeline_enable(8)
    empty = sim.timeline()
    assert len(empty["round"]) == 0 and empty["pairs"].shape == (0, 4) and (empty["first_seen"] == gpu.SIM_NEVER).all()
    sim.step_async(3)
    twin.step(5)
    want = _model_run(twin, case, 3, start=5).result()
    got = sim.timeline()
    assert got["round"].tolist() == [5, 6, 7]
    assert tm.same(got, want) is None, tm.same(got, want)
    sim.timeline_enable(0)
    sim.step(2)
    recs = np.zeros(4, dtype=gpu._TL_REC)
    fs = np.full((n, 3), 77, dtype=np.uint32)
    cnt, first = ctypes.c_uint32(9), ctypes.c_uint64()
    for h in (sim, twin):  # turned off; never enabled
        gpu.check(gpu.lib().rp_sim_timeline_read(h._h, recs.ctypes.data, 4, ctypes.byref(cnt), ctypes.byref(first),
                                                 fs.ctypes.data))
        assert cnt.value == 0 and (fs == 77).all()
        assert len(h.timeline()["round"]) == 0
    # the run went on as the twin's
    twin.step(2)
    assert np.array_equal(sim.checksums(), twin.checksums()) and sim.stats() == twin.stats()
    sim.close()
    twin.close()


# ---- (e) sharded

def _sharded(gpu, case, bounds):
    S = synth()
    n = case["n"]
    names = [S.c2_addr(i) for i in range(n)]
    return gpu.ShardedGossipSim(names, S.c3_members(n)[2], np.array(case["dead"], dtype=np.uint8), len(bounds) - 1,
                                seed=case["seed"], suspicion_rounds=case["suspRounds"], now0=case["now0"],
                                events=case["events"], bounds=np.array(bounds, dtype=np.uint32))


SHARDED = [(cid, shape) for cid in ("n6-two", "n8-join-leave-healed", "n65") for shape in _shapes(_case(cid)["n"])]


@pytest.mark.parametrize("cid,shape", SHARDED)
def test_sharded_timeline_equals_unsharded(gpu, cid, shape):
    """2 and 3 shards, empty shards, one node a shard: the reduced timeline is the one handle's."""
    case = _case(cid)
    one, _ = _twin(gpu, cid)
    sim = _sharded(gpu, case, _shapes(case["n"])[shape])
    sim.timeline_enable(case["rounds"])
    sim.step(case["rounds"])
    got = sim.timeline()
    assert tm.same(got, one) is None, (cid, shape, tm.same(got, one))
    parts = [s.timeline() for s in sim.shards]
    assert sum(int(p["observers"].sum()) for p in parts) == int(one["observers"].sum())
    parts[0]["round"] = parts[0]["round"] + np.uint64(1)
    with pytest.raises(ValueError):
        gpu.timeline_reduce(parts)
    sim.close()


def test_timeline_mid_round_on_a_sharded_handle_raises(gpu):
    case = NET["n6-two"]
    sim = _sharded(gpu, case, _shapes(6)["g2"])
    sim.timeline_enable(16)
    sim.step(7)
    sim._joins()
    for k in range(gpu.SIM_STAGES):
        for s in sim.shards:
            s.stage(k)
        if k < gpu.SIM_STAGES - 1:
            with pytest.raises(gpu.RingpopAmdError, match="round boundary"):
                sim.shards[0].timeline()
            with pytest.raises(gpu.RingpopAmdError, match="round boundary"):
                sim.shards[1].timeline_enable(4)
            gpu.check(gpu.lib().rp_sim_exchange_local(sim._arr, sim.G))
    got = sim.timeline()  # the refused calls changed nothing
    one, _ = _twin(gpu, "n6-two")
    assert got["round"].tolist() == list(range(8))
    for k in tm.FIELDS + ("converged",):
        assert np.array_equal(got[k], one[k][:8]), k
    sim.close()


# ---- (f) rounds to convergence

@pytest.mark.parametrize("susp,rounds,converges", [(3, 40, True), (25, 10, False)])
def test_rounds_to_convergence(gpu, susp, rounds, converges):
    S = synth()
    n = 30
    names = [S.c2_addr(i) for i in range(n)]
    args = (names, S.c3_members(n)[2], S.kill_set(n, 2, 5))
    a = gpu.GossipSim(*args, seed=5, suspicion_rounds=susp)
    b = gpu.GossipSim(*args, seed=5, suspicion_rounds=susp)
    a.timeline_enable(rounds)
    a.step_async(rounds)
    first = None
    for r in range(rounds):
        b.step()
        if first is None and b.converged():
            first = r
    assert (first is not None) == converges and (first is None or first > 0)
    assert gpu.rounds_to_convergence(a.timeline()) == first
    a.close()
    b.close()
