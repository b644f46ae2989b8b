"""GPU tests of GossipSim.ring_checksums (rp_sim_ring_checksums): every node's ring checksum
against tests/proxy_model.py over ring rows that do not come from the device: the reference
modules' own rings (tests/golden/sim_ring_golden.json) and, beyond the fixture, the CPU oracle's.

(a) every fixture case, after every round, every node (those that are down too), with the twin
    classes on and off
(b) the sharded shapes of tests/test_sim_ring_gpu.py on its cases with suspect rows outside the ring
(c) one string a batch (RP_SIM_RCK_BYTES below one slot), twins on and off
(d) 63, 64, 65, 129 and 513 nodes of the flap scenario: around one and two bitmap words, a last
    word that is partly filled, more bitmap words than one (17 at 513); the strings' 16-byte
    boundaries move with every absent member
Exact comparisons throughout."""
import numpy as np
import pytest

import golden_util as gu
import proxy_model as pm
from test_sim_gpu import _golden_sim
from test_sim_ring_gpu import FLAPS, SUSPECT_OUT, _sharded, checkpoints, cluster, oracle_run
from test_sim_tiny_gpu import _shapes
import sim_ring_cases as ringc

pytestmark = pytest.mark.gpu

RING = gu.load_sim_ring()
_MODEL = {}


def model(case_name):
    """Per round the model's ring checksum of every node, from the fixture alone; once a case."""
    if case_name not in _MODEL:
        case = RING[case_name]
        names = _names(case["n"])
        cache = {}
        _MODEL[case_name] = [pm.ring_checksums(names, case["rings"][r], cache) for r in range(case["rounds"])]
    return _MODEL[case_name]


def _names(n):
    return cluster(n)[0]


def both_twins(sim, monkeypatch):
    """ring_checksums() with the twin classes on (the default) and off."""
    monkeypatch.delenv("RP_SIM_RCK_TWINS", raising=False)
    on = sim.ring_checksums()
    monkeypatch.setenv("RP_SIM_RCK_TWINS", "0")
    off = sim.ring_checksums()
    monkeypatch.setenv("RP_SIM_RCK_TWINS", "1")
    on1 = sim.ring_checksums()
    monkeypatch.delenv("RP_SIM_RCK_TWINS", raising=False)
    assert np.array_equal(on, on1)
    return on, off


# ---- (a) the fixture's cases

def test_fixture_holds_empty_rings_and_split_rounds():
    """From the fixture alone: an empty ring (a node that left and holds everyone else faulty)
    and rounds whose nodes fall into more than one ring-checksum class, some into many."""
    empty = split = most = rounds = 0
    first_empty = None
    for name in RING:
        case = RING[name]
        for r, want in enumerate(model(name)):
            rounds += 1
            e = int(np.count_nonzero(~np.asarray(case["rings"][r]).astype(bool).any(axis=1)))
            if e and first_empty is None:
                first_empty = name
            empty += e
            classes = len(set(want.tolist()))
            split += classes > 1
            most = max(most, classes)
    assert len(RING) == 149 and rounds == 6374
    assert (empty, split, most, first_empty) == (68, 4161, 37, "rand07-n2")


@pytest.mark.parametrize("case_name", list(RING))
def test_ring_checksums_match_model_on_reference_rings(gpu, monkeypatch, case_name):
    """One handle: after every round the membership checksums equal the reference's (they pin the
    rows) and every node's ring checksum, with twins on and off, equals the model over the
    reference's ring rows; down nodes included; an empty ring gives hash32("")."""
    case = RING[case_name]
    want = model(case_name)
    _, sim = _golden_sim(gpu, case)
    for r in range(case["rounds"]):
        sim.step()
        assert sim.checksums().tolist() == case["checksums"][r], (case_name, r)
        on, off = both_twins(sim, monkeypatch)
        assert on.dtype == np.uint32 and np.array_equal(on, want[r]), (case_name, r, "twins on")
        assert np.array_equal(off, want[r]), (case_name, r, "twins off")
        nobody = ~np.asarray(case["rings"][r]).astype(bool).any(axis=1)
        assert np.all(on[nobody] == pm.EMPTY_RING), (case_name, r)
    sim.close()


def test_ring_checksum_is_not_the_membership_checksum():
    """From the fixture alone: rand10-n12 holds suspect rows, so in some round its up nodes hold more
    membership checksums than ring checksums (the device's values are pinned to both above)."""
    case = RING["rand10-n12"]
    seen = False
    for r, rck in enumerate(model("rand10-n12")):
        ck = np.array(case["checksums"][r], dtype=np.uint32)
        up = ck != 0
        seen |= len(set(ck[up].tolist())) > len(set(rck[up].tolist()))
    assert seen


# ---- (b) sharded

SHARDED = [(name, shape) for name in SUSPECT_OUT + FLAPS for shape in _shapes(RING[name]["n"])
           if shape in ("g2", "g3", "empty", "g=n")]


@pytest.mark.parametrize("case_name,shape", SHARDED)
def test_sharded_ring_checksums_match_model(gpu, monkeypatch, case_name, shape):
    """2 and 3 shards, empty shards and one node a shard, gathered in id order."""
    case = RING[case_name]
    want = model(case_name)
    sim = _sharded(gpu, case, _shapes(case["n"])[shape])
    for r in range(case["rounds"]):
        sim.step()
        on, off = both_twins(sim, monkeypatch)
        assert np.array_equal(on, want[r]) and np.array_equal(off, want[r]), (case_name, shape, r)
    sim.close()


def test_sharded_handle_answers_only_at_a_round_boundary(gpu):
    case = RING["flap-n17"]
    sim = _sharded(gpu, case, _shapes(case["n"])["g2"])
    sim.step()
    for s in sim.shards:
        s.stage(0)
    with pytest.raises(gpu.RingpopAmdError):
        sim.shards[0].ring_checksums()
    sim.close()


# ---- (c) one string a batch

@pytest.mark.parametrize("twins", ["0", "1"])
def test_one_string_a_batch(gpu, monkeypatch, twins):
    monkeypatch.setenv("RP_SIM_RCK_BYTES", "1")
    monkeypatch.setenv("RP_SIM_RCK_TWINS", twins)
    for name in SUSPECT_OUT + ["flap-n17", "rand07-n2"]:
        case = RING[name]
        want = model(name)
        _, sim = _golden_sim(gpu, case)
        for r in range(case["rounds"]):
            sim.step()
            assert np.array_equal(sim.ring_checksums(), want[r]), (name, twins, r)
        sim.close()


# ---- (d) beyond the fixture: the flap scenario against the oracle's ring rows

@pytest.mark.parametrize("n", [63, 64, 65, 129, 513])
def test_ring_checksums_vs_oracle_rows_at_boundaries(gpu, orc, monkeypatch, n):
    """At each checkpoint of tests/test_sim_ring_gpu.py's flap run: the model over the ORACLE's ring
    rows, twins on and off; 65 and 513 also with one string a batch and in three shards of 1, n - 2
    and 1 nodes. The run splits the nodes into more than one class at some checkpoint."""
    run = oracle_run(orc, n)
    names, inc0, dead, now0 = cluster(n)
    kw = dict(seed=ringc.SEED, suspicion_rounds=ringc.SUSP, now0=now0, events=run["events"])
    g = gpu.GossipSim(names, inc0, dead, **kw)
    sh = None
    if n in (65, 513):
        sh = gpu.ShardedGossipSim(names, inc0, dead, 3, bounds=np.array([0, 1, n - 1, n], dtype=np.uint32), **kw)
    cache = {}
    most = 0
    for r in checkpoints(n):
        g.step(r + 1 - g.round)
        assert np.array_equal(g.checksums(), run["ck"][r]), r
        want = pm.ring_checksums(names, run["ring"][r], cache)
        most = max(most, len(set(want.tolist())))
        on, off = both_twins(g, monkeypatch)
        assert np.array_equal(on, want) and np.array_equal(off, want), (n, r)
        if sh is not None:
            sh.step(r + 1 - sh.round)
            assert np.array_equal(sh.ring_checksums(), want), (n, r, "three shards")
            monkeypatch.setenv("RP_SIM_RCK_BYTES", "1")
            assert np.array_equal(g.ring_checksums(), want), (n, r, "one string a batch")
            monkeypatch.delenv("RP_SIM_RCK_BYTES", raising=False)
    g.close()
    if sh is not None:
        sh.close()
    assert most > 1


# ---- (e) more bitmap words than the build covers in one pass

def test_ring_checksums_past_one_build_chunk(gpu, monkeypatch):
    """8,300 nodes: 260 bitmap words, four past the 256 the build workgroup covers a pass, so the
    bytes deleted in the first pass shift the second. The killed nodes sit at address ranks 5, 8190,
    8191, 8192, 8193 and 8299 (both sides of the pass boundary and the last rank); suspicion lasts
    two rounds, and the check is made after each of rounds 3..12, while some views have dropped them
    and others have not (a view drops a member when its own timer fires, and the suspicions reach
    the views in different rounds), and after round 30, when all have. Reference: the model over the ring rows of 48 nodes read back with
    ring_members (a bit the tests of tests/test_sim_ring_gpu.py pin), among them every node whose
    description differs from node 0's as far as the sample reaches; all nodes must agree between
    twins on and off, and with one string a batch."""
    n = 8300
    names, inc0, dead, now0 = cluster(n)
    by_rank = sorted(range(n), key=lambda a: names[a])
    killed = [by_rank[k] for k in (5, 8190, 8191, 8192, 8193, 8299)]
    sim = gpu.GossipSim(names, inc0, dead, seed=ringc.SEED, suspicion_rounds=2, now0=now0,
                        events=[(1, "kill", v) for v in killed])
    cache = {}
    classes = []
    split = False
    for rounds in list(range(3, 13)) + [30]:
        sim.step(rounds - sim.round)
        on, off = both_twins(sim, monkeypatch)
        assert np.array_equal(on, off), rounds
        odd = np.flatnonzero(on != on[0])[:24].tolist()
        sample = sorted(set(odd + killed + list(range(0, n, n // 16))))[:48]
        rows = np.stack([sim.ring_members(v) for v in sample])
        assert np.array_equal(on[sample], pm.ring_checksums(names, rows, cache)), rounds
        classes.append(len(set(on.tolist())))
        if classes[-1] > 1 and not split:
            split = True
            monkeypatch.setenv("RP_SIM_RCK_BYTES", "1")
            monkeypatch.setenv("RP_SIM_RCK_TWINS", "1")
            assert np.array_equal(sim.ring_checksums(), on)
            monkeypatch.delenv("RP_SIM_RCK_BYTES", raising=False)
            monkeypatch.delenv("RP_SIM_RCK_TWINS", raising=False)
    up = np.ones(n, dtype=bool)
    up[killed] = False
    assert split and len(set(on[up].tolist())) == 1  # mid-churn, then one ring among the nodes that are up
    gone = sim.ring_members(int(np.flatnonzero(up)[0]))
    assert not gone[killed].any() and gone.sum() == n - len(killed)
    sim.close()
