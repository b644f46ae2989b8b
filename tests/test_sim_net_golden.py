"""CPU checks of the partition goldens (tests/golden/sim_net_golden.json, the reference modules
under tests/golden/ref_sim_net.js): the harness with a network that can be cut is pinned to the
untouched harness (the control cases) and to the untouched oracle (a side of an unhealed split
lives through what a kill of everyone else would give it), and the fixture shows what the DESIGN
says about short and long partitions."""
import numpy as np
import pytest

import golden_util as gu
import sim_net_cases as net
from test_sim_gpu import synth

NET = net.load()
PARTITION = [c for c in NET.values() if c["family"] != "control"]
OPEN = [c["name"] for c in PARTITION if net.open_split(c["n"], c["events"])]


def test_fixture_holds_the_cases_of_the_generator():
    want = [(seed, fam, c[0]) for seed, fam, c in net.all_cases()]
    assert [(c["seed"], c["family"], c["name"]) for c in NET.values()] == want
    for (_, _, (name, n, dead, rounds, susp, events)), c in zip(net.all_cases(), NET.values()):
        assert (c["n"], c["dead"], c["rounds"], c["suspRounds"], c["events"]) == (n, dead, rounds, susp, events), name
        assert c["sides"] == net.sides_after(n, events, rounds), name
        if c["family"] != "control":
            assert 2 <= n <= 17 and rounds <= 70 and susp in (2, 3), name
    assert sum(c["family"] == "random" for c in NET.values()) == 20
    # the per-side check below covers structured and random cases
    assert {NET[n]["family"] for n in OPEN} == {"structured", "random"}


def test_control_cases_equal_the_tiny_goldens():
    """Without a side event the new harness is the old one: same checksums, piggyback counts,
    full syncs and views as committed in sim_tiny_golden.json."""
    tiny = {c["name"]: c for c in gu.load_sim("sim_tiny_golden.json")["cases"]}
    controls = [c for c in NET.values() if c["family"] == "control"]
    assert [c["name"] for c in controls] == list(net.CONTROLS)
    for c in controls:
        t = tiny[c["name"]]
        assert not any(e[1] in ("side", "heal") for e in c["events"])
        for key in ("n", "seed", "dead", "events", "suspRounds", "checksums", "maxPiggyback", "fullSyncs", "views",
                    "finalViews"):
            assert c[key] == t[key], (c["name"], key)
        assert c["branches"]["unreachable"] == 0
        assert {k: v for k, v in c["branches"].items() if k != "unreachable"} == t["branches"]


def test_every_partition_case_cut_something():
    assert len(PARTITION) >= 40
    for c in PARTITION:
        assert c["branches"]["unreachable"] > 0, c["name"]
        assert any(any(row) for row in c["sides"]), c["name"]


@pytest.mark.parametrize("case_name", OPEN)
def test_each_side_of_an_open_split_matches_the_oracle(orc, case_name):
    """A split that is never healed: for each side s, the untouched oracle runs the same events,
    except that at the split every node outside s is killed instead and later events on those nodes
    are dropped. The golden checksums of the nodes of s equal the oracle's, round by round."""
    c = NET[case_name]
    n = c["n"]
    S = synth()
    _, side = net.open_split(n, c["events"])
    for s in sorted(set(side)):
        sim = orc.Sim([S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], np.array(c["dead"], dtype=np.uint8),
                      seed=c["seed"], susp_rounds=c["suspRounds"], now0=c["now0"],
                      events=net.kill_equivalent(n, c["events"], s))
        mine = [v for v in range(n) if side[v] == s]
        for r, want in enumerate(c["checksums"]):
            sim.step()
            got = sim.checksums().tolist()
            assert [got[v] for v in mine] == [want[v] for v in mine], (case_name, s, r)


@pytest.mark.parametrize("n", sorted(net.LENGTH_NS))
def test_short_splits_heal_and_long_ones_do_not(n):
    """The length family. A 1-round split ends with all live checksums equal; the longest ends
    with the two sides' checksums different: once each side holds the other faulty, faulty members
    are not pingable and nothing crosses the healed cut. Between them the outcome switches once."""
    fam = [NET["n%d-len%02d" % (n, k)] for k in range(1, net.LENGTH_NS[n] + 11)]
    half = n // 2
    healed = []
    for c in fam:
        last = c["checksums"][-1]
        assert all(last) and not any(c["sides"][-1])  # everyone is up, the cut is gone
        assert len(set(last[:half])) == 1 and len(set(last[half:])) == 1, c["name"]
        healed.append(last[0] == last[-1])
    assert healed[0] and not healed[-1]
    assert healed == sorted(healed, reverse=True), healed
