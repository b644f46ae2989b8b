"""CPU tests: the oracle's ring membership bit (oracle/orc_sim.c `in_ring`, read through
Sim.ring_members) equals, for every node after every round, the servers the REFERENCE HashRing of
that node held (tests/golden/sim_ring_golden.json: every tiny and net case and the flap family of
tests/sim_ring_cases.py). The ring keeps a member that turns suspect as it was, so the bit cannot be
derived from the status; the fixture holds suspect rows outside the ring, and the counts below say
where. The GPU tests at sizes beyond the fixture (tests/test_sim_ring_gpu.py) rest on this file.

The oracle has no network to cut. A net case without a side event runs as it is; a case whose one
split is never healed runs once per side as sim_net_cases.kill_equivalent (everyone outside the side
is killed at the split instead), which pins the nodes of that side; the cases that heal or split
in more than one round (oracle_runs returns None for them) are compared with the fixture on the
device only (tests/test_sim_ring_gpu.py, where the invariants are checked for them too)."""
import numpy as np
import pytest

import golden_util as gu
import sim_net_cases as net
import sim_ring_cases as ringc
from test_oracle_sim import synth

RING = gu.load_sim_ring()
SUSPECT_OUT = {"rand10-n12": 8, "rand13-n7": 6, "rand24-n17": 2, "rand31-n15": 5}  # measured on the oracle


def oracle_runs(case):
    """[(events, nodes)]: the oracle runs that together pin every node of the case, or None when
    the oracle cannot live through the case's events (a healed or repeated split)."""
    n, events = case["n"], case["events"]
    if not any(e[1] in ("side", "heal") for e in events):
        return [(events, list(range(n)))]
    if not net.open_split(n, events):
        return None
    side = net.open_split(n, events)[1]
    return [(net.kill_equivalent(n, events, s), [v for v in range(n) if side[v] == s]) for s in sorted(set(side))]


ORACLE_CASES = [name for name, c in RING.items() if oracle_runs(c)]
_RUN = {}


def oracle_rows(orc, case, threads=1):
    """(status, ring) = uint8[rounds][n][n] of the oracle, every node taken from the run that pins
    it; the checksums and piggyback counts of those nodes equal the fixture's round by round, which
    pins the status rows. Once per process and thread count; callers do not modify it."""
    key = (case["name"], threads)
    if key not in _RUN:
        S = synth()
        n = case["n"]
        st = np.zeros((case["rounds"], n, n), dtype=np.uint8)
        ring = np.zeros_like(st)
        for events, nodes in oracle_runs(case):
            sim = orc.Sim([S.c2_addr(i) for i in range(n)], S.c3_members(n)[2], np.array(case["dead"], dtype=np.uint8),
                          seed=case["seed"], susp_rounds=case["suspRounds"], now0=case["now0"], events=events,
                          threads=threads)
            for r in range(case["rounds"]):
                sim.step()
                ck, pb = sim.checksums().tolist(), sim.piggyback().tolist()
                assert [ck[v] for v in nodes] == [case["checksums"][r][v] for v in nodes], (case["name"], r)
                assert [pb[v] for v in nodes] == [case["maxPiggyback"][r][v] for v in nodes], (case["name"], r)
                for v in nodes:
                    st[r, v] = sim.view(v)[0]
                    ring[r, v] = sim.ring_members(v)
        _RUN[key] = (st, ring)
    return _RUN[key]


def test_ring_fixture_holds_the_cases_of_the_generators():
    """Every tiny case, every net case (the two controls are tiny cases) and the flap family, with
    the flap inputs as tests/sim_ring_cases.py gives them; what the oracle cannot run is exactly the
    net cases that heal or split in more than one round."""
    tiny = [c["name"] for c in gu.load_sim("sim_tiny_golden.json")["cases"]]
    nets = [name for name, c in net.load().items() if c["family"] != "control"]
    flap = ringc.flap_cases()
    assert list(RING) == tiny + nets + [c[0] for c in flap]
    assert len(tiny) == 86 and len(nets) == 59
    assert [c[0] for c in flap] == ["flap-n9", "flap-n17", "flap-n33", "flap-n65"]
    S = synth()
    for name, n, dead, rounds, susp, events in flap:
        c = RING[name]
        assert (c["n"], c["dead"], c["rounds"], c["suspRounds"], c["events"]) == (n, dead, rounds, susp, events), name
        assert (c["seed"], c["now0"], c["source"]) == (ringc.SEED, S.NOW0, "flap"), name
    for name, c in RING.items():
        assert c["rings"].shape == (c["rounds"], c["n"], c["n"]), name
        cut = {e[0] for e in c["events"] if e[1] == "side"}
        assert (name in ORACLE_CASES) == (not any(e[1] == "heal" for e in c["events"]) and len(cut) <= 1), name
    assert len(ORACLE_CASES) == 108  # 86 tiny, 4 flap and the 18 net cases whose split stays open


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case_name", ORACLE_CASES)
def test_sim_oracle_ring_members_match_reference(orc, case_name, threads):
    """ring_members(v) of every node after every round equals the reference ring's servers."""
    case = RING[case_name]
    _, ring = oracle_rows(orc, case, threads)
    for r in range(case["rounds"]):
        assert np.array_equal(ring[r], case["rings"][r]), (case_name, "round %d" % r)


def suspect_out(orc, case):
    """How many (round, view, member) rows are suspect (the oracle's status, pinned by the
    checksums) and outside the reference's ring."""
    st, _ = oracle_rows(orc, case)
    return int(np.count_nonzero((st == 1) & (case["rings"] == 0)))


def test_fixture_holds_suspect_rows_outside_the_ring(orc):
    """The class that separates a kept ring bit from one derived from the status: every flap case
    has it, and the four tiny cases hold it as often as measured on the oracle; no other tiny case
    does."""
    got = {name: suspect_out(orc, RING[name]) for name in ORACLE_CASES}
    for name in got:
        if name.startswith("flap-"):
            assert got[name] >= 1, name
    tiny = {name: k for name, k in got.items() if RING[name]["source"] == "tiny" and k}
    assert tiny == SUSPECT_OUT


def test_alive_is_in_the_ring_and_faulty_or_leave_is_out(orc):
    """No fixture row is alive and outside the ring, or faulty / leave and inside it."""
    for name in ORACLE_CASES:
        st, _ = oracle_rows(orc, RING[name])
        rings = RING[name]["rings"]
        assert not np.any((st == 0) & (rings == 0)), name
        assert not np.any((st >= 2) & (rings == 1)), name
