"""CPU tests: the gossip round-model oracle (oracle/orc_sim.c) reproduces, round by round,
every live node's membership checksum and maxPiggybackCount that the REFERENCE modules produced
when driven through the same round model (tests/golden/ref_sim.js), plus the full syncs they
sent and final member tables — for the kill-only cases and the scenario cases (leave, crash
mid-run, revive with refutation and full sync, ring size crossing a power of ten, fresh
processes joining from join responses), and for the tiny clusters of sim_tiny_golden.json
(2..17 nodes: no ping target, fewer than three ping-req helpers or join responders, everyone gone).
A join that no live node could answer is refused."""
import importlib.util
import os

import numpy as np
import pytest

import golden_util as gu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT = {"alive": 0, "suspect": 1, "faulty": 2, "leave": 3}
GOLDEN = {c["name"]: c for f in ("sim_golden.json", "sim_tiny_golden.json") for c in gu.load_sim(f)["cases"]}
CASES = list(GOLDEN)
STRUCTURED = [c for c in GOLDEN.values() if c.get("family") == "structured"]


def synth():
    spec = importlib.util.spec_from_file_location("rp_synth", os.path.join(REPO, "ringpop-node_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case_name", CASES)
def test_sim_oracle_matches_reference(orc, case_name, threads):
    _check_case(orc, GOLDEN[case_name], threads)


def _check_case(orc, case, threads):
    S = synth()
    n = case["n"]
    names = [S.c2_addr(i) for i in range(n)]
    inc0 = S.c3_members(n)[2]
    sim = orc.Sim(names, inc0, np.array(case["dead"], dtype=np.uint8), seed=case["seed"],
                  susp_rounds=case["suspRounds"], now0=case["now0"], events=case["events"], threads=threads)
    for r, want in enumerate(case["checksums"]):
        sim.step()
        assert sim.checksums().tolist() == want, "round %d" % r
        assert sim.piggyback().tolist() == case["maxPiggyback"][r], "round %d" % r
    assert sim.stats()["fullsyncs"] == case["fullSyncs"]
    for v, view in zip(case["views"], case["finalViews"]):
        st, inc = sim.view(v)
        got = {names[i]: (int(st[i]), int(inc[i])) for i in range(n)}
        assert got == {a: (STAT[s], i) for a, s, i in view}


def test_sim_oracle_windowed_order_matches_tiny_goldens(orc, monkeypatch):
    """The members-array window path (ORC_SIM_ORDER_BYTES=100: N^2 order entries never fit) at the
    sizes of the structured tiny families, joins from one and two responders included."""
    assert len(STRUCTURED) == 46
    monkeypatch.setenv("ORC_SIM_ORDER_BYTES", "100")
    for case in STRUCTURED:
        _check_case(orc, case, 2)


def test_tiny_fixture_reaches_every_small_cluster_branch():
    """The reference took each branch the tiny fixture exists for (counted by ref_sim.js): no ping
    target, a ping-req with 0, 1 and 2 helpers, a helper that is down, a join answered by 1 and
    by 2 nodes, a leave refused as redundant."""
    tiny = gu.load_sim("sim_tiny_golden.json")["cases"]
    assert len(tiny) == 86 and len(STRUCTURED) == 46
    keys = ["noTarget", "pingReq0", "pingReq1", "pingReq2", "helperDown", "join1", "join2", "leaveRedundant"]
    for k in keys:
        assert sum(c["branches"][k] for c in tiny) > 0, k
    assert all(2 <= c["n"] <= 17 and c["rounds"] <= 60 for c in tiny)


def test_sim_oracle_refuses_a_join_nobody_can_answer(orc):
    """The reference's join never completes without a live node to answer it; the model refuses
    the event (ref_sim.js throws, the device raises): the step that reaches it raises, whether
    the others are down from the start or were killed, and a join one node can answer passes."""
    S = synth()
    for n, dead, events in [(2, [0, 1], [(3, "kill", 0), (4, "join", 1)]),
                            (3, [1, 1, 1], [(0, "join", 2)]),
                            (4, [0, 0, 0, 0], [(1, "kill", 1), (1, "kill", 2), (1, "kill", 3), (2, "join", 0)])]:
        names = [S.c2_addr(i) for i in range(n)]
        sim = orc.Sim(names, S.c3_members(n)[2], np.array(dead, dtype=np.uint8), seed=5, susp_rounds=3, events=events)
        bad = max(e[0] for e in events)
        for _ in range(bad):
            sim.step()
        with pytest.raises(ValueError, match="join"):
            sim.step()
        assert sim.round == bad
    sim = orc.Sim(names, S.c3_members(n)[2], np.array([0, 1, 1, 1], dtype=np.uint8), seed=5, susp_rounds=3,
                  events=[(1, "join", 2)])
    for _ in range(4):
        sim.step()
    assert np.count_nonzero(sim.checksums()) == 2


def test_sim_oracle_windowed_order_matches_whole(orc, monkeypatch):
    """The members-array window (used when N^2 order entries exceed ORC_SIM_ORDER_BYTES, as at
    C5) regenerates exactly the whole-array walk, including reshuffles on wrap."""
    S = synth()
    n, k, seed = 300, 30, 2
    names = [S.c2_addr(i) for i in range(n)]
    inc0 = S.c3_members(n)[2]
    dead = S.kill_set(n, k, seed)
    ev = [(40, "revive", int(np.flatnonzero(dead)[0])), (5, "leave", 7), (60, "join", int(np.flatnonzero(dead)[1])),
          (90, "join", 7), (90, "join", 11)]
    whole = orc.Sim(names, inc0, dead, seed=seed, susp_rounds=3, events=ev)
    monkeypatch.setenv("ORC_SIM_ORDER_BYTES", "100")
    win = orc.Sim(names, inc0, dead, seed=seed, susp_rounds=3, events=ev, threads=3)
    for r in range(360):  # > N rounds: every iterator wraps and reshuffles
        whole.step()
        win.step()
        assert np.array_equal(whole.checksums(), win.checksums()), "round %d" % r
    assert whole.stats() == win.stats()
