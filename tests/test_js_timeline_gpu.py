"""GPU parity of the timeline in the Node N-API host (ringpop-node_amd/js): GossipSim.timeline on a
30-node scenario reproduces the Python binding's result (pinned against the numpy model in
test_sim_timeline_gpu.py), through a ring of records shorter than the run."""
import shutil

import pytest

from test_js_moved_gpu import run_node
from test_sim_census_gpu import cluster
from test_sim_route_gpu import NOW0, SUSP, scenario

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]

JS_NAME = {"round": "round", "observers": "observers", "ck_min": "ckMin", "ck_max": "ckMax", "pairs": "pairs",
           "in_ring": "inRing", "unmet": "unmet", "false_faulty": "falseFaulty", "stats": "stats",
           "converged": "converged"}


def test_js_timeline_matches_python(gpu, tmp_path):
    n, rounds, cap = 30, 22, 16
    names, inc0, dead = cluster(n)
    ev = scenario(n)
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev)
    g.timeline_enable(cap)
    g.step_async(rounds)
    tl = g.timeline()
    g.close()
    assert tl["round"].tolist() == list(range(rounds - cap, rounds))
    assert tl["unmet"].any() and (tl["first_seen"] != gpu.SIM_NEVER).any()
    want = {"firstRound": rounds - cap, "firstSeen": tl["first_seen"].reshape(-1).tolist(),
            "rounds": [{JS_NAME[k]: tl[k][i].tolist() for k in JS_NAME} for i in range(cap)]}
    res = run_node("timeline_parity.js", {"names": names, "inc0": [int(x) for x in inc0], "dead": dead.tolist(),
                                          "seed": 7, "suspRounds": SUSP, "now0": NOW0, "events": [list(e) for e in ev],
                                          "cap": cap, "rounds": rounds, "want": want}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 1 + 2 + cap * (len(JS_NAME) + 1) + 2 + 1
