"""GPU parity of the census in the Node N-API host (ringpop-node_amd/js): GossipSim.census on a
30-node scenario reproduces the Python binding's result (pinned against the numpy model in
test_sim_census_gpu.py) while the kills spread, after the revival and after the join."""
import shutil

import numpy as np
import pytest

from test_js_moved_gpu import run_node
from test_sim_census_gpu import cluster
from test_sim_route_gpu import NOW0, SUSP, scenario

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]

JS_NAME = {"status": "status", "in_ring": "inRing", "max_inc": "maxInc", "at_max": "atMax", "behind": "behind"}


def test_js_census_matches_python(gpu, tmp_path):
    n = 30
    names, inc0, dead = cluster(n)
    ev = scenario(n)
    g = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=SUSP, now0=NOW0, events=ev)
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    third[n - 1] = True
    samples = []
    deviated = 0
    for rnd in (0, 5, 13, 20):
        if rnd > g.round:
            g.step(rnd - g.round)
        sets = []
        for name, obs in (("default", None), ("third", third)):
            c = g.census(obs)
            deviated += int((c["status"][:, 0] != c["observers"]).sum())
            want = {JS_NAME[k]: c[k].reshape(-1).tolist() for k in JS_NAME}
            want["observers"] = c["observers"]
            sets.append({"name": name, "observe": None if obs is None else obs.astype(int).tolist(), "want": want})
        samples.append({"round": rnd, "sets": sets})
    g.close()
    assert deviated > 0
    res = run_node("census_parity.js", {"names": names, "inc0": [int(x) for x in inc0], "dead": dead.tolist(),
                                        "seed": 7, "suspRounds": SUSP, "now0": NOW0,
                                        "events": [list(e) for e in ev], "samples": samples}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 6 * 2 * len(samples) + 1
