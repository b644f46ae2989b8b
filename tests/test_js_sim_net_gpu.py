"""GPU parity of the Node N-API GossipSim under network partitions: three cases of
tests/golden/sim_net_golden.json replayed from node (tests/js/sim_net_parity.js): 'side' and 'heal'
events, sides() and sideSummary()."""
import shutil

import numpy as np
import pytest

import sim_net_cases as net
from test_js_gpu import run_node
from test_sim_gpu import STAT, synth
from test_sim_net_gpu import _observers

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]

CASES = ("n6-two", "n6-side-all-down-revive", "n8-join-leave-healed")


def _cross_final(case, names, up, obs):
    """cross_pingable after the last round, from the fixture's final views (every node's: n <= 8)."""
    n = case["n"]
    assert case["views"] == list(range(n))
    side = np.array(case["sides"][-1])
    cross = [0] * 256
    for v, view in zip(case["views"], case["finalViews"]):
        if not obs[v]:
            continue
        st = {a: STAT[s] for a, s, _ in view}
        pingable = np.array([st[a] <= STAT["suspect"] for a in names])
        cross[side[v]] += int(np.count_nonzero(pingable & (~up | (side != side[v]))))
    return cross


def test_js_gossipsim_replays_partition_goldens(gpu, tmp_path):
    S = synth()
    NET = net.load()
    cases = []
    for name in CASES:
        c = NET[name]
        n = c["n"]
        names = [S.c2_addr(i) for i in range(n)]
        seen = _observers(c)
        up, obs = seen[-1]
        cases.append(dict(c, names=names, inc0=[int(x) for x in S.c3_members(n)[2]],
                          observers=[np.flatnonzero(o).tolist() for _, o in seen],
                          firstEvent=min(e[0] for e in c["events"]), crossFinal=_cross_final(c, names, up, obs)))
    res = run_node("sim_net_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == sum(3 * c["rounds"] + 1 for c in cases) + 2
