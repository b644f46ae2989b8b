"""GPU parity of routeShare in the Node N-API host (ringpop-node_amd/js): ring.routeShare on a
20-server ring reproduces the Python binding's result for the same views and truth (pinned against
the numpy model in test_ring_route_share_gpu.py)."""
import shutil

import numpy as np
import pytest

from test_js_moved_gpu import run_node

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]


def test_js_route_share_matches_python(gpu, orc, tmp_path):
    servers = [orc.c2_addr(i) for i in range(20)]
    rng = np.random.default_rng(3)
    views = [[s for s in servers if rng.random() < 0.8] for _ in range(2)]
    views += [[], servers[9:10], servers + ["10.9.9.9:1"]]
    truth = [s for s in servers if rng.random() < 0.7]
    cases = []
    for name, tr in (("truth", truth), ("no-truth", None)):
        ring = gpu.HashRing()
        ring.addRemoveServers(servers, None)
        got = ring.routeShare(views, tr)
        assert sum(got["wrong"]) > 0 and (tr is None or sum(got["lost"]) > 0) and got["disputed"] == 1 << 32
        by_id = sorted(servers, key=ring.server_id)
        ids = ring.route_share_ids(np.array([[s in set(v) for s in by_id] for v in views]),
                                   None if tr is None else np.array([s in set(tr) for s in by_id]))
        assert ids["wrong"].tolist() == got["wrong"] and ids["lost"].tolist() == got["lost"]
        got["posWrong"] = [int(x) for x in ids["pos_wrong"]]
        cases.append({"name": name, "servers": servers, "views": views, "truth": tr, "want": got})
        ring.close()
    res = run_node("route_share_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 6 * len(cases) + 1
