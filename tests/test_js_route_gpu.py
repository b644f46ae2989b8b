"""GPU parity of routeViews in the Node N-API host (ringpop-node_amd/js): ring.routeViews on a
64-server ring reproduces the Python binding's result for the same keys, views and truth (pinned
against the numpy model in test_ring_route_gpu.py)."""
import shutil

import numpy as np
import pytest

from test_js_moved_gpu import run_node

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]


def test_js_route_views_match_python(gpu, orc, tmp_path):
    servers = [orc.c2_addr(i) for i in range(64)]
    keys = [bytes(k).decode() for k in orc.uuid_keys(42, 0, 600)] + ["k%d" % i for i in range(100)]
    rng = np.random.default_rng(3)
    views = [[s for s in servers if rng.random() < 0.9] for _ in range(66)]
    views += [[], servers[9:10], servers + ["10.9.9.9:1"]]
    truth = [s for s in servers if rng.random() < 0.8]
    cases = []
    for name, tr, rev in (("truth", truth, False), ("no-truth", None, False), ("hashFunc", truth, True)):
        ring = gpu.HashRing({"hashFunc": lambda s: orc.hash32(s[::-1])} if rev else None)
        ring.addRemoveServers(servers, None)
        got = ring.routeViews(keys, views, tr)
        assert sum(got["wrong"]) > 0 and (tr is None or sum(got["lost"]) > 0)
        ids = ring.route_view_ids(keys, np.array([[s in set(v) for s in sorted(servers, key=ring.server_id)]
                                                  for v in views]),
                                  None if tr is None else np.array([s in set(tr) for s in
                                                                    sorted(servers, key=ring.server_id)]))
        got["keyWrong"] = [int(x) for x in ids["key_wrong"]]
        assert ids["wrong"].tolist() == got["wrong"]
        cases.append({"name": name, "reverseHash": rev, "servers": servers, "keys": keys, "views": views, "truth": tr,
                      "want": got})
        ring.close()
    res = run_node("route_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 8 * len(cases)
