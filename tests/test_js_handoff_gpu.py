"""GPU parity of the hand-off plan in the Node N-API host (ringpop-node_amd/js): ring.handoffPlan /
ring.handoffNames on a 64-server ring reproduce the Python binding's result for the same keys
(pinned against the CPU oracle and the numpy model in test_ring_handoff_gpu.py)."""
import shutil

import pytest

from test_js_moved_gpu import run_node

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]


def test_js_handoff_plan_matches_python(gpu, orc, tmp_path):
    initial = [orc.c2_addr(i) for i in range(64)]
    add, remove = [orc.c2_addr(64)], [initial[8]]
    whoami = initial[9]
    keys = [bytes(k).decode() for k in orc.uuid_keys(42, 0, 2055)] + ["k%d" % i for i in range(300)]
    cases = []
    for name, n, rev in (("n1", 1, False), ("n3", 3, False), ("n3-hashFunc", 3, True)):
        ring = gpu.HashRing({"hashFunc": lambda s: orc.hash32(s[::-1])} if rev else None)
        ring.addRemoveServers(initial, None)
        snap = ring.snapshot()
        ring.addRemoveServers(add, remove)
        dests, goff, kidx, src, slot = ring.handoff_ids(keys, snap, n)
        assert 0 < len(kidx) < len(keys) and ring.handoff_count == len(kidx)
        plan = ring.handoffPlan(keys, snap, n)
        md, mg, mk, _, _ = ring.handoff_ids(keys, snap, n, only_src=ring.server_id(whoami))
        cases.append({"name": name, "n": n, "reverseHash": rev, "initial": initial, "add": add, "remove": remove,
                      "keys": keys, "whoami": whoami,
                      "want": {"groupOff": goff.tolist(), "keyIdx": kidx.tolist(), "slot": slot.tolist(),
                               "dests": list(plan), "transfers": [[[k, s] for k, s in v] for v in plan.values()],
                               "mine": {"keyIdx": mk.tolist(), "groupOff": mg.tolist()}}})
        snap.close()
        ring.close()
    res = run_node("handoff_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 11 * len(cases)
