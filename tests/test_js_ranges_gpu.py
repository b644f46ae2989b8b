"""GPU parity of movedRanges in the Node N-API host (ringpop-node_amd/js): ring.movedRanges /
ring.movedRangeNames / snap.dump() on a 64-server ring reproduce the Python binding's result for
the same ring change (pinned against the CPU oracle in test_ring_ranges_gpu.py)."""
import shutil

import pytest

from test_js_moved_gpu import run_node

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]


def test_js_moved_ranges_match_python(gpu, orc, tmp_path):
    initial = [orc.c2_addr(i) for i in range(64)]
    add, remove = [orc.c2_addr(64)], [initial[8]]
    cases = []
    for n in (1, 3):
        ring = gpu.HashRing()
        ring.addRemoveServers(initial, None)
        snap = ring.snapshot()
        ring.addRemoveServers(add, remove)
        got = ring.movedRanges(snap, n)
        assert 0 < len(got) == ring.moved_range_count and 0 < ring.moved_hash_count < 1 << 32
        tokens, owners = snap.dump()
        cases.append({"name": "n%d" % n, "n": n, "initial": initial, "add": add, "remove": remove,
                      "want": {"lo": [l for l, _, _, _ in got], "hi": [h for _, h, _, _ in got],
                               "before": [b for _, _, b, _ in got], "after": [a for _, _, _, a in got],
                               "movedHashes": ring.moved_hash_count, "tokens": [int(t) for t in tokens],
                               "owners": [ring.name(o) for o in owners]}})
        snap.close()
        ring.close()
    res = run_node("ranges_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 14 * len(cases)
