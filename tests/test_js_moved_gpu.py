"""GPU parity of ring snapshots and movedKeys in the Node N-API host (ringpop-node_amd/js):
ring.snapshot() / ring.movedKeys / ring.movedNames on a 64-server ring reproduce the Python
binding's result for the same keys (pinned against the CPU oracle in test_ring_moved_gpu.py)."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None, reason="node not in this image")]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_node(script, payload, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "ringpop-node_amd", "js")])
    inp = tmp_path / "in.json"
    inp.write_text(json.dumps(payload))
    out = subprocess.run(["node", os.path.join(REPO, "tests", "js", script), str(inp)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_js_moved_keys_match_python(gpu, orc, tmp_path):
    initial = [orc.c2_addr(i) for i in range(64)]
    add, remove = [orc.c2_addr(64)], [initial[8]]
    keys = [bytes(k).decode() for k in orc.uuid_keys(42, 0, 2055)] + ["k%d" % i for i in range(300)]
    cases = []
    for name, n, rev in (("n1", 1, False), ("n3", 3, False), ("n3-hashFunc", 3, True)):
        ring = gpu.HashRing({"hashFunc": lambda s: orc.hash32(s[::-1])} if rev else None)
        ring.addRemoveServers(initial, None)
        snap = ring.snapshot()
        tokens = snap.info()["tokens"]
        ring.addRemoveServers(add, remove)
        got = ring.movedKeys(keys, snap, n)
        assert 0 < len(got) < len(keys)
        cases.append({"name": name, "n": n, "reverseHash": rev, "initial": initial, "add": add, "remove": remove,
                      "keys": keys,
                      "want": {"idx": [keys.index(k) for k, _, _ in got], "before": [b for _, b, _ in got],
                               "after": [a for _, _, a in got], "tokens": tokens}})
        snap.close()
        ring.close()
    res = run_node("moved_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 11 * len(cases)
