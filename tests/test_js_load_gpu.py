"""GPU parity of ownerLoad / ownerShare in the Node N-API host (ringpop-node_amd/js): on a
64-server ring (+1 / -1 server) they equal values computed here from the CPU oracle: lookupN rows
counted per server and slot, and the gaps of the sorted token array summed per owner."""
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


def test_js_owner_load_and_share_match_the_oracle(gpu, orc, tmp_path):
    import numpy as np

    initial = [orc.c2_addr(i) for i in range(64)]
    add, remove = [orc.c2_addr(64)], [initial[8]]
    servers = [s for s in initial if s not in remove] + add  # Object.keys(servers)
    keys = [bytes(k).decode() for k in orc.uuid_keys(42, 0, 2055)] + ["k%d" % i for i in range(300)]
    cases = []
    for name, n, rev in (("n1", 1, False), ("n3", 3, False), ("n3-hashFunc", 3, True)):
        hf = (lambda s: orc.hash32(s[::-1])) if rev else orc.hash32
        tk = (lambda ns: np.array([hf(s + str(i)) for s in ns for i in range(100)], dtype=np.uint32)) if rev \
            else (lambda ns: None)
        oracle = orc.Ring(100)
        oracle.add_remove(initial, None, add_tokens=tk(initial))
        oracle.add_remove(add, remove, add_tokens=tk(add), rem_tokens=tk(remove))
        load = {s: [0] * n for s in servers}
        for k in keys:
            row = oracle.lookupn_hash(hf(k), n)
            assert len(row) == n
            for q, o in enumerate(row):
                load[oracle.name(o)][q] += 1
        tok, own = oracle.dump()
        share = {s: 0 for s in servers}
        for i in range(len(tok)):
            gap = int(tok[i]) - int(tok[i - 1]) if i else int(tok[0]) + (1 << 32) - int(tok[-1])
            share[oracle.name(int(own[i]))] += gap
        assert sum(share.values()) == 1 << 32 and sum(v[0] for v in load.values()) == len(keys)
        cases.append({"name": name, "n": n, "reverseHash": rev, "initial": initial, "add": add, "remove": remove,
                      "keys": keys, "want": {"servers": servers, "load": load, "share": share}})
    res = run_node("load_parity.js", {"cases": cases}, tmp_path)
    assert res["nfail"] == 0, res["fails"]
    assert res["checks"] == 9 * len(cases)
