"""GPU test of DistGossipSim.census: two ranks (gloo, one box) run the two-phase protocol with
all-reduces (MAX of max_inc, then SUM of the counts); every rank's result equals the unsharded
simulator's, `behind` its own nodes' slice. A revival makes some nodes lag, so the reference
incarnation matters."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_sim_census_gpu import cluster
from test_sim_shard_gpu import REPO, _free_port

sys.path.insert(0, os.path.join(REPO, "tests", "workers"))

pytestmark = pytest.mark.gpu


def test_dist_census_equals_unsharded(gpu, tmp_path):
    from dist_census_worker import scenario
    n, rounds, G = 120, 8, 2
    out = str(tmp_path / "census")
    port = _free_port()
    worker = os.path.join(REPO, "tests", "workers", "dist_census_worker.py")
    procs = []
    for r in range(G):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(G), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, str(n), str(rounds), out], env=env))
    names, inc0, dead = cluster(n)
    ref = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=6, events=scenario(n))
    ref.step(rounds)
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    want = {"default": ref.census(), "third": ref.census(third)}
    ref.close()
    assert want["default"]["behind"].any() and (want["default"]["at_max"] < want["default"]["observers"]).any()
    assert [p.wait(timeout=100) for p in procs] == [0] * G
    for r in range(G):
        d = np.load("%s.%d.npz" % (out, r))
        v0, nl = int(d["v0"]), int(d["nl"])
        for tag, w in want.items():
            assert int(d[tag + "_observers"]) == w["observers"], (r, tag)
            for k in ("status", "in_ring", "max_inc", "at_max"):
                got = d[tag + "_" + k]
                assert got.dtype == w[k].dtype and np.array_equal(got, w[k]), (r, tag, k)
            assert np.array_equal(d[tag + "_behind"], w["behind"][v0:v0 + nl]), (r, tag)
