"""GPU test of DistGossipSim through a network partition: two ranks (gloo, one box) take the side
and heal events, and gather side_summary() over the group; every rank's checksums, sides() and
summary after every round equal the unsharded simulator's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_sim_census_gpu import cluster
from test_sim_shard_gpu import REPO, _free_port

sys.path.insert(0, os.path.join(REPO, "tests", "workers"))

pytestmark = pytest.mark.gpu


def test_dist_partition_equals_unsharded(gpu, tmp_path):
    from dist_sim_net_worker import FIELDS, scenario
    n, rounds, G = 61, 16, 2
    out = str(tmp_path / "net")
    port = _free_port()
    worker = os.path.join(REPO, "tests", "workers", "dist_sim_net_worker.py")
    procs = []
    for r in range(G):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(G), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, str(n), str(rounds), out], env=env))
    names, inc0, dead = cluster(n)
    ref = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=3, events=scenario(n))
    want = {k: [] for k in FIELDS + ("checksums", "sides")}
    for _ in range(rounds):
        ref.step()
        want["checksums"].append(ref.checksums())
        want["sides"].append(ref.sides())
        s = ref.side_summary()
        for k in FIELDS:
            want[k].append(s[k])
    ref.close()
    want = {k: np.stack(v) for k, v in want.items()}
    # the run sees three sides with observers, pingable members across the cut, and the heal
    assert (want["nodes"][5, :3] > 0).all() and want["cross_pingable"][3].any() and not want["sides"][-1].any()
    assert [p.wait(timeout=100) for p in procs] == [0] * G
    for r in range(G):
        d = np.load("%s.%d.npz" % (out, r))
        for k, w in want.items():
            assert d[k].dtype == w.dtype and np.array_equal(d[k], w), (r, k)
