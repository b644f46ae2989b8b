"""GPU test of DistGossipSim.timeline(): two ranks (gloo, one box) run a kill, a three-way split, a
leave and a heal with the timeline on; every rank's all-reduced timeline equals the unsharded
simulator's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import timeline_model as tm
from test_sim_census_gpu import cluster
from test_sim_shard_gpu import REPO, _free_port

sys.path.insert(0, os.path.join(REPO, "tests", "workers"))

pytestmark = pytest.mark.gpu


def test_dist_timeline_equals_unsharded(gpu, tmp_path):
    from dist_sim_net_worker import scenario
    n, rounds, G = 61, 16, 2
    out = str(tmp_path / "tl")
    port = _free_port()
    worker = os.path.join(REPO, "tests", "workers", "dist_timeline_worker.py")
    procs = []
    for r in range(G):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(G), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, str(n), str(rounds), out], env=env))
    names, inc0, dead = cluster(n)
    ref = gpu.GossipSim(names, inc0, dead, seed=7, suspicion_rounds=3, events=scenario(n))
    ref.timeline_enable(rounds)
    ref.step_async(rounds)
    want = ref.timeline()
    ref.close()
    # the run sees live members dropped across the cut, unmet wanted statuses and a leave
    assert want["false_faulty"].any() and want["unmet"].any() and (want["first_seen"][:, 2] != gpu.SIM_NEVER).any()
    assert [p.wait(timeout=100) for p in procs] == [0] * G
    for r in range(G):
        d = np.load("%s.%d.npz" % (out, r))
        assert tm.same(d, want) is None, (r, tm.same(d, want))
