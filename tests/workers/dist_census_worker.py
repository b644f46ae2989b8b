"""One rank of a DistGossipSim census (launched by tests/test_sim_census_dist_gpu.py as WORLD_SIZE
processes on the same box). Every rank writes its census after ROUNDS rounds, for the default
observers and for every third node, to OUT.<rank>.npz.

    RANK=r WORLD_SIZE=g MASTER_ADDR=127.0.0.1 MASTER_PORT=p python dist_census_worker.py n rounds out
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dist_sim_worker import REPO, load  # noqa: E402


def scenario(n):
    return [(1, "kill", 2), (1, "kill", n // 2), (1, "kill", n - 1), (6, "revive", 2)]


def main():
    n, rounds, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    rpa = load("ringpop_node_amd", os.path.join(REPO, "ringpop-node_amd", "__init__.py"))
    S = load("rp_synth", os.path.join(REPO, "ringpop-node_amd", "synth.py"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    names = [S.c2_addr(i) for i in range(n)]
    sim = rpa.DistGossipSim(names, S.c3_members(n)[2], np.zeros(n, dtype=np.uint8), seed=7, suspicion_rounds=6,
                            device=0, events=scenario(n))
    sim.step(rounds)
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    res = {}
    for tag, obs in (("default", None), ("third", third)):
        for k, v in sim.census(obs).items():
            res[tag + "_" + k] = np.asarray(v)
    np.savez("%s.%d.npz" % (out, dist.get_rank()), v0=sim.shard.v0, nl=sim.shard.NL, **res)
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
