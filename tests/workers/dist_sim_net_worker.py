"""One rank of a DistGossipSim run through a network partition (launched by
tests/test_sim_net_dist_gpu.py as WORLD_SIZE processes on the same box). Every rank writes the
gathered checksums, sides() and side_summary() after each round to OUT.<rank>.npz.

    RANK=r WORLD_SIZE=g MASTER_ADDR=127.0.0.1 MASTER_PORT=p python dist_sim_net_worker.py n rounds out
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dist_sim_worker import REPO, load  # noqa: E402

FIELDS = ("nodes", "ck_min", "ck_max", "cross_pingable", "settled")


def scenario(n):
    """A kill, a three-way split at round 2 (the cut crosses the ranks' bound), a leave on one side,
    a heal at round 9."""
    return ([(1, "kill", 1)] + [(2, "side", v, v % 3) for v in range(n) if v % 3] + [(4, "leave", 3)] +
            [(9, "heal", 0)])


def main():
    n, rounds, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    rpa = load("ringpop_node_amd", os.path.join(REPO, "ringpop-node_amd", "__init__.py"))
    S = load("rp_synth", os.path.join(REPO, "ringpop-node_amd", "synth.py"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    names = [S.c2_addr(i) for i in range(n)]
    sim = rpa.DistGossipSim(names, S.c3_members(n)[2], np.zeros(n, dtype=np.uint8), seed=7, suspicion_rounds=3,
                            device=0, events=scenario(n))
    res = {k: [] for k in FIELDS + ("checksums", "sides")}
    for _ in range(rounds):
        sim.step()
        res["checksums"].append(sim.checksums())
        res["sides"].append(sim.sides())
        s = sim.side_summary()
        for k in FIELDS:
            res[k].append(s[k])
    np.savez("%s.%d.npz" % (out, dist.get_rank()), **{k: np.stack(v) for k, v in res.items()})
    sim.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
