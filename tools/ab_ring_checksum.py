"""A/B timing of rp_sim_ring_checksums against the composition a caller needs without it, in ONE
process, legs alternating.

    python tools/ab_ring_checksum.py [--nodes 10000] [--kills 100] [--suspicion 3] [--churn-rounds 6]
                                     [--settle-rounds 60] [--compose 64] [--rounds 7] [--out FILE]

A GossipSim of `nodes` nodes; `kills` of them are killed at round 1. Two states are measured: after
`churn-rounds` rounds (mid-churn: some views have dropped killed members, others not yet, so the
views fall into many ring-checksum classes) and after `settle-rounds` more (every node that is up
holds the same ring; the killed nodes keep the full ring they went down with).

  fused        GossipSim.ring_checksums() over all nodes, twin classes on (the default)
  no twins     the same with RP_SIM_RCK_TWINS=0: every view is built and hashed
  composition  on `compose` of the nodes, per node: ring_members(v), a host join of the sorted
               names it holds, and rp_hash32 of the string

Every leg ends with its result on the host, so the legs are timed with the wall clock; one warm-up
round, then `rounds` timed rounds, legs alternating. The tool checks in every round that the
composition's checksums equal the fused ones and that both fused legs agree. Prints one JSON
object: medians with min-max, the per-view times and their ratio (goal: fused per view <=
composition per view), and the classes at each state.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--kills", type=int, default=100)
    ap.add_argument("--suspicion", type=int, default=3)
    ap.add_argument("--churn-rounds", type=int, default=6)
    ap.add_argument("--settle-rounds", type=int, default=60)
    ap.add_argument("--compose", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_ring_checksum.py needs a HIP device (there is no CPU fallback)")
    rpa = bench.load_pkg()
    S = bench._synth()
    N = a.nodes
    names = [S.c2_addr(i) for i in range(N)]
    order = np.array(sorted(range(N), key=lambda i: names[i]))
    sorted_names = np.array([names[i] for i in order], dtype=object)
    killed = np.flatnonzero(S.kill_set(N, a.kills, 11))
    up = np.ones(N, dtype=bool)
    up[killed] = False
    sim = rpa.GossipSim(names, S.c3_members(N)[2], np.zeros(N, dtype=np.uint8), suspicion_rounds=a.suspicion,
                        events=[(1, "kill", int(v)) for v in killed])

    def fused(twins):
        if twins:
            os.environ.pop("RP_SIM_RCK_TWINS", None)
        else:
            os.environ["RP_SIM_RCK_TWINS"] = "0"
        t0 = time.perf_counter()
        out = sim.ring_checksums()
        ms = (time.perf_counter() - t0) * 1e3
        os.environ.pop("RP_SIM_RCK_TWINS", None)
        return ms, out

    def compose(pick):
        t0 = time.perf_counter()
        out = [rpa.hash32(";".join(sorted_names[sim.ring_members(int(v))[order]])) for v in pick]
        return (time.perf_counter() - t0) * 1e3, np.array(out, dtype=np.uint32)

    def measure(label):
        ms, ck = fused(True)  # (also the warm-up of the fused leg)
        odd = np.flatnonzero(ck != ck[0])
        pick = np.unique(np.concatenate([odd[np.linspace(0, len(odd) - 1, a.compose // 2).astype(int)] if len(odd) else
                                         np.zeros(0, dtype=np.int64), np.linspace(0, N - 1, a.compose).astype(np.int64)]))
        pick = pick[:a.compose]
        compose(pick[:2])
        fused(False)
        t_on, t_off, t_cmp, identical = [], [], [], True
        for _ in range(a.rounds):
            m1, c1 = fused(True)
            m2, c2 = compose(pick)
            m3, c3 = fused(False)
            t_on.append(m1)
            t_cmp.append(m2)
            t_off.append(m3)
            identical &= bool(np.array_equal(c1, c3) and np.array_equal(c1[pick], c2))
        on, off, cmp_ = stat(t_on), stat(t_off), stat(t_cmp)
        return {
            "state": label, "round": int(sim.round), "classes_all_nodes": int(len(set(ck.tolist()))),
            "classes_up_nodes": int(len(set(ck[up].tolist()))), "identical": identical,
            "fused_ms": on, "fused_no_twins_ms": off, "composition_ms": cmp_, "composed_views": int(len(pick)),
            "fused_us_per_view": on["median"] * 1e3 / N, "no_twins_us_per_view": off["median"] * 1e3 / N,
            "composition_us_per_view": cmp_["median"] * 1e3 / len(pick),
            "ratio_composition_over_fused_per_view": (cmp_["median"] / len(pick)) / (on["median"] / N),
        }

    sim.step(a.churn_rounds)
    churn = measure("mid-churn")
    sim.step(a.settle_rounds)
    settled = measure("settled")
    res = {"tool": "ab_ring_checksum", "nodes": N, "kills": int(len(killed)), "suspicion_rounds": a.suspicion,
           "timed_rounds": a.rounds, "converged": bool(sim.converged()), "states": [churn, settled]}
    sim.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not (churn["identical"] and settled["identical"]):
        sys.exit("the legs disagree")


if __name__ == "__main__":
    main()
